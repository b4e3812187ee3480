"""NumPy model of MXFP4 (sleekit_amd.mx), written from the format and the definition of its scale choice alone.

Scales: per (row, block of 32 columns) the reference's grid search (oracle.scaling_ref: no_clip_scale, quantize_scaled,
grid_error and the strict first-minimum walk) over the power-of-two candidates 0.125, 0.25, 0.5, 1 times the smallest power
of two at or above the non-saturating scale.  Codes, bytes and values: bit by bit, sharing nothing with the kernels' word
arithmetic.  tests/test_mx_cpu.py pins the model to the reference's own results (tests/golden/mx.npz), so the GPU tests
may use it as their oracle beyond the fixtures' shapes.
"""

import numpy as np

from oracle import grid, scaling_ref

BLOCK = 32
VALUES = [-6, -4, -3, -2, -1.5, -1, -0.5, 0, 0.5, 1, 1.5, 2, 3, 4, 6]
MAGNITUDES = np.array([0, 0.5, 1, 1.5, 2, 3, 4, 6], np.float32)
FACTORS = (0.125, 0.25, 0.5, 1.0)


def e2m1_grid():
    return grid.TableGrid(VALUES)


def pow2_at_or_above(x):
    """The smallest power of two >= x, for positive normal float32 x."""
    m, e = np.frexp(np.asarray(x, np.float32))  # x = m 2^e, 0.5 <= m < 1
    return np.ldexp(np.float32(1), e - (m == 0.5)).astype(np.float32)


def block_scales(block, hdiag, mode):
    """The scales of one column block (R, 32) -> (R,) float32, and whether any candidate's error was below +inf."""
    g = e2m1_grid()
    base = pow2_at_or_above(scaling_ref.no_clip_scale(block, g, 0))
    if mode == "max":
        return base, np.ones(base.size, bool)
    chosen = np.full(base.size, np.inf, dtype=np.float32)
    lowest = np.full(base.size, np.inf, dtype=np.float32)
    for f in FACTORS:
        sc = np.float32(f) * base
        with np.errstate(over="ignore", invalid="ignore"):
            err = scaling_ref.grid_error(hdiag, scaling_ref.quantize_scaled(block, sc, g) - block)
        better = err < lowest
        lowest[better] = err[better]
        chosen[better] = f
    found = np.isfinite(chosen)
    chosen[~found] = 1.0  # no error below +inf (squares that overflow): the non-saturating base is kept
    return base * chosen, found


def scales_model(W, H=None, mode="mse", want_found=False):
    """compute_mx_scales as NumPy: (S float32, E uint8), (R, n / 32) each."""
    assert mode in ("max", "mse", "diag") and W.shape[1] % BLOCK == 0
    W = np.asarray(W, np.float32)
    hd = None if mode != "diag" else np.asarray(H).diagonal()
    cols = [block_scales(W[:, k:k + BLOCK], None if hd is None else hd[k:k + BLOCK], mode) for k in range(0, W.shape[1], BLOCK)]
    S = np.stack([c[0] for c in cols], axis=1).astype(np.float32)
    found = np.stack([c[1] for c in cols], axis=1)
    return (S, encode_model(S), found) if want_found else (S, encode_model(S))


def encode_model(S):
    """float32 powers of two -> E8M0 bytes; ValueError for anything else."""
    S = np.asarray(S, np.float32)
    m, e = np.frexp(S)
    if not ((m == 0.5) & (e - 1 >= -126) & (e - 1 <= 127)).all():
        raise ValueError("not a power of two E8M0 holds")
    return (e - 1 + 127).astype(np.uint8)


def decode_model(E):
    E = np.asarray(E, np.uint8)
    assert (E != 255).all()
    return np.ldexp(np.float32(1), E.astype(np.int32) - 127).astype(np.float32)


def codes_of(idx):
    """Table index -> code: i < 7 is 8 | (7 - i), otherwise i - 7; an index above 14 is stored as code 7."""
    i = np.minimum(np.asarray(idx).astype(np.int32), 14)
    return np.where(i < 7, 8 | (7 - i), i - 7).astype(np.uint8)


def indices_of(code):
    """Code -> table index; 0x8 (-0) reads as index 7."""
    c = np.asarray(code).astype(np.int32)
    return np.where(c >= 8, 7 - (c & 7), c + 7).astype(np.uint8)


def pack_model(idx, S):
    """(codes uint8 (R, n / 2), scales uint8 (R, n / 32))."""
    c = codes_of(idx)
    return (c[:, 0::2] | (c[:, 1::2] << 4)).astype(np.uint8), encode_model(S)


def nibbles(codes):
    codes = np.asarray(codes, np.uint8)
    out = np.empty((codes.shape[0], 2 * codes.shape[1]), np.uint8)
    out[:, 0::2] = codes & 15
    out[:, 1::2] = codes >> 4
    return out


def unpack_model(codes, scales):
    return indices_of(nibbles(codes)), decode_model(scales)


def dequantize_model(codes, scales):
    """float32 (R, n): +-magnitude * 2^(b - 127), code 0x8 as +0."""
    c = nibbles(codes)
    mag = MAGNITUDES[c & 7]
    val = np.where((c >> 3).astype(bool) & (mag != 0), -mag, mag).astype(np.float32)
    with np.errstate(over="ignore"):  # (6 * 2^127 is +inf in float32, as it is on the device)
        return np.ldexp(val, np.repeat(np.asarray(scales).astype(np.int32) - 127, BLOCK, axis=1)).astype(np.float32)


def case_layer(c):
    """The layer of a fixture case (tests/golden/make_golden_mx.py): the synthetic generator's, then what `special` says --
    ["zero", k]: block k all zeros; ["negative", k]: block k all negative; ["outlier"]: one element of every block of every
    row 8 to 64 times larger (so that scales below the non-saturating one win)."""
    from sleekit_amd import synth

    L = synth.make_layer(c["R"], c["n"], c["seed"])
    W = L["W"]
    special = c.get("special")
    if special:
        kind = special[0]
        if kind == "zero":
            W[:, special[1] * BLOCK:(special[1] + 1) * BLOCK] = 0
        elif kind == "negative":
            blk = W[:, special[1] * BLOCK:(special[1] + 1) * BLOCK]
            blk[...] = -np.abs(blk) - np.float32(1e-3)
        elif kind == "outlier":
            for r in range(c["R"]):
                for k in range(c["n"] // BLOCK):
                    W[r, k * BLOCK + (7 * r + 3 * k) % BLOCK] *= np.float32(8 << ((r + k) % 4))
        else:
            raise ValueError(special)
    return L
