"""NumPy model of MXFP6 (E2M3) layers (sleekit_amd.mx: compute_mx_scales(weights="mxfp6_e2m3"), pack_mxfp6, unpack_mxfp6,
dequantize_mxfp6, quantize_mxfp6, matmul_mx(weights="mxfp6_e2m3")), written from the format and the definition of the scale
choice alone.

The element grid is the 63-entry table -7.5 .. 7.5 with np.digitize on its midpoints (oracle.grid.TableGrid: a tie goes
upward).  Scales: tests/mx_model.py's rule -- the reference's grid search over 0.125, 0.25, 0.5, 1 times the smallest power of
two at or above the non-saturating scale -- with this table in place of E2M1's.  Codes, the stream of 6-bit codes and the
values: bit by bit (the stream is tests/mx_act6_model.py's, the activations' own form).  tests/test_mx6_cpu.py pins the
model to the reference's own results (tests/golden/mx6.npz), so the GPU tests may use it beyond the fixtures' shapes.
"""

import numpy as np

import mx_act6_model as act6
import mx_model
from mx_model import BLOCK, FACTORS, decode_model, encode_model, pow2_at_or_above  # noqa: F401  (the scales are MXFP4's)
from oracle import grid, scaling_ref

MAGNITUDES = act6.GRID.astype(np.float32)          # by code 0 .. 31
VALUES = [-float(v) for v in act6.GRID[:0:-1]] + [float(v) for v in act6.GRID]   # the 63 table entries, index 31 is 0
LARGEST = 7.5


def e2m3_grid():
    return grid.TableGrid(VALUES)


def block_scales(block, hdiag, mode):
    """mx_model.block_scales with the E2M3 table: (scales (R,) float32, whether any candidate's error was below +inf)."""
    g = e2m3_grid()
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
    chosen[~found] = 1.0
    return base * chosen, found


def scales_model(W, H=None, mode="mse", want_found=False):
    """compute_mx_scales(..., weights="mxfp6_e2m3") as NumPy: (S float32, E uint8), (R, n / 32) each."""
    assert mode in ("max", "mse", "diag") and W.shape[1] % BLOCK == 0
    W = np.asarray(W, np.float32)
    hd = None if mode != "diag" else np.asarray(H).diagonal()
    cols = [block_scales(W[:, k:k + BLOCK], None if hd is None else hd[k:k + BLOCK], mode) for k in range(0, W.shape[1], BLOCK)]
    S = np.stack([c[0] for c in cols], axis=1).astype(np.float32)
    found = np.stack([c[1] for c in cols], axis=1)
    return (S, encode_model(S), found) if want_found else (S, encode_model(S))


def codes_of(idx):
    """Table index -> code: i < 31 is 0x20 | (31 - i), otherwise i - 31; an index above 62 is stored as code 0x1f."""
    i = np.minimum(np.asarray(idx).astype(np.int32), 62)
    return np.where(i < 31, 0x20 | (31 - i), i - 31).astype(np.uint8)


def indices_of(code):
    """Code -> table index; 0x20 (-0) reads as index 31."""
    c = np.asarray(code).astype(np.int32)
    return np.where(c & 0x20, 31 - (c & 31), c + 31).astype(np.uint8)


def pack_model(idx, S):
    """(codes uint8 (R, 3 n / 4), scales uint8 (R, n / 32))."""
    return act6.pack_codes(codes_of(idx)), encode_model(S)


def unpack_model(codes, scales):
    return indices_of(act6.unpack_codes(codes)), decode_model(scales)


def dequantize_model(codes, scales):
    """float32 (R, n): +-magnitude * 2^(b - 127); code 0x20 as -0 * s (never written by the pack)."""
    c = act6.unpack_codes(codes)
    mag = MAGNITUDES[c & 31]
    val = np.where((c & 0x20).astype(bool), -mag, mag).astype(np.float32)
    with np.errstate(over="ignore"):
        return np.ldexp(val, np.repeat(np.asarray(scales).astype(np.int32) - 127, BLOCK, axis=1)).astype(np.float32)


OUTLIERS = (1.5, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128)


def case_layer(c):
    """The layer of a fixture case (tests/golden/make_golden_mx6.py): mx_model.case_layer's, and one more `special` --
    ["small_diag", j]: column j of every block carries an outlier, OUTLIERS[(r + 5 k) % 14] times the block's largest other
    magnitude in row r, block k, and H becomes D H D with D = 1e-2 on those columns and 1 elsewhere, so their diagonal
    entries are 1e-4 of what they were and H stays positive definite: the less the outlier's saturation weighs, the lower
    the factor that wins under "diag"."""
    special = c.get("special")
    if not special or special[0] != "small_diag":
        return mx_model.case_layer(c)
    L = mx_model.case_layer(dict(c, special=None))
    W, H, j = L["W"], L["H"], special[1]
    d = np.ones(c["n"], H.dtype)
    for k in range(c["n"] // BLOCK):
        col = k * BLOCK + j
        d[col] = 1e-2
        rest = np.abs(np.delete(W[:, k * BLOCK:(k + 1) * BLOCK], j, axis=1)).max(axis=1)
        mult = np.array([OUTLIERS[(r + 5 * k) % len(OUTLIERS)] for r in range(c["R"])], W.dtype)
        W[:, col] = np.where(np.arange(c["R"]) % 2 == 0, 1, -1).astype(W.dtype) * rest * mult
    H[...] = d[:, None] * H * d[None, :]
    return L


def matmul_model(a_values, w_codes, w_scales, bias=None):
    """(Y float64 (M, N), sum_k |a w| (M, N)) of de-quantized activations A (float64 (M, K)) against an MXFP6 layer."""
    A, W = np.asarray(a_values, np.float64), dequantize_model(w_codes, w_scales).astype(np.float64)
    Y = A @ W.T
    if bias is not None:
        Y = Y + np.asarray(bias, np.float64)[None, :]
    return Y, np.abs(A) @ np.abs(W).T
