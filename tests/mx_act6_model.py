"""NumPy model of the MXFP6 (E2M3) activation format (sleekit_amd.mx: quantize_mxfp6_act, dequantize_mxfp6_act,
matmul_mx(activations="mxfp6_e2m3")), written from the rules alone.

Scale of a block of 32: b0 = max(amax / float32(7.5), float32(1e-16)) in float32, the smallest power of two >= b0, its
exponent + 127 as a byte.  Elements: x / s (exact) rounded to nearest onto OCP E2M3 (bias 1, subnormals m / 8, normals
2^(e - 1) (1 + m / 8) for e = 1 .. 3) -- found here by exact float64 arithmetic on the grid's spacing (0.125 below 2, 0.25
below 4, 0.5 above) with np.rint, sharing nothing with the kernels' word arithmetic -- ties to the even code, clamped at 7.5,
code = sign << 5 | e << 3 | m, a zero magnitude as 0x00.  A row of a_codes is a little-endian bit stream, element k at bits
6 k .. 6 k + 5: four codes c0 .. c3 are the three bytes of c0 | c1 << 6 | c2 << 12 | c3 << 18.
"""

import numpy as np

import mx_model

BLOCK = 32
# the 32 magnitudes, by code
GRID = np.array([m / 8.0 for m in range(8)] + [2.0 ** (e - 1) * (1 + m / 8.0) for e in (1, 2, 3) for m in range(8)])
MIDPOINTS = (GRID[:-1] + GRID[1:]) / 2  # 31 of them; midpoint i lies between codes i and i + 1, one odd and one even
LARGEST = 7.5


def act_scales_model(X):
    """(M, K) -> E8M0 bytes (M, K / 32)."""
    X = np.asarray(X).astype(np.float32)
    M, K = X.shape
    assert K % BLOCK == 0
    amax = np.abs(X.reshape(M, K // BLOCK, BLOCK)).max(axis=2)
    b0 = np.maximum(amax / np.float32(LARGEST), np.float32(1e-16)).astype(np.float32)
    s = mx_model.pow2_at_or_above(b0)
    return (np.log2(s.astype(np.float64)).round().astype(np.int64) + 127).astype(np.uint8)


def e2m3_encode(y):
    """float64 y (already divided by the scale) -> E2M3 codes 0 .. 63, one an element: nearest, ties to the even code,
    clamped at +-7.5, never 0x20."""
    y = np.asarray(y, np.float64)
    a = np.minimum(np.abs(y), LARGEST)
    step = np.where(a < 2.0, 0.125, np.where(a < 4.0, 0.25, 0.5))  # the grid's spacing around a
    # exact quotient; np.rint takes a tie to the even multiple of the step, which is the even code in every span (the spans
    # start at 0, 2 and 4: even multiples with even codes 0x00, 0x10, 0x18), and 2 or 4 reached from below are on the grid
    v = np.rint(a / step) * step
    code = np.searchsorted(GRID, v)
    assert (GRID[code] == v).all()
    return np.where((code > 0) & (y < 0), code | 0x20, code).astype(np.uint8)


def e2m3_decode(codes):
    """E2M3 codes -> float64 values."""
    c = np.asarray(codes).astype(np.int64)
    return np.where(c & 0x20, -GRID[c & 31], GRID[c & 31])


def pack_codes(c):
    """(M, K) codes, one an element -> (M, 3 K / 4) bytes of the bit stream."""
    c = np.asarray(c).astype(np.uint32)
    M, K = c.shape
    assert K % 4 == 0 and (c < 64).all()
    q = c.reshape(M, K // 4, 4)
    word = q[:, :, 0] | (q[:, :, 1] << 6) | (q[:, :, 2] << 12) | (q[:, :, 3] << 18)
    return np.stack([word & 0xff, (word >> 8) & 0xff, (word >> 16) & 0xff], axis=2).astype(np.uint8).reshape(M, 3 * K // 4)


def unpack_codes(b):
    """(M, 3 K / 4) bytes -> (M, K) codes."""
    b = np.asarray(b).astype(np.uint32)
    M, W = b.shape
    assert W % 3 == 0
    t = b.reshape(M, W // 3, 3)
    word = t[:, :, 0] | (t[:, :, 1] << 8) | (t[:, :, 2] << 16)
    return np.stack([(word >> (6 * i)) & 63 for i in range(4)], axis=2).astype(np.uint8).reshape(M, 4 * W // 3)


def quantize_act6_model(X):
    """(a_codes (M, 3 K / 4), a_scales (M, K / 32))."""
    X = np.asarray(X).astype(np.float32)
    E = act_scales_model(X)
    y = X.astype(np.float64) * 2.0 ** (127.0 - np.repeat(E.astype(np.float64), BLOCK, axis=1))
    return pack_codes(e2m3_encode(y)), E


def dequantize_act6_model(a_codes, a_scales, dtype=np.float64):
    """value(code) * 2^(b - 127), (M, K): float64 (exact), or rounded once to `dtype`."""
    v = e2m3_decode(unpack_codes(a_codes)) * 2.0 ** (np.repeat(np.asarray(a_scales).astype(np.float64), BLOCK, axis=1) - 127.0)
    return v.astype(dtype)


def matmul_model(a_codes, a_scales, w_codes, w_scales, bias=None):
    """(Y float64 (M, N), sum_k |a w| (M, N)) of MXFP6 activations against an MXFP4 layer."""
    A, W = dequantize_act6_model(a_codes, a_scales), mx_model.dequantize_model(w_codes, w_scales).astype(np.float64)
    Y = A @ W.T
    if bias is not None:
        Y = Y + np.asarray(bias, np.float64)[None, :]
    return Y, np.abs(A) @ np.abs(W).T
