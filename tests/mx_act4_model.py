"""NumPy model of the MXFP4 activation format (sleekit_amd.mx: quantize_mxfp4_act, matmul_mx(activations="mxfp4")), written
from the rules alone.

Scale of a block of 32: b0 = max(amax / float32(6), float32(1e-16)) in float32, the smallest power of two >= b0, its
exponent + 127 as a byte.  Elements: x / s (exact) rounded to nearest onto 0, .5, 1, 1.5, 2, 3, 4, 6 -- found here by exact
float64 arithmetic on the grid's spacing (0.5 below 2, 1 below 4, 2 above), sharing nothing with the kernels' word
arithmetic -- ties to the even code, clamped at 6, code = sign << 3 | index, a zero magnitude as 0x0; two codes a byte, the
even k in the low nibble.  De-quantizing is tests/mx_model.py's dequantize_model: the layout is the weights'.
"""

import numpy as np

import mx_model

BLOCK = 32
MIDPOINTS = np.array([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0])


def act_scales_model(X):
    """(M, K) -> E8M0 bytes (M, K / 32)."""
    X = np.asarray(X).astype(np.float32)
    M, K = X.shape
    assert K % BLOCK == 0
    amax = np.abs(X.reshape(M, K // BLOCK, BLOCK)).max(axis=2)
    b0 = np.maximum(amax / np.float32(6), np.float32(1e-16)).astype(np.float32)
    s = mx_model.pow2_at_or_above(b0)
    return (np.log2(s.astype(np.float64)).round().astype(np.int64) + 127).astype(np.uint8)


def e2m1_encode(y):
    """float64 y (already divided by the scale) -> E2M1 codes 0 .. 15, one an element: nearest, ties to the even code,
    clamped at +-6, never 0x8."""
    y = np.asarray(y, np.float64)
    a = np.minimum(np.abs(y), 6.0)
    step = np.where(a < 2.0, 0.5, np.where(a < 4.0, 1.0, 2.0))  # the grid's spacing around a
    v = np.rint(a / step) * step  # exact quotient; np.rint takes a tie to the even multiple, which is the even code in every span
    grid = mx_model.MAGNITUDES.astype(np.float64)
    index = np.searchsorted(grid, v)
    assert (grid[index] == v).all()
    return np.where((index > 0) & (y < 0), index | 8, index).astype(np.uint8)


def pack_nibbles(c):
    return (c[:, 0::2] | (c[:, 1::2] << 4)).astype(np.uint8)


def quantize_act4_model(X):
    """(a_codes (M, K / 2), a_scales (M, K / 32))."""
    X = np.asarray(X).astype(np.float32)
    E = act_scales_model(X)
    y = X.astype(np.float64) * 2.0 ** (127.0 - np.repeat(E.astype(np.float64), BLOCK, axis=1))
    return pack_nibbles(e2m1_encode(y)), E


def dequantize_act4_model(a_codes, a_scales):
    """value(code) * 2^(b - 127) as float64 (exact)."""
    return mx_model.dequantize_model(a_codes, a_scales).astype(np.float64)


def matmul_model(a_codes, a_scales, w_codes, w_scales, bias=None):
    """(Y float64 (M, N), sum_k |a w| (M, N)) of MXFP4 activations against an MXFP4 layer."""
    A, W = dequantize_act4_model(a_codes, a_scales), dequantize_act4_model(w_codes, w_scales)
    Y = A @ W.T
    if bias is not None:
        Y = Y + np.asarray(bias, np.float64)[None, :]
    return Y, np.abs(A) @ np.abs(W).T
