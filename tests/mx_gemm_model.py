"""NumPy model of the MXFP8 activation format and of the packed product (sleekit_amd.mx: quantize_mxfp8, dequantize_mxfp8,
matmul_mx), written from the rules alone.

Scale of a block of 32: b0 = max(amax / float32(448), float32(1e-16)) in float32, the smallest power of two >= b0, its
exponent + 127 as a byte.  Elements: x / s (exact) rounded to nearest even onto the OCP E4M3 grid -- found here by
exact float64 arithmetic on the grid's spacing, sharing nothing with the kernels' word arithmetic -- clamped at 448,
code = sign << 7 | exp << 3 | man, a zero magnitude as 0x00.  The product is the float64 product of the de-quantized
operands; the weights' side is tests/mx_model.py's dequantize_model.
"""

import numpy as np

import mx_model

BLOCK = 32


def act_scales_model(X):
    """(M, K) -> E8M0 bytes (M, K / 32)."""
    X = np.asarray(X).astype(np.float32)
    M, K = X.shape
    assert K % BLOCK == 0
    amax = np.abs(X.reshape(M, K // BLOCK, BLOCK)).max(axis=2)
    b0 = np.maximum(amax / np.float32(448), np.float32(1e-16)).astype(np.float32)
    s = mx_model.pow2_at_or_above(b0)
    return (np.log2(s.astype(np.float64)).round().astype(np.int64) + 127).astype(np.uint8)


def e4m3_encode(y):
    """float64 y (already divided by the scale) -> E4M3 codes: nearest, ties to even, clamped at +-448, no -0."""
    y = np.asarray(y, np.float64)
    a = np.minimum(np.abs(y), 448.0)
    # the binade of a, not below the first normal one: the grid's spacing there is 2^(e - 3) (subnormals: 2^-9)
    e = np.maximum(np.floor(np.log2(np.maximum(a, 2.0 ** -6))), -6.0)
    step = 2.0 ** (e - 3)
    k = np.rint(a / step)  # exact quotient (a power of two), np.rint rounds a tie to even; k <= 16
    v = k * step  # the rounded magnitude (k = 16: the next binade's first value)
    code = np.zeros(a.shape, np.int64)
    nz = v > 0
    ev = np.floor(np.log2(np.where(nz, v, 1.0)))
    normal = nz & (ev >= -6)
    code[normal] = (((ev[normal] + 7).astype(np.int64)) << 3) | np.rint(v[normal] / 2.0 ** ev[normal] * 8 - 8).astype(np.int64)
    sub = nz & (ev < -6)
    code[sub] = np.rint(v[sub] * 512).astype(np.int64)
    code = np.minimum(code, 0x7e)
    return np.where(nz & (y < 0), code | 0x80, code).astype(np.uint8)


def e4m3_decode(codes):
    """E4M3 codes -> float64 values (0x7f / 0xff: NaN)."""
    c = np.asarray(codes).astype(np.int64)
    e, m = (c >> 3) & 15, c & 7
    mag = np.where(e > 0, (1 + m / 8.0) * 2.0 ** (e - 7.0), m * 2.0 ** -9)
    mag = np.where((c & 0x7f) == 0x7f, np.nan, mag)
    return np.where(c & 0x80, -mag, mag)


def quantize_act_model(X):
    """(a_codes (M, K), a_scales (M, K / 32))."""
    X = np.asarray(X).astype(np.float32)
    E = act_scales_model(X)
    y = X.astype(np.float64) * 2.0 ** (127.0 - np.repeat(E.astype(np.float64), BLOCK, axis=1))
    return e4m3_encode(y), E


def dequantize_act_model(codes, E, dtype=np.float64):
    """value(code) * 2^(b - 127); float64 (exact), or rounded once to float32."""
    v = e4m3_decode(codes) * 2.0 ** (np.repeat(np.asarray(E).astype(np.float64), BLOCK, axis=1) - 127.0)
    return v.astype(dtype)


def weights_model(w_codes, w_scales):
    """The de-quantized layer (N, K) as float64."""
    return mx_model.dequantize_model(w_codes, w_scales).astype(np.float64)


def matmul_model(a_codes, a_scales, w_codes, w_scales, bias=None):
    """(Y float64 (M, N), sum_k |a w| (M, N))."""
    A, W = dequantize_act_model(a_codes, a_scales), weights_model(w_codes, w_scales)
    Y = A @ W.T
    if bias is not None:
        Y = Y + np.asarray(bias, np.float64)[None, :]
    return Y, np.abs(A) @ np.abs(W).T
