"""CPU checks of MXFP6 (E2M3) activations: the NumPy model of the format against its grid, its known answers and its own
round trip; a NumPy emulation of the kernels' integer encoder (sleekit_amd/csrc/mxquant.h: mxa_scale_byte<MXA_E2M3>,
e2m3_code, mxa_code<MXA_E2M3>, the bit-stream pack) against that model; the four new entry points in the header, the ctypes
table and the Python surface, their argument errors (raised on the host before any launch); and the output-error table of
DESIGN.md section 20 (W4A8, W4A6 and W4A4, with and without a rotation, and with exact weights)."""

import os
import re

import numpy as np
import pytest
import torch

import mx_act4_model
import mx_act6_model as model
import mx_gemm_model
import rotation_model
from conftest import ROOT

GRID, MID = model.GRID, model.MIDPOINTS
# what the 31 midpoints round to: the even one of codes i and i + 1
MID_CODES = [i if i % 2 == 0 else i + 1 for i in range(31)]
ENTRIES = (("slk_mx_quantize_act6", 8), ("slk_mx_dequantize_act6", 8), ("slk_mx_gemm_a6", 11), ("slk_mx_rotate_quantize_act6", 10))


def block_of(values, amax):
    x = np.zeros((1, 32), np.float32)
    x[0, :len(values)] = values
    x[0, 31] = amax
    return x


def codes_of(a_codes):
    return model.unpack_codes(a_codes)


# ---------------------------------------------------------------------------------------------------------------- grid
def test_the_grid_is_the_one_of_the_format():
    assert GRID.tolist() == ([k * 0.125 for k in range(16)] + [2 + k * 0.25 for k in range(8)] + [4 + k * 0.5 for k in range(8)])
    assert len(GRID) == 32 and GRID[-1] == 7.5 and (np.diff(GRID) > 0).all()
    assert model.e2m3_decode(np.arange(64)).tolist() == GRID.tolist() + (-GRID).tolist()


def test_every_grid_point_and_midpoint():
    assert model.e2m3_encode(GRID).tolist() == list(range(32))
    assert model.e2m3_encode(-GRID).tolist() == [0] + list(range(33, 64))  # -0 is 0x00, never 0x20
    assert model.e2m3_encode(MID).tolist() == MID_CODES and all(c % 2 == 0 for c in MID_CODES)
    assert model.e2m3_encode(-MID).tolist() == [c | 0x20 if c else 0 for c in MID_CODES]
    # one float64 step off a midpoint goes to the nearer side
    assert model.e2m3_encode(np.nextafter(MID, 10.0)).tolist() == list(range(1, 32))
    assert model.e2m3_encode(np.nextafter(MID, -10.0)).tolist() == list(range(31))
    assert model.e2m3_encode(-np.nextafter(MID, 10.0)).tolist() == [c | 0x20 for c in range(1, 32)]
    assert model.e2m3_encode([7.5, 7.75, 8.0, 1e9, -7.6, -1e30]).tolist() == [31, 31, 31, 31, 63, 63]  # clamped at 7.5
    values = np.concatenate([GRID[:31], -GRID[:31]])
    for e in (-30, -3, 0, 5, 40):  # the same through the scale: amax 7.5 * 2^e holds the scale at 2^e
        s = 2.0 ** e
        for part, want in ((values[:31], list(range(31))), (values[31:], [0] + list(range(33, 63))), (MID, MID_CODES),
                           (-MID, [c | 0x20 if c else 0 for c in MID_CODES])):
            a_codes, E = model.quantize_act6_model(block_of(part * s, 7.5 * s))
            assert E[0, 0] == 127 + e and a_codes.shape == (1, 24)
            c = codes_of(a_codes)[0]
            assert c[:31].tolist() == want and c[31] == 0x1f and not (c == 0x20).any(), (e, c.tolist())


def test_known_answers():
    for values, amax, byte, codes, packed in (
            ([7.5, -0.3, 0.0625, 0.1875], 7.5, 127, [0x1f, 0x22, 0x00, 0x02], [0x9f, 0x08, 0x08]),
            ([1.0, -1.0, 0.3, 0.0625], 1.0, 125, [0x18, 0x38, 0x0a, 0x02], [0x18, 0xae, 0x08]),
            ([1.0625, 3.9, -3.875, 5.25], 7.5, 127, [0x08, 0x18, 0x38, 0x1a], [0x08, 0x86, 0x6b])):
        a_codes, E = model.quantize_act6_model(block_of(values, amax))
        assert E[0, 0] == byte and codes_of(a_codes)[0, :4].tolist() == codes and a_codes[0, :3].tolist() == packed, values
    a_codes, E = model.quantize_act6_model(block_of([1.75, -1.75], 1.75))
    assert E[0, 0] == 125 and codes_of(a_codes)[0, :2].tolist() == [0x1e, 0x3e] and codes_of(a_codes)[0, 31] == 0x1e
    a_codes, E = model.quantize_act6_model(np.zeros((2, 64), np.float32))
    assert (E == 74).all() and not a_codes.any() and a_codes.shape == (2, 48)
    # amax exactly 7.5 * 2^e: the scale is 2^e and the element is code 1f; one float above takes the next scale (3.75 -> 0x17)
    for e in (-20, 0, 9):
        top = np.float32(7.5 * 2.0 ** e)
        a_codes, E = model.quantize_act6_model(block_of([], top))
        assert E[0, 0] == 127 + e and codes_of(a_codes)[0, 31] == 0x1f
        a_codes, E = model.quantize_act6_model(block_of([], -np.nextafter(top, np.float32(np.inf))))
        assert E[0, 0] == 128 + e and codes_of(a_codes)[0, 31] == 0x20 | 0x17
    # tiny values keep the floor: byte 74 is 2^-53, and 1e-20 / 2^-53 is 9e-5, code 0
    a_codes, E = model.quantize_act6_model(block_of([1e-20, -1e-20], 1e-20))
    assert E[0, 0] == 74 and not a_codes.any()


def test_the_bit_stream():
    rng = np.random.default_rng(5)
    c = rng.integers(0, 64, (5, 96)).astype(np.uint8)
    b = model.pack_codes(c)
    assert b.shape == (5, 72) and b.dtype == np.uint8 and np.array_equal(model.unpack_codes(b), c)
    # element k at bits 6 k .. 6 k + 5 of the row read as one little-endian integer
    for r in range(5):
        stream = int.from_bytes(b[r].tobytes(), "little")
        assert [(stream >> (6 * k)) & 63 for k in range(96)] == c[r].tolist()


def test_no_minus_zero_and_the_round_trip():
    rng = np.random.default_rng(8)
    mag = 2.0 ** rng.integers(-12, 13, (40, 8))
    X = (rng.standard_normal((40, 256)) * np.repeat(mag, 32, axis=1)).astype(np.float32)
    X[rng.random(X.shape) < 0.2] = 0
    X[3] = -np.abs(X[3])
    X[4, :64] = -0.0
    a_codes, E = model.quantize_act6_model(X)
    assert a_codes.shape == (40, 192) and E.shape == (40, 8) and a_codes.dtype == np.uint8 and E.dtype == np.uint8
    assert not (codes_of(a_codes) == 0x20).any()
    s = 2.0 ** (np.repeat(E.astype(np.float64), 32, axis=1) - 127)
    y = X.astype(np.float64) / s
    assert np.abs(y).max() <= 7.5  # the scale does not saturate: nothing was clamped here
    back = model.dequantize_act6_model(a_codes, E) / s
    # within half a local step of x / s: the step is 0.125 below 2, 0.25 below 4 and 0.5 above
    half = np.where(np.abs(y) < 2, 0.0625, np.where(np.abs(y) < 4, 0.125, 0.25))
    assert (np.abs(back - y) <= half).all()
    assert (np.sign(back) * np.sign(y) >= 0).all()
    # what the model writes, it reads back: quantizing the de-quantized values changes nothing but a scale that may shrink
    deq = model.dequantize_act6_model(a_codes, E, np.float32)
    assert np.array_equal(deq.astype(np.float64), model.dequantize_act6_model(a_codes, E))  # 4 bits: exact in float32
    again, E2 = model.quantize_act6_model(deq)
    assert (E2 <= E).all() and np.array_equal(model.dequantize_act6_model(again, E2), model.dequantize_act6_model(a_codes, E))


# ---------------------------------------------------------------------------------------------------------------- encoder
def f32_bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def emulate_encoder(X):
    """The kernels' word arithmetic (mxquant.h) in NumPy, operation for operation: the integer maximum of the magnitude
    bits, the float32 divide by 7.5 and the floor 1e-16, the exponent field rounded up, the exact product with the inverse
    scale, then e2m3_code on the magnitude's bits and the sign from bit 31."""
    X = np.ascontiguousarray(X, np.float32)
    M, K = X.shape
    top = (f32_bits(X) & np.uint32(0x7fffffff)).reshape(M, K // 32, 32).max(axis=2)
    top = np.minimum(top, np.uint32(0x7f7fffff))
    b0 = np.maximum(top.view(np.float32) / np.float32(7.5), np.float32(1.0e-16)).astype(np.float32)
    eb = ((f32_bits(b0).astype(np.uint64) + 0x7fffff) >> 23) & 0xff
    inv = ((254 - eb) << 23).astype(np.uint32).view(np.float32)
    with np.errstate(over="ignore", under="ignore"):
        u = f32_bits(X * np.repeat(inv, 32, axis=1)).astype(np.uint64)
    a = u & 0x7fffffff
    normal = np.minimum(((a + 0x7ffff + ((a >> 20) & 1)) >> 20) - (126 << 3), 0x1f)
    sub = np.rint(a.astype(np.uint32).view(np.float32) * np.float32(8.0)).astype(np.uint64)
    c = np.where(a >= 0x3f800000, normal, sub)
    c = np.where(c != 0, c | ((u >> 26) & 0x20), 0).astype(np.uint32)
    # the pack: a lane's sixteen codes into three words, code e at bits 6 e, a straddling code split over two words
    words = np.zeros((M, K // 16, 3), np.uint32)
    lanes = c.reshape(M, K // 16, 16)
    for e in range(16):
        word, shift = (6 * e) >> 5, (6 * e) & 31
        words[:, :, word] |= lanes[:, :, e] << np.uint32(shift)
        if shift + 6 > 32:
            words[:, :, word + 1] |= lanes[:, :, e] >> np.uint32(32 - shift)
    return words.reshape(M, 3 * K // 16).astype("<u4").view(np.uint8).reshape(M, 3 * K // 4), eb.astype(np.uint8)


def test_the_integer_encoder_equals_the_model():
    rng = np.random.default_rng(12)
    # random blocks over 2^-40 .. 2^40
    mag = 2.0 ** rng.integers(-40, 41, (256, 16))
    X = (rng.standard_normal((256, 512)) * np.repeat(mag, 32, axis=1)).astype(np.float32)
    X[rng.random(X.shape) < 0.1] = 0
    # every grid point and midpoint (and one float32 either side) under both signs, times 2^e, amax 7.5 * 2^e in the block
    points = np.concatenate([GRID, MID])
    rows = []
    for e in (-40, -30, -3, 0, 1, 5, 40):
        s = np.float32(2.0 ** e)
        for sign in (1.0, -1.0):
            for v in (points, np.nextafter(points.astype(np.float32), np.float32(10)), np.nextafter(points.astype(np.float32), np.float32(-10))):
                v = (np.abs(v.astype(np.float32)) * s * np.float32(sign)).astype(np.float32)
                row = np.zeros(96, np.float32)
                row[:31], row[32:63], row[64:65] = v[:31], v[31:62], v[62:]
                row[31] = row[63] = row[95] = np.float32(7.5) * s
                rows.append(row)
    G = np.array(rows, np.float32)
    Z = np.zeros((3, 64), np.float32)
    T = np.full((2, 64), 1e-20, np.float32)
    T[1, ::3] *= -1
    for data in (X, G, Z, T):
        got_codes, got_E = emulate_encoder(data)
        want_codes, want_E = model.quantize_act6_model(data)
        assert np.array_equal(got_E, want_E)
        wrong = np.argwhere(codes_of(got_codes) != codes_of(want_codes))
        assert wrong.size == 0, (len(wrong), wrong[:4].tolist())
        assert np.array_equal(got_codes, want_codes)
    assert (emulate_encoder(Z)[1] == 74).all() and (emulate_encoder(T)[1] == 74).all() and not emulate_encoder(T)[0].any()


# ---------------------------------------------------------------------------------------------------------------- surface
def test_the_entries_are_named_in_every_layer():
    import sleekit_amd
    from sleekit_amd import _lib, mx, rotation

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sleekit_amd.h")).read(), flags=re.S)
    for name, args in ENTRIES:
        found = re.search(r"\b%s\s*\(([^)]*)\)" % name, header)
        assert found and len(found.group(1).split(",")) == args, name
        assert name in _lib.PROTOTYPES and hasattr(_lib.lib, name), name
        assert len(_lib.PROTOTYPES[name][1]) == args
    assert re.search(r"#define\s+SLK_MX_ACT_FP8\s+0\b", header) and re.search(r"#define\s+SLK_MX_ACT_FP4\s+1\b", header)
    assert hasattr(mx, "quantize_mxfp6_act") and hasattr(mx, "dequantize_mxfp6_act")
    assert sleekit_amd.MXLinear is mx.MXLinear and hasattr(rotation, "RotatedLinear")
    assert _lib.lib.slk_abi_version() == 8


def test_argument_errors_do_not_touch_the_gpu():
    from sleekit_amd import _lib

    lib, p = _lib.lib, 4096  # (an aligned address that is never followed)
    F32, BF16 = _lib.DTYPE_F32, _lib.DTYPE_BF16
    # slk_mx_quantize_act6(X, x_dtype, M, K, a_codes, a_scales, flag, stream)
    for M, K in ((4, 48), (0, 64), (4, 0), (4, 16), (-1, 64)):
        assert lib.slk_mx_quantize_act6(p, F32, M, K, p, p, p, None) == _lib.E_ARG, (M, K)
    assert lib.slk_mx_quantize_act6(p, F32, 4, 48, p, p, p, None) == _lib.E_ARG and b"32" in lib.slk_last_error()
    for dtype in (3, 9, -1):
        assert lib.slk_mx_quantize_act6(p, dtype, 4, 64, p, p, p, None) == _lib.E_ARG and b"dtype" in lib.slk_last_error()
    for args in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):  # the flag is required
        assert lib.slk_mx_quantize_act6(args[0], BF16, 4, 64, args[1], args[2], args[3], None) == _lib.E_ARG
        assert b"null" in lib.slk_last_error()
    assert lib.slk_mx_quantize_act6(p + 2, BF16, 4, 64, p, p, p, None) == _lib.E_ARG and b"aligned" in lib.slk_last_error()
    assert lib.slk_mx_quantize_act6(p, BF16, 4, 64, p + 8, p, p, None) == _lib.E_ARG and b"aligned" in lib.slk_last_error()
    # slk_mx_dequantize_act6(a_codes, a_scales, M, K, out_dtype, out, flag, stream): the flag may be NULL
    for M, K in ((4, 48), (0, 64), (4, 0), (4, 16), (-1, 64)):
        assert lib.slk_mx_dequantize_act6(p, p, M, K, F32, p, None, None) == _lib.E_ARG, (M, K)
    assert lib.slk_mx_dequantize_act6(p, p, 4, 48, F32, p, None, None) == _lib.E_ARG and b"32" in lib.slk_last_error()
    assert lib.slk_mx_dequantize_act6(p, p, 4, 64, 3, p, None, None) == _lib.E_ARG and b"dtype" in lib.slk_last_error()
    for args in ((None, p, p), (p, None, p), (p, p, None)):
        assert lib.slk_mx_dequantize_act6(args[0], args[1], 4, 64, BF16, args[2], None, None) == _lib.E_ARG
        assert b"null" in lib.slk_last_error()
    assert lib.slk_mx_dequantize_act6(p + 8, p, 4, 64, F32, p, None, None) == _lib.E_ARG and b"aligned" in lib.slk_last_error()
    assert lib.slk_mx_dequantize_act6(p, p, 4, 64, F32, p + 4, None, None) == _lib.E_ARG and b"aligned" in lib.slk_last_error()
    # slk_mx_gemm_a6
    for M, N, K in ((4, 4, 48), (4, 4, 0), (4, 4, 16), (0, 4, 64), (4, 0, 64), (-1, 4, 64)):
        assert lib.slk_mx_gemm_a6(p, p, p, p, None, M, N, K, F32, p, None) == _lib.E_ARG, (M, N, K)
    assert lib.slk_mx_gemm_a6(p, p, p, p, None, 4, 4, 48, F32, p, None) == _lib.E_ARG and b"32" in lib.slk_last_error()
    assert lib.slk_mx_gemm_a6(p, p, p, p, None, 4, 4, 64, 7, p, None) == _lib.E_ARG and b"dtype" in lib.slk_last_error()
    for args in ((None, p, p, p, p), (p, None, p, p, p), (p, p, None, p, p), (p, p, p, None, p), (p, p, p, p, None)):
        assert lib.slk_mx_gemm_a6(args[0], args[1], args[2], args[3], None, 4, 4, 64, F32, args[4], None) == _lib.E_ARG
        assert b"null" in lib.slk_last_error()
    assert lib.slk_mx_gemm_a6(p + 8, p, p, p, None, 4, 4, 64, F32, p, None) == _lib.E_ARG and b"aligned" in lib.slk_last_error()
    assert lib.slk_mx_gemm_a6(p, p, p + 4, p, None, 4, 4, 64, F32, p, None) == _lib.E_ARG and b"aligned" in lib.slk_last_error()
    assert lib.slk_mx_gemm_a6(p, p, p, p, None, 4, 4, 64, F32, p + 2, None) == _lib.E_ARG and b"aligned" in lib.slk_last_error()
    # slk_mx_rotate_quantize_act6(X, x_dtype, rows, n, block, signs, a_codes, a_scales, flag, stream)
    fused = lib.slk_mx_rotate_quantize_act6
    for n, block in ((48, 16), (16, 16), (0, 2)):  # n % 32
        assert fused(p, F32, 4, n, block, p, p, p, p, None) == _lib.E_ARG and b"32" in lib.slk_last_error(), (n, block)
    for block in (0, 1, 3, 24, 48, 8192, -4):  # not a power of two in 2 .. 4096
        assert fused(p, F32, 4, 96, block, p, p, p, p, None) == _lib.E_ARG and b"power of two" in lib.slk_last_error(), block
    assert fused(p, F32, 4, 96, 64, p, p, p, p, None) == _lib.E_ARG and b"divide" in lib.slk_last_error()
    assert fused(p, F32, 0, 64, 64, p, p, p, p, None) == _lib.E_ARG
    for dtype in (_lib.DTYPE_F64, 9, -1):
        assert fused(p, dtype, 4, 64, 64, p, p, p, p, None) == _lib.E_ARG and b"x_dtype" in lib.slk_last_error()
    for args in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        assert fused(args[0], BF16, 4, 64, 64, None, args[1], args[2], args[3], None) == _lib.E_ARG
        assert b"null" in lib.slk_last_error()
    for args in ((p + 2, p, p), (p, p + 4, p), (p, p, p + 8)):
        assert fused(args[0], BF16, 4, 64, 64, args[1], args[2], p, p, None) == _lib.E_ARG and b"aligned" in lib.slk_last_error()
    # the older entry still knows two formats only
    assert lib.slk_mx_rotate_quantize_act(p, F32, 4, 64, 64, p, 2, p, p, p, None) == _lib.E_ARG and b"fmt" in lib.slk_last_error()


def test_python_refusals_come_before_the_device():
    """Shape, dtype and option errors are ValueError and need no GPU."""
    from sleekit_amd import mx, rotation

    codes, scales = np.zeros((8, 32), np.uint8), np.full((8, 2), 127, np.uint8)  # a layer of K = 64
    x = np.zeros((4, 64), np.float32)
    A6 = "mxfp6_e2m3"
    with pytest.raises(ValueError, match="32"):
        mx.quantize_mxfp6_act(np.zeros((4, 48), np.float32))
    with pytest.raises(ValueError):
        mx.quantize_mxfp6_act(np.zeros((4, 64), np.float64))
    with pytest.raises(ValueError):
        mx.quantize_mxfp6_act(np.zeros(64, np.float32))
    for bad in ("mxfp6", "mxfp6_e3m2", "MXFP6_E2M3", "fp6", None, 6, ("mxfp6_e2m3",)):
        with pytest.raises(ValueError, match="activations"):
            mx.linear_mxfp4(x, codes, scales, activations=bad)
        with pytest.raises(ValueError, match="activations"):
            mx.matmul_mx(np.zeros((4, 48), np.uint8), np.zeros((4, 2), np.uint8), codes, scales, activations=bad)
        with pytest.raises(ValueError, match="activations"):
            mx.MXLinear(64, 8, activations=bad)
    with pytest.raises(ValueError, match="columns"):  # (4, 96) bytes are 128 columns of MXFP6
        mx.matmul_mx(np.zeros((4, 96), np.uint8), np.zeros((4, 4), np.uint8), codes, scales, activations=A6)
    for width in (32, 64, 47):  # the layer's MXFP4 and MXFP8 widths, and no whole number of codes
        with pytest.raises(ValueError, match="columns"):
            mx.matmul_mx(np.zeros((4, width), np.uint8), np.zeros((4, 2), np.uint8), codes, scales, activations=A6)
    with pytest.raises(ValueError, match="scale bytes"):
        mx.matmul_mx(np.zeros((4, 48), np.uint8), np.zeros((4, 1), np.uint8), codes, scales, activations=A6)
    with pytest.raises(ValueError):
        mx.matmul_mx(np.zeros((4, 48), np.float32), np.zeros((4, 2), np.uint8), codes, scales, activations=A6)
    with pytest.raises(ValueError, match="bias"):
        mx.matmul_mx(np.zeros((4, 48), np.uint8), np.zeros((4, 2), np.uint8), codes, scales, np.zeros(7, np.float32), activations=A6)
    with pytest.raises(ValueError, match="columns"):
        mx.linear_mxfp4(np.zeros((4, 96), np.float32), codes, scales, activations=A6)
    with pytest.raises(ValueError):
        mx.linear_mxfp4(x.astype(np.float64), codes, scales, activations=A6)
    with pytest.raises(ValueError, match="bfloat16"):
        mx.linear_mxfp4(x, codes, scales, dtype=torch.bfloat16, activations=A6)
    with pytest.raises(ValueError, match="columns"):
        mx.dequantize_mxfp6_act(np.zeros((4, 32), np.uint8), np.zeros((4, 1), np.uint8))
    with pytest.raises(ValueError, match="scale bytes"):
        mx.dequantize_mxfp6_act(np.zeros((4, 48), np.uint8), np.zeros((4, 1), np.uint8))
    with pytest.raises(ValueError, match="bfloat16"):
        mx.dequantize_mxfp6_act(np.zeros((4, 48), np.uint8), np.zeros((4, 2), np.uint8), dtype=torch.bfloat16)
    rot = rotation.Rotation._of(torch.ones(128), 32)  # (signs on the host: nothing here reaches a kernel)
    with pytest.raises(ValueError, match="features"):
        mx.linear_mxfp4(x, codes, scales, activations=A6, rotation=rot)
    inner = mx.MXLinear(128, 8, activations=A6)
    assert inner.activations == A6 and A6 in inner.extra_repr()
    assert rotation.RotatedLinear(inner, rot, fused=True).fused and not rotation.RotatedLinear(inner, rot).fused


def test_state_dicts_keep_their_keys():
    """`activations` is extra state that a default module does not write, and the new value travels through it."""
    from sleekit_amd import mx, rotation

    A6 = "mxfp6_e2m3"
    plain, a6 = mx.MXLinear(64, 8), mx.MXLinear(64, 8, activations=A6)
    assert sorted(plain.state_dict()) == ["bias", "codes", "scales"]
    assert sorted(a6.state_dict()) == ["_extra_state", "bias", "codes", "scales"]
    assert a6.state_dict()["_extra_state"] == {"activations": A6}
    other = mx.MXLinear(64, 8)
    other.load_state_dict(a6.state_dict())
    assert other.activations == A6
    other.load_state_dict(plain.state_dict())  # no key: "mxfp8"
    assert other.activations == "mxfp8"
    other.load_state_dict(mx.MXLinear(64, 8, activations="mxfp4").state_dict())
    assert other.activations == "mxfp4"
    for bad in ("mxfp6", "mxfp6_e3m2", ["mxfp6_e2m3"]):
        with pytest.raises(RuntimeError, match="activations"):
            other.load_state_dict(dict(plain.state_dict(), _extra_state={"activations": bad}))
    rot = rotation.Rotation._of(torch.ones(64), 32)
    fused = rotation.RotatedLinear(mx.MXLinear(64, 8, activations=A6), rot, fused=True)
    copy = rotation.RotatedLinear(mx.MXLinear(64, 8), rotation.Rotation._of(torch.ones(64), 64))
    copy.load_state_dict(fused.state_dict())
    assert copy.fused and copy.block == 32 and copy.inner.activations == A6
    default = rotation.RotatedLinear(mx.MXLinear(64, 8), rot)
    assert default.state_dict()["_extra_state"] == {"block": 32} and sorted(default.inner.state_dict()) == ["bias", "codes", "scales"]
    copy.load_state_dict(default.state_dict())
    assert not copy.fused and copy.inner.activations == "mxfp8"


# ---------------------------------------------------------------------------------------------------------------- error table
SEEDS = (4242, 7, 19, 101, 2024, 31337)


def output_errors(seed):
    """Relative output error |y - y_ref| / |y_ref| (Frobenius) of the MODELS on the synthetic 64 x 256 layer and 128 tokens of
    its activations (outlier channels: sleekit_amd.synth), against the float64 product of the unquantized x and W -- the
    recipe of tests/test_mx_act4_cpu.py's output_errors with a W4A6 column and, with the weights left exact, the
    activations' own share.  Rows (plain, rotated by a block of 256), columns (A8, A6, A4) x (MXFP4 weights, exact weights):
    an array (2, 2, 3) indexed [rotated][exact weights][format]."""
    from sleekit_amd import synth

    W = synth.make_weights(64, 256, seed)
    x = synth.make_activations(128, 256, seed).astype(np.float32)
    want = x.astype(np.float64) @ W.astype(np.float64).T
    signs = rotation_model.signs_for(256, seed)
    out = np.zeros((2, 2, 3))
    for rotated in (False, True):
        xr = rotation_model.transform(x, 256, signs) if rotated else x
        Wr = rotation_model.transform(W, 256, signs) if rotated else W
        Wq = mx_act4_model.dequantize_act4_model(*mx_act4_model.quantize_act4_model(Wr))
        a8 = mx_gemm_model.dequantize_act_model(*mx_gemm_model.quantize_act_model(xr))
        a6 = model.dequantize_act6_model(*model.quantize_act6_model(xr))
        a4 = mx_act4_model.dequantize_act4_model(*mx_act4_model.quantize_act4_model(xr))
        for exact, weights in enumerate((Wq, np.asarray(Wr, np.float64))):
            out[int(rotated), exact] = [np.linalg.norm(a @ weights.T - want) / np.linalg.norm(want) for a in (a8, a6, a4)]
    return out


def test_output_error_table():
    t = np.array([output_errors(seed) for seed in SEEDS])  # (seed, rotated, exact weights, format)
    names = {(0, 0): "plain", (1, 0): "rotated, block 256", (0, 1): "activations only (exact W), plain", (1, 1): "activations only, rotated"}
    for (r, e), name in names.items():
        print(f"{name:36s} " + "  ".join(f"{fmt} {t[:, r, e, i].mean():.4f} [{t[:, r, e, i].min():.4f} .. {t[:, r, e, i].max():.4f}]"
                                        for i, fmt in enumerate(("A8", "A6", "A4"))))
    assert np.isfinite(t).all() and (t > 0).all()
    for r in (0, 1):  # plain and rotated, on every seed
        a8, a6, a4 = t[:, r, 0].T
        assert (1.1 * a6 < a4).all() and (a6 < 1.1 * a8).all(), (r, a8, a6, a4)
        a8, a6, a4 = t[:, r, 1].T  # activations only
        assert (3 * a6 < a4).all(), (r, a6, a4)
    a8, a6, _ = t[:, 0, 1].T
    assert (1.1 * a8 < a6).all(), (a8, a6)
    a8, a6, _ = t[:, 1, 1].T
    assert (a8 < a6).all() and (a6 < 1.15 * a8).all(), (a8, a6)
