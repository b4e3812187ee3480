"""CPU checks of the packed linear layer: the NumPy model of the MXFP8 activation format against its known answers and
against torch.float8_e4m3fn, the three new entry points in the header, the ctypes table and sleekit_amd.mx, and their
argument errors, which are raised on the host before any launch."""

import os
import re

import numpy as np
import torch

import mx_gemm_model as model
from conftest import ROOT


def block_of(values, amax):
    x = np.zeros((1, 32), np.float32)
    x[0, :len(values)] = values
    x[0, 31] = amax
    return x


def test_known_answers():
    codes, E = model.quantize_act_model(block_of([1.0, -0.3, 0.001, 0.0], 1.0))
    assert E[0, 0] == 119 and list(codes[0, :4]) == [0x78, 0xea, 0x28, 0x00] and codes[0, 31] == 0x78
    codes, E = model.quantize_act_model(block_of([1.75, -1.75, 0.01, 1e-5], 1.75))
    assert E[0, 0] == 119 and list(codes[0, :4]) == [0x7e, 0xfe, 0x42, 0x01]
    codes, E = model.quantize_act_model(np.zeros((2, 64), np.float32))
    assert (E == 74).all() and not codes.any()
    assert list(model.e4m3_encode([17.0, 19.0, 2.0 ** -10, 1.5 * 2.0 ** -9, -2.0 ** -10, 448.0, 1e9, -1e9, 464.0])) == \
        [0x58, 0x5a, 0x00, 0x02, 0x00, 0x7e, 0x7e, 0xfe, 0x7e]
    assert model.e4m3_decode([0x58, 0x5a, 0x7e, 0x01, 0x08, 0x88]).tolist() == [16.0, 20.0, 448.0, 2.0 ** -9, 2.0 ** -6, -2.0 ** -6]
    assert np.isnan(model.e4m3_decode([0x7f, 0xff])).all()
    # every code but the two NaNs and -0 survives decode -> encode
    every = np.array([c for c in range(256) if c & 0x7f != 0x7f and c != 0x80], np.uint8)
    assert np.array_equal(model.e4m3_encode(model.e4m3_decode(every)), every)
    # amax exactly 448 * 2^e: the scale is 2^e and the element is 0x7e; one float above takes the next scale
    for e in (-20, 0, 9):
        top = np.float32(448 * 2.0 ** e)
        codes, E = model.quantize_act_model(block_of([], top))
        assert E[0, 0] == 127 + e and codes[0, 31] == 0x7e
        codes, E = model.quantize_act_model(block_of([], np.nextafter(top, np.float32(np.inf))))
        assert E[0, 0] == 128 + e and codes[0, 31] == 0x76  # 224
    assert model.dequantize_act_model(np.full((1, 32), 0x78, np.uint8), np.full((1, 1), 119, np.uint8))[0, 0] == 1.0


def test_model_rounds_like_torch_float8_e4m3fn():
    rng = np.random.default_rng(5)
    x = np.concatenate([rng.uniform(-448, 448, 150000), rng.normal(0, 1, 30000), rng.normal(0, 2.0 ** -7, 20000),
                        model.e4m3_decode(np.arange(0x7f)), (model.e4m3_decode(np.arange(0x7e)) + model.e4m3_decode(np.arange(1, 0x7f))) / 2])
    x = x.astype(np.float32)
    t = torch.from_numpy(x).to(torch.float8_e4m3fn)
    want_codes = t.view(torch.uint8).numpy()
    got = model.e4m3_encode(x.astype(np.float64))
    want_codes = np.where(want_codes == 0x80, 0, want_codes)  # (torch keeps -0; the format here writes 0x00)
    assert np.array_equal(got, want_codes)
    assert np.array_equal(model.e4m3_decode(got), t.to(torch.float32).numpy().astype(np.float64))


def test_the_entries_are_named_in_every_layer():
    from sleekit_amd import _lib, mx
    import sleekit_amd

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sleekit_amd.h")).read(), flags=re.S)
    for name in ("slk_mx_quantize_act", "slk_mx_dequantize_act", "slk_mx_gemm"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.PROTOTYPES and hasattr(_lib.lib, name), name
    assert len(_lib.PROTOTYPES["slk_mx_quantize_act"][1]) == 8 and len(_lib.PROTOTYPES["slk_mx_dequantize_act"][1]) == 8
    assert len(_lib.PROTOTYPES["slk_mx_gemm"][1]) == 11
    for name in ("quantize_mxfp8", "dequantize_mxfp8", "matmul_mx", "linear_mxfp4", "MXLinear"):
        assert hasattr(mx, name), name
    assert sleekit_amd.MXLinear is mx.MXLinear and issubclass(mx.MXLinear, torch.nn.Module)
    assert _lib.lib.slk_abi_version() == 8


def test_argument_errors_do_not_touch_the_gpu():
    from sleekit_amd import _lib

    lib, p = _lib.lib, 4096  # (an aligned address that is never followed)
    for M, N, K in ((4, 4, 48), (4, 4, 0), (4, 4, 16), (0, 4, 64), (4, 0, 64), (-1, 4, 64)):
        assert lib.slk_mx_gemm(p, p, p, p, None, M, N, K, _lib.DTYPE_F32, p, None) == _lib.E_ARG, (M, N, K)
    assert lib.slk_mx_gemm(p, p, p, p, None, 4, 4, 48, _lib.DTYPE_F32, p, None) == _lib.E_ARG
    assert b"32" in lib.slk_last_error()
    assert lib.slk_mx_gemm(p, p, p, p, None, 4, 4, 64, 7, p, None) == _lib.E_ARG and b"dtype" in lib.slk_last_error()
    assert lib.slk_mx_gemm(p, None, p, p, None, 4, 4, 64, _lib.DTYPE_F32, p, None) == _lib.E_ARG
    assert lib.slk_mx_gemm(p, p, p, p, None, 4, 4, 64, _lib.DTYPE_F32, None, None) == _lib.E_ARG
    assert lib.slk_mx_gemm(p + 8, p, p, p, None, 4, 4, 64, _lib.DTYPE_F32, p, None) == _lib.E_ARG and b"aligned" in lib.slk_last_error()
    assert lib.slk_mx_gemm(p, p, p + 4, p, None, 4, 4, 64, _lib.DTYPE_F32, p, None) == _lib.E_ARG
    for M, K in ((4, 48), (0, 64), (4, 0)):
        assert lib.slk_mx_quantize_act(p, _lib.DTYPE_F32, M, K, p, p, p, None) == _lib.E_ARG, (M, K)
        assert lib.slk_mx_dequantize_act(p, p, M, K, _lib.DTYPE_F32, p, None, None) == _lib.E_ARG, (M, K)
    assert lib.slk_mx_quantize_act(p, 3, 4, 64, p, p, p, None) == _lib.E_ARG
    assert lib.slk_mx_quantize_act(p, _lib.DTYPE_BF16, 4, 64, p, p, None, None) == _lib.E_ARG  # the flag is required
    assert lib.slk_mx_quantize_act(p + 2, _lib.DTYPE_BF16, 4, 64, p, p, p, None) == _lib.E_ARG
    assert lib.slk_mx_dequantize_act(p, p, 4, 64, 9, p, None, None) == _lib.E_ARG
    assert lib.slk_mx_dequantize_act(p, p, 4, 64, _lib.DTYPE_F16, p + 2, None, None) == _lib.E_ARG


def test_every_requirement_of_the_dense_products_has_its_text():
    """Each requirement of slk_mx_gemm, _a4, _a6 and _w6, tripped alone, with a word of its text in slk_last_error()."""
    from sleekit_amd import _lib

    lib, p, F32 = _lib.lib, 4096, _lib.DTYPE_F32
    entries = [(getattr(lib, name), ()) for name in ("slk_mx_gemm", "slk_mx_gemm_a4", "slk_mx_gemm_a6")]
    entries += [(lib.slk_mx_gemm_w6, (a_fmt,)) for a_fmt in (_lib.MX_ACT_FP8, _lib.MX_ACT_FP6)]
    for entry, a_fmt in entries:
        def call(a=p, asc=p, w=p, ws=p, M=4, N=4, K=64, out_dtype=F32, out=p):
            return entry(a, asc, w, ws, None, M, N, K, *a_fmt, out_dtype, out, None)

        for kw, word in ((dict(M=0), b"at least 1"), (dict(N=0), b"at least 1"), (dict(M=-1), b"at least 1"),
                         (dict(K=0), b"multiple of 32"), (dict(K=16), b"multiple of 32"), (dict(K=48), b"multiple of 32"),
                         (dict(out_dtype=7), b"out_dtype"),
                         (dict(a=None), b"null pointer"), (dict(asc=None), b"null pointer"), (dict(w=None), b"null pointer"),
                         (dict(ws=None), b"null pointer"), (dict(out=None), b"null pointer"),
                         (dict(a=p + 8), b"aligned to 16"), (dict(w=p + 4), b"aligned to 16"), (dict(out=p + 2), b"aligned to 16"),
                         (dict(M=65535 * 64 + 1), b"row tiles")):
            assert call(**kw) == _lib.E_ARG, kw
            assert word in lib.slk_last_error(), (kw, lib.slk_last_error())
    for a_fmt in (_lib.MX_ACT_FP4, 3, -1):   # slk_mx_gemm_w6 has one text for every a_fmt it does not take
        assert lib.slk_mx_gemm_w6(p, p, p, p, None, 4, 4, 64, a_fmt, F32, p, None) == _lib.E_ARG
        assert b"MXFP6 layer takes" in lib.slk_last_error() and b"a_fmt = %d" % a_fmt in lib.slk_last_error()


def test_python_refusals_come_before_the_device():
    """Shape and dtype errors are ValueError and need no GPU."""
    import pytest

    from sleekit_amd import mx

    codes, scales = np.zeros((8, 32), np.uint8), np.full((8, 2), 127, np.uint8)
    with pytest.raises(ValueError, match="32"):
        mx.quantize_mxfp8(np.zeros((4, 48), np.float32))
    with pytest.raises(ValueError):
        mx.quantize_mxfp8(np.zeros((4, 64), np.float64))
    with pytest.raises(ValueError, match="columns"):
        mx.linear_mxfp4(np.zeros((4, 96), np.float32), codes, scales)
    with pytest.raises(ValueError, match="scale bytes"):
        mx.linear_mxfp4(np.zeros((4, 64), np.float32), codes, scales[:, :1])
    with pytest.raises(ValueError, match="bfloat16"):
        mx.linear_mxfp4(np.zeros((4, 64), np.float32), codes, scales, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="bias"):
        mx.linear_mxfp4(np.zeros((4, 64), np.float32), codes, scales, bias=np.zeros(7, np.float32))
    with pytest.raises(ValueError):
        mx.MXLinear.from_result(torch.nn.Conv1d(64, 8, 1), None)
    with pytest.raises(ValueError, match="32"):
        mx.MXLinear(48, 8)
