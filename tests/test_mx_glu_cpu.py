"""CPU checks of the gated MX MLP: the header and the prototypes of the three entries, their argument errors before any
launch, the Python refusals before the device, the NumPy model of the gate (tests/mx_glu_model.py) against the formulas it
stands for, and the state dicts of MXGatedMLP and MXExpertsMLP.  Nothing here needs a GPU."""

import ctypes
import os
import re

import numpy as np
import pytest
import torch

import mx_glu_model as model
from conftest import ROOT

ENTRIES = ("slk_mx_glu", "slk_mx_gemm_glu", "slk_mx_gemm_glu_experts")
INF = float("inf")


def test_header_declares_the_entries_with_prototypes():
    from sleekit_amd import _lib

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sleekit_amd.h")).read(), flags=re.S)
    for name in ENTRIES:
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
        assert decl, f"{name} is not declared"
        args = [a.strip() for a in decl.group(1).split(",")]
        res, argtypes = _lib.PROTOTYPES[name]
        assert res is ctypes.c_int and len(argtypes) == len(args), name
        for a, t in zip(args, argtypes):  # float arguments are c_float, ints c_int, pointers and the stream addresses
            scalar = {"float": ctypes.c_float, "int": ctypes.c_int, "size_t": ctypes.c_size_t}.get(a.split()[0]) if "*" not in a else None
            want = scalar or ctypes.c_void_p
            assert t is want, (name, a)
        assert sum(a.startswith("float ") for a in args) == 3 and "int interleaved" in args
        assert hasattr(_lib.lib, name)
    assert _lib.lib.slk_abi_version() == 8


def test_argument_errors_do_not_touch_the_gpu():
    """Bad arguments are rejected on the host before any launch (safe without a GPU); 16 and 64 stand for aligned pointers."""
    from sleekit_amd import _lib

    L, p, q = _lib.lib, 64, 72  # q: off 16-byte alignment
    F32, FP8, FP4, FP6, W4, W6 = _lib.DTYPE_F32, _lib.MX_ACT_FP8, _lib.MX_ACT_FP4, _lib.MX_ACT_FP6, _lib.MX_W_FP4, _lib.MX_W_FP6

    def glu(Y=p, x_dtype=F32, M=4, N=32, alpha=1.0, limit=INF, shift=0.0, interleaved=0, out_dtype=F32, H=p):
        return L.slk_mx_glu(Y, x_dtype, M, N, alpha, limit, shift, interleaved, out_dtype, H, None)

    def gemm(a=p, asc=p, w=p, ws=p, bias=None, M=4, N=32, K=32, a_fmt=FP8, w_fmt=W4, alpha=1.0, limit=INF, shift=0.0, interleaved=0, h=p, hs=p, flag=p):
        return L.slk_mx_gemm_glu(a, asc, w, ws, bias, M, N, K, a_fmt, w_fmt, alpha, limit, shift, interleaved, h, hs, flag, None)

    def experts(a=p, asc=p, w=p, ws=p, bias=None, offsets=p, E=2, M=4, N=32, K=32, a_fmt=FP8, w_fmt=W4, alpha=1.0, limit=INF, shift=0.0, interleaved=0,
                h=p, hs=p, flag=p, work=p, ws_bytes=1 << 20):
        return L.slk_mx_gemm_glu_experts(a, asc, w, ws, bias, offsets, E, M, N, K, a_fmt, w_fmt, alpha, limit, shift, interleaved, h, hs, flag, work,
                                         ws_bytes, None)

    def refused(rc, word):
        assert rc == _lib.E_ARG
        assert word.encode() in L.slk_last_error(), (word, L.slk_last_error())

    # the gate parameters, the same for all three
    for call in (glu, gemm, experts):
        refused(call(limit=0.0), "limit")
        refused(call(limit=-1.0), "limit")
        refused(call(limit=float("nan")), "limit")
        refused(call(alpha=INF), "alpha")
        refused(call(alpha=float("nan")), "alpha")
        refused(call(shift=-INF), "shift")
        refused(call(interleaved=2), "interleaved")
        refused(call(M=0), "M")
    # slk_mx_glu
    refused(glu(Y=None), "null")
    refused(glu(H=None), "null")
    refused(glu(Y=q), "aligned")
    refused(glu(H=q), "aligned")
    refused(glu(N=0), "N")
    refused(glu(x_dtype=7), "x_dtype")
    refused(glu(out_dtype=3), "out_dtype")
    # the two products
    for call in (gemm, experts):
        for name in ("a", "asc", "w", "ws", "h", "hs"):
            refused(call(**{name: None}), "null")
        refused(call(flag=None), "flag")
        for name in ("a", "w", "h"):
            refused(call(**{name: q}), "aligned")
        for N in (0, 16, 48, -32):
            refused(call(N=N), "multiple of 32")
        for K in (0, 16, 48):
            refused(call(K=K), "K must be")
        refused(call(a_fmt=3), "a_fmt")
        refused(call(w_fmt=2), "w_fmt")
        refused(call(a_fmt=FP4, w_fmt=W6), "MXFP6 layer")
    refused(gemm(M=65535 * 64 + 1), "row tiles")
    for call in (gemm, experts):
        refused(call(N=1 << 30), "below 2^30")    # (which also bounds the column tiles of one launch: that text has no input of its own)
        refused(call(N=-(1 << 30)), "multiple of 32")
    refused(experts(M=64 * 65535, ws_bytes=1 << 30), "row tiles")
    refused(experts(offsets=None), "offsets")
    refused(experts(E=0), "experts")
    refused(experts(E=_lib.MX_MAX_EXPERTS + 1), "experts")
    refused(experts(work=None), "workspace")
    refused(experts(work=66), "workspace")
    refused(experts(ws_bytes=L.slk_mx_experts_workspace_bytes(2, 4) - 1), "too small")
    assert L.slk_mx_experts_workspace_bytes(2, 4) == 4 * (4 + 3 * (2 + 2))  # unchanged


def operands(M=4, N=32, K=64, E=None, bits_a=8, bits_w=4):
    lead = () if E is None else (E,)
    return (np.zeros((M, K * bits_a // 8), np.uint8), np.full((M, K // 32), 127, np.uint8),
            np.zeros(lead + (2 * N, K * bits_w // 8), np.uint8), np.full(lead + (2 * N, K // 32), 127, np.uint8))


def test_python_refusals_come_before_the_device():
    """Every call here would need the GPU if it got past its checks: NumPy operands, and a ValueError, never a RuntimeError."""
    from sleekit_amd import mx

    a, asc, w, ws = operands(N=64)
    x = np.zeros((4, 64), np.float32)
    down, downs = np.zeros((8, 32), np.uint8), np.full((8, 2), 127, np.uint8)
    offsets = np.array([0, 2, 4], np.int32)
    ea, easc, ew, ews = operands(N=64, E=2)
    for call in (
        lambda: mx.matmul_mx_glu(a[:, :32], asc, w, ws),                                   # mismatched widths
        lambda: mx.matmul_mx_glu(a, asc[:, :1], w, ws),
        lambda: mx.matmul_mx_glu(a, asc, w[:, :16], ws[:, :1]),                            # K of the layer is not the activations'
        lambda: mx.matmul_mx_glu(a, asc, w[:32], ws[:32]),                                 # N = 16: no multiple of 32
        lambda: mx.matmul_mx_glu(a, asc, w[:96], ws[:96]),                                 # N = 48
        lambda: mx.matmul_mx_glu(a, asc, w[:63], ws[:63]),                                 # an odd row count
        lambda: mx.matmul_mx_glu(a, asc, w, ws, activations="mxfp6"),                      # unknown formats and the refused pair
        lambda: mx.matmul_mx_glu(a, asc, w, ws, weights="mxfp8"),
        lambda: mx.matmul_mx_glu(a[:, :32], asc, np.zeros((128, 48), np.uint8), ws, activations="mxfp4", weights="mxfp6_e2m3"),
        lambda: mx.matmul_mx_glu(a, asc, w, ws, bias=np.zeros(32, np.float32)),            # a bias of N, not 2 N, entries
        lambda: mx.matmul_mx_glu(a, asc, w, ws, limit=0.0),
        lambda: mx.matmul_mx_glu(a, asc, w, ws, limit=-7.0),
        lambda: mx.matmul_mx_glu(a, asc, w, ws, alpha=float("nan")),
        lambda: mx.matmul_mx_glu(a, asc, w, ws, shift=INF),
        lambda: mx.matmul_mx_glu(a, asc, w, ws, interleaved=2),
        lambda: mx.matmul_mx_glu_experts(ea, easc, ew, ews, offsets[:2]),
        lambda: mx.matmul_mx_glu_experts(ea, easc, ew, ews, offsets.astype(np.int64)),
        lambda: mx.matmul_mx_glu_experts(ea, easc, ew[:, :63], ews[:, :63], offsets),
        lambda: mx.matmul_mx_glu_experts(ea, easc, ew[:, :32], ews[:, :32], offsets),
        lambda: mx.matmul_mx_glu_experts(ea, easc, ew, ews, offsets, bias=np.zeros((2, 32), np.float32)),
        lambda: mx.matmul_mx_glu_experts(ea, easc, w, ws, offsets),                        # a dense layer where a stack belongs
        lambda: mx.glu(np.zeros((4, 7), np.float32)),                                      # an odd width
        lambda: mx.glu(np.zeros((4, 8), np.float64)),
        lambda: mx.glu(np.zeros((4, 8), np.float32), limit=0),
        lambda: mx.glu(np.zeros((4, 8), np.float32), dtype=torch.bfloat16),                # NumPy has no bfloat16
        lambda: mx.gated_mlp_mx(x[:, :32], w, ws, down, downs),                            # x is not the up layer's width
        lambda: mx.gated_mlp_mx(x, w, ws, np.zeros((8, 16), np.uint8), np.full((8, 1), 127, np.uint8)),   # the down layer's K is not N
        lambda: mx.gated_mlp_mx(x, w[:63], ws[:63], down, downs),
        lambda: mx.gated_mlp_mx(x, w, ws, down, downs, up_bias=np.zeros(32, np.float32)),
        lambda: mx.gated_mlp_mx(x, w, ws, down, downs, down_bias=np.zeros(9, np.float32)),
        lambda: mx.gated_mlp_mx(x, w, ws, down, downs, activations="fp8"),
        lambda: mx.gated_mlp_mx(x, w, ws, down, downs, rotation=object()),
    ):
        with pytest.raises(ValueError):
            call()
    # modules: mismatched sub-modules are refused when the module is built
    up, dn = mx.MXLinear(64, 64), mx.MXLinear(32, 8)
    assert mx.MXGatedMLP(up, dn).hidden_features == 32
    for make in (lambda: mx.MXGatedMLP(mx.MXLinear(64, 62), dn), lambda: mx.MXGatedMLP(mx.MXLinear(64, 63), dn), lambda: mx.MXGatedMLP(up, mx.MXLinear(64, 8)),
                 lambda: mx.MXGatedMLP(up, mx.MXLinear(32, 8, activations="mxfp4")), lambda: mx.MXGatedMLP(up, torch.nn.Linear(32, 8)),
                 lambda: mx.MXGatedMLP(up, dn, limit=0.0), lambda: mx.MXExpertsMLP(up, dn),
                 lambda: mx.MXExpertsMLP(mx.MXExperts(2, 64, 64), mx.MXExperts(3, 32, 8)), lambda: mx.MXExpertsMLP(mx.MXExperts(2, 64, 64), mx.MXExperts(2, 64, 8))):
        with pytest.raises(ValueError):
            make()


def test_every_route_refuses_with_its_own_text():
    """The checks the routes share -- activations as codes or as floats, the layer, its bias, the rotation, the offsets, the
    format pair -- each reached through every public route that has it, one bad argument at a time, with that route's text."""
    from sleekit_amd import mx
    from sleekit_amd.rotation import Rotation

    W6 = "mxfp6_e2m3"
    x, x96 = np.zeros((4, 64), np.float32), np.zeros((4, 96), np.float32)
    a8, a4, aE = np.zeros((4, 64), np.uint8), np.zeros((4, 32), np.uint8), np.full((4, 2), 127, np.uint8)
    a96, aE96 = np.zeros((4, 96), np.uint8), np.full((4, 3), 127, np.uint8)
    c, c6, s = np.zeros((8, 32), np.uint8), np.zeros((8, 48), np.uint8), np.full((8, 2), 127, np.uint8)
    ec, ec6, es = np.zeros((2, 8, 32), np.uint8), np.zeros((2, 8, 48), np.uint8), np.full((2, 8, 2), 127, np.uint8)
    up, ups = np.zeros((128, 32), np.uint8), np.full((128, 2), 127, np.uint8)        # N = 64 hidden columns; the down layer is (c, s)
    eup, eups = np.zeros((2, 128, 32), np.uint8), np.full((2, 128, 2), 127, np.uint8)
    off = np.array([0, 2, 4], np.int32)
    rot128 = Rotation(128, device="cpu")
    float_dtypes = "x must be torch.float32, torch.bfloat16 or torch.float16"
    for call, text in (
        # x given as floats: dtype, dimensions, width
        (lambda: mx.linear_mxfp4(x.astype(np.float64), c, s), float_dtypes),
        (lambda: mx.linear_mxfp6(x.astype(np.float64), c6, s), float_dtypes),
        (lambda: mx.gated_mlp_mx(x.astype(np.float64), up, ups, c, s), float_dtypes),
        (lambda: mx.linear_mx_experts(x.astype(np.float64), ec, es, off), r"x must be torch.float32 \(got float64\)"),
        (lambda: mx.linear_mxfp4(np.zeros((), np.float32), c, s), "x must be a NumPy array or torch tensor of at least one dimension"),
        (lambda: mx.linear_mxfp6(np.zeros((), np.float32), c6, s), "x must be a NumPy array or torch tensor of at least one dimension"),
        (lambda: mx.gated_mlp_mx(np.zeros((), np.float32), up, ups, c, s), "x must be a NumPy array or torch tensor of at least one dimension"),
        (lambda: mx.linear_mx_experts(x[0], ec, es, off), "x must be a 2-D NumPy array or torch tensor"),
        (lambda: mx.linear_mxfp4(x96, c, s), "x has 96 columns but the layer has 64"),
        (lambda: mx.linear_mxfp6(x96, c6, s), "x has 96 columns but the layer has 64"),
        (lambda: mx.linear_mx_experts(x96, ec, es, off), "x has 96 columns but the experts' layers have 64"),
        (lambda: mx.gated_mlp_mx(x96, up, ups, c, s), "x has 96 columns but the up layer has 64"),
        # activations given as codes
        (lambda: mx.matmul_mx(a8[0], aE, c, s), "a_codes must be a 2-D NumPy array or torch tensor"),
        (lambda: mx.matmul_mx_experts(a8[0], aE, ec, es, off), "a_codes must be a 2-D NumPy array or torch tensor"),
        (lambda: mx.matmul_mx(a8.astype(np.int32), aE, c, s), r"a_codes must be torch.uint8 \(got int32\)"),
        (lambda: mx.matmul_mx_experts(a8.astype(np.int32), aE, ec, es, off), r"a_codes must be torch.uint8 \(got int32\)"),
        (lambda: mx.matmul_mx(a8, aE[:, :1], c, s), r"activation scale bytes must be \(4, 2\)"),
        (lambda: mx.matmul_mx_experts(a8, aE[:, :1], ec, es, off), r"activation scale bytes must be \(4, 2\)"),
        (lambda: mx.matmul_mx(a96, aE96, c, s), "a_codes has 96 columns but the layer has 64"),
        (lambda: mx.matmul_mx_experts(a96, aE96, ec, es, off), "a_codes has 96 columns but the experts' layers have 64"),
        # the rotation: its type, and its size for `rotation` and for `down_rotation`
        (lambda: mx.linear_mxfp4(x, c, s, rotation="hadamard"), r"rotation must be a Rotation \(got str\)"),
        (lambda: mx.linear_mxfp6(x, c6, s, rotation="hadamard"), r"rotation must be a Rotation \(got str\)"),
        (lambda: mx.linear_mx_experts(x, ec, es, off, rotation="hadamard"), r"rotation must be a Rotation \(got str\)"),
        (lambda: mx.gated_mlp_mx(x, up, ups, c, s, rotation="hadamard"), r"^rotation must be a Rotation \(got str\)"),
        (lambda: mx.gated_mlp_mx(x, up, ups, c, s, down_rotation="hadamard"), r"^down_rotation must be a Rotation \(got str\)"),
        (lambda: mx.linear_mxfp4(x, c, s, rotation=rot128), "the rotation has 128 features but the layer has 64"),
        (lambda: mx.linear_mxfp6(x, c6, s, rotation=rot128), "the rotation has 128 features but the layer has 64"),
        (lambda: mx.linear_mx_experts(x, ec, es, off, rotation=rot128), "the rotation has 128 features but the layers have 64"),
        (lambda: mx.gated_mlp_mx(x, up, ups, c, s, rotation=rot128), "the rotation has 128 features but the layer has 64"),
        (lambda: mx.gated_mlp_mx(x, up, ups, c, s, down_rotation=rot128), "the down_rotation has 128 features but the layer has 64"),
        # the bias
        (lambda: mx.matmul_mx(a8, aE, c, s, bias=np.zeros(7, np.float32)), r"bias must be \(8,\); got \(7,\)"),
        (lambda: mx.linear_mxfp4(x, c, s, bias=np.zeros(7, np.float32)), r"bias must be \(8,\); got \(7,\)"),
        (lambda: mx.linear_mxfp6(x, c6, s, bias=np.zeros((1, 8), np.float32)), r"bias must be \(8,\); got \(1, 8\)"),
        (lambda: mx.matmul_mx_experts(a8, aE, ec, es, off, bias=np.zeros(8, np.float32)), r"bias must be \(2, 8\); got \(8,\)"),
        (lambda: mx.linear_mx_experts(x, ec, es, off, bias=np.zeros((2, 7), np.float32)), r"bias must be \(2, 8\); got \(2, 7\)"),
        (lambda: mx.gated_mlp_mx(x, up, ups, c, s, up_bias=np.zeros(64, np.float32)), r"bias must be \(128,\); got \(64,\)"),
        (lambda: mx.gated_mlp_mx(x, up, ups, c, s, down_bias=np.zeros(9, np.float32)), r"bias must be \(8,\); got \(9,\)"),
        (lambda: mx.matmul_mx_glu_experts(a8, aE, eup, eups, off, bias=np.zeros((2, 64), np.float32)), r"bias must be \(2, 128\); got \(2, 64\)"),
        # the offsets: dtype and length
        (lambda: mx.matmul_mx_experts(a8, aE, ec, es, off.astype(np.int64)), r"offsets must be int32 \(3,\).*got int64 \(3,\)"),
        (lambda: mx.linear_mx_experts(x, ec, es, off.astype(np.int64)), r"offsets must be int32 \(3,\).*got int64 \(3,\)"),
        (lambda: mx.matmul_mx_experts(a8, aE, ec, es, off[:2]), r"offsets must be int32 \(3,\).*got int32 \(2,\)"),
        (lambda: mx.linear_mx_experts(x, ec, es, off[:2]), r"offsets must be int32 \(3,\).*got int32 \(2,\)"),
        # a dense layer where a stack belongs, and the reverse
        (lambda: mx.matmul_mx_experts(a8, aE, c, s, off), "codes of stacked experts must be a 3-D"),
        (lambda: mx.linear_mx_experts(x, c, s, off), "codes of stacked experts must be a 3-D"),
        (lambda: mx.matmul_mx(a8, aE, ec, es), "codes must be a 2-D NumPy array or torch tensor"),
        (lambda: mx.linear_mxfp4(x, ec, es), "codes must be a 2-D NumPy array or torch tensor"),
        (lambda: mx.linear_mxfp6(x, ec6, es), "codes must be a 2-D NumPy array or torch tensor"),
        (lambda: mx.gated_mlp_mx(x, eup, eups, c, s), "codes must be a 2-D NumPy array or torch tensor"),
        (lambda: mx.gated_mlp_mx(x, up, ups, ec, es), "codes must be a 2-D NumPy array or torch tensor"),
        # the refused pair
        (lambda: mx.matmul_mx(a4, aE, c6, s, activations="mxfp4", weights=W6), 'an MXFP6 layer takes "mxfp8" or "mxfp6_e2m3" activations \\(got "mxfp4"\\)'),
        (lambda: mx.matmul_mx_experts(a4, aE, ec6, es, off, activations="mxfp4", weights=W6), 'an MXFP6 layer takes .* \\(got "mxfp4"\\)'),
        (lambda: mx.linear_mxfp6(x, c6, s, activations="mxfp4"), 'an MXFP6 layer takes .* \\(got "mxfp4"\\)'),
        (lambda: mx.linear_mx_experts(x, ec6, es, off, activations="mxfp4", weights=W6), 'an MXFP6 layer takes .* \\(got "mxfp4"\\)'),
        (lambda: mx.gated_mlp_mx(x, np.zeros((128, 48), np.uint8), ups, c6, s, activations="mxfp4", weights=W6), 'an MXFP6 layer takes .* \\(got "mxfp4"\\)'),
    ):
        with pytest.raises(ValueError, match=text):
            call()


def test_model_is_silu_times_up_and_the_gpt_oss_formula():
    rng = np.random.default_rng(5)
    g, u = (rng.standard_normal(4000) * 6).astype(np.float32), (rng.standard_normal(4000) * 6).astype(np.float32)
    want = torch.nn.functional.silu(torch.from_numpy(g).double()) * torch.from_numpy(u).double()
    assert np.abs(model.gate_f64(g, u, **model.SWIGLU) - want.numpy()).max() <= 1e-12
    # gpt-oss, written out: the gate clamped from above at 7, up to +-7, g * sigmoid(1.702 g) * (u + 1)
    a = np.float64(np.float32(1.702))
    gc, uc = np.minimum(g.astype(np.float64), 7.0), np.clip(u.astype(np.float64), -7.0, 7.0)
    want = (uc + 1.0) * (gc / (1.0 + np.exp(-a * gc)))
    got = model.gate_f64(g, u, **model.GPT_OSS)
    assert (np.abs(g) > 7).any() and (np.abs(u) > 7).any()
    assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    # the float32 model: the float64 one up to float32's roundings, and exact where it has no transcendental (alpha = 0)
    assert np.abs(model.gate_f32(g, u, **model.GPT_OSS) - got).max() <= 2.0 ** -19 * np.abs(got).max()
    h = model.gate_f32(g, u, alpha=0.0, limit=3.0, shift=1.0)
    gc32, uc32 = np.minimum(g, np.float32(3)), np.clip(u, np.float32(-3), np.float32(3))
    assert h.dtype == np.float32 and np.array_equal(h, (uc32 + np.float32(1)) * (gc32 * np.float32(0.5)))
    # a NaN passes through both clamps
    nan = np.float32("nan")
    assert np.isnan(model.gate_f32([nan, 1.0], [1.0, nan], **model.GPT_OSS)).all() and np.isnan(model.gate_f64([nan, 1.0], [1.0, nan])).all()
    assert model.gate_f64([100.0], [-100.0], **model.GPT_OSS)[0] == (-7.0 + 1.0) * (7.0 / (1.0 + np.exp(-a * 7.0)))


def test_interleaved_picks_the_stated_columns():
    Y = np.arange(3 * 8, dtype=np.float32).reshape(3, 8)
    g, u = model.split(Y, interleaved=False)
    assert np.array_equal(g, Y[:, 0:4]) and np.array_equal(u, Y[:, 4:8])
    g, u = model.split(Y, interleaved=True)
    assert np.array_equal(g, Y[:, 0::2]) and np.array_equal(u, Y[:, 1::2])
    assert [c.tolist() for c in model.columns(3, False)] == [[0, 1, 2], [3, 4, 5]] and [c.tolist() for c in model.columns(3, True)] == [[0, 2, 4], [1, 3, 5]]
    # a layer stored one way is the other's rows permuted: the gate sees the same pairs
    perm = np.empty(8, np.int64)
    perm[0::2], perm[1::2] = np.arange(4), 4 + np.arange(4)
    assert np.array_equal(model.glu_f32(Y[:, perm], interleaved=True, **model.GPT_OSS), model.glu_f32(Y, interleaved=False, **model.GPT_OSS))


def fill(module, seed):
    g = torch.Generator().manual_seed(seed)
    for b in module.buffers():
        b.copy_(torch.randint(0, 200, b.shape, generator=g).to(b.dtype))


def test_state_dicts_round_trip():
    from sleekit_amd import MXExpertsMLP, MXGatedMLP, mx

    gate = dict(alpha=1.702, limit=7.0, shift=1.0, interleaved=True)
    for make, keys in ((lambda **kw: MXGatedMLP(mx.MXLinear(64, 128, **kw), mx.MXLinear(64, 32, **kw)), 6),
                       (lambda **kw: MXExpertsMLP(mx.MXExperts(3, 64, 128, **kw), mx.MXExperts(3, 64, 32, **kw)), 6)):
        plain = make()
        fill(plain, 1)
        state = plain.state_dict()
        assert sorted(state) == ["down.bias", "down.codes", "down.scales", "up.bias", "up.codes", "up.scales"] and len(state) == keys
        copy = make()
        copy.load_state_dict(state)
        assert all(torch.equal(a, b) for a, b in zip(copy.buffers(), plain.buffers())) and copy.gate == plain.gate == (1.0, None, 0.0, False)
        # the gate parameters, and the sub-modules' own extra state, travel only when they are not the defaults
        other = type(plain)(make(activations="mxfp4").up, make(activations="mxfp4").down, **gate)
        fill(other, 2)
        state = other.state_dict()
        assert state["_extra_state"] == gate and state["up._extra_state"] == {"activations": "mxfp4"} == state["down._extra_state"]
        copy.load_state_dict(state)
        assert (copy.alpha, copy.limit, copy.shift, copy.interleaved) == (1.702, 7.0, 1.0, True) and copy.activations == "mxfp4"
        assert all(torch.equal(a, b) for a, b in zip(copy.buffers(), other.buffers()))
        copy.load_state_dict(plain.state_dict())   # a state without the key means the defaults again
        assert copy.gate == (1.0, None, 0.0, False) and copy.activations == "mxfp8"
        half = type(plain)(make().up, make().down, shift=1.0)
        assert half.state_dict()["_extra_state"] == {"shift": 1.0}
        bad = dict(plain.state_dict(), _extra_state={"limit": -1.0})
        with pytest.raises(RuntimeError, match="limit"):
            copy.load_state_dict(bad)
