"""The weight-only MX layers without a GPU: the float64 model against hand-computed answers, every refusal of the Python
surface before anything touches a device, the C entries' argument checks (which launch nothing), and `activations` through
state_dict and extra_repr of the modules.
"""

import ctypes

import numpy as np
import pytest
import torch

import mx_a16_model as model

W4, W6 = "mxfp4", "mxfp6_e2m3"
HALVES = ("bfloat16", "float16")


# ---------------------------------------------------------------------------------------------------------------- the model
def test_model_against_hand_computed_answers():
    """One block of known codes.  E2M1: codes 0 .. 15 are 0, .5, 1, 1.5, 2, 3, 4, 6 and their negatives (0x8 reads as +0).
    E2M3: 0x01 = 0.125, 0x08 = 1, 0x0f = 1.875, 0x1f = 7.5, 0x21 = -0.125, 0x3f = -7.5.  Scale byte 128 doubles."""
    c4 = np.zeros((1, 32), np.uint8)
    c4[0, :16] = np.arange(16)
    codes = model.pack_codes(c4, W4)
    assert codes.shape == (1, 16) and codes[0, 0] == 0x10 and codes[0, 7] == 0xFE
    Wc, W32 = model.weights_model(codes, np.array([[128]], np.uint8), W4, torch.bfloat16)
    want = 2 * np.array([0, .5, 1, 1.5, 2, 3, 4, 6, 0, -.5, -1, -1.5, -2, -3, -4, -6] + [0] * 16)
    assert np.array_equal(Wc[0], want) and np.array_equal(W32[0], want.astype(np.float32))
    x = np.zeros((2, 32), np.float32)
    x[0, 7], x[0, 15], x[1, :8] = 3.0, 1.0, 1.0          # 3 * 12 - 12 = 24;  0 + 1 + 2 + 3 + 4 + 6 + 8 + 12 = 36
    Y, A = model.linear_model(x, codes, np.array([[128]], np.uint8), W4, torch.float16, bias=np.array([0.5], np.float32))
    assert Y.tolist() == [[24.5], [36.5]] and A.tolist() == [[48.5], [36.5]]

    c6 = np.zeros((1, 32), np.uint8)
    c6[0, :6] = [0x01, 0x08, 0x0F, 0x1F, 0x21, 0x3F]
    codes6 = model.pack_codes(c6, W6)
    assert codes6.shape == (1, 24)
    Wc6, _ = model.weights_model(codes6, np.array([[126]], np.uint8), W6, torch.float16)
    assert Wc6[0, :7].tolist() == [0.0625, 0.5, 0.9375, 3.75, -0.0625, -3.75, 0.0]

    # Xc is x rounded to the compute type: 1 + 2^-9 is a float16 and rounds to 1 in bfloat16; 257 is neither's tie (256 | 258)
    x = np.array([[1 + 2.0 ** -9] + [0] * 31], np.float32)
    ones = model.pack_codes(np.full((1, 32), 2, np.uint8), W4)  # every weight 1
    one = np.array([[127]], np.uint8)
    assert model.linear_model(x, ones, one, W4, torch.float16)[0][0, 0] == 1 + 2.0 ** -9
    assert model.linear_model(x, ones, one, W4, torch.bfloat16)[0][0, 0] == 1.0
    assert model.linear_model(257 * x / x[0, 0], ones, one, W4, torch.bfloat16)[0][0, 0] == 256.0

    # the promised ranges: the smallest and the largest non-zero magnitude are normal numbers at both ends.  float16's range is
    # tight -- one byte outside it something is not; bfloat16's is the one slk_hessian_accumulate_experts_mx words, which
    # E4M3's 2^-9 and 448 set, and these formats have room to spare inside it
    for compute, tiny, huge in ((torch.bfloat16, 2.0 ** -126, 2.0 ** 128), (torch.float16, 2.0 ** -14, 65520.0)):
        lo, hi = model.NORMAL_BYTES[compute]
        for weights, least, most in ((W4, 0.5, 6.0), (W6, 0.125, 7.5)):
            assert least * 2.0 ** (lo - 127) >= tiny and most * 2.0 ** (hi - 127) < huge
    lo, hi = model.NORMAL_BYTES[torch.float16]
    assert 0.125 * 2.0 ** (lo - 1 - 127) < 2.0 ** -14 and 7.5 * 2.0 ** (hi + 1 - 127) >= 65520.0


def test_experts_model_is_the_dense_model_per_slice():
    rng = np.random.default_rng(3)
    codes = rng.integers(0, 256, (3, 4, 16), dtype=np.uint8)
    scales = rng.integers(125, 130, (3, 4, 1), dtype=np.uint8)
    x = rng.integers(-3, 4, (5, 32)).astype(np.float32)
    Y, _ = model.experts_model(x, codes, scales, [0, 2, 2, 5], W4, torch.bfloat16)
    assert np.array_equal(Y[:2], model.linear_model(x[:2], codes[0], scales[0], W4, torch.bfloat16)[0])
    assert np.array_equal(Y[2:], model.linear_model(x[2:], codes[2], scales[2], W4, torch.bfloat16)[0])


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_activation_names():
    from sleekit_amd import mx

    assert tuple(mx._FORMATS) == ("mxfp8", "mxfp4", "mxfp6_e2m3")  # the coded formats only
    assert tuple(mx._HALVES) == HALVES and mx._ACTIVATIONS == tuple(mx._FORMATS) + HALVES
    for name in mx._ACTIVATIONS:
        assert f'"{name}"' in mx._ACTIVATIONS_ARE
    assert mx._HALVES["bfloat16"].dtype == torch.bfloat16 and mx._HALVES["float16"].dtype == torch.float16


def test_python_refusals_come_before_the_device():
    from sleekit_amd import mx, rotation, statistics

    codes, scales = np.zeros((8, 32), np.uint8), np.full((8, 2), 127, np.uint8)       # an MXFP4 layer of K = 64
    codes6 = np.zeros((8, 48), np.uint8)                                              # the MXFP6 layer of that shape
    up, up_s = np.zeros((64, 32), np.uint8), np.full((64, 2), 127, np.uint8)          # gate and up: N = 32 hidden columns
    down, down_s = np.zeros((8, 16), np.uint8), np.full((8, 1), 127, np.uint8)
    a, a_s = np.zeros((4, 64), np.uint8), np.full((4, 2), 127, np.uint8)
    x, offsets = np.zeros((4, 64), np.float32), np.array([0, 4], np.int32)
    for half in HALVES:
        # matmul_mx* take coded activations; the message points to linear_*
        for call in (lambda: mx.matmul_mx(a, a_s, codes, scales, activations=half),
                     lambda: mx.matmul_mx(a, a_s, codes6, scales, activations=half, weights=W6),
                     lambda: mx.matmul_mx_experts(a, a_s, codes[None], scales[None], offsets, activations=half)):
            with pytest.raises(ValueError, match=r"matmul_mx\* multiply activations that exist as MX codes.*linear_mxfp4, linear_mxfp6 or linear_mx_experts"):
                call()
        # the gated surface: a 16-bit hidden activation through the gated epilogue is not built
        for call in (lambda: mx.matmul_mx_glu(a, a_s, up, up_s, activations=half),
                     lambda: mx.matmul_mx_glu_experts(a, a_s, up[None], up_s[None], offsets, activations=half),
                     lambda: mx.gated_mlp_mx(x, up, up_s, down, down_s, activations=half),
                     lambda: mx.MXGatedMLP(mx.MXLinear(64, 64, activations=half), mx.MXLinear(32, 8, activations=half)),
                     lambda: mx.MXExpertsMLP(mx.MXExperts(2, 64, 64, activations=half), mx.MXExperts(2, 32, 8, activations=half)),
                     lambda: mx._gated_mlp_experts(x, (up[None], up_s[None], None), (down[None], down_s[None], None), offsets, None, half, None, None, None, True,
                                           mx._FP4, mx._FP4)):
            with pytest.raises(ValueError, match="gated epilogue are not supported"):
                call()
        with pytest.raises(ValueError, match="add_codes takes rows that exist as MX codes"):
            statistics.ExpertStatistics.add_codes(None, a, a_s, offsets, activations=half)
        # what the weight-only calls themselves refuse, still on the host
        with pytest.raises(ValueError, match="columns"):
            mx.linear_mxfp4(np.zeros((4, 96), np.float32), codes, scales, activations=half)
        with pytest.raises(ValueError):
            mx.linear_mxfp6(x.astype(np.float64), codes6, scales, activations=half)
        with pytest.raises(ValueError, match="NumPy has no bfloat16"):
            mx.linear_mxfp4(x, codes, scales, dtype=torch.bfloat16, activations=half)
        with pytest.raises(ValueError, match="bias"):
            mx.linear_mxfp4(x, codes, scales, np.zeros(7, np.float32), activations=half)
        with pytest.raises(ValueError, match="offsets"):
            mx.linear_mx_experts(x, codes[None], scales[None], offsets[:1], activations=half)
        rot = rotation.Rotation._of(torch.ones(128), 32)  # (signs on the host: nothing here reaches a kernel)
        with pytest.raises(ValueError, match="features"):
            mx.linear_mxfp4(x, codes, scales, activations=half, rotation=rot)
    for bad in ("bf16", "fp16", "float32", "BFLOAT16", torch.bfloat16, None):
        with pytest.raises(ValueError, match="activations must be .*\"bfloat16\" or \"float16\""):
            mx.linear_mxfp4(x, codes, scales, activations=bad)
        with pytest.raises(ValueError, match="activations"):
            mx.MXLinear(64, 8, activations=bad)
        with pytest.raises(ValueError, match="activations"):
            mx.MXExperts(2, 64, 8, activations=bad)


def test_c_entries_refuse_before_any_launch():
    """SLK_E_ARG with a text, from arguments alone (the pointers are never followed)."""
    from sleekit_amd import _lib

    lib = _lib.lib
    P = ctypes.c_void_p
    F32, BF16, F16 = _lib.DTYPE_F32, _lib.DTYPE_BF16, _lib.DTYPE_F16
    p = 4096

    def dense(X=p, xd=BF16, wc=p, wsc=p, wf=_lib.MX_W_FP4, M=4, N=8, K=64, cd=BF16, od=F32, out=p):
        return lib.slk_mx_gemm_a16(P(X), xd, P(wc), P(wsc), wf, None, M, N, K, cd, od, P(out), None)

    def experts(X=p, xd=BF16, wc=p, wsc=p, wf=_lib.MX_W_FP4, offsets=p, E=2, M=4, N=8, K=64, cd=BF16, od=F32, out=p, flag=p, ws=p, ws_bytes=1 << 20):
        return lib.slk_mx_gemm_experts_a16(P(X), xd, P(wc), P(wsc), wf, None, P(offsets), E, M, N, K, cd, od, P(out), P(flag), P(ws), ws_bytes, None)

    shared = [(dict(K=48), b"multiple of 32"), (dict(K=0), b"multiple of 32"), (dict(M=0), b"at least 1"), (dict(N=0), b"at least 1"),
              (dict(X=None), b"null"), (dict(wc=None), b"null"), (dict(wsc=None), b"null"), (dict(out=None), b"null"),
              (dict(xd=3), b"x_dtype"), (dict(od=7), b"out_dtype"), (dict(cd=F32), b"compute_dtype"), (dict(cd=5), b"compute_dtype"),
              (dict(wf=2), b"w_fmt"), (dict(X=p + 8), b"aligned"), (dict(wc=p + 4), b"aligned"), (dict(out=p + 2), b"aligned")]
    for entry in (dense, experts):
        for kw, text in shared:
            assert entry(**kw) == _lib.E_ARG, kw
            assert text in lib.slk_last_error(), (kw, lib.slk_last_error())
    for kw, text in [(dict(E=0), b"experts"), (dict(E=_lib.MX_MAX_EXPERTS + 1), b"experts"), (dict(flag=None), b"flag"),
                     (dict(offsets=None), b"offsets"), (dict(ws=None), b"workspace"), (dict(ws=p + 2), b"workspace"),
                     (dict(ws_bytes=8), b"too small")]:
        assert experts(**kw) == _lib.E_ARG, kw
        assert text in lib.slk_last_error(), (kw, lib.slk_last_error())
    assert lib.slk_abi_version() == 8


# ---------------------------------------------------------------------------------------------------------------- modules
@pytest.mark.parametrize("half", HALVES)
@pytest.mark.parametrize("weights", [W4, W6])
def test_modules_carry_activations_through_state_and_repr(half, weights):
    from sleekit_amd import mx, rotation

    lin = mx.MXLinear(64, 8, activations=half, weights=weights)
    assert lin.activations == half and f"activations={half}" in lin.extra_repr()
    state = lin.state_dict()
    assert state["_extra_state"]["activations"] == half
    other = mx.MXLinear(64, 8, weights=weights)
    assert other.activations == "mxfp8"
    other.load_state_dict(state)
    assert other.activations == half and f"activations={half}" in repr(other)
    other.load_state_dict(mx.MXLinear(64, 8, weights=weights).state_dict())   # no key: "mxfp8" again
    assert other.activations == "mxfp8"

    ex = mx.MXExperts(3, 64, 8, activations=half, weights=weights)
    assert f"activations={half}" in ex.extra_repr()
    loaded = mx.MXExperts(3, 64, 8, weights=weights)
    loaded.load_state_dict(ex.state_dict())
    assert loaded.activations == half

    rot = rotation.Rotation._of(torch.ones(64), 32)
    for fused in (False, True):   # `fused` stays stored and round-trips, whatever the inner layer's activations
        turned = rotation.RotatedLinear(mx.MXLinear(64, 8, activations=half, weights=weights), rot, fused=fused)
        assert turned.fused is fused and turned._weight_only()
        copy = rotation.RotatedLinear(mx.MXLinear(64, 8, weights=weights), rotation.Rotation._of(torch.ones(64), 64), fused=not fused)
        copy.load_state_dict(turned.state_dict())
        assert copy.fused is fused and copy.block == 32 and copy.inner.activations == half and copy._weight_only()
    assert not rotation.RotatedLinear(mx.MXLinear(64, 8, weights=weights), rot)._weight_only()


# ---------------------------------------------------------------------------------------------------------------- error table
def output_errors(seed):
    """tests/test_mx6_cpu.py's output_errors (the same layer, tokens, rotation and seeds; the weights rounded to nearest in
    MXFP4 and in MXFP6 under their non-saturating scales) with bfloat16 activations, the weight-only product's operands: x --
    behind the rotation x R -- rounded to bfloat16, and the de-quantized weights, which are bfloat16 values already.
    Relative output error of W4A16 and W6A16 beside W4A8 and W6A8, an array (2, 4) indexed [rotated][case]."""
    import mx_act4_model
    import mx_act6_model
    import mx_gemm_model
    import rotation_model
    from sleekit_amd import synth

    W = synth.make_weights(64, 256, seed)
    x = synth.make_activations(128, 256, seed).astype(np.float32)
    want = x.astype(np.float64) @ W.astype(np.float64).T
    signs = rotation_model.signs_for(256, seed)
    out = np.zeros((2, 4))
    for rotated in (False, True):
        xr = rotation_model.transform(x, 256, signs) if rotated else x
        Wr = rotation_model.transform(W, 256, signs) if rotated else W
        W4q = mx_act4_model.dequantize_act4_model(*mx_act4_model.quantize_act4_model(Wr))
        W6q = mx_act6_model.dequantize_act6_model(*mx_act6_model.quantize_act6_model(Wr))
        for w in (W4q, W6q):
            assert np.array_equal(model.round_to(np.asarray(w, np.float32), torch.bfloat16), np.asarray(w, np.float64))
        a16 = model.round_to(np.asarray(xr, np.float32), torch.bfloat16)
        a8 = mx_gemm_model.dequantize_act_model(*mx_gemm_model.quantize_act_model(xr))
        out[int(rotated)] = [np.linalg.norm(a @ np.asarray(w, np.float64).T - want) / np.linalg.norm(want)
                             for w, a in ((W4q, a16), (W6q, a16), (W4q, a8), (W6q, a8))]
    return out


def test_output_error_table():
    """The accuracy ladder's floor: what the weights alone cost.  Asserted on every seed, plain and
    rotated: MXFP6 weights below MXFP4 weights, and 16-bit activations not above MXFP8 ones by more than bfloat16's own
    rounding of x could add (2^-9 relative to the output's norm is generous: the two errors are independent)."""
    from test_mx_act6_cpu import SEEDS

    t = np.array([output_errors(seed) for seed in SEEDS])  # (seed, rotated, case)
    for r, name in enumerate(("plain", "rotated, block 256")):
        print(f"{name:20s} " + "  ".join(f"{case} {t[:, r, i].mean():.4f} [{t[:, r, i].min():.4f} .. {t[:, r, i].max():.4f}]"
                                        for i, case in enumerate(("W4A16", "W6A16", "W4A8", "W6A8"))))
    assert np.isfinite(t).all() and (t > 0).all()
    for r in (0, 1):
        w4a16, w6a16, w4a8, w6a8 = t[:, r].T
        assert (w6a16 < w4a16).all(), (r, t[:, r])
        assert (w4a16 <= w4a8 + 2.0 ** -9).all() and (w6a16 <= w6a8 + 2.0 ** -9).all(), (r, t[:, r])
