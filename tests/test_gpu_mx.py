"""MXFP4 on the MI355X (sleekit_amd.mx; slk_mx_scale_search, slk_mx_pack, slk_mx_unpack, slk_mx_dequantize) against the
reference's own results (tests/golden/mx.npz), the NumPy model (tests/mx_model.py), the existing grouped scale search as a
second oracle on the device, and itself.  Every comparison is bit for bit; a searched row may differ from the reference's
only where one of its decisions was a proven near-tie (tests/ls_evidence.py).

Run on the GPU box:  python -m pytest tests/test_gpu_mx.py -m gpu -q
"""

import numpy as np
import pytest
import torch

import mx_model
from packing_model import pack_model as pack_bits
from test_mx_cpu import CASES, FIX, case_inputs, check_codes, check_indices

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def gpu():
    assert torch.cuda.is_available(), "these tests need the GPU"
    torch.cuda.set_device(0)


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def host(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t


def fuzz_layer(rng, R, n, magnitude):
    """Weights of a few magnitudes around `magnitude` with outliers, zero blocks, one-signed blocks and exact ties, and a
    positive diagonal."""
    W = rng.standard_normal((R, n)).astype(np.float32)
    W *= np.exp2(rng.integers(-3, 4, (R, n // 32))).astype(np.float32).repeat(32, axis=1)
    out = rng.random((R, n)) < 0.02
    W[out] *= rng.choice(np.array([4, 8, 16, 32, 64], np.float32), int(out.sum()))
    blocks = W.reshape(R, n // 32, 32)
    kind = rng.integers(0, 12, (R, n // 32))
    blocks[kind == 0] = 0
    blocks[kind == 1] = np.abs(blocks[kind == 1])
    blocks[kind == 2] = -np.abs(blocks[kind == 2])
    ties = kind == 3  # multiples of a quarter: many elements sit exactly on a limit of some candidate
    blocks[ties] = np.round(blocks[ties] * 4) / 4
    W = (blocks.reshape(R, n) * np.float32(magnitude)).astype(np.float32)
    H = np.diag(rng.uniform(0.05, 4.0, n).astype(np.float32)) + np.float32(0.01)
    return W, H.astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- scales
@pytest.mark.parametrize("i", range(len(CASES)))
def test_scales_equal_the_reference(i):
    from sleekit_amd import mx

    c = CASES[i]
    W, H, S = case_inputs(i)
    got_S, got_E = mx.compute_mx_scales(W, H, c["mode"])
    assert got_E.dtype == np.uint8 and np.array_equal(got_E, FIX[f"E_{i}"]), f"case {i}: {c}"
    assert got_S.dtype == np.float32 and np.array_equal(bits(got_S), bits(S))


def existing_route(Wd, Hd, base, mode):
    """slk_scale_search_grouped with the power-of-two base and the four factors: the grouped search that was there before."""
    from sleekit_amd import _device as dev, _lib, engine, mx

    R, n = Wd.shape
    levels, lo, hi, table = engine.require_uniform(mx.E2M1)
    factors = torch.tensor(mx_model.FACTORS, dtype=torch.float32, device=Wd.device)
    hd = Hd.diagonal().contiguous() if mode == "diag" else None
    out = torch.empty(R * (n // 32), dtype=torch.float32, device=Wd.device)
    _lib.check(_lib.lib.slk_scale_search_grouped(dev.ptr(Wd), dev.ptr(base), dev.ptr(factors), 4, dev.ptr(hd), 32, R, n, levels, lo, hi,
                                                 dev.ptr(table), dev.ptr(out), dev.stream_handle()))
    return out.view(R, n // 32)


@pytest.mark.parametrize("R,n,magnitude,seed", [
    (1, 32, 1.0, 1), (3, 96, 1e-16, 2), (7, 160, 1e-9, 3), (64, 256, 1.0, 4), (33, 1056, 1e6, 5), (600, 128, 1e-3, 6),
    (130, 4096, 0.02, 7), (17, 352, 1e15, 8), (9, 64, 1e30, 9), (257, 96, 1e-12, 10),
])
def test_scales_equal_the_model_and_the_existing_search(R, n, magnitude, seed):
    from sleekit_amd import mx

    rng = np.random.default_rng(9000 + seed)
    W, H = fuzz_layer(rng, R, n, magnitude)
    # an unaligned view: the layer starts 4 bytes into its buffer (and 12 bytes for the diagonal's matrix)
    buf = torch.empty(R * n + 1, dtype=torch.float32, device="cuda")
    Wd = buf[1:].view(R, n)
    Wd.copy_(torch.from_numpy(W))
    assert Wd.data_ptr() % 16 == 4
    Hd = torch.from_numpy(H).cuda()
    for mode in ("max", "mse", "diag"):
        want_S, want_E, found = mx_model.scales_model(W, H, mode, want_found=True)
        S, E = mx.compute_mx_scales(Wd, Hd, mode)
        assert S.is_cuda and E.is_cuda and E.dtype == torch.uint8
        assert np.array_equal(host(E), want_E), (mode, R, n)
        assert np.array_equal(bits(S), bits(want_S))
        assert want_E.min() >= 71 and want_E.max() <= 253
        if mode != "max":
            base = mx.compute_mx_scales(Wd, None, "max")[0]
            old = host(existing_route(Wd, Hd, base.reshape(-1).contiguous(), mode))
            # where every candidate's error overflows float32 the search that was there answers base * inf; elsewhere bit for bit
            assert np.array_equal(np.isfinite(old), found), (mode, R, n)
            assert np.array_equal(bits(old)[found], bits(S)[found]), (mode, R, n)
            assert found.all() or magnitude >= 1e15


def test_every_factor_and_the_floor_are_reached():
    """One outlier a block, 1.5 to 96 times the rest, in a column the diagonal barely weighs: the smaller the weight of the
    outlier's saturation, the lower the factor that wins."""
    from sleekit_amd import mx

    rng = np.random.default_rng(78)
    mult = np.array([1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64], np.float32)
    W = rng.uniform(-1, 1, (len(mult) * 8, 64)).astype(np.float32)
    W[:, 0] = np.repeat(mult, 8) * 1.5
    W[:, 32] = -np.repeat(mult, 8) * 1.5
    H = np.eye(64, dtype=np.float32)
    H[0, 0] = H[32, 32] = 1e-6
    base = mx.compute_mx_scales(W, None, "max")[1].astype(np.int32)
    E = mx.compute_mx_scales(W, H, "diag")[1]
    assert np.array_equal(E, mx_model.scales_model(W, H, "diag")[1])
    assert set(np.unique(E.astype(np.int32) - base)) == {-3, -2, -1, 0}
    zero = np.zeros((2, 64), np.float32)
    assert mx.compute_mx_scales(zero, None, "max")[1].tolist() == [[74, 74]] * 2
    assert mx.compute_mx_scales(zero, None, "mse")[1].tolist() == [[71, 71]] * 2


# ---------------------------------------------------------------------------------------------------------------- the layer
@pytest.mark.parametrize("i", range(len(CASES)))
def test_quantize_equals_the_reference(i):
    from sleekit_amd import mx

    c = CASES[i]
    W, H, S = case_inputs(i)
    res = mx.quantize_mxfp4(W, H, c["act_order"], c["damp"], c["mode"], c["moves"], None, c["min_block_size"], c["num_blocks"])
    assert np.array_equal(res.scales, FIX[f"E_{i}"]) and np.array_equal(bits(res.S), bits(S))
    trace = None
    if c["moves"]:
        Wd, Hd = torch.from_numpy(W).cuda(), torch.from_numpy(H).cuda()
        packed, layer = mx.quantize_layer_mxfp4(Wd, Hd, c["act_order"], c["damp"], c["mode"], c["moves"], want_ls_trace=True)
        assert torch.equal(packed.idx.cpu(), torch.from_numpy(res.idx))
        trace = layer.ls_trace.cpu().numpy()
    bad = check_indices(i, res.idx, trace)
    check_codes(i, res.codes, bad)
    # the packed form is the layer: codes and scale bytes rebuild Q bit for bit, and they are the model's pack of idx
    codes, E = mx_model.pack_model(res.idx, res.S)
    assert np.array_equal(res.codes, codes) and np.array_equal(res.scales, E)
    assert np.array_equal(bits(mx.dequantize_mxfp4(res.codes, res.scales)), bits(res.Q))
    assert np.array_equal(bits(mx_model.dequantize_model(res.codes, res.scales)), bits(res.Q))


def test_given_scales_and_the_grouped_path_agree():
    from sleekit_amd import groups, mx

    W, H, S = case_inputs(6)
    a = mx.quantize_mxfp4(W, H, scale_mode="max")
    b = mx.quantize_mxfp4(W, H, scales=a.S)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    Q, idx = groups.quantize_grouped(W, a.S, mx.E2M1, H, 32, return_indices=True)
    assert np.array_equal(bits(Q), bits(a.Q)) and np.array_equal(idx, a.idx)
    with pytest.raises(ValueError):
        mx.quantize_mxfp4(W, H, scales=a.S * np.float32(1.5))


# ---------------------------------------------------------------------------------------------------------------- pack
@pytest.mark.parametrize("R,n,seed", [(1, 32, 1), (5, 64, 2), (33, 96, 3), (257, 1056, 4), (600, 4096, 5), (64, 16384, 6)])
def test_pack_unpack_dequantize_follow_the_model(R, n, seed):
    from sleekit_amd import mx, packing

    rng = np.random.default_rng(9100 + seed)
    idx = rng.integers(0, 15, (R, n)).astype(np.uint8)
    E = rng.integers(71, 254, (R, n // 32)).astype(np.uint8)
    E.reshape(-1)[:4] = [0, 1, 254, 127][: min(4, E.size)]
    S = mx_model.decode_model(E)
    S_pack = np.where(E == 0, np.float32(1), S)  # 2^-127 is a denormal float32: a scale byte 0 can be read, not written
    idx_d = torch.from_numpy(idx).cuda()
    codes, scales = mx.pack_mxfp4(idx_d, torch.from_numpy(S_pack).cuda())
    assert codes.is_cuda and scales.is_cuda and codes.dtype == scales.dtype == torch.uint8
    want_codes = mx_model.pack_model(idx, S_pack)[0]
    assert np.array_equal(host(codes), want_codes)
    assert np.array_equal(host(scales), np.where(E == 0, 127, E))
    # ... the bytes of the generic 4-bit packing applied to the codes
    words = packing.pack_indices(torch.from_numpy(mx_model.codes_of(idx)).cuda(), 4)
    assert np.array_equal(host(words).view(np.uint8).reshape(R, -1), host(codes))
    assert np.array_equal(pack_bits(mx_model.codes_of(idx), 4).view(np.uint8).reshape(R, -1), host(codes))
    E_d = torch.from_numpy(E).cuda()
    back_idx, back_S = mx.unpack_mxfp4(codes, E_d)
    assert back_idx.is_cuda and torch.equal(back_idx, idx_d) and np.array_equal(bits(back_S), bits(S))
    want = mx_model.dequantize_model(want_codes, E)
    got = mx.dequantize_mxfp4(codes, E_d)
    assert got.is_cuda and got.dtype == torch.float32 and np.array_equal(bits(got), bits(want))
    for dtype in (torch.bfloat16, torch.float16):
        low = mx.dequantize_mxfp4(codes, E_d, dtype=dtype)
        assert low.dtype == dtype and torch.equal(low.view(torch.int16), got.to(dtype).view(torch.int16)), dtype
    # NumPy in, NumPy out
    c2, s2 = mx.pack_mxfp4(idx, S_pack)
    assert isinstance(c2, np.ndarray) and np.array_equal(c2, want_codes)
    i2, S2 = mx.unpack_mxfp4(c2, E)
    assert isinstance(i2, np.ndarray) and np.array_equal(i2, idx) and np.array_equal(bits(S2), bits(S))
    assert np.array_equal(bits(mx.dequantize_mxfp4(c2, E)), bits(want))
    assert mx.dequantize_mxfp4(c2, E, dtype=torch.float16).dtype == np.float16


def test_known_answers_on_the_device():
    from sleekit_amd import mx

    idx = np.full((1, 32), 7, np.uint8)
    idx[0, :15] = np.arange(15)
    codes, scales = mx.pack_mxfp4(idx, np.array([[0.0078125]], np.float32))
    assert "".join(f"{c:x}" for c in mx_model.nibbles(codes)[0, :15]) == "fedcba901234567" and scales.tolist() == [[120]]
    idx[0, :4] = mx_model.indices_of(np.array([1, 2, 0xF, 0]))
    assert mx.pack_mxfp4(idx, np.ones((1, 1), np.float32))[0][0, :2].tolist() == [0x21, 0x0F]
    assert mx.encode_scales(np.array([[0.0078125, 1.0, 2.0 ** -56, 2.0 ** 126]], np.float32)).tolist() == [[120, 127, 71, 253]]
    assert mx.decode_scales(np.array([[120, 127, 0]], np.uint8)).tolist() == [[0.0078125, 1.0, 2.0 ** -127]]
    # an index above 14 is stored as code 7; code 0x8 reads back as index 7, value +0
    wide = np.full((1, 32), 200, np.uint8)
    wide[0, 1] = 15
    assert (mx_model.nibbles(mx.pack_mxfp4(wide, np.ones((1, 1), np.float32))[0]) == 7).all()
    minus_zero = np.full((1, 16), 0x88, np.uint8)
    one = np.full((1, 1), 127, np.uint8)
    assert (mx.unpack_mxfp4(minus_zero, one)[0] == 7).all()
    assert not bits(mx.dequantize_mxfp4(minus_zero, one)).any()


def test_refusals():
    from sleekit_amd import mx

    idx = torch.zeros((4, 64), dtype=torch.uint8, device="cuda")
    for bad in (3.0, 0.0, -1.0, float("inf"), float("nan"), 2.0 ** -127, 1.0000001):
        S = torch.ones((4, 2), device="cuda")
        S[2, 1] = bad
        with pytest.raises(ValueError, match="powers of two"):
            mx.pack_mxfp4(idx, S)
        with pytest.raises(ValueError, match="powers of two"):
            mx.encode_scales(S)
    codes = torch.zeros((4, 32), dtype=torch.uint8, device="cuda")
    E = torch.full((4, 2), 127, dtype=torch.uint8, device="cuda")
    E[3, 0] = 255
    for call in (lambda: mx.unpack_mxfp4(codes, E), lambda: mx.dequantize_mxfp4(codes, E), lambda: mx.decode_scales(E),
                 lambda: mx.dequantize_mxfp4(codes, E, dtype=torch.bfloat16)):
        with pytest.raises(ValueError, match="255"):
            call()
    W = torch.zeros((4, 48), device="cuda")
    with pytest.raises(ValueError, match="32"):
        mx.compute_mx_scales(W)
    with pytest.raises(ValueError, match="32"):
        mx.quantize_mxfp4(W, torch.eye(48, device="cuda"))
    with pytest.raises(ValueError, match="32"):
        mx.pack_mxfp4(torch.zeros((4, 48), dtype=torch.uint8, device="cuda"), torch.ones((4, 1), device="cuda"))
    with pytest.raises(ValueError):
        mx.compute_mx_scales(torch.zeros((4, 64), device="cuda"), mode="diag")


def test_unaligned_views_are_handled():
    from sleekit_amd import mx

    rng = np.random.default_rng(5)
    idx = rng.integers(0, 15, (6, 64)).astype(np.uint8)
    buf = torch.zeros(6 * 64 + 3, dtype=torch.uint8, device="cuda")
    view = buf[3:].view(6, 64)
    view.copy_(torch.from_numpy(idx))
    S = torch.ones((6, 2), device="cuda")
    codes, scales = mx.pack_mxfp4(view, S)
    assert np.array_equal(host(codes), mx_model.pack_model(idx, np.ones((6, 2), np.float32))[0])
    cbuf = torch.zeros(6 * 32 + 5, dtype=torch.uint8, device="cuda")
    cview = cbuf[5:].view(6, 32)
    cview.copy_(codes)
    assert torch.equal(mx.unpack_mxfp4(cview, scales)[0], view)
    assert torch.equal(mx.dequantize_mxfp4(cview, scales), mx.dequantize_mxfp4(codes, scales))


# ---------------------------------------------------------------------------------------------------------------- Sleekit
@pytest.mark.parametrize("bias_correction,moves", [(False, 0), (True, 0), (True, 10)])
def test_sleekit_layer(bias_correction, moves):
    import torch.nn as nn

    from sleekit_amd import Sleekit, _device as dev, _lib, mx

    torch.manual_seed(3)
    layer = nn.Linear(256, 96).cuda()
    W = layer.weight.data.clone().float()
    bias = layer.bias.data.clone()
    st = Sleekit(layer)
    for _ in range(3):
        st.add_batch(torch.randn(64, 256, device="cuda") + 0.3)
    res = st.quantize_mxfp4(scale_mode="diag", order_mode="sqerr", bias_correction=bias_correction, damp=0.03, nb_ls_moves=moves)
    H = st.hessian
    if bias_correction:
        H = torch.empty_like(st.hessian)
        _lib.check(_lib.lib.slk_hessian_strip_mean(dev.ptr(st.hessian), dev.ptr(st.mean), 256, dev.ptr(H), dev.stream_handle()))
    want = mx.quantize_mxfp4(W, H, "sqerr", 0.03, "diag", moves)
    assert want.codes.is_cuda and torch.equal(res.codes, want.codes) and torch.equal(res.scales, want.scales)
    assert torch.equal(res.S, want.S) and torch.equal(res.idx, want.idx)
    assert res.codes.shape == (96, 128) and res.scales.shape == (96, 8)
    assert np.array_equal(bits(layer.weight.data), bits(want.Q))
    assert np.array_equal(bits(mx.dequantize_mxfp4(res.codes, res.scales)), bits(layer.weight.data))
    shift = ((W - want.Q) * st.mean).sum(dim=1) if bias_correction else torch.zeros_like(bias)
    assert torch.equal(layer.bias.data, bias + shift)
    assert bias_correction is False or shift.abs().max() > 0


def test_sleekit_quantize_keeps_its_refusals():
    import torch.nn as nn

    from sleekit_amd import Sleekit

    st = Sleekit(nn.Linear(64, 8).cuda())
    st.add_batch(torch.randn(32, 64, device="cuda"))
    with pytest.raises(NotImplementedError):
        st.quantize(4, group_size=32, nb_ls_moves=5)
    layer = nn.Linear(48, 8).cuda()
    st = Sleekit(layer)
    st.add_batch(torch.randn(32, 48, device="cuda"))
    with pytest.raises(ValueError, match="32"):
        st.quantize_mxfp4()


# ---------------------------------------------------------------------------------------------------------------- scale
def test_4096_layer_round_trip():
    from sleekit_amd import mx, synth

    L = synth.make_layer_device(4096, 4096, 9301, "cuda")
    res = mx.quantize_mxfp4(L["W"], L["H"], scale_mode="diag")
    assert all(t.is_cuda for t in res) and res.codes.shape == (4096, 2048) and res.scales.shape == (4096, 128)
    assert torch.equal(mx.dequantize_mxfp4(res.codes, res.scales).view(torch.int32), res.Q.view(torch.int32))
    assert torch.equal(mx.dequantize_mxfp4(res.codes, res.scales, dtype=torch.bfloat16).view(torch.int16),
                       res.Q.to(torch.bfloat16).view(torch.int16))
    idx, S = mx.unpack_mxfp4(res.codes, res.scales)
    assert torch.equal(idx, res.idx) and torch.equal(S, res.S)
    rows = np.arange(0, 4096, 64)  # (blocks are independent: the model follows a sample of the rows)
    want = mx_model.scales_model(host(L["W"])[rows], host(L["H"]), "diag")[1]
    assert np.array_equal(host(res.scales)[rows], want)
    E = host(res.scales)
    assert E.min() >= 71 and E.max() <= 253
