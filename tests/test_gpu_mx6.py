"""MXFP6 (E2M3) layers on the MI355X: the E2M3 B operand map of the block-scaled MFMA with one-hot data, exact integer
products bit for bit, random data within the derived bound, scale selection, pack, unpack and de-quantize against the NumPy
model (tests/mx6_model.py) bit for bit, whole layers against the reference's own results (tests/golden/mx6.npz), and the
Python surface.

`bound` and the helpers are those of tests/test_gpu_mx_gemm.py (its docstring has the tile sizes the shapes come from):
|y - y64| <= adds * 2^-23 * sum_k |a_k w_k|, the products being exact (4 + 4 significant bits at most).  Largest
|err| / sum |a w| seen on the MI355X: DESIGN.md section 22.
"""

import collections

import numpy as np
import pytest
import torch

import mx6_model as model
import mx_act6_model as act6
import mx_gemm_model as act8
from test_gpu_mx_act4 import K_IN, N_OUT
from test_gpu_mx_act6 import A_INT_CODES, STRADDLERS, one_hot_positions6
from test_gpu_mx_gemm import bits, block_gaussian, bound
from test_mx6_cpu import CASES, FIX, case_inputs, check_codes, check_indices

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
W6 = "mxfp6_e2m3"
ACTS = ["mxfp8", W6]
W_CODES = np.array([c for c in range(64) if c != 0x20], np.uint8)  # the 63 values; 0x20 (-0) is never written


@pytest.fixture(scope="module", autouse=True)
def gpu():
    assert torch.cuda.is_available(), "these tests need the GPU"
    torch.cuda.set_device(0)


def host(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t


def fbits(a):
    return np.ascontiguousarray(host(a), dtype=np.float32).view(np.uint32)


def random_weights(rng, N, K, lo, hi):
    return act6.pack_codes(W_CODES[rng.integers(0, 63, (N, K))]), rng.integers(lo, hi + 1, (N, K // 32)).astype(np.uint8)


def act_model(X, activations):
    """(a_codes, a_scales, the de-quantized values as float64) of X by the model of the activation format."""
    if activations == W6:
        c, s = act6.quantize_act6_model(X)
        return c, s, act6.dequantize_act6_model(c, s)
    c, s = act8.quantize_act_model(X)
    return c, s, act8.dequantize_act_model(c, s)


def act_values(a_codes, a_scales, activations):
    return act6.dequantize_act6_model(a_codes, a_scales) if activations == W6 else act8.dequantize_act_model(a_codes, a_scales)


def act_pack(codes, activations):
    return act6.pack_codes(codes) if activations == W6 else codes


# ---------------------------------------------------------------------------------------------------------------- 1. map
@pytest.mark.parametrize("activations", ACTS)
@pytest.mark.parametrize("M,N,K", [(16, 16, 128), (17, 33, 160)])
def test_operand_map_one_hot(M, N, K, activations):
    """One non-zero E2M3 code in W and one non-zero code in A: y[m][n] = a w s_a s_w exactly when the two k agree, and zero
    everywhere else.  Every (row, block) has its own scale byte on both sides.  The partners: k ^ 1 catches swapped
    neighbours, k ^ 16 the other 12-byte half of the block, k + 32 swapped blocks; the W codes 0x15 and 0x2a differ in every
    bit, 0x01 and 0x3f are the lowest bit alone and all six, so a reversed or shifted bit order inside an element changes the
    value.  The positions include the elements of the first and of the last block whose 6 bits straddle or start a dword."""
    from sleekit_amd import mx

    assert set(STRADDLERS) == {4, 5, 6, 10, 11, 15, 16, 17, 21, 26}
    rng = np.random.default_rng(11)
    a_scales = rng.permutation(np.arange(M * (K // 32)) % 23 + 116).reshape(M, K // 32).astype(np.uint8)
    w_scales = rng.permutation(np.arange(N * (K // 32)) % 19 + 118).reshape(N, K // 32).astype(np.uint8)
    a_hot = (0x15, 0x2a) if activations == W6 else (0x3c, 0xc9)
    w_hot = (0x15, 0x2a, 0x01, 0x3f)
    for i, (m, n, k) in enumerate(one_hot_positions6(M, N, K)):
        if k // 32 + 1 < K // 32:  # the block's right-hand neighbours differ from it on both sides
            a_scales[m, k // 32 + 1] = a_scales[m, k // 32] + 3
            w_scales[n, k // 32 + 1] = w_scales[n, k // 32] - 2
        for j, k2 in enumerate((k, k, (k + 32) % K, k ^ 1, k ^ 16)):
            a_code, w_code = a_hot[j % 2], w_hot[(i + j) % 4]
            a = np.zeros((M, K), np.uint8)
            w = np.zeros((N, K), np.uint8)
            a[m, k] = a_code
            w[n, k2] = w_code
            got = mx.matmul_mx(act_pack(a, activations), a_scales, act6.pack_codes(w), w_scales, activations=activations, weights=W6)
            want = np.zeros((M, N), np.float64)
            if k2 == k:
                av = float(act6.e2m3_decode(a_code) if activations == W6 else act8.e4m3_decode(a_code))
                want[m, n] = (av * 2.0 ** (int(a_scales[m, k // 32]) - 127)) * (float(act6.e2m3_decode(w_code)) * 2.0 ** (int(w_scales[n, k // 32]) - 127))
            hot = np.argwhere(got != 0)
            assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64), want), (
                f"A[{m}][{k}] = {a_code:#x}, W[{n}][{k2}] = {w_code:#x}: want y[{m}][{n}] = {want[m, n]!r}, got non-zeros at "
                f"{hot.tolist()[:8]} = {got[got != 0].tolist()[:8]}")


# ---------------------------------------------------------------------------------------------------------------- 2. exact
# M = 1, 16, 17, 64 (split-K), 65 (tiled); N = 1, 15, 33; K = 32, 160 (no multiple of 128), 2176 (past one split-K pass of 2048)
EXACT_SHAPES = [(1, 1, 32), (16, 15, 160), (17, 33, 2176), (64, 33, 160), (65, 15, 2176), (65, 33, 32), (1, 33, 2176),
                (16, 1, 160), (64, 15, 2176), (17, 1, 32), (65, 1, 160)]


@pytest.mark.parametrize("activations", ACTS)
@pytest.mark.parametrize("M,N,K", EXACT_SHAPES)
def test_exact_integers_bit_for_bit(M, N, K, activations):
    from sleekit_amd import mx

    assert sorted(act6.e2m3_decode(A_INT_CODES).tolist()) == list(range(-7, 8))  # 0, +-1 .. +-7
    rng = np.random.default_rng(M * 1000 + N * 7 + K)
    w_codes = act6.pack_codes(A_INT_CODES[rng.integers(0, len(A_INT_CODES), (N, K))])
    w_scales = (127 + rng.integers(-1, 2, (N, K // 32))).astype(np.uint8)
    if activations == W6:
        a_codes = act6.pack_codes(A_INT_CODES[rng.integers(0, len(A_INT_CODES), (M, K))])
    else:
        a_codes = act8.e4m3_encode(rng.integers(-7, 8, (M, K)).astype(np.float64))
    a_scales = (127 + rng.integers(-1, 2, (M, K // 32))).astype(np.uint8)
    bias = (rng.integers(-64, 65, N) / 8.0).astype(np.float32)
    # the test's own inputs make every order of float32 additions exact: A and W are multiples of 1 / 2 of magnitude at most
    # 14, so all terms are multiples of 1 / 4 of magnitude at most 196 and, with the bias, every partial sum is a multiple of
    # q = 2^-3 below 2^24 q = 2^21
    A, W = act_values(a_codes, a_scales, activations), model.dequantize_model(w_codes, w_scales).astype(np.float64)
    assert np.abs(A).max() <= 14 and np.abs(W).max() <= 14 and (A * 2 == np.rint(A * 2)).all() and (W * 2 == np.rint(W * 2)).all()
    assert K * 196 + 8 < 2 ** 21
    for b in (None, bias):
        want, _ = model.matmul_model(A, w_codes, w_scales, b)
        assert (want == want.astype(np.float32)).all()
        for dtype in DTYPES:
            got = mx.matmul_mx(torch.from_numpy(a_codes).cuda(), a_scales, w_codes, w_scales, b, dtype=dtype, activations=activations, weights=W6)
            assert tuple(got.shape) == (M, N) and got.dtype == dtype
            ref = torch.from_numpy(want.astype(np.float32)).to(dtype)
            wrong = np.argwhere(bits(got) != bits(ref))
            assert wrong.size == 0, (f"{dtype}, bias {b is not None}: {len(wrong)} of {M * N} differ, first at {wrong[:4].tolist()}: got "
                                     f"{got[tuple(wrong[0])].item()}, want {want[tuple(wrong[0])]}")


# ---------------------------------------------------------------------------------------------------------------- 3. bound
@pytest.mark.parametrize("activations", ACTS)
@pytest.mark.parametrize("M,N,K", [(17, 33, 160), (64, 80, 1024)])
def test_random_data_within_the_bound(M, N, K, activations):
    from sleekit_amd import mx

    rng = np.random.default_rng(K + M)
    a_codes, a_scales, A = act_model(block_gaussian(rng, M, K), activations)
    w_codes, w_scales = random_weights(rng, N, K, 118, 123)
    bias = rng.standard_normal(N).astype(np.float32)
    want, sum_abs = model.matmul_model(A, w_codes, w_scales)
    got = mx.matmul_mx(a_codes, a_scales, w_codes, w_scales, activations=activations, weights=W6).astype(np.float64)
    err = np.abs(got - want)
    print(f"mx_gemm_w6 {activations} {M}x{N}x{K}: max |err| / sum|aw| = {(err / sum_abs).max():.3e} (bound {K * 2.0 ** -23:.3e})")
    assert (err <= bound(K, sum_abs)).all(), (err / sum_abs).max()
    got = mx.matmul_mx(a_codes, a_scales, w_codes, w_scales, bias, activations=activations, weights=W6).astype(np.float64)
    assert (np.abs(got - (want + bias)) <= bound(K + 1, sum_abs + np.abs(bias)[None, :])).all()


# ---------------------------------------------------------------------------------------------------------------- 4. format
LIMITS = ((np.array(model.VALUES[:-1]) + np.array(model.VALUES[1:])) / 2).astype(np.float32)  # the 62 limits of the table


def fuzz_layer(rng, R, n):
    """Blocks of a few magnitudes: zeros, negative only, one outlier, amax exactly 7.5 * 2^e with the rest on limits of some
    candidate scale, and plain Gaussian ones; a positive diagonal."""
    W = block_gaussian(rng, R, n)
    blocks = W.reshape(R * (n // 32), 32)  # a view: edits land in W
    for b in range(len(blocks)):
        kind = b % 6
        if kind == 1:
            blocks[b] = 0
        elif kind == 2:
            blocks[b] = -np.abs(blocks[b]) - 1e-3
        elif kind == 3:
            blocks[b, rng.integers(0, 32)] *= np.float32(8 << (b % 4))
        elif kind == 4:
            e = np.float32(2.0 ** rng.integers(-6, 7))
            f = np.float32(2.0 ** -rng.integers(0, 4))  # the limits of the candidate f * base
            blocks[b] = np.resize(rng.permutation(LIMITS), 32) * e * f
            blocks[b, rng.integers(0, 32)] = np.float32(7.5) * e * (1 if b % 2 else -1)
    H = np.diag(rng.uniform(0.05, 4.0, n).astype(np.float32)) + np.float32(0.01)
    return W, H.astype(np.float32)


SHAPES = [(1, 32), (3, 96), (17, 160), (9, 288)]  # 96, 160: rows on 8 bytes, not on 16; 288: 9 blocks, the wave's repeated tail


@pytest.mark.parametrize("R,n", SHAPES)
def test_scales_follow_the_model(R, n):
    from sleekit_amd import mx

    W, H = fuzz_layer(np.random.default_rng(R + n), R, n)
    Wd, Hd = torch.from_numpy(W).cuda(), torch.from_numpy(H).cuda()
    for mode in ("max", "mse", "diag"):
        want_S, want_E, found = model.scales_model(W, H, mode, want_found=True)
        assert found.all()
        S, E = mx.compute_mx_scales(Wd, Hd, mode, weights=W6)
        assert S.is_cuda and E.dtype == torch.uint8 and tuple(E.shape) == (R, n // 32)
        wrong = np.argwhere(host(E) != want_E)
        assert wrong.size == 0, (mode, wrong[:4].tolist(), host(E)[tuple(wrong[0])], want_E[tuple(wrong[0])])
        assert np.array_equal(fbits(S), fbits(want_S))
        S2, E2 = mx.compute_mx_scales(W, H, mode, weights=W6)  # NumPy in, NumPy out
        assert isinstance(E2, np.ndarray) and np.array_equal(E2, want_E) and np.array_equal(fbits(S2), fbits(want_S))


@pytest.mark.parametrize("R,n", SHAPES)
def test_pack_unpack_dequantize_follow_the_model(R, n):
    from sleekit_amd import mx

    rng = np.random.default_rng(9100 + R + n)
    idx = rng.integers(0, 63, (R, n)).astype(np.uint8)
    idx.reshape(-1)[:3] = [0, 62, 31]
    E = rng.integers(71, 254, (R, n // 32)).astype(np.uint8)
    E.reshape(-1)[-1] = 1
    S = model.decode_model(E)
    idx_d, E_d = torch.from_numpy(idx).cuda(), torch.from_numpy(E).cuda()
    codes, scales = mx.pack_mxfp6(idx_d, torch.from_numpy(S).cuda())
    want_codes = model.pack_model(idx, S)[0]
    assert codes.is_cuda and codes.dtype == scales.dtype == torch.uint8 and tuple(codes.shape) == (R, 3 * n // 4)
    assert np.array_equal(host(codes), want_codes) and np.array_equal(host(scales), E)
    back_idx, back_S = mx.unpack_mxfp6(codes, E_d)
    assert torch.equal(back_idx, idx_d) and np.array_equal(fbits(back_S), fbits(S))
    want = model.dequantize_model(want_codes, E)
    got = mx.dequantize_mxfp6(codes, E_d)
    assert got.is_cuda and got.dtype == torch.float32 and np.array_equal(fbits(got), fbits(want))
    for dtype in (torch.bfloat16, torch.float16):
        low = mx.dequantize_mxfp6(codes, E_d, dtype=dtype)
        assert low.dtype == dtype and torch.equal(low.view(torch.int16), got.to(dtype).view(torch.int16)), dtype
    # the values are the codebook's: Q = values[idx] / (1 / s)
    s = np.repeat(S, 32, axis=1)
    with np.errstate(over="ignore"):  # (7.5 * 2^127 is +inf in float32, as it is on the device)
        assert np.array_equal(fbits(want), fbits((mx.E2M3.values[idx].astype(np.float32) / (np.float32(1) / s)).astype(np.float32)))
    # NumPy in, NumPy out; a view off 16 bytes
    c2, s2 = mx.pack_mxfp6(idx, S)
    assert isinstance(c2, np.ndarray) and np.array_equal(c2, want_codes) and np.array_equal(s2, E)
    i2, S2 = mx.unpack_mxfp6(c2, E)
    assert isinstance(i2, np.ndarray) and np.array_equal(i2, idx) and np.array_equal(fbits(S2), fbits(S))
    assert np.array_equal(fbits(mx.dequantize_mxfp6(c2, E)), fbits(want))
    buf = torch.zeros(codes.numel() + 5, dtype=torch.uint8, device="cuda")
    view = buf[5:].view(R, 3 * n // 4)
    view.copy_(codes)
    assert torch.equal(mx.unpack_mxfp6(view, E_d)[0], idx_d) and torch.equal(mx.dequantize_mxfp6(view, E_d), got)


def test_known_answers_and_refusals_on_the_device():
    from sleekit_amd import mx

    idx = np.full((1, 32), 31, np.uint8)
    idx[0, :7] = [0, 1, 30, 31, 32, 61, 62]
    codes, scales = mx.pack_mxfp6(idx, np.array([[0.0078125]], np.float32))
    assert " ".join(f"{c:02x}" for c in act6.unpack_codes(codes)[0, :7]) == "3f 3e 21 00 01 1e 1f" and scales.tolist() == [[120]]
    idx[0, :4] = model.indices_of(np.array([1, 2, 0x3f, 0]))
    assert mx.pack_mxfp6(idx, np.ones((1, 1), np.float32))[0][0, :3].tolist() == [0x81, 0xf0, 0x03]
    idx[0, :4] = [0, 62, 31, 32]
    assert mx.pack_mxfp6(idx, np.ones((1, 1), np.float32))[0][0, :3].tolist() == [0xff, 0x07, 0x04]
    # an index above 62 is stored as code 0x1f; code 0x20 reads back as index 31
    wide = np.full((1, 32), 200, np.uint8)
    wide[0, 1] = 63
    assert (act6.unpack_codes(mx.pack_mxfp6(wide, np.ones((1, 1), np.float32))[0]) == 0x1f).all()
    minus_zero = act6.pack_codes(np.full((1, 32), 0x20, np.uint8))
    one = np.full((1, 1), 127, np.uint8)
    assert (mx.unpack_mxfp6(minus_zero, one)[0] == 31).all()
    idx_d = torch.zeros((4, 64), dtype=torch.uint8, device="cuda")
    for bad in (3.0, 0.0, -1.0, float("inf"), float("nan"), 2.0 ** -127, 1.0000001):
        S = torch.ones((4, 2), device="cuda")
        S[2, 1] = bad
        with pytest.raises(ValueError, match="powers of two"):
            mx.pack_mxfp6(idx_d, S)
        with pytest.raises(ValueError, match="powers of two"):
            mx.quantize_mxfp6(torch.zeros((4, 64), device="cuda"), torch.eye(64, device="cuda"), scales=S)
    codes = torch.zeros((4, 48), dtype=torch.uint8, device="cuda")
    E = torch.full((4, 2), 127, dtype=torch.uint8, device="cuda")
    E[3, 0] = 255
    for call in (lambda: mx.unpack_mxfp6(codes, E), lambda: mx.dequantize_mxfp6(codes, E),
                 lambda: mx.dequantize_mxfp6(codes, E, dtype=torch.bfloat16)):
        with pytest.raises(ValueError, match="255"):
            call()


# ---------------------------------------------------------------------------------------------------------------- 5. layers
@pytest.mark.parametrize("i", range(len(CASES)))
def test_quantize_equals_the_reference(i):
    from sleekit_amd import mx

    c = CASES[i]
    W, H, S = case_inputs(i)
    got_S, got_E = mx.compute_mx_scales(W, H, c["mode"], weights=W6)
    assert np.array_equal(got_E, FIX[f"E_{i}"]) and np.array_equal(fbits(got_S), fbits(S)), f"case {i}: {c}"
    res = mx.quantize_mxfp6(W, H, c["act_order"], c["damp"], c["mode"], c["moves"], None, c["min_block_size"], c["num_blocks"])
    assert np.array_equal(res.scales, FIX[f"E_{i}"]) and np.array_equal(fbits(res.S), fbits(S))
    trace = None
    if c["moves"]:
        Wd, Hd = torch.from_numpy(W).cuda(), torch.from_numpy(H).cuda()
        packed, layer = mx.quantize_layer_mxfp6(Wd, Hd, c["act_order"], c["damp"], c["mode"], c["moves"], want_ls_trace=True)
        assert torch.equal(packed.idx.cpu(), torch.from_numpy(res.idx))
        trace = layer.ls_trace.cpu().numpy()
        loop = mx.quantize_mxfp6(W, H, c["act_order"], c["damp"], c["mode"], 0)  # ... and after the loop alone
        from test_mx_cpu import sha

        assert sha(loop.idx) == c["sha256_idx0"]
    bad = check_indices(i, res.idx, trace)
    check_codes(i, res.codes, bad)
    codes, E = model.pack_model(res.idx, res.S)
    assert res.codes.shape == (c["R"], 3 * c["n"] // 4) and np.array_equal(res.codes, codes) and np.array_equal(res.scales, E)
    assert np.array_equal(fbits(mx.dequantize_mxfp6(res.codes, res.scales)), fbits(res.Q))
    assert np.array_equal(fbits(model.dequantize_model(res.codes, res.scales)), fbits(res.Q))


def test_layer_error_is_below_mxfp4s():
    from sleekit_amd import mx, obq, synth

    L = synth.make_layer(64, 256, 4242)
    e4 = float(obq.quantization_error(L["W"], mx.quantize_mxfp4(L["W"], L["H"]).Q, L["H"]))
    e6 = float(obq.quantization_error(L["W"], mx.quantize_mxfp6(L["W"], L["H"]).Q, L["H"]))
    print(f"layer error 64 x 256: MXFP4 {e4:.6g}, MXFP6 {e6:.6g}, ratio {e6 / e4:.4f}")
    assert 0 < e6 < e4


# ---------------------------------------------------------------------------------------------------------------- 6. surface
@pytest.fixture(scope="module")
def layer():
    rng = np.random.default_rng(77)
    codes, scales = (torch.from_numpy(t).cuda() for t in random_weights(rng, N_OUT, K_IN, 118, 123))
    return codes, scales, torch.from_numpy(rng.standard_normal(N_OUT).astype(np.float32)).cuda()


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


@pytest.mark.parametrize("activations", ACTS)
def test_linear_mxfp6(layer, activations):
    from sleekit_amd import mx

    codes, scales, bias = layer
    for dtype in DTYPES:
        x = torch.from_numpy(block_gaussian(np.random.default_rng(3), 6, K_IN)).reshape(2, 3, K_IN).to(dtype).cuda()
        want_codes, want_scales, A = act_model(x.float().cpu().numpy().reshape(6, K_IN), activations)
        for out in DTYPES:
            y = mx.linear_mxfp6(x, codes, scales, bias, dtype=out, activations=activations)
            assert y.is_cuda and y.dtype == out and tuple(y.shape) == (2, 3, N_OUT)
            assert same_bits(y.reshape(6, N_OUT), mx.matmul_mx(torch.from_numpy(want_codes).cuda(), torch.from_numpy(want_scales).cuda(), codes,
                                                             scales, bias, dtype=out, activations=activations, weights=W6))
        y = mx.linear_mxfp6(x, codes, scales, bias, activations=activations)  # the output dtype follows x
        assert same_bits(y, mx.linear_mxfp6(x, codes, scales, bias, dtype=dtype, activations=activations))
        y32 = mx.linear_mxfp6(x, codes, scales, bias, dtype=torch.float32, activations=activations)
        want, sum_abs = model.matmul_model(A, host(codes), host(scales), host(bias))
        got = host(y32).reshape(6, N_OUT).astype(np.float64)
        assert (np.abs(got - want) <= bound(K_IN + 1, sum_abs + np.abs(host(bias))[None, :])).all()
        if dtype != torch.bfloat16:  # NumPy in, NumPy out
            z = mx.linear_mxfp6(host(x), host(codes), host(scales), host(bias), activations=activations)
            assert isinstance(z, np.ndarray) and np.array_equal(bits(z), bits(y))
    assert tuple(mx.linear_mxfp6(x[0, 0], codes, scales, activations=activations).shape) == (N_OUT,)


@pytest.mark.parametrize("activations", ACTS)
def test_linear_with_a_rotation(layer, activations):
    from sleekit_amd import mx, rotation

    codes, scales, bias = layer
    rot = rotation.Rotation(K_IN, seed=3)
    for dtype in DTYPES:
        x = torch.from_numpy(block_gaussian(np.random.default_rng(4), 6, K_IN)).reshape(2, 3, K_IN).to(dtype).cuda()
        for out in DTYPES:
            got = mx.linear_mxfp6(x, codes, scales, bias, dtype=out, activations=activations, rotation=rot)
            want = mx.linear_mxfp6(rot.apply(x, dtype=torch.float32), codes, scales, bias, dtype=out, activations=activations)
            assert tuple(got.shape) == (2, 3, N_OUT) and same_bits(got, want), (dtype, out)
        assert mx.linear_mxfp6(x, codes, scales, bias, activations=activations, rotation=rot).dtype == dtype


Result = collections.namedtuple("Result", "codes scales rotation")


def test_modules(layer):
    import torch.nn as nn

    from sleekit_amd import MXLinear, mx, rotation
    from sleekit_amd.rotation import RotatedLinear

    codes, scales, bias = layer
    rot = rotation.Rotation(K_IN, seed=6)
    lin = nn.Linear(K_IN, N_OUT).cuda()
    lin.bias.data.copy_(bias)
    res = Result(codes, scales, rot)
    x = torch.from_numpy(block_gaussian(np.random.default_rng(5), 10, K_IN)).reshape(2, 5, K_IN).cuda()
    for activations in ACTS:
        m = MXLinear.from_result(lin, res, activations=activations)
        assert m.weights == W6 and m.activations == activations and tuple(m.codes.shape) == (N_OUT, 3 * K_IN // 4)
        for t in (x, x.bfloat16(), x.half()):
            assert same_bits(m(t), mx.linear_mxfp6(t, codes, scales, bias, activations=activations))
        # the state dict round trip, on the device
        copy = MXLinear(K_IN, N_OUT, weights=W6).cuda()
        copy.load_state_dict(m.state_dict())
        assert copy.activations == activations and copy.weights == W6 and same_bits(copy(x), m(x))
        # an MXFP6 state loaded into an MXFP4 module is an error, not a silent reshape
        fp4 = MXLinear(K_IN, N_OUT).cuda()
        before = fp4.codes.clone()
        with pytest.raises(RuntimeError):
            fp4.load_state_dict(m.state_dict())
        assert fp4.weights == "mxfp4" and torch.equal(fp4.codes, before) and tuple(fp4.codes.shape) == (N_OUT, K_IN // 2)
        # RotatedLinear: plain and fused
        plain = RotatedLinear.from_result(lin, res, activations=activations)
        fused = RotatedLinear.from_result(lin, res, fused=True, activations=activations)
        assert not plain.fused and fused.fused and plain.inner.weights == fused.inner.weights == W6
        for t in (x, x.bfloat16(), x.half()):
            assert same_bits(plain(t), m(rot.apply(t)))
            assert same_bits(fused(t), mx.linear_mxfp6(t, codes, scales, bias, activations=activations, rotation=rot))
            assert same_bits(fused(t), mx.linear_mxfp6(rot.apply(t, dtype=torch.float32), codes, scales, bias, dtype=t.dtype, activations=activations))
        assert same_bits(fused(x), plain(x))
        other = RotatedLinear(MXLinear(K_IN, N_OUT, weights=W6).cuda(), rotation.Rotation(K_IN, block=16, seed=1))
        other.load_state_dict(fused.state_dict())
        assert other.fused and other.block == rot.block and other.inner.activations == activations and same_bits(other(x.half()), fused(x.half()))
    # a default module keeps exactly its keys
    assert sorted(MXLinear(K_IN, N_OUT).cuda().state_dict()) == ["bias", "codes", "scales"]
    assert not torch.equal(MXLinear.from_result(lin, res)(x), MXLinear.from_result(lin, res, activations=W6)(x))


def test_sleekit_layer():
    import torch.nn as nn

    from sleekit_amd import MXLinear, Sleekit, mx, rotation

    torch.manual_seed(3)
    layer = nn.Linear(256, 96).cuda()
    W = layer.weight.data.clone().float()
    st = Sleekit(layer)
    for _ in range(3):
        st.add_batch(torch.randn(64, 256, device="cuda") + 0.3)
    res = st.quantize_mxfp6(scale_mode="diag", order_mode="sqerr", damp=0.03, nb_ls_moves=10)
    want = mx.quantize_mxfp6(W, st.hessian, "sqerr", 0.03, "diag", 10)
    assert want.codes.is_cuda and torch.equal(res.codes, want.codes) and torch.equal(res.scales, want.scales)
    assert torch.equal(res.S, want.S) and torch.equal(res.idx, want.idx)
    assert res.codes.shape == (96, 192) and res.scales.shape == (96, 8)
    assert np.array_equal(fbits(layer.weight.data), fbits(want.Q))
    assert np.array_equal(fbits(mx.dequantize_mxfp6(res.codes, res.scales)), fbits(layer.weight.data))
    m = MXLinear.from_result(layer, res, activations=W6)
    x = torch.randn(5, 256, device="cuda")
    assert m.weights == W6 and same_bits(m(x), mx.linear_mxfp6(x, res.codes, res.scales, layer.bias.data.float(), activations=W6))
    # with the object's rotation: blocks of rotated features, and RotatedLinear.from_result takes the result
    layer2 = nn.Linear(256, 96).cuda()
    st2 = Sleekit(layer2, rotation=rotation.Rotation(256, seed=2))
    st2.add_batch(torch.randn(64, 256, device="cuda"))
    res2 = st2.quantize_mxfp6()
    r = rotation.RotatedLinear.from_result(layer2, res2, fused=True, activations=W6)
    assert r.inner.weights == W6 and tuple(r(x).shape) == (5, 96)
    st3 = Sleekit(nn.Linear(48, 8).cuda())
    st3.add_batch(torch.randn(32, 48, device="cuda"))
    with pytest.raises(ValueError, match="32"):
        st3.quantize_mxfp6()


@pytest.mark.parametrize("M", [1, 64, 65])
def test_repeated_calls_are_bit_equal(M):
    """M = 1 and 64 run the split-K kernel, 65 the tiled one."""
    from sleekit_amd import mx, rotation

    rng = np.random.default_rng(M)
    N, K = 200, 4128
    x = torch.from_numpy(block_gaussian(rng, M, K)).cuda()
    w_codes, w_scales = (torch.from_numpy(t).cuda() for t in random_weights(rng, N, K, 118, 123))
    rot = rotation.Rotation(K, seed=M)
    for kw in (dict(activations="mxfp8"), dict(activations=W6), dict(activations=W6, rotation=rot)):
        first = mx.linear_mxfp6(x, w_codes, w_scales, **kw)
        for _ in range(3):
            assert torch.equal(mx.linear_mxfp6(x, w_codes, w_scales, **kw).view(torch.int32), first.view(torch.int32))


def test_refusals():
    from sleekit_amd import mx

    codes = torch.zeros((8, 48), dtype=torch.uint8, device="cuda")
    scales = torch.full((8, 2), 127, dtype=torch.uint8, device="cuda")
    x = torch.zeros((4, 64), device="cuda")
    a8, a8s = mx.quantize_mxfp8(x)
    a6, a4 = mx.quantize_mxfp6_act(x)[0], mx.quantize_mxfp4_act(x)[0]
    assert not mx.matmul_mx(a8, a8s, codes, scales, weights=W6).any() and not mx.matmul_mx(a6, a8s, codes, scales, activations=W6, weights=W6).any()
    for call in (lambda: mx.matmul_mx(a8, a8s, codes, scales, weights="mxfp6"),
                 lambda: mx.linear_mxfp6(x, codes, scales, activations="mxfp6"),
                 lambda: mx.matmul_mx(a4, a8s, codes, scales, activations="mxfp4", weights=W6),
                 lambda: mx.linear_mxfp6(x, codes, scales, activations="mxfp4"),
                 lambda: mx.MXLinear(64, 8, activations="mxfp4", weights=W6),
                 lambda: mx.matmul_mx(a8, a8s, codes[:, :36], scales, weights=W6),           # 48 codes: no whole number of blocks
                 lambda: mx.linear_mxfp6(x, codes[:, :32].contiguous(), scales),             # 42.7 codes a row
                 lambda: mx.matmul_mx(a8, a8s, torch.zeros((8, 72), dtype=torch.uint8, device="cuda"),
                                      torch.full((8, 3), 127, dtype=torch.uint8, device="cuda"), weights=W6),   # mismatched K
                 lambda: mx.linear_mxfp6(torch.zeros((4, 96), device="cuda"), codes, scales),
                 lambda: mx.matmul_mx(a8, a8s, codes, scales),                                # 48 bytes a row are 96 columns of MXFP4
                 lambda: mx.linear_mxfp6(x, codes, scales, dtype=torch.float64),
                 lambda: mx.linear_mxfp6(x, codes, scales, bias=torch.zeros(7, device="cuda"))):
        with pytest.raises(ValueError):
            call()
