"""The packed linear layer on the MI355X: the block-scaled MFMA's operand map with one-hot data, exact integer products
bit for bit, random data within a derived bound, the activation quantizer against the NumPy model bit for bit, and the
Python surface end to end.

Tile sizes the shapes were chosen from: up to M = 64 a workgroup is one 16 x 16 tile of Y whose 8
waves take two 128-steps each per pass (2048 columns of K a pass); above, a workgroup is a 64 x 64 tile, 128 columns a step.

The one tolerance of this file is `bound`: |y - y64| <= adds * 2^-23 * sum_k |a_k w_k|, the first-order worst case of
`adds` float32 additions in any order, rounded or truncated (the products themselves are exact: 4 + 2 significant bits).
A misplaced element costs about sum |a w| / sqrt(K), far above it.  Largest |err| / sum |a w| seen on the MI355X:
see DESIGN.md section 12.
"""

import numpy as np
import pytest
import torch

import mx_gemm_model as model
import mx_model

pytestmark = pytest.mark.gpu

W_CODES = np.array([c for c in range(16) if c != 8], np.uint8)  # the 15 values; 0x8 (-0) is never written


def bits(x):
    if isinstance(x, torch.Tensor):  # (NumPy has no bfloat16: the bits leave torch as integers)
        x = x.contiguous().view({2: torch.int16, 4: torch.int32}[x.element_size()]).cpu().numpy()
    x = np.asarray(x)
    return np.ascontiguousarray(x).view({2: np.uint16, 4: np.uint32}[x.dtype.itemsize])


def pack_nibbles(c):
    return (c[:, 0::2] | (c[:, 1::2] << 4)).astype(np.uint8)


def bound(adds, sum_abs):
    return adds * 2.0 ** -23 * sum_abs


def random_weights(rng, N, K, lo, hi):
    return pack_nibbles(W_CODES[rng.integers(0, 15, (N, K))]), rng.integers(lo, hi + 1, (N, K // 32)).astype(np.uint8)


def block_gaussian(rng, M, K):
    """Gaussian data whose blocks of 32 have magnitudes 2^-3 .. 2^3."""
    mag = 2.0 ** rng.integers(-3, 4, (M, K // 32))
    return (rng.standard_normal((M, K)) * np.repeat(mag, 32, axis=1)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- 1. map
def one_hot_positions(M, N, K):
    ks = sorted({k for k in (0, 1, 30, 31, 32, 33, 63, 64, 65, 94, 95, 96, 97, 126, 127, 128, 129, 158, 159) if k < K})
    rows = sorted({0, 5 % M, 15, M - 1})
    cols = sorted({0, 9 % N, 15, 16 % N, N - 1})
    out = []
    for i, k in enumerate(ks):  # every k with a walk over the rows and columns, and the corners at every k-group's ends
        out.append((rows[i % len(rows)], cols[(i // 2) % len(cols)], k))
        if k % 32 in (0, 31):
            out += [(0, 0, k), (M - 1, N - 1, k), (0, N - 1, k), (M - 1, 0, k)]
    return out


@pytest.mark.parametrize("M,N,K", [(16, 16, 128), (17, 33, 160)])
def test_operand_map_one_hot(M, N, K):
    """One non-zero element on each side: y[m][n] = a w s_a s_w exactly when the two k agree, and zero everywhere else.
    Every block has its own scale byte, so a scale taken from a neighbouring block or row changes the answer."""
    from sleekit_amd import mx

    rng = np.random.default_rng(11)
    a_scales = rng.permutation(np.arange(M * (K // 32)) % 23 + 116).reshape(M, K // 32).astype(np.uint8)
    w_scales = rng.permutation(np.arange(N * (K // 32)) % 19 + 118).reshape(N, K // 32).astype(np.uint8)
    for m, n, k in one_hot_positions(M, N, K):
        if k // 32 + 1 < K // 32:  # the block's right-hand neighbours differ from it on both sides
            a_scales[m, k // 32 + 1] = a_scales[m, k // 32] + 3
            w_scales[n, k // 32 + 1] = w_scales[n, k // 32] - 2
        for a_code, w_code, k2 in ((0x3c, 0xd, k), (0xc9, 0x3, k), (0x3c, 0x5, (k + 32) % K), (0x45, 0x7, k ^ 1)):
            a_codes = np.zeros((M, K), np.uint8)
            nib = np.zeros((N, K), np.uint8)
            a_codes[m, k] = a_code
            nib[n, k2] = w_code
            got = mx.matmul_mx(a_codes, a_scales, pack_nibbles(nib), w_scales)
            want = np.zeros((M, N), np.float64)
            if k2 == k:
                a = model.e4m3_decode(a_code) * 2.0 ** (int(a_scales[m, k // 32]) - 127)
                w = mx_model.MAGNITUDES[w_code & 7] * (-1.0 if w_code & 8 else 1.0) * 2.0 ** (int(w_scales[n, k // 32]) - 127)
                want[m, n] = a * w
            hot = np.argwhere(got != 0)
            assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64), want), (
                f"A[{m}][{k}] = {a_code:#x}, W[{n}][{k2}] = {w_code:#x}: want y[{m}][{n}] = {want[m, n]!r}, got non-zeros at "
                f"{hot.tolist()[:8]} = {got[got != 0].tolist()[:8]}")


# ---------------------------------------------------------------------------------------------------------------- 2. exact
EXACT_SHAPES = [(1, 1, 32), (1, 16, 128), (16, 1, 96), (17, 33, 160), (15, 47, 4128), (130, 200, 544),
                (64, 17, 160), (65, 17, 160), (33, 16, 2080)]


@pytest.mark.parametrize("M,N,K", EXACT_SHAPES)
def test_exact_integers_bit_for_bit(M, N, K):
    from sleekit_amd import mx

    rng = np.random.default_rng(M * 1000 + N * 7 + K)
    a_codes = model.e4m3_encode(rng.integers(-4, 5, (M, K)).astype(np.float64))
    a_scales = (127 + rng.integers(-1, 2, (M, K // 32))).astype(np.uint8)
    w_codes, w_scales = random_weights(rng, N, K, 126, 128)
    bias = (rng.integers(-64, 65, N) / 8.0).astype(np.float32) if (M + N) % 2 else None
    # the test's own inputs make every order of float32 additions exact: all terms (and the bias) are multiples of
    # q = 2^-3 of magnitude at most 96, so every partial sum is a multiple of q below 2^24 q
    A, W = model.dequantize_act_model(a_codes, a_scales), model.weights_model(w_codes, w_scales)
    q = 2.0 ** -3
    assert np.abs(A).max() <= 8 and np.abs(W).max() <= 12 and (A * 2 == np.rint(A * 2)).all() and (W * 4 == np.rint(W * 4)).all()
    assert K * 96 + 8 < 2 ** 24 * q
    want, _ = model.matmul_model(a_codes, a_scales, w_codes, w_scales, bias)
    got = mx.matmul_mx(a_codes, a_scales, w_codes, w_scales, bias)
    assert got.shape == (M, N) and got.dtype == np.float32
    wrong = np.argwhere(got.astype(np.float64) != want)
    assert wrong.size == 0, f"{len(wrong)} of {M * N} differ, first at {wrong[:4].tolist()}: got {got[tuple(wrong[0])]}, want {want[tuple(wrong[0])]}"
    assert np.array_equal(bits(got), bits(want.astype(np.float32)))


# ---------------------------------------------------------------------------------------------------------------- 3. bound
@pytest.mark.parametrize("M,N,K", [(17, 33, 160), (64, 80, 1024), (8, 8, 11008)])
def test_random_data_within_the_bound(M, N, K):
    from sleekit_amd import mx

    rng = np.random.default_rng(K + M)
    a_codes, a_scales = model.quantize_act_model(block_gaussian(rng, M, K))
    w_codes, w_scales = random_weights(rng, N, K, 118, 123)
    bias = rng.standard_normal(N).astype(np.float32)
    want, sum_abs = model.matmul_model(a_codes, a_scales, w_codes, w_scales)
    got = mx.matmul_mx(a_codes, a_scales, w_codes, w_scales).astype(np.float64)
    err = np.abs(got - want)
    print(f"mx_gemm {M}x{N}x{K}: max |err| / sum|aw| = {(err / sum_abs).max():.3e} (bound {K * 2.0 ** -23:.3e})")
    assert (err <= bound(K, sum_abs)).all(), (err / sum_abs).max()
    got = mx.matmul_mx(a_codes, a_scales, w_codes, w_scales, bias).astype(np.float64)
    assert (np.abs(got - (want + bias)) <= bound(K + 1, sum_abs + np.abs(bias)[None, :])).all()


# ---------------------------------------------------------------------------------------------------------------- 4. quantizer
def fuzz_activations(rng, M, K):
    X = block_gaussian(rng, M, K)
    B = K // 32
    blocks = X.reshape(M * B, 32)  # a view: edits land in X
    mids = (model.e4m3_decode(np.arange(0x7e)) + model.e4m3_decode(np.arange(1, 0x7f))) / 2  # all 126 E4M3 midpoints
    for b in range(len(blocks)):
        kind = b % 7
        if kind == 1:
            blocks[b] = 0
        elif kind == 2:
            blocks[b] = -np.abs(blocks[b]) - 1e-3
        elif kind == 3:
            blocks[b, rng.integers(0, 32, 6)] = 1e-20
            if b % 2:
                blocks[b] = 1e-20 * rng.integers(-3, 4, 32)
        elif kind == 4:  # amax exactly 448 * 2^e, everything else on the grid's midpoints
            e = 2.0 ** rng.integers(-3, 4)
            blocks[b] = rng.choice(mids, 32) * rng.choice([-1.0, 1.0], 32) * e
            blocks[b, rng.integers(0, 32)] = 448 * e * (1 if b % 2 else -1)
        elif kind == 5:
            blocks[b] = np.abs(blocks[b])
    return X


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("M,K", [(1, 32), (3, 96), (17, 160), (64, 4096)])
def test_activation_quantizer_follows_the_model(M, K, dtype):
    from sleekit_amd import mx

    rng = np.random.default_rng(M + K)
    X = torch.from_numpy(fuzz_activations(rng, M, K)).to(dtype)  # exactly M K elements
    want_codes, want_E = model.quantize_act_model(X.float().numpy())
    codes, E = mx.quantize_mxfp8(X.cuda())
    assert codes.is_cuda and codes.dtype == torch.uint8 and tuple(codes.shape) == (M, K) and tuple(E.shape) == (M, K // 32)
    assert np.array_equal(E.cpu().numpy(), want_E)
    wrong = np.argwhere(codes.cpu().numpy() != want_codes)
    assert wrong.size == 0, (len(wrong), wrong[:4].tolist())
    assert not np.isin(want_codes, (0x7f, 0x80, 0xff)).any()
    # a view that starts off a 16-byte boundary
    buf = torch.zeros(M * K + 3, dtype=dtype, device="cuda")
    view = buf[3:].view(M, K)
    view.copy_(X)
    assert view.data_ptr() % 16 != 0
    c2, E2 = mx.quantize_mxfp8(view)
    assert torch.equal(c2, codes) and torch.equal(E2, E)
    # and back
    deq = model.dequantize_act_model(want_codes, want_E, np.float32)
    back = mx.dequantize_mxfp8(codes, E)
    assert back.dtype == torch.float32 and np.array_equal(bits(back), bits(deq))
    for low in (torch.bfloat16, torch.float16):
        assert torch.equal(mx.dequantize_mxfp8(codes, E, dtype=low).view(torch.int16), back.to(low).view(torch.int16)), low
    if dtype != torch.bfloat16:  # NumPy in, NumPy out
        c3, E3 = mx.quantize_mxfp8(X.numpy())
        assert isinstance(c3, np.ndarray) and np.array_equal(c3, want_codes) and np.array_equal(E3, want_E)
        assert np.array_equal(bits(mx.dequantize_mxfp8(c3, E3)), bits(deq))


def test_quantizer_known_answers_and_refusals():
    from sleekit_amd import mx

    x = np.zeros((2, 64), np.float32)
    x[0, :4], x[0, 31] = [1.0, -0.3, 0.001, 0.0], 1.0
    x[1, 32:36] = [1.75, -1.75, 0.01, 1e-5]
    codes, E = mx.quantize_mxfp8(x)
    assert E.tolist() == [[119, 74], [74, 119]]
    assert codes[0, :4].tolist() == [0x78, 0xea, 0x28, 0x00] and codes[1, 32:36].tolist() == [0x7e, 0xfe, 0x42, 0x01]
    assert not codes[0, 32:].any() and not codes[1, :32].any()
    for bad in (np.nan, np.inf, -np.inf):
        y = x.copy()
        y[1, 40] = bad
        with pytest.raises(ValueError, match="finite"):
            mx.quantize_mxfp8(y)
        with pytest.raises(ValueError, match="finite"):
            mx.linear_mxfp4(torch.from_numpy(y).cuda().half(), np.zeros((4, 32), np.uint8), np.full((4, 2), 127, np.uint8))
    E = np.full((2, 2), 127, np.uint8)
    E[1, 1] = 255
    with pytest.raises(ValueError, match="255"):
        mx.dequantize_mxfp8(codes, E)


# ---------------------------------------------------------------------------------------------------------------- 5. end to end
@pytest.fixture(scope="module")
def layer():
    from sleekit_amd import mx, synth

    L = synth.make_layer(48, 160, 4242)
    return mx.quantize_mxfp4(L["W"], L["H"]), np.random.default_rng(2).standard_normal(48).astype(np.float32)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_linear_end_to_end(layer, dtype):
    from sleekit_amd import mx

    res, bias = layer
    x = torch.from_numpy(block_gaussian(np.random.default_rng(3), 10, 160)).reshape(2, 5, 160).to(dtype).cuda()
    a_codes, a_scales = model.quantize_act_model(x.float().cpu().numpy().reshape(10, 160))
    A = model.dequantize_act_model(a_codes, a_scales)
    Q = res.Q.astype(np.float64)
    want = A @ Q.T + bias
    limit = bound(160 + 1, np.abs(A) @ np.abs(Q).T + np.abs(bias)[None, :])
    y32 = mx.linear_mxfp4(x, res.codes, res.scales, bias, dtype=torch.float32)
    assert y32.is_cuda and y32.dtype == torch.float32 and tuple(y32.shape) == (2, 5, 48)
    assert (np.abs(y32.cpu().numpy().reshape(10, 48).astype(np.float64) - want) <= limit).all()
    y = mx.linear_mxfp4(x, res.codes, res.scales, bias)  # the output dtype follows x
    assert y.dtype == dtype and tuple(y.shape) == (2, 5, 48) and np.array_equal(bits(y), bits(y32.to(dtype)))
    for explicit in (torch.bfloat16, torch.float16):
        z = mx.linear_mxfp4(x, res.codes, res.scales, bias, dtype=explicit)
        assert z.dtype == explicit and np.array_equal(bits(z), bits(y32.to(explicit)))
    # the pieces give the same bits, and no bias is a bias of zeros
    c, s = mx.quantize_mxfp8(x.reshape(10, 160))
    assert np.array_equal(c.cpu().numpy(), a_codes) and np.array_equal(s.cpu().numpy(), a_scales)
    assert np.array_equal(bits(mx.matmul_mx(c, s, torch.from_numpy(res.codes).cuda(), torch.from_numpy(res.scales).cuda(),
                                            torch.from_numpy(bias).cuda())), bits(y32.reshape(10, 48)))
    nb = mx.linear_mxfp4(x, res.codes, res.scales, dtype=torch.float32).cpu().numpy().reshape(10, 48).astype(np.float64)
    assert (np.abs(nb - A @ Q.T) <= bound(160, np.abs(A) @ np.abs(Q).T)).all()
    assert tuple(mx.linear_mxfp4(x[0, 0], res.codes, res.scales).shape) == (48,)


def test_module_from_a_quantized_layer():
    import torch.nn as nn

    from sleekit_amd import MXLinear, Sleekit, mx

    torch.manual_seed(5)
    lin = nn.Linear(160, 48).cuda()
    st = Sleekit(lin)
    for _ in range(3):
        st.add_batch(torch.randn(64, 160, device="cuda") + 0.3)
    res = st.quantize_mxfp4(bias_correction=True)
    mod = MXLinear.from_result(lin, res)
    x = torch.randn(2, 5, 160, device="cuda")
    want = mx.linear_mxfp4(x, res.codes, res.scales, lin.bias.data)
    got = mod(x)
    assert got.dtype == torch.float32 and torch.equal(got.view(torch.int32), want.view(torch.int32))
    # the packed layer is the quantized layer: against nn.Linear on the de-quantized activations, within the bound
    c, s = mx.quantize_mxfp8(x.reshape(10, 160))
    A = mx.dequantize_mxfp8(c, s).double()
    ref = A @ lin.weight.data.double().T + lin.bias.data.double()
    limit = bound(161, (A.abs() @ lin.weight.data.double().abs().T + lin.bias.data.double().abs()).cpu().numpy())
    assert (np.abs((got.reshape(10, 48).double() - ref).cpu().numpy()) <= limit).all()
    assert sorted(mod.state_dict()) == ["bias", "codes", "scales"]
    copy = MXLinear(160, 48).cuda()
    copy.load_state_dict(mod.state_dict())
    assert torch.equal(copy(x).view(torch.int32), want.view(torch.int32))
    half = mod(x.half())
    assert half.dtype == torch.float16
    nobias = MXLinear.from_result(nn.Linear(160, 48, bias=False).cuda(), res)
    assert nobias.bias is None and sorted(nobias.state_dict()) == ["codes", "scales"]
    assert torch.equal(nobias(x), mx.linear_mxfp4(x, res.codes, res.scales))
    with pytest.raises(ValueError):
        MXLinear.from_result(nn.Conv1d(160, 48, 1).cuda(), res)
    with pytest.raises(ValueError):
        MXLinear.from_result(nn.Linear(128, 48).cuda(), res)


# ---------------------------------------------------------------------------------------------------------------- 6. the rest
@pytest.mark.parametrize("M", [16, 130])
def test_repeated_calls_are_bit_equal(M):
    from sleekit_amd import mx

    rng = np.random.default_rng(M)
    N, K = 200, 4128
    x = torch.from_numpy(block_gaussian(rng, M, K)).cuda()
    w_codes, w_scales = (torch.from_numpy(t).cuda() for t in random_weights(rng, N, K, 118, 123))
    first = mx.linear_mxfp4(x, w_codes, w_scales)
    for _ in range(3):
        assert torch.equal(mx.linear_mxfp4(x, w_codes, w_scales).view(torch.int32), first.view(torch.int32))


def test_refusals():
    from sleekit_amd import mx

    codes = torch.zeros((8, 32), dtype=torch.uint8, device="cuda")
    scales = torch.full((8, 2), 127, dtype=torch.uint8, device="cuda")
    x = torch.zeros((4, 64), device="cuda")
    a_codes, a_scales = mx.quantize_mxfp8(x)
    with pytest.raises(ValueError, match="32"):
        mx.quantize_mxfp8(torch.zeros((4, 48), device="cuda"))
    with pytest.raises(ValueError, match="32"):
        mx.linear_mxfp4(torch.zeros((4, 48), device="cuda"), torch.zeros((8, 24), dtype=torch.uint8, device="cuda"), scales)
    with pytest.raises(ValueError, match="32"):
        mx.matmul_mx(torch.zeros((4, 48), dtype=torch.uint8, device="cuda"), a_scales, codes, scales)
    for call in (lambda: mx.linear_mxfp4(x, codes, scales[:, :1]), lambda: mx.linear_mxfp4(x, codes, scales[:4]),
                 lambda: mx.matmul_mx(a_codes, a_scales[:, :1], codes, scales), lambda: mx.matmul_mx(a_codes, a_scales, codes[:, :16], scales),
                 lambda: mx.linear_mxfp4(torch.zeros((4, 96), device="cuda"), codes, scales),
                 lambda: mx.linear_mxfp4(x, codes, scales, bias=torch.zeros(7, device="cuda")),
                 lambda: mx.dequantize_mxfp8(a_codes, a_scales[:2])):
        with pytest.raises(ValueError):
            call()
    for call in (lambda: mx.linear_mxfp4(x.double(), codes, scales), lambda: mx.linear_mxfp4(x, codes.int(), scales),
                 lambda: mx.linear_mxfp4(x, codes, scales.float()), lambda: mx.matmul_mx(a_codes.float(), a_scales, codes, scales),
                 lambda: mx.quantize_mxfp8(x.long()), lambda: mx.linear_mxfp4(x, codes, scales, dtype=torch.float64),
                 lambda: mx.dequantize_mxfp8(a_codes, a_scales, dtype=torch.int8)):
        with pytest.raises(ValueError):
            call()
    for call in (lambda: mx.linear_mxfp4(x.cpu().numpy(), codes, scales, dtype=torch.bfloat16),
                 lambda: mx.matmul_mx(a_codes.cpu().numpy(), a_scales, codes, scales, dtype=torch.bfloat16),
                 lambda: mx.dequantize_mxfp8(a_codes.cpu().numpy(), a_scales, dtype=torch.bfloat16)):
        with pytest.raises(ValueError, match="bfloat16"):
            call()
