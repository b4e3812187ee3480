"""Weight-only MX layers on the MI355X (activations="bfloat16" / "float16": slk_mx_gemm_a16, slk_mx_gemm_experts_a16): the
MFMA operand map with identity activations bit for bit, the ends of the promised scale range, exact integer products bit for
bit, random data within a derived bound against the float64 model, operand equality with the de-quantizer through the public
surface, the expert-grouped form against the dense one, rotation and modules, and repeated calls.

Sizes the shapes were chosen from: up to 64 rows of x a workgroup is one 16 x 16 tile of Y whose 8
waves take steps of 4 blocks (128 columns of K) in turn, 1024 columns a pass, the step K % 128 leaves going to the wave whose
turn it is; above 64 rows a workgroup is a 64 x 64 tile of Y and a K-step is 128 columns.  So K = 32 is one block and a
partial step alone, 96 and 160 an odd number of blocks, 2080 two passes and a partial step; N = 1, 17, 48, 80 are off
every tile width; M = 1, 5, 16, 17, 64, 65, 130 sits on both sides of 16 and of 64.

The one tolerance of this file is `bound`, the packed layer's (tests/test_gpu_packed_gemm.py): |y - y64| <= adds * 2^-23 *
sum_k |x_k w_k|, the first-order worst case of `adds` float32 additions in any order, rounded or truncated (the products are
exact in float32: 8 + 8 or 11 + 11 significant bits); adds is K, or K + 1 with a bias.  A misplaced element costs about
sum |x w| / sqrt(K), far above it.  Largest |err| / bound seen on the MI355X: DESIGN.md section 30.
"""

import functools

import numpy as np
import pytest
import torch

import mx_a16_model as model

pytestmark = pytest.mark.gpu

W4, W6 = "mxfp4", "mxfp6_e2m3"
WEIGHTS = [W4, W6]
COMPUTE = [torch.bfloat16, torch.float16]
NAME = {torch.bfloat16: "bfloat16", torch.float16: "float16"}


def bits_of(x):
    if isinstance(x, torch.Tensor):  # (NumPy has no bfloat16: the bits leave torch as integers)
        x = x.contiguous().view({2: torch.int16, 4: torch.int32}[x.element_size()]).cpu().numpy()
    x = np.asarray(x)
    return np.ascontiguousarray(x).view({2: np.uint16, 4: np.uint32}[x.dtype.itemsize])


def bound(adds, sum_abs):
    return adds * 2.0 ** -23 * sum_abs


def linear(x, codes, scales, weights, compute, bias=None, **kw):
    from sleekit_amd import mx

    f = mx.linear_mxfp4 if weights == W4 else mx.linear_mxfp6
    return f(x, codes, scales, bias, activations=NAME[compute], **kw)


def cuda(*arrays):
    return tuple(None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays)


def identity_check(codes, scales, weights, compute, N, K, what):
    """x = rows of 4 I_K in the compute type, in slices of 16 rows (the few-rows form) and whole where K > 64 (the tiled
    form): Y must be 4 Wc^T bit for bit -- one product a sum, and the zeros stay zeros."""
    Wc, _ = model.weights_model(codes, scales, weights, compute)
    lo, hi = model.NORMAL_BYTES[compute]
    assert lo <= scales.min() and scales.max() <= hi
    tiny = 2.0 ** -126 if compute == torch.bfloat16 else 2.0 ** -14
    assert np.isfinite(Wc).all() and (np.abs(Wc[Wc != 0]) >= tiny).all()  # every weight finite and normal
    # (K, N): row m of Y is column m of Wc, times 4.  (+ 0.0: E2M3's code 0x20 is -0, and a sum of the one product -0 and K - 1
    # products +0 is +0 under round to nearest, in any order -- the identity holds the values, and of a zero the sum's sign)
    want = (4.0 * Wc.T + 0.0).astype(np.float32)
    assert np.isfinite(want).all()
    X = torch.eye(K, dtype=compute, device="cuda") * 4
    cd, sd = cuda(codes, scales)
    calls = [(m0, min(m0 + 16, K)) for m0 in range(0, K, 16)] + ([(0, K)] if K > 64 else [])
    for m0, m1 in calls:
        got = linear(X[m0:m1], cd, sd, weights, compute, dtype=torch.float32).cpu().numpy()
        assert got.shape == (m1 - m0, N) and got.dtype == np.float32
        wrong = np.argwhere(bits_of(got) != bits_of(want[m0:m1]))
        if wrong.size:
            m, col = wrong[0]
            read = np.flatnonzero(want[:, col] == got[m, col]).tolist()
            raise AssertionError(f"{what}, K = {K}, N = {N}, rows {m0}:{m1}: {len(wrong)} differ, first y[{m0 + m}][{col}] = "
                                 f"{got[m, col]!r}, want 4 W[{col}][{m0 + m}] = {want[m0 + m, col]!r}; it is 4 W[{col}][k] for k in {read[:6]}")


# ---------------------------------------------------------------------------------------------------------------- 1. map
@pytest.mark.parametrize("compute", COMPUTE)
@pytest.mark.parametrize("weights", WEIGHTS)
def test_operand_map_identity(weights, compute):
    """Neighbouring codes differ, and so do the scale bytes of neighbouring rows and blocks (121 .. 135: every weight is
    finite and normal in float16 too), so a neighbour's code, block, scale or row changes the answer."""
    levels = model.LEVELS[weights]
    for K in (64, 96):
        for N in (16, 33):
            n, k = np.meshgrid(np.arange(N), np.arange(K), indexing="ij")
            codes = model.pack_codes(((7 * n + 3 * k) % levels).astype(np.uint8), weights)
            nb, kb = np.meshgrid(np.arange(N), np.arange(K // 32), indexing="ij")
            scales = (127 + (7 * nb + 3 * kb) % 15 - 6).astype(np.uint8)
            identity_check(codes, scales, weights, compute, N, K, f"{weights} in {NAME[compute]}")


# ---------------------------------------------------------------------------------------------------------------- 2. range
@pytest.mark.parametrize("weights", WEIGHTS)
def test_bfloat16_scale_range_ends(weights):
    """Scale bytes 10, 11, 126, 127, 128, 244, 245, one a block along K = 7 * 32, on both forms: the promised range of the
    bfloat16 compute type held at its ends (2^-117 .. 2^118: the largest weight times 4 is still a float32)."""
    levels, N, K = model.LEVELS[weights], 33, 7 * 32
    n, k = np.meshgrid(np.arange(N), np.arange(K), indexing="ij")
    codes = model.pack_codes(((7 * n + 3 * k) % levels).astype(np.uint8), weights)
    scales = np.tile(np.array([10, 11, 126, 127, 128, 244, 245], np.uint8), (N, 1))
    identity_check(codes, scales, weights, torch.bfloat16, N, K, f"{weights} at the ends of the range")


# ---------------------------------------------------------------------------------------------------------------- 3. exact
EXACT = [(1, 1, 32), (1, 16, 128), (16, 1, 96), (17, 33, 160), (5, 48, 2080), (64, 17, 160), (65, 17, 160), (130, 80, 544)]
X_DTYPES = [torch.float32, torch.bfloat16, torch.float16]


@pytest.mark.parametrize("compute", COMPUTE)
@pytest.mark.parametrize("weights", WEIGHTS)
@pytest.mark.parametrize("case", range(len(EXACT)))
def test_exact_integers_bit_for_bit(case, weights, compute):
    M, N, K = EXACT[case]
    rng = np.random.default_rng(M * 1000 + N * 7 + K)
    codes = model.pack_codes(rng.integers(0, model.LEVELS[weights], (N, K)).astype(np.uint8), weights)  # the whole table
    scales = rng.choice(np.array([126, 127, 128], np.uint8), (N, K // 32))
    x = torch.from_numpy(rng.integers(-4, 5, (M, K)).astype(np.float32)).to(X_DTYPES[case % 3])
    bias = (rng.integers(-64, 65, N) / 8.0).astype(np.float32) if (M + N) % 2 else None
    # the test's own inputs make every order of float32 additions exact: a weight is a multiple of 2^-4 (E2M3's 1/8 under the
    # scale 1/2) of magnitude at most 15 that both compute types hold exactly, x an integer of magnitude at most 4, so all
    # terms (and the bias) are multiples of q = 2^-4 of magnitude at most 60, and every partial sum is a multiple of q below 2^20
    Wc, W32 = model.weights_model(codes, scales, weights, compute)
    assert np.array_equal(Wc, W32.astype(np.float64)) and np.abs(Wc).max() <= 15 and (Wc * 16 == np.rint(Wc * 16)).all()
    assert K * 60 + 8 < 2 ** 20
    want, _ = model.linear_model(x, codes, scales, weights, compute, bias)
    got = linear(x.cuda(), *cuda(codes, scales), weights, compute, *cuda(bias), dtype=torch.float32).cpu().numpy()
    assert got.shape == (M, N) and got.dtype == np.float32
    wrong = np.argwhere(got.astype(np.float64) != want)
    assert wrong.size == 0, f"{len(wrong)} of {M * N} differ, first at {wrong[:4].tolist()}: got {got[tuple(wrong[0])]}, want {want[tuple(wrong[0])]}"
    assert np.array_equal(bits_of(got), bits_of(want.astype(np.float32)))


# ---------------------------------------------------------------------------------------------------------------- 4. random
def block_gaussian(rng, M, K):
    """Gaussian rows with a few outlier columns (what a rotation is for)."""
    X = rng.standard_normal((M, K)).astype(np.float32)
    X[:, rng.choice(K, max(1, K // 64), replace=False)] *= 24.0
    return X


@functools.lru_cache(maxsize=None)
def quantized_layer(N, K, weights, seed=0):
    """(MXResult, the synthetic layer) of a random (N, K) layer, quantized once per shape and format and shared."""
    from sleekit_amd import mx, synth

    L = synth.make_layer(N, K, 5100 + N + K + seed)
    return (mx.quantize_mxfp4 if weights == W4 else mx.quantize_mxfp6)(L["W"], L["H"]), L


@pytest.mark.parametrize("compute", COMPUTE)
@pytest.mark.parametrize("weights", WEIGHTS)
@pytest.mark.parametrize("M,N,K", [(3, 40, 256), (64, 48, 96), (65, 48, 96), (130, 200, 544)])
def test_random_data_within_the_bound(M, N, K, weights, compute):
    res, _ = quantized_layer(N, K, weights)
    rng = np.random.default_rng(M + N + K)
    x = block_gaussian(rng, M, K)
    bias = rng.standard_normal(N).astype(np.float32)
    want, sum_abs = model.linear_model(x, res.codes, res.scales, weights, compute, bias)
    got = linear(*cuda(x, res.codes, res.scales), weights, compute, *cuda(bias), dtype=torch.float32).cpu().numpy().astype(np.float64)
    ratio = np.abs(got - want) / bound(K + 1, sum_abs)
    print(f"{weights} {NAME[compute]} ({M}, {N}, {K}): largest |err| / bound = {ratio.max():.4f}, |err| / sum|xw| = "
          f"{(np.abs(got - want) / sum_abs).max():.3e}")
    assert (ratio <= 1.0).all(), f"largest |err| / bound = {ratio.max()} at {np.unravel_index(ratio.argmax(), ratio.shape)}"


# ---------------------------------------------------------------------------------------------------------------- 5. surface
@pytest.mark.parametrize("compute", COMPUTE)
@pytest.mark.parametrize("weights", WEIGHTS)
def test_operands_are_the_dequantizer_s(weights, compute):
    """linear(eye) in float32 is the de-quantizer's compute-type output transposed, on a quantized layer -- both forms."""
    from sleekit_amd import mx

    N, K = 48, 96
    res, _ = quantized_layer(N, K, weights)
    cd, sd = cuda(res.codes, res.scales)
    deq = (mx.dequantize_mxfp4 if weights == W4 else mx.dequantize_mxfp6)(cd, sd, dtype=compute)
    assert deq.dtype == compute and tuple(deq.shape) == (N, K)
    want = deq.t().float().contiguous()
    eye = torch.eye(K, dtype=compute, device="cuda")
    assert np.array_equal(bits_of(linear(eye, cd, sd, weights, compute, dtype=torch.float32)), bits_of(want))          # tiled
    assert np.array_equal(bits_of(linear(eye[32:48], cd, sd, weights, compute, dtype=torch.float32)), bits_of(want[32:48]))  # few rows
    # the result's dtype follows x; NumPy in, NumPy out -- a float32 NumPy x is rounded in the kernel
    x = torch.from_numpy(block_gaussian(np.random.default_rng(2), 5, K)).cuda()
    y32 = linear(x, cd, sd, weights, compute)
    assert y32.dtype == torch.float32 and linear(x.to(compute), cd, sd, weights, compute).dtype == compute
    assert np.array_equal(bits_of(y32), bits_of(linear(x.to(compute), cd, sd, weights, compute, dtype=torch.float32)))
    ynp = linear(x.cpu().numpy(), np.asarray(res.codes), np.asarray(res.scales), weights, compute)
    assert isinstance(ynp, np.ndarray) and np.array_equal(bits_of(ynp), bits_of(y32))
    # a NaN or an infinity in x is not refused: it propagates to its row and to no other
    x[2, 7] = float("inf")
    y = linear(x, cd, sd, weights, compute)
    assert not torch.isfinite(y[2]).all() and torch.isfinite(y[[0, 1, 3, 4]]).all()
    assert np.array_equal(bits_of(y[[0, 1, 3, 4]]), bits_of(y32[[0, 1, 3, 4]]))


# ---------------------------------------------------------------------------------------------------------------- 6. experts
COUNTS = (0, 1, 17, 70)  # an empty expert, one and two 16-row tiles, and the tiled form


@pytest.fixture(scope="module", params=WEIGHTS)
def experts(request):
    """E = 4 random layers of 48 x 96 in either format under scale bytes 120 .. 130, their biases, x sorted by expert."""
    weights = request.param
    rng = np.random.default_rng(61)
    E, N, K, M = len(COUNTS), 48, 96, sum(COUNTS)
    codes = np.stack([model.pack_codes(rng.integers(0, model.LEVELS[weights], (N, K)).astype(np.uint8), weights) for _ in range(E)])
    scales = rng.integers(120, 131, (E, N, K // 32)).astype(np.uint8)
    bias = rng.standard_normal((E, N)).astype(np.float32)
    offsets = np.concatenate([[0], np.cumsum(COUNTS)]).astype(np.int32)
    return weights, cuda(codes, scales, bias, offsets), block_gaussian(rng, M, K)


@pytest.mark.parametrize("compute", COMPUTE)
def test_experts_equal_the_dense_call_per_slice(experts, compute):
    from sleekit_amd import mx

    weights, (codes, scales, bias, offsets), x = experts
    for xd in (torch.float32, compute):
        xg = torch.from_numpy(x).cuda().to(xd)
        got = mx.linear_mx_experts(xg, codes, scales, offsets, bias, dtype=torch.float32, activations=NAME[compute], weights=weights)
        assert got.dtype == torch.float32 and tuple(got.shape) == (sum(COUNTS), 48)
        lo = 0
        for e, count in enumerate(COUNTS):
            if count:
                want = linear(xg[lo:lo + count], codes[e], scales[e], weights, compute, bias[e], dtype=torch.float32)
                assert np.array_equal(bits_of(got[lo:lo + count]), bits_of(want)), f"expert {e} ({count} rows)"
            lo += count
    want64, sum_abs = model.experts_model(x, codes.cpu().numpy(), scales.cpu().numpy(), offsets.cpu().numpy(), weights, compute, bias.cpu().numpy())
    assert (np.abs(got.cpu().numpy().astype(np.float64) - want64) <= bound(96 + 1, sum_abs)).all()
    assert mx.linear_mx_experts(xg, codes, scales, offsets, bias, activations=NAME[compute], weights=weights).dtype == compute


def test_invalid_offsets_raise_and_leave_no_tile(experts):
    """As tests/test_gpu_mx_experts.py checks "nothing": the flag's error, and both tile counts 0 -- every workgroup of the
    products returned at once."""
    from sleekit_amd import mx

    weights, (codes, scales, bias, offsets), x = experts
    M, E = sum(COUNTS), len(COUNTS)
    xg = torch.from_numpy(x).cuda()
    for bad in ([0, 5, 3, 40, M], [0, 1, 18, 70, M - 1], [1, 1, 18, 70, M], [0, 1, 18, 2 ** 31 - 1, M], [-4, 1, 18, 70, M]):
        with pytest.raises(ValueError, match=r"offsets\[0\] == 0"):
            mx.linear_mx_experts(xg, codes, scales, torch.tensor(bad, dtype=torch.int32, device="cuda"), bias, activations="bfloat16", weights=weights)
        got16, got64 = mx._expert_tile_tables(E, M)
        assert len(got16) == 0 and len(got64) == 0
    good = mx.linear_mx_experts(xg, codes, scales, offsets, bias, activations="bfloat16", weights=weights)  # the next call is not held up
    assert torch.isfinite(good).all()
    got16, got64 = mx._expert_tile_tables(E, M)
    assert len(got16) == 1 + 2 and len(got64) == 2


@pytest.mark.parametrize("gated", [True, False])
def test_forward_tokens_against_per_expert_calls(experts, gated):
    """T = 9 tokens, k = 2 of E = 4 experts, as tests/test_gpu_mx_experts.py computes it: the reference runs the dense call
    of every expert on every token (float32: the grouped product's bits for that row), picks each token's k outputs and adds
    them in float64 after rounding each gated output to float32 and the sum to float32 -- the module's own roundings."""
    from sleekit_amd import mx

    weights, (codes, scales, bias, _), xs = experts
    T, k, E = 9, 2, 4
    mod = mx.MXExperts(E, 96, 48, activations="bfloat16", weights=weights).cuda()
    mod.codes.copy_(codes), mod.scales.copy_(scales), mod.bias.copy_(bias)
    rng = np.random.default_rng(12)
    x = torch.from_numpy(xs[:T].copy()).cuda()
    ids = np.stack([rng.permutation(E)[:k] for _ in range(T)])
    gates = rng.random((T, k)).astype(np.float32) if gated else None
    per_expert = np.stack([linear(x, codes[e], scales[e], weights, torch.bfloat16, bias[e]).cpu().numpy() for e in range(E)])  # (E, T, N)
    picked = np.stack([per_expert[ids[:, j], np.arange(T)] for j in range(k)], axis=1).astype(np.float64)               # (T, k, N)
    if gated:
        picked = (picked * gates.astype(np.float64)[:, :, None]).astype(np.float32).astype(np.float64)
    want = (picked[:, 0] + picked[:, 1]).astype(np.float32)
    got = mod.forward_tokens(x, torch.from_numpy(ids).cuda(), None if gates is None else torch.from_numpy(gates).cuda())
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (T, 48)
    assert np.array_equal(bits_of(got), bits_of(want))
    order, offsets = mx.sort_by_expert(torch.from_numpy(ids).cuda(), E)
    rows = mod(x[order // k], offsets)   # forward on sorted rows is what forward_tokens runs
    assert np.array_equal(bits_of(rows), bits_of(per_expert[ids.reshape(-1), np.repeat(np.arange(T), k)][order.cpu().numpy()]))
    beyond = ids.copy()
    beyond[T // 2, 1] = E
    with pytest.raises(ValueError, match="0 .. 3"):
        mod.forward_tokens(x, torch.from_numpy(beyond).cuda())
    loaded = mx.MXExperts(E, 96, 48, weights=weights).cuda()
    loaded.load_state_dict(mod.state_dict())
    assert loaded.activations == "bfloat16" and np.array_equal(bits_of(loaded(x[order // k], offsets)), bits_of(rows))
    from_results = mx.MXExperts.from_results([mx.MXResult(None, None, None, codes[e], scales[e]) for e in range(E)], bias, activations="float16")
    assert from_results.activations == "float16"
    assert np.array_equal(bits_of(from_results(x[order // k], offsets)),
                          bits_of(mx.linear_mx_experts(x[order // k], codes, scales, offsets, bias, activations="float16", weights=weights)))


# ---------------------------------------------------------------------------------------------------------------- 7. rotation
@pytest.mark.parametrize("weights", WEIGHTS)
def test_rotation_and_modules(weights):
    from sleekit_amd import mx, rotation

    N, K = 40, 256
    res, L = quantized_layer(N, K, weights)
    cd, sd = cuda(res.codes, res.scales)
    bias = torch.from_numpy(np.random.default_rng(4).standard_normal(N).astype(np.float32)).cuda()
    rot = rotation.Rotation(K, block=64, seed=11)
    layer = torch.nn.Linear(K, N).cuda()
    with torch.no_grad():
        layer.bias.copy_(bias)
    for M in (5, 70):
        x = torch.from_numpy(block_gaussian(np.random.default_rng(M), M, K)).cuda()
        for compute in COMPUTE:
            plain = linear(x, cd, sd, weights, compute, bias)
            turned = linear(x, cd, sd, weights, compute, bias, rotation=rot)
            assert turned.dtype == torch.float32 and not np.array_equal(bits_of(turned), bits_of(plain))
            assert np.array_equal(bits_of(turned), bits_of(linear(rot.apply(x, dtype=compute), cd, sd, weights, compute, bias, dtype=torch.float32)))
            mod = mx.MXLinear.from_result(layer, res, activations=NAME[compute])
            assert mod.activations == NAME[compute] and mod.weights == weights and NAME[compute] in mod.extra_repr()
            assert np.array_equal(bits_of(mod(x)), bits_of(plain)) and np.array_equal(bits_of(mod(x, rotation=rot)), bits_of(turned))
            loaded = mx.MXLinear(K, N, weights=weights).cuda()   # default activations: the state carries the name
            loaded.load_state_dict(mod.state_dict())
            assert loaded.activations == NAME[compute] and np.array_equal(bits_of(loaded(x)), bits_of(plain))
            for fused in (True, False):
                wrapped = rotation.RotatedLinear(mod, rot, fused=fused)
                assert wrapped.fused is fused and np.array_equal(bits_of(wrapped(x)), bits_of(turned))
            half_x = x.to(compute)   # x in the compute type: the result follows it
            assert np.array_equal(bits_of(rotation.RotatedLinear(mod, rot)(half_x)),
                                  bits_of(linear(rot.apply(half_x), cd, sd, weights, compute, bias)))


# ---------------------------------------------------------------------------------------------------------------- 8. repeats
@pytest.mark.parametrize("M", [16, 130])
def test_repeated_calls_are_bit_equal(M):
    N, K = 200, 544
    rng = np.random.default_rng(M)
    x, = cuda(block_gaussian(rng, M, K))
    for weights in WEIGHTS:
        res, _ = quantized_layer(N, K, weights)
        cd, sd = cuda(res.codes, res.scales)
        first = linear(x, cd, sd, weights, torch.bfloat16)
        for _ in range(5):
            assert np.array_equal(bits_of(linear(x, cd, sd, weights, torch.bfloat16)), bits_of(first))
