"""The expert-grouped MX product on the MI355X: exact integer products bit for bit against the NumPy model
(tests/mx_experts_model.py), the grouped call against a loop of dense calls bit for bit and against the float64 model
within a derived bound, the prologue's tile tables against the model's, the Python surface end to end, and
quantize_experts against the single-layer calls.

The shapes put experts on both sides of the form rule (up to 64 rows: 16-row tiles on the split-K form; above: 64-row tiles
on the 2 x 2 tiled form), at its edge (64 and 65 rows), with no rows at all (first, last and in the middle), with row counts
that are no multiple of a tile, N that is no multiple of 16 or 64, and K that is no multiple of 128 (160) or of the 2048
columns the split-K form takes a pass (4128).

The one tolerance of this file is `bound`, tests/test_gpu_mx_gemm.py's re-derived: the products a w are exact in float32 (4 +
2 significant bits, or 4 + 4; power-of-two scales), so a result is a sum of K exact terms (and a bias) by float32 additions
in some fixed order; each addition errs by at most 2^-24 relative to its own result if rounded, 2^-23 if truncated, and every
partial result is at most sum_k |a_k w_k| (+ |bias|) up to second order, so |y - y64| <= adds * 2^-23 * sum |a w| whatever
the order.  A misplaced row, expert or scale costs about sum |a w| / sqrt(K), far above it.  Largest |err| / sum |a w| seen
on the MI355X: DESIGN.md section 23.
"""

import numpy as np
import pytest
import torch

import mx6_model
import mx_act4_model
import mx_act6_model
import mx_experts_model as model
import mx_gemm_model

pytestmark = pytest.mark.gpu

W4, W6 = "mxfp4", "mxfp6_e2m3"
PAIRS = [("mxfp8", W4), ("mxfp4", W4), ("mxfp6_e2m3", W4), ("mxfp8", W6), ("mxfp6_e2m3", W6)]
# (counts of rows per expert, N, K)
SHAPES = [((0, 1, 17, 65, 0), 33, 160), ((64, 65, 16), 17, 160), ((15, 0, 47, 130), 47, 4128)]
CASES = [(0, a, w) for a, w in PAIRS] + [(1, "mxfp8", W4), (2, "mxfp8", W4)]
E2M1_CODES = np.array([c for c in range(16) if c != 8], np.uint8)     # -0 is never written
E2M3_CODES = np.array([c for c in range(64) if c != 0x20], np.uint8)


def bits(x):
    if isinstance(x, torch.Tensor):  # (NumPy has no bfloat16: the bits leave torch as integers)
        x = x.contiguous().view({2: torch.int16, 4: torch.int32}[x.element_size()]).cpu().numpy()
    x = np.asarray(x)
    return np.ascontiguousarray(x).view({2: np.uint16, 4: np.uint32}[x.dtype.itemsize])


def bound(adds, sum_abs):
    return adds * 2.0 ** -23 * sum_abs


def random_experts(rng, E, N, K, lo, hi, weights):
    """Every expert its own random codes and scale bytes: (codes (E, N, K bits / 8), scales (E, N, K / 32))."""
    if weights == W4:
        codes = np.stack([mx_act4_model.pack_nibbles(E2M1_CODES[rng.integers(0, 15, (N, K))]) for _ in range(E)])
    else:
        codes = np.stack([mx_act6_model.pack_codes(E2M3_CODES[rng.integers(0, 63, (N, K))]) for _ in range(E)])
    return codes, rng.integers(lo, hi + 1, (E, N, K // 32)).astype(np.uint8)


ENCODE = {"mxfp8": mx_gemm_model.e4m3_encode,
          "mxfp4": lambda y: mx_act4_model.pack_nibbles(mx_act4_model.e2m1_encode(y)),
          "mxfp6_e2m3": lambda y: mx_act6_model.pack_codes(mx_act6_model.e2m3_encode(y))}
QUANTIZE = {"mxfp8": mx_gemm_model.quantize_act_model, "mxfp4": mx_act4_model.quantize_act4_model,
            "mxfp6_e2m3": mx_act6_model.quantize_act6_model}


def block_gaussian(rng, M, K):
    """Gaussian data whose blocks of 32 have magnitudes 2^-3 .. 2^3."""
    mag = 2.0 ** rng.integers(-3, 4, (M, K // 32))
    return (rng.standard_normal((M, K)) * np.repeat(mag, 32, axis=1)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- 1. exact
@pytest.mark.parametrize("shape,activations,weights", CASES)
def test_exact_integers_bit_for_bit(shape, activations, weights):
    """Shares nothing with the dense kernels: integer activations in +-4 under scale bytes 126 .. 128, weights under the
    same, a bias in multiples of 1 / 8 -- every term and every partial sum is a multiple of q below 2^24 q, so every order of
    float32 additions is exact and the float64 model's value is the only right answer."""
    from sleekit_amd import mx

    counts, N, K = SHAPES[shape]
    E, M = len(counts), sum(counts)
    rng = np.random.default_rng(1000 * shape + 7 * N + K + len(activations) + 3 * len(weights))
    a_codes = ENCODE[activations](rng.integers(-4, 5, (M, K)).astype(np.float64))
    a_scales = (127 + rng.integers(-1, 2, (M, K // 32))).astype(np.uint8)
    codes, scales = random_experts(rng, E, N, K, 126, 128, weights)
    bias = (rng.integers(-64, 65, (E, N)) / 8.0).astype(np.float32)
    offsets = model.offsets_of(counts)
    A = model.DEQUANTIZE_ACT[activations](a_codes, a_scales)
    Wmax = max(np.abs(mx6_model.dequantize_model(c, s) if weights == W6 else mx_gemm_model.weights_model(c, s)).max() for c, s in zip(codes, scales))
    q = 2.0 ** -3 if weights == W4 else 2.0 ** -5   # A in halves; W in quarters (E2M1) or sixteenths (E2M3)
    assert np.abs(A).max() <= 8 and (A * 2 == np.rint(A * 2)).all() and Wmax <= (12 if weights == W4 else 15)
    assert K * 8 * Wmax + 8 < 2 ** 24 * q and (weights != W4 or K * 96 + 8 < 2 ** 21)
    want, _ = model.matmul_model(a_codes, a_scales, codes, scales, offsets, bias, activations, weights)
    got = mx.matmul_mx_experts(a_codes, a_scales, codes, scales, offsets, bias, activations=activations, weights=weights)
    assert got.shape == (M, N) and got.dtype == np.float32
    wrong = np.argwhere(got.astype(np.float64) != want)
    assert wrong.size == 0, (f"{len(wrong)} of {M * N} differ, first at {wrong[:4].tolist()}: got {got[tuple(wrong[0])]}, "
                             f"want {want[tuple(wrong[0])]} (offsets {offsets.tolist()})")
    assert np.array_equal(bits(got), bits(want.astype(np.float32)))


# ---------------------------------------------------------------------------------------------------------------- 2. the loop
@pytest.fixture(scope="module")
def random_case():
    """(operands on the device, the float64 model) of a CASE with block-Gaussian data, made once and left unchanged."""
    made = {}

    def get(shape, activations, weights):
        key = (shape, activations, weights)
        if key not in made:
            counts, N, K = SHAPES[shape]
            E, M = len(counts), sum(counts)
            rng = np.random.default_rng(77 + 1000 * shape + len(activations) + 3 * len(weights))
            a_codes, a_scales = QUANTIZE[activations](block_gaussian(rng, M, K))
            codes, scales = random_experts(rng, E, N, K, 118, 123, weights)
            bias = rng.standard_normal((E, N)).astype(np.float32)
            offsets = model.offsets_of(counts)
            want, sum_abs = model.matmul_model(a_codes, a_scales, codes, scales, offsets, None, activations, weights)
            dev = tuple(torch.from_numpy(t).cuda() for t in (a_codes, a_scales, codes, scales, offsets, bias))
            made[key] = (dev, offsets, bias, want, sum_abs)
        return made[key]

    return get


# (all five pairs and the three output dtypes on the first shape, MXFP8 x MXFP4 in float32 on the others)
LOOP_CASES = [c + (d,) for c in CASES for d in (torch.float32, torch.bfloat16, torch.float16) if c[0] == 0 or d == torch.float32]


@pytest.mark.parametrize("shape,activations,weights,dtype", LOOP_CASES)
def test_grouped_call_equals_the_loop(random_case, shape, activations, weights, dtype):
    from sleekit_amd import mx

    (a_codes, a_scales, codes, scales, offsets_d, bias_d), offsets, bias, want, sum_abs = random_case(shape, activations, weights)
    counts, N, K = SHAPES[shape]
    kw = dict(dtype=dtype, activations=activations, weights=weights)
    for b in (None, bias_d):
        got = mx.matmul_mx_experts(a_codes, a_scales, codes, scales, offsets_d, b, **kw)
        assert got.is_cuda and got.dtype == dtype and tuple(got.shape) == (sum(counts), N)
        for e in range(len(counts)):
            lo, hi = int(offsets[e]), int(offsets[e + 1])
            if hi > lo:
                alone = mx.matmul_mx(a_codes[lo:hi], a_scales[lo:hi], codes[e], scales[e], None if b is None else b[e], **kw)
                assert np.array_equal(bits(got[lo:hi]), bits(alone)), f"expert {e} of {counts}, rows {lo} .. {hi - 1}"
        if dtype == torch.float32:
            y = got.cpu().numpy().astype(np.float64)
            if b is None:
                err = np.abs(y - want)
                print(f"mx_gemm_experts {counts} x {N} x {K} {activations} x {weights}: max |err| / sum|aw| = "
                      f"{(err / sum_abs).max():.3e} (bound {K * 2.0 ** -23:.3e})")
                assert (err <= bound(K, sum_abs)).all(), (err / sum_abs).max()
            else:
                rows = np.repeat(bias, counts, axis=0)  # every row's bias is its expert's
                assert (np.abs(y - (want + rows)) <= bound(K + 1, sum_abs + np.abs(rows))).all()


# ---------------------------------------------------------------------------------------------------------------- 3. the tables
def tiny_operands(E, M, N=16, K=32):
    a = torch.zeros((M, K), dtype=torch.uint8, device="cuda"), torch.full((M, K // 32), 127, dtype=torch.uint8, device="cuda")
    w = torch.zeros((E, N, K // 2), dtype=torch.uint8, device="cuda"), torch.full((E, N, K // 32), 127, dtype=torch.uint8, device="cuda")
    return a + w


@pytest.mark.parametrize("offsets", [[0, 0, 1, 18, 83, 83], [0, 64, 129], [0, 5, 5, 5], [0, 16, 80, 209, 209, 273]])
def test_tile_tables_follow_the_model(offsets):
    from sleekit_amd import mx

    E, M = len(offsets) - 1, offsets[-1]
    valid, t16, t64 = model.tile_tables(offsets, M)
    assert valid
    out = mx.matmul_mx_experts(*tiny_operands(E, M), torch.tensor(offsets, dtype=torch.int32, device="cuda"))
    assert tuple(out.shape) == (M, 16) and not out.any()
    got16, got64 = mx._expert_tile_tables(E, M)
    assert got16.tolist() == t16.tolist() and got64.tolist() == t64.tolist()


def test_no_rows_at_all_is_refused():
    """[0, 0, 0] is valid for the model (M = 0: no tile) but no call: the surface takes at least one row."""
    from sleekit_amd import mx

    valid, t16, t64 = model.tile_tables([0, 0, 0], 0)
    assert valid and len(t16) == 0 and len(t64) == 0
    a_codes, a_scales, codes, scales = tiny_operands(2, 1)
    with pytest.raises(ValueError):
        mx.matmul_mx_experts(a_codes[:0], a_scales[:0], codes, scales, torch.zeros(3, dtype=torch.int32, device="cuda"))


@pytest.mark.parametrize("offsets", [[0, 5, 3, 9], [0, 3, 8], [1, 3, 9], [0, 3, 2 ** 31 - 1], [-4, 3, 9]])
def test_invalid_offsets_raise_and_leave_no_tile(offsets):
    """The first three are the CPU test's; two more with values an unchecked address would run far away with."""
    from sleekit_amd import mx

    M, E = 9, len(offsets) - 1
    assert not model.tile_tables(offsets, M)[0]
    ops = tiny_operands(E, M)
    bad = torch.tensor(offsets, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match=r"offsets\[0\] == 0"):
        mx.matmul_mx_experts(*ops, bad)
    got16, got64 = mx._expert_tile_tables(E, M)   # both counts 0: the products' workgroups all returned at once
    assert len(got16) == 0 and len(got64) == 0
    with pytest.raises(ValueError, match=r"offsets\[0\] == 0"):
        mx.linear_mx_experts(torch.zeros((M, 32), device="cuda"), ops[2], ops[3], bad)
    good = torch.tensor([0] * E + [M], dtype=torch.int32, device="cuda")   # and the next call is not held up by the last flag
    assert not mx.matmul_mx_experts(*ops, good).any()


def test_two_raised_flags_give_the_first_message():
    """E = 2, M = 4, K = 32, N = 16, MXFP8 on MXFP4.  A NaN in x with offsets that break the rule: the finite message, which
    linear_mx_experts reads first.  A NaN in x with an expert id of E: the id message, which forward_tokens reads first.
    (Invalid offsets are refused by the prologue before any address is made from them.)"""
    from sleekit_amd import mx

    E, M, N, K = 2, 4, 16, 32
    _, _, codes, scales = tiny_operands(E, M, N, K)
    x = torch.ones((M, K), device="cuda")
    x[2, 5] = float("nan")
    with pytest.raises(ValueError) as raised:
        mx.linear_mx_experts(x, codes, scales, torch.tensor([0, 3, 2], dtype=torch.int32, device="cuda"))
    assert str(raised.value) == mx._H_FINITE
    mod = mx.MXExperts(E, K, N, bias=False).cuda()
    ids = torch.tensor([[0], [1], [E], [0]], device="cuda")
    with pytest.raises(ValueError) as raised:
        mod.forward_tokens(x, ids)
    assert str(raised.value) == mx._ids_message(E)
    with pytest.raises(ValueError) as raised:   # ... and each of the two alone still has its own
        mod.forward_tokens(x, ids.clamp(0, E - 1))
    assert str(raised.value) == mx._H_FINITE


# ---------------------------------------------------------------------------------------------------------------- 4. surface
@pytest.mark.parametrize("activations,weights", PAIRS)
def test_linear_is_quantizer_then_product(activations, weights):
    from sleekit_amd import mx, rotation

    counts, N, K = SHAPES[0]
    E, M = len(counts), sum(counts)
    rng = np.random.default_rng(31)
    x = torch.from_numpy(block_gaussian(rng, M, K)).cuda()
    codes, scales = (torch.from_numpy(t).cuda() for t in random_experts(rng, E, N, K, 118, 123, weights))
    bias = torch.from_numpy(rng.standard_normal((E, N)).astype(np.float32)).cuda()
    offsets = torch.from_numpy(model.offsets_of(counts)).cuda()
    quantize = {"mxfp8": mx.quantize_mxfp8, "mxfp4": mx.quantize_mxfp4_act, "mxfp6_e2m3": mx.quantize_mxfp6_act}[activations]
    kw = dict(activations=activations, weights=weights)
    want = mx.matmul_mx_experts(*quantize(x), codes, scales, offsets, bias, **kw)
    got = mx.linear_mx_experts(x, codes, scales, offsets, bias, **kw)
    assert got.dtype == torch.float32 and np.array_equal(bits(got), bits(want))
    half = mx.linear_mx_experts(x.half(), codes, scales, offsets, bias, **kw)  # the output dtype follows x
    assert half.dtype == torch.float16 and tuple(half.shape) == (M, N)
    assert np.array_equal(bits(mx.linear_mx_experts(x.half(), codes, scales, offsets, bias, dtype=torch.float32, **kw).half()), bits(half))
    rot = rotation.Rotation(K, block=32, seed=9)
    turned = mx.linear_mx_experts(x, codes, scales, offsets, bias, rotation=rot, **kw)
    assert np.array_equal(bits(turned), bits(mx.linear_mx_experts(rot.apply(x, dtype=torch.float32), codes, scales, offsets, bias, **kw)))
    assert not np.array_equal(bits(turned), bits(got))
    # NumPy in, NumPy out
    y = mx.linear_mx_experts(x.cpu().numpy(), codes.cpu().numpy(), scales.cpu().numpy(), offsets.cpu().numpy(), bias.cpu().numpy(), **kw)
    assert isinstance(y, np.ndarray) and np.array_equal(bits(y), bits(got))
    bad = x.clone()
    bad[M - 1, 7] = float("inf")
    with pytest.raises(ValueError, match="finite"):
        mx.linear_mx_experts(bad, codes, scales, offsets, bias, **kw)


@pytest.mark.parametrize("shape,E", [((7,), 3), ((9, 2), 4), ((64, 4), 128), ((3, 5, 2), 6)])
def test_sort_by_expert(shape, E):
    from sleekit_amd import mx

    ids = np.random.default_rng(E).integers(0, E, shape)
    order, offsets = mx.sort_by_expert(torch.from_numpy(ids).cuda(), E)
    assert order.is_cuda and order.dtype == torch.int64 and offsets.is_cuda and offsets.dtype == torch.int32
    assert np.array_equal(order.cpu().numpy(), np.argsort(ids.reshape(-1), kind="stable"))
    want = np.concatenate([[0], np.cumsum(np.bincount(ids.reshape(-1), minlength=E))])
    assert tuple(offsets.shape) == (E + 1,) and np.array_equal(offsets.cpu().numpy(), want)
    o2, f2 = mx.sort_by_expert(ids.astype(np.int32), E)  # NumPy in, NumPy out; int32 ids
    assert isinstance(o2, np.ndarray) and np.array_equal(o2, order.cpu().numpy()) and f2.dtype == np.int32 and np.array_equal(f2, want)
    for bad in (E, -1, E + 1000):
        wrong = ids.copy().reshape(-1)
        wrong[len(wrong) // 2] = bad
        with pytest.raises(ValueError, match=f"0 .. {E - 1}"):
            mx.sort_by_expert(torch.from_numpy(wrong).cuda(), E)


@pytest.fixture(scope="module")
def experts():
    """E = 4 quantized experts of the synthetic 48 x 160 layer (different seeds), their biases, and the module."""
    from sleekit_amd import mx, synth

    layers = [synth.make_layer(48, 160, 4300 + e) for e in range(4)]
    results = [mx.quantize_mxfp4(L["W"], L["H"]) for L in layers]
    biases = np.random.default_rng(8).standard_normal((4, 48)).astype(np.float32)
    return results, biases, mx.MXExperts.from_results(results, biases).cuda()


@pytest.mark.parametrize("gated", [True, False])
def test_forward_tokens_against_per_expert_calls(experts, gated):
    """T = 9 tokens, k = 2 of E = 4 experts: the reference runs linear_mxfp4 of every expert on every token (float32, the
    grouped product's bits for that row), picks each token's k outputs and adds them in float64 after rounding each gated
    output to float32 and the sum to float32 -- the module's own roundings, j = 0 then 1 -- so equality is exact."""
    from sleekit_amd import mx

    results, biases, mod = experts
    T, k, E = 9, 2, 4
    rng = np.random.default_rng(12)
    x = torch.from_numpy(block_gaussian(rng, T, 160)).cuda()
    ids = np.stack([rng.permutation(E)[:k] for _ in range(T)])
    gates = rng.random((T, k)).astype(np.float32) if gated else None
    per_expert = np.stack([mx.linear_mxfp4(x, r.codes, r.scales, biases[e]).cpu().numpy() for e, r in enumerate(results)])  # (E, T, N)
    picked = np.stack([per_expert[ids[:, j], np.arange(T)] for j in range(k)], axis=1).astype(np.float64)                      # (T, k, N)
    if gated:
        picked = (picked * gates.astype(np.float64)[:, :, None]).astype(np.float32).astype(np.float64)
    want = (picked[:, 0] + picked[:, 1]).astype(np.float32)
    got = mod.forward_tokens(x, torch.from_numpy(ids).cuda(), None if gates is None else torch.from_numpy(gates).cuda())
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (T, 48)
    assert np.array_equal(bits(got), bits(want))
    for _ in range(3):
        again = mod.forward_tokens(x, torch.from_numpy(ids).cuda(), None if gates is None else torch.from_numpy(gates).cuda())
        assert np.array_equal(bits(again), bits(got))
    # forward on sorted rows is what forward_tokens runs
    order, offsets = mx.sort_by_expert(torch.from_numpy(ids).cuda(), E)
    rows = mod(x[order // k], offsets)
    assert np.array_equal(bits(rows), bits(per_expert[ids.reshape(-1), np.repeat(np.arange(T), k)][order.cpu().numpy()]))
    beyond = ids.copy()
    beyond[T // 2, 1] = E
    with pytest.raises(ValueError, match="0 .. 3"):
        mod.forward_tokens(x, torch.from_numpy(beyond).cuda())
    for call in (lambda: mod.forward_tokens(x, torch.from_numpy(ids[:5]).cuda()), lambda: mod.forward_tokens(x, torch.from_numpy(ids[:, 0]).cuda()),
                 lambda: mod.forward_tokens(x, torch.from_numpy(ids).cuda(), torch.ones((T, 3), device="cuda")),
                 lambda: mod.forward_tokens(x, torch.from_numpy(ids).cuda().float()), lambda: mod.forward_tokens(x[:, :128], torch.from_numpy(ids).cuda()),
                 lambda: mod(x, offsets[:3]), lambda: mod(x, offsets.long()), lambda: mod(x.double(), offsets)):
        with pytest.raises(ValueError):
            call()


def test_module_state_round_trip_and_repeats(experts):
    from sleekit_amd import MXExperts

    results, biases, mod = experts
    assert sorted(mod.state_dict()) == ["bias", "codes", "scales"] and tuple(mod.codes.shape) == (4, 48, 80)
    x = torch.from_numpy(block_gaussian(np.random.default_rng(4), 70, 160)).cuda()
    offsets = torch.tensor([0, 3, 3, 69, 70], dtype=torch.int32, device="cuda")   # 66 rows of one expert: the tiled form
    first = mod(x, offsets)
    copy = MXExperts(4, 160, 48).cuda()
    copy.load_state_dict(mod.state_dict())
    assert np.array_equal(bits(copy(x, offsets)), bits(first))
    for _ in range(3):
        assert np.array_equal(bits(mod(x, offsets)), bits(first))
    a4 = MXExperts.from_results(results, biases, activations="mxfp4").cuda()
    assert a4.state_dict()["_extra_state"] == {"activations": "mxfp4"}
    copy.load_state_dict(a4.state_dict())
    assert copy.activations == "mxfp4" and np.array_equal(bits(copy(x, offsets)), bits(a4(x, offsets)))
    assert not np.array_equal(bits(a4(x, offsets)), bits(first))


# ---------------------------------------------------------------------------------------------------------------- 5. quantize_experts
@pytest.mark.parametrize("act_order", ["diag", "sqerr"])
@pytest.mark.parametrize("weights", [W4, W6])
def test_quantize_experts_equals_the_single_calls(weights, act_order):
    from sleekit_amd import mx, synth

    layers = [synth.make_layer(48, 160, 5100 + 17 * e) for e in range(3)]
    single = mx.quantize_mxfp4 if weights == W4 else mx.quantize_mxfp6
    got = mx.quantize_experts(np.stack([L["W"] for L in layers]), [L["H"] for L in layers], weights=weights, act_order=act_order)
    assert len(got) == 3
    for e, (L, r) in enumerate(zip(layers, got)):
        want = single(L["W"], L["H"], act_order=act_order)
        for name in mx.MXResult._fields:
            a, b = getattr(r, name), getattr(want, name)
            assert isinstance(a, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape, (e, name)
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"expert {e}: {name} differs from the single call"
    mod = mx.MXExperts.from_results(got)
    assert mod.weights == weights and mod.codes.is_cuda and mod.bias is None
    x = torch.from_numpy(block_gaussian(np.random.default_rng(6), 5, 160)).cuda()
    y = mod(x, torch.tensor([0, 2, 2, 5], dtype=torch.int32, device="cuda"))
    linear = mx.linear_mxfp4 if weights == W4 else mx.linear_mxfp6
    assert np.array_equal(bits(y[2:]), bits(linear(x[2:], got[2].codes, got[2].scales)))
