"""The MoE route on the GPU (sleekit_amd/routing.py, sleekit_amd/csrc/moe.hip): top-k ids against the model and torch.topk,
gates bit for bit where exp is exact and against float64 elsewhere, the counting sort against torch's stable sort, the
row-mapped quantizer against the plain one on the gathered rows, the combine against forward_tokens' torch expression, and
forward_logits against forward_tokens on route_topk's ids and gates.  The shapes are the smallest at which each kernel takes
another path: E around the 64 lanes of a wave and at the register forms' limits, T past one workgroup's four waves, n around
the one-workgroup sort's 1024, a wave's chunk of 2048 and a workgroup's 8192, N around the combine's 16-byte pieces."""

import numpy as np
import pytest
import torch

import moe_route_model as model
from test_gpu_mx_experts import W4, W6, bits, block_gaussian, random_experts

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
EXPERTS = (1, 3, 63, 64, 65, 128, 1000, 1024)
KS = (1, 2, 4, 8, 16)
TOKENS = (1, 5, 67)


def device(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def as_f32(t):
    return t.float().cpu().numpy()


def topk(logits, k, gating="selected"):
    """The C entry on device logits: (ids, gates, flag) as NumPy."""
    from sleekit_amd import routing

    T, E = logits.shape
    ids, gates, flag = routing._topk(logits.contiguous(), T, E, k, gating)
    return ids.cpu().numpy(), gates.cpu().numpy(), int(flag.item())


# ---------------------------------------------------------------------------------------------------------------- top-k
_LOGITS = {}


def random_logits(dtype):
    """{(T, E): device logits of `dtype`}, made once a dtype: Gaussian rows, some of them large, so that gates spread."""
    if dtype not in _LOGITS:
        rng = np.random.default_rng(2024)
        _LOGITS[dtype] = {(T, E): device(rng.standard_normal((T, E)).astype(np.float32) * rng.choice([0.5, 3.0, 12.0], (T, 1)).astype(np.float32), dtype)
                          for T in TOKENS for E in EXPERTS}
    return _LOGITS[dtype]


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_topk_ids_equal_the_model(dtype):
    for (T, E), L in random_logits(dtype).items():
        ref = as_f32(L)
        for k in (k for k in KS if k <= E):
            ids, gates, flag = topk(L, k)
            assert flag == 0 and ids.dtype == np.int32 and gates.dtype == np.float32
            assert np.array_equal(ids, model.topk_ids(ref, k)), (T, E, k)


def test_topk_ties():
    for E, k in ((1, 1), (3, 3), (64, 16), (65, 16), (200, 16), (1024, 16)):   # all logits equal: the first k experts
        ids, gates, flag = topk(torch.full((5, E), -2.5, device="cuda"), k)
        assert flag == 0 and (ids == np.arange(k)).all(), E
    rng = np.random.default_rng(5)
    for E in (200, 1000):
        v = rng.permutation(E).astype(np.float32)
        rows = np.stack([v] * 4)
        top = float(v.max()) + 1
        rows[0, [7, 71]] = top            # the same lane, experts e and e + 64
        rows[1, [71, 7 + 128]] = top
        rows[2, [20, 21]] = top           # neighbouring lanes
        rows[3, [63, 64]] = top           # the last lane of a round and the first of the next
        ids, _, flag = topk(device(rows), 3)
        assert flag == 0 and np.array_equal(ids, model.topk_ids(rows, 3))
        assert ids[:, :2].tolist() == [[7, 71], [71, 135], [20, 21], [63, 64]]
    zeros = np.array([[-0.0, 0.0, -1.0, 0.0, -0.0], [0.0, -0.0, 1.0, -0.0, 0.0]], np.float32)   # +0 against -0
    for dtype in DTYPES:
        ids, gates, flag = topk(device(zeros, dtype), 3)
        assert flag == 0 and ids.tolist() == [[0, 1, 3], [2, 0, 1]]
        assert (gates[0] == np.float32(1) / np.float32(3)).all()
    rows = device(rng.standard_normal((67, 300)).astype(np.float32), torch.bfloat16)             # bfloat16 rows tie on their own
    ref = as_f32(rows)
    assert min(len(np.unique(r)) for r in ref) < 300
    assert np.array_equal(topk(rows, 16)[0], model.topk_ids(ref, 16))


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_topk_agrees_with_torch_on_distinct_values(dtype):
    rng = np.random.default_rng(6)
    for E in (e for e in EXPERTS if dtype != torch.bfloat16 or e <= 256):
        rows = np.stack([rng.permutation(E) - E // 2 for _ in range(5)]).astype(np.float32)   # integers: exact in every dtype
        L = device(rows, dtype)
        assert all(len(np.unique(r)) == E for r in as_f32(L)), "the test's own premise: distinct after conversion"
        for k in (k for k in KS if k <= E):
            ids, _, flag = topk(L, k)
            assert flag == 0 and np.array_equal(ids, torch.topk(L.float(), k, dim=1).indices.cpu().numpy()), (E, k)


def test_gates_bit_for_bit_where_exp_is_exact():
    one = np.float32(1)
    for E in (3, 64, 130, 1000, 1024):
        for k in (k for k in KS if k <= E):
            flat = torch.full((5, E), 1.75, device="cuda")
            assert (topk(flat, k, "selected")[1] == one / np.float32(k)).all(), (E, k)      # all selected logits equal: 1 / k
            assert (topk(flat, k, "all")[1] == one / np.float32(E)).all(), (E, k)           # all E equal: 1 / E
            masked = np.full((5, E), -np.inf, np.float32)                                    # the unselected logits are -inf
            rng = np.random.default_rng(E + k)
            chosen = np.stack([rng.permutation(E)[:k] for _ in range(5)])
            np.put_along_axis(masked, chosen, np.float32(-3.0), axis=1)
            for gating in ("selected", "all"):
                ids, gates, flag = topk(device(masked), k, gating)
                assert flag == 0 and np.array_equal(ids, np.sort(chosen, axis=1)) and (gates == one / np.float32(k)).all(), (E, k, gating)


GATE_BOUND = 2.0 ** -18
# Absolute, for one gate g = e / s against float64 on the same float32 logits.  d = v - m is rounded once (relative 2^-24,
# so an absolute |d| 2^-24 in the exponent) and expf is allowed 2 ulp (2^-22 relative, twice what the device library
# documents): a term's relative error is at most |d| 2^-24 + 2^-22, and g |d| <= 1 / e bounds the |d| part of g's.  s has the
# weighted mean of its terms' relative errors, the same bound, plus its own adds: at most 15 within a lane (E = 1024), 4 across
# a row of lanes and 2 across the rows, 21 <= 22 rounded adds of positive terms, 22 * 2^-24.  The quotient rounds once more,
# 2^-24.  With g <= 1: 2 (2^-24 / e + 2^-22) + 22 * 2^-24 + 2^-24 < 32 * 2^-24 = 2^-19 < 2^-18.


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_gates_against_float64(dtype):
    worst = 0.0
    for (T, E), L in random_logits(dtype).items():
        ref = as_f32(L)
        for k in (k for k in (1, 4, 16) if k <= E):
            for gating in ("selected", "all"):
                _, gates, _ = topk(L, k, gating)
                want = model.gates_f64(ref, k, gating)
                worst = max(worst, float(np.abs(gates - want).max()))
                if gating == "selected":
                    np.testing.assert_allclose(gates.astype(np.float64).sum(axis=1), 1.0, atol=1e-5)
    print(f"largest gate error against float64, {dtype}: {worst:.3e} = {worst * 2.0 ** 24:.2f} * 2^-24 (bound {GATE_BOUND:.3e})")
    assert worst <= GATE_BOUND


def test_flagged_rows():
    from sleekit_amd import routing

    rng = np.random.default_rng(8)
    for E, k in ((7, 4), (65, 16), (1000, 8)):
        good = rng.standard_normal((6, E)).astype(np.float32)
        cases = {"nan": good.copy(), "inf": good.copy(), "masked": good.copy()}
        cases["nan"][2, E // 2] = np.nan
        cases["inf"][2, E - 1] = np.inf
        cases["masked"][2, k - 1:] = -np.inf          # k - 1 logits left
        for name, rows in cases.items():
            with pytest.raises(ValueError, match="router logits"):
                routing.route_topk(device(rows), k)
            with pytest.raises(ValueError, match="router logits"):
                routing.route_topk(rows, k, gating="all")
            ids, gates, flag = topk(device(rows), k)
            assert flag == 1, name
            assert ((ids >= 0) & (ids < E)).all() and all(len(set(r)) == k for r in ids.tolist()), name
            assert (gates[2] == 0).all(), name
            keep = [0, 1, 3, 4, 5]
            assert np.array_equal(ids[keep], model.topk_ids(good, k)[keep]) and np.abs(gates[keep].sum(axis=1) - 1).max() < 1e-5
        edge = good.copy()
        edge[2, k:] = -np.inf                          # exactly k left: legal
        ids, gates, flag = topk(device(edge), k)
        assert flag == 0 and sorted(ids[2].tolist()) == list(range(k))
        allnan = np.full((3, E), np.nan, np.float32)   # nothing to rank: still k distinct experts
        ids, gates, flag = topk(device(allnan), k)
        assert flag == 1 and (ids == np.arange(k)).all() and (gates == 0).all()
    r = routing.route_topk(good, 8)                    # NumPy in, NumPy out
    assert all(isinstance(a, np.ndarray) for a in r) and r.expert_ids.shape == (6, 8) and r.offsets.shape == (1001,)
    r = routing.route_topk(device(good), 8)
    assert all(a.is_cuda for a in r) and [a.dtype for a in r] == [torch.int32, torch.float32, torch.int32, torch.int32, torch.int32]


# ---------------------------------------------------------------------------------------------------------------- sort
def torch_sort(ids, E):
    """What mx._sorted_by_expert does: the reference."""
    ids = ids.long()
    key, order = torch.sort(ids.clamp(0, E - 1), stable=True)
    offsets = torch.searchsorted(key, torch.arange(E + 1, device=ids.device, dtype=key.dtype), out_int32=True)
    return order, offsets


def check_sort(ids, E, want_flag=0):
    from sleekit_amd import routing

    n = ids.numel()
    order, pos, offsets, flag = routing._sort(ids, n, E)
    want_order, want_offsets = torch_sort(ids, E)
    assert int(flag.item()) == want_flag
    assert torch.equal(order.long(), want_order), (n, E)
    assert torch.equal(offsets, want_offsets), (n, E)
    assert torch.equal(pos[order.long()].long(), torch.arange(n, device="cuda")), (n, E)
    return order, pos, offsets


SORT_SIZES = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 8191, 8192, 8193)


def test_sort_equals_torch_stable_sort():
    rng = np.random.default_rng(9)
    for n in SORT_SIZES:
        for E in (5, 128):
            check_sort(device(rng.integers(0, E, n).astype(np.int32)), E)
    check_sort(device(rng.integers(0, 128, 40000).astype(np.int32)), 128)           # many chunks
    check_sort(device((rng.random(40000) ** 4 * 1000).astype(np.int32)), 1000)      # skewed, E above the counters of one round
    for n in (5, 1000, 3000):
        check_sort(torch.zeros(n, dtype=torch.int32, device="cuda"), 1)             # E = 1
        check_sort(device(rng.integers(0, 1024, n).astype(np.int32)), 1024)         # E = 1024 (n = 5 among them)
        check_sort(torch.full((n,), 3, dtype=torch.int32, device="cuda"), 7)        # all ids equal
        ids = device(np.sort(rng.integers(0, 40, n)).astype(np.int32))
        check_sort(ids, 40)                                                         # already sorted
        check_sort(ids.flip(0).contiguous(), 40)                                    # reversed


def test_sort_flags_bad_ids_and_repeats_its_bits():
    from sleekit_amd import routing

    rng = np.random.default_rng(10)
    for n in (9, 1024, 5000):
        E = 6
        ids = rng.integers(0, E, n).astype(np.int32)
        for bad in (-1, E, np.iinfo(np.int32).min, np.iinfo(np.int32).max):
            broken = ids.copy()
            broken[n // 3] = bad
            _, _, offsets = check_sort(device(broken), E, want_flag=1)              # clamped: the outputs still obey the rule
            off = offsets.cpu().numpy()
            assert off[0] == 0 and off[-1] == n and (np.diff(off) >= 0).all()
            with pytest.raises(ValueError, match="0 .. 5"):
                routing.sort_experts(device(broken), E)
        d = device(ids)
        first, again = routing._sort(d, n, E), routing._sort(d, n, E)
        assert all(torch.equal(a, b) for a, b in zip(first, again))
        order, pos, offsets = routing.sort_experts(ids.reshape(-1, 1).astype(np.int64), E)   # NumPy, int64, any shape
        want = model.sort_model(ids, E)
        assert all(a.dtype == np.int32 and np.array_equal(a, w) for a, w in zip((order, pos, offsets), want[:3]))
    with pytest.raises(ValueError, match="0 .. 5"):
        routing.sort_experts(np.array([1, 1 << 40], np.int64), 6)


# ---------------------------------------------------------------------------------------------------------------- quantizer
FORMATS = ("mxfp8", "mxfp4", "mxfp6_e2m3")


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("activations", FORMATS)
def test_mapped_quantizer_equals_the_plain_one_on_the_gathered_rows(activations, dtype):
    from sleekit_amd import mx, routing

    fmt = mx._FORMATS[activations]
    rng = np.random.default_rng(11)
    for K in (32, 160):
        for M in (1, 67):
            for div in (1, 4):
                T = 9
                x = device(block_gaussian(rng, T, K), dtype)
                rows = device(rng.integers(0, T * div, M).astype(np.int32))
                codes, scales, flags = routing._quantize_rows(x, T, K, rows, div, M, fmt.c_fmt, fmt.bits)
                want_codes, want_scales, _ = mx._quantize_act(x[(rows // div).long()].contiguous(), M, K, fmt)
                assert flags.tolist() == [0, 0] and torch.equal(codes, want_codes) and torch.equal(scales, want_scales), (K, M, div)
    # a NaN raises flag[0] where its row is mapped and not where it is not; a row index of T raises flag[1] and nothing else
    T, K, M, div = 9, 160, 67, 4
    x = device(block_gaussian(rng, T, K), dtype)
    rows = device(rng.integers(0, (T - 1) * div, M).astype(np.int32))          # row T - 1 is not mapped
    poisoned = x.clone()
    poisoned[T - 1, 40] = float("nan")
    assert routing._quantize_rows(poisoned, T, K, rows, div, M, fmt.c_fmt, fmt.bits)[2].tolist() == [0, 0]
    for value in (float("nan"), float("inf")):
        mapped = poisoned.clone()
        mapped[int(rows[5]) // div, 3] = value
        assert routing._quantize_rows(mapped, T, K, rows, div, M, fmt.c_fmt, fmt.bits)[2].tolist() == [1, 0], value
    for bad in (T * div, T * div + 3, -1, -5, np.iinfo(np.int32).max):
        beyond = rows.clone()
        beyond[11] = int(bad)
        codes, scales, flags = routing._quantize_rows(x, T, K, beyond, div, M, fmt.c_fmt, fmt.bits)
        gathered = x[(rows // div).long()].contiguous()
        gathered[11] = 0                                                        # encoded from zeros
        want_codes, want_scales, _ = mx._quantize_act(gathered, M, K, fmt)
        assert flags.tolist() == [0, 1] and torch.equal(codes, want_codes) and torch.equal(scales, want_scales), bad


# ---------------------------------------------------------------------------------------------------------------- combine
def routed_sum(y, T, k, gates):
    """The torch expression of mx._route_tokens, inlined: (T k, N) rows in (T, k) order -> the ordered float32 sum."""
    y = y.reshape(T, k, -1).float()
    total = y[:, 0] if gates is None else y[:, 0] * gates[:, 0:1]
    for j in range(1, k):
        total = total + (y[:, j] if gates is None else y[:, j] * gates[:, j:j + 1])
    return total


@pytest.mark.parametrize("y_dtype", DTYPES, ids=str)
def test_combine_equals_the_torch_expression(y_dtype):
    from sleekit_amd import routing

    rng = np.random.default_rng(12)
    for k in (1, 2, 4):
        for N in (1, 33, 257, 64, 264):          # 64 and 264 = 8 * 33 take the 16-byte pieces, the others a column a thread
            for T in (1, 37):
                n = T * k
                y = device(block_gaussian(rng, n, 32 * ((N + 31) // 32))[:, :N], y_dtype).contiguous()
                pos = device(rng.permutation(n).astype(np.int32))
                given = device(rng.standard_normal((T, k)).astype(np.float32))
                for gates in (None, given):
                    want = routed_sum(y[pos.long()], T, k, gates)
                    for out_dtype in DTYPES:
                        out, flag = routing._combine(y, pos, gates, T, k, N, out_dtype)
                        assert int(flag.item()) == 0 and out.dtype == out_dtype
                        assert np.array_equal(bits(out), bits(want.to(out_dtype))), (k, N, T, gates is None, out_dtype)
    # -0 as the only term stays -0 (the sum starts from the first term, not from 0)
    out, _ = routing._combine(torch.full((2, 8), -0.0, device="cuda"), device(np.array([1, 0], np.int32)), None, 2, 1, 8, torch.float32)
    assert (bits(out) == 0x80000000).all()
    # a pos of T k raises the flag, and that term is left out
    T, k, N = 5, 2, 33
    y = device(block_gaussian(rng, T * k, 64)[:, :N]).contiguous()
    pos = device(rng.permutation(T * k).astype(np.int32))
    gates = device(rng.standard_normal((T, k)).astype(np.float32))
    for bad in (T * k, -1):
        beyond = pos.clone()
        beyond[3] = bad                                                          # token 1, j = 1
        out, flag = routing._combine(y, beyond, gates, T, k, N, torch.float32)
        want = routed_sum(y[pos.long()], T, k, gates)
        want[1] = y[pos[2].long()] * gates[1, 0]
        assert int(flag.item()) == 1 and np.array_equal(bits(out), bits(want))


# ---------------------------------------------------------------------------------------------------------------- modules
def experts_module(mx, rng, E, K, N, activations, weights=W4, bias=True):
    mod = mx.MXExperts(E, K, N, bias=bias, activations=activations, weights=weights).cuda()
    c, s = random_experts(rng, E, N, K, 118, 123, weights)
    mod.codes.copy_(torch.from_numpy(c)), mod.scales.copy_(torch.from_numpy(s))
    if bias:
        mod.bias.copy_(torch.from_numpy(rng.standard_normal((E, N)).astype(np.float32)))
    return mod


def routes(rng):
    """(T, k, E, logits): 8 tokens take 2 of 4 experts; 5 tokens take 4 of 7 experts, two of which are masked for every token."""
    yield 8, 2, 4, device(rng.standard_normal((8, 4)).astype(np.float32))
    masked = rng.standard_normal((5, 7)).astype(np.float32)
    masked[:, [2, 5]] = -np.inf
    yield 5, 4, 7, device(masked)


LAYERS = [("mxfp8", W4), ("mxfp4", W4), ("mxfp6_e2m3", W6), ("bfloat16", W4), ("float16", W4)]   # W4A8, W4A4, W6A6, W4A16


@pytest.mark.parametrize("activations,weights", LAYERS)
def test_forward_logits_equals_forward_tokens_on_the_routed_ids(activations, weights):
    from sleekit_amd import mx, routing

    rng = np.random.default_rng(13)
    K, N = 160, 48
    for T, k, E, logits in routes(rng):
        experts = experts_module(mx, rng, E, K, N, activations, weights)
        for gating in ("selected", "all"):
            r = routing.route_topk(logits, k, gating)
            if E == 7:
                counts = np.diff(r.offsets.cpu().numpy())
                assert counts[2] == 0 and counts[5] == 0 and counts.sum() == T * k
            for x_dtype in DTYPES:
                x = device(block_gaussian(rng, T, K), x_dtype)
                got = experts.forward_logits(x, logits, k, gating)
                want = experts.forward_tokens(x, r.expert_ids, r.gates)
                assert got.dtype == x_dtype and tuple(got.shape) == (T, N)
                assert np.array_equal(bits(got), bits(want)), (T, gating, x_dtype)
        x = block_gaussian(rng, T, K)                                              # NumPy in, NumPy out
        got = experts.forward_logits(x, logits.cpu().numpy(), k)
        assert isinstance(got, np.ndarray) and np.array_equal(bits(got), bits(experts.forward_logits(device(x), logits, k)))


@pytest.mark.parametrize("fused", [True, False])
def test_mlp_forward_logits_equals_forward_tokens(fused):
    from sleekit_amd import mx, routing

    rng = np.random.default_rng(14)
    K, N, Nd = 160, 96, 48
    for T, k, E, logits in routes(rng):
        mlp = mx.MXExpertsMLP(experts_module(mx, rng, E, K, 2 * N, "mxfp8"), experts_module(mx, rng, E, N, Nd, "mxfp8"),
                              alpha=1.702, limit=7.0, shift=1.0, interleaved=True)
        r = routing.route_topk(logits, k)
        x = device(block_gaussian(rng, T, K))
        got = mlp.forward_logits(x, logits, k, fused=fused)
        assert tuple(got.shape) == (T, Nd)
        assert np.array_equal(bits(got), bits(mlp.forward_tokens(x, r.expert_ids, r.gates, fused=fused)))
        assert np.array_equal(bits(got), bits(mlp.forward_logits(x, logits, k, fused=not fused)))


def test_forward_logits_behind_a_rotation():
    from sleekit_amd import mx, rotation

    rng = np.random.default_rng(15)
    K, N, Nd = 160, 96, 48
    R = rotation.Rotation(K, block=32, seed=3)
    for T, k, E, logits in routes(rng):
        x = device(block_gaussian(rng, T, K))
        rotated = R.apply(x, dtype=torch.float32)
        for activations in ("mxfp8", "mxfp4"):
            experts = experts_module(mx, rng, E, K, N, activations)
            assert np.array_equal(bits(experts.forward_logits(x, logits, k, rotation=R)), bits(experts.forward_logits(rotated, logits, k)))
        half = experts_module(mx, rng, E, K, N, "bfloat16")
        assert np.array_equal(bits(half.forward_logits(x, logits, k, rotation=R)),
                              bits(half.forward_logits(R.apply(x, dtype=torch.bfloat16).float(), logits, k)))
        mlp = mx.MXExpertsMLP(experts_module(mx, rng, E, K, 2 * N, "mxfp8"), experts_module(mx, rng, E, N, Nd, "mxfp8"))
        assert np.array_equal(bits(mlp.forward_logits(x, logits, k, rotation=R)), bits(mlp.forward_logits(rotated, logits, k)))


def test_forward_logits_messages():
    from sleekit_amd import mx

    rng = np.random.default_rng(16)
    T, k, E, K, N = 8, 2, 4, 64, 32
    experts = experts_module(mx, rng, E, K, N, "mxfp8")
    mlp = mx.MXExpertsMLP(experts_module(mx, rng, E, K, 2 * N, "mxfp8"), experts_module(mx, rng, E, N, 16, "mxfp8"))
    x = device(block_gaussian(rng, T, K))
    logits = device(rng.standard_normal((T, E)).astype(np.float32))
    bad_logits, bad_x = logits.clone(), x.clone()
    bad_logits[3, 1] = float("nan")
    bad_x[5, 7] = float("nan")
    for module in (experts, mlp):
        with pytest.raises(ValueError, match="router logits"):
            module.forward_logits(x, bad_logits, k)
        with pytest.raises(ValueError, match="activations must be finite"):
            module.forward_logits(bad_x, logits, k)
        with pytest.raises(ValueError, match="router logits"):          # both: the logits' message comes first
            module.forward_logits(bad_x, bad_logits, k)
        with pytest.raises(ValueError, match=r"logits must be \(8, 4\)"):
            module.forward_logits(x, logits[:, :3], k)
        with pytest.raises(ValueError, match=r"logits must be \(8, 4\)"):
            module.forward_logits(x, logits[:5], k)
        with pytest.raises(ValueError, match="x has 32 columns"):
            module.forward_logits(x[:, :32].contiguous(), logits, k)
