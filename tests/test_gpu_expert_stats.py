"""The expert-grouped running statistics on the MI355X (slk_hessian_accumulate_experts, slk_hessian_accumulate_experts_mx,
sleekit_amd.ExpertStatistics) against tests/expert_stats_model.py.

What is held:
  * float rows, exact inputs (stats_model's integers and three-piece builders): H, mean and counts bit for bit the model's
    on both paths, over two batches with different routing, from a count past 2^31, H bit-wise symmetric;
  * float rows, random data: bit for bit the loop of slk_hessian_accumulate over the slices, on both paths;
  * experts without rows, and the bytes behind every buffer, come back as the same bits; offsets that break the rule change
    nothing, raise the flag and, through ExpertStatistics, a ValueError;
  * coded rows of the three activation formats: on inputs whose float64 product is asserted exact in float32 in any order of
    summation, bit for bit the model on the decoded rows (E4M3's two NaN codes are no values and are left out: with them no
    product is exact); on random codes, per entry |H - H64| <= T_e 2^-23 (|X|^T |X|) / c';
  * the calibration recipe of INTEGRATION.md, end to end.
tests/test_expert_stats_cpu.py shows, without a GPU, that each comparison here fails for each mistake it is there to find.
"""

import numpy as np
import pytest
import torch

import expert_stats_model as xm
import stats_model as sm

pytestmark = pytest.mark.gpu

GUARD = 64  # floats behind H and mean, int64 behind counts, that must come back as they were


def host(t):
    return t.detach().cpu().numpy()


def cuda(a):
    return torch.from_numpy(np.array(a)).cuda()


class State:
    """H, mean and counts on the device, each with a guard band behind it."""

    def __init__(self, E, n, start=None, fill=None):
        self.E, self.n = E, n
        self.h = torch.zeros(E * n * n + GUARD, dtype=torch.float32, device="cuda")
        self.m = torch.zeros(E * n + GUARD, dtype=torch.float32, device="cuda")
        self.c = torch.zeros(E + GUARD, dtype=torch.int64, device="cuda")
        self.h[E * n * n:] = float("nan")
        self.m[E * n:] = float("nan")
        self.c[E:] = -7
        if start is not None:
            self.c[:E] = cuda(np.array(start, np.int64))
        if fill is not None:  # (experts to pre-fill with the sentinel bit pattern)
            bits = torch.full((1,), int(np.float32(xm.SENTINEL).view(np.int32)), dtype=torch.int32, device="cuda").view(torch.float32)
            for e in fill:
                self.h[e * n * n:(e + 1) * n * n] = bits
                self.m[e * n:(e + 1) * n] = bits
        self.guards = self.bands()

    def bands(self):
        E, n = self.E, self.n
        return [host(self.h[E * n * n:]).view(np.uint32).copy(), host(self.m[E * n:]).view(np.uint32).copy(), host(self.c[E:]).copy()]

    def get(self):
        E, n = self.E, self.n
        return host(self.h[:E * n * n]).reshape(E, n, n), host(self.m[:E * n]).reshape(E, n), host(self.c[:E])

    def assert_guards(self, what):
        for name, before, after in zip(("H", "mean", "counts"), self.guards, self.bands()):
            assert np.array_equal(before, after), f"{what}: the bytes behind {name} changed"


def workspace(E, n, M, ws):
    from sleekit_amd import _device as dev, _lib

    if ws is None:
        return 0, 0
    scratch, _ = dev.scratch(_lib.lib.slk_hessian_experts_workspace_bytes(E, n, M), "expert_stats_test")
    return scratch.data_ptr(), int(_lib.lib.slk_hessian_experts_workspace_bytes(E, n, M))


def accumulate_experts(state, X, offsets, ws="full"):
    """slk_hessian_accumulate_experts on device tensors; returns the flag.  ws: "full" or None (a NULL workspace)."""
    from sleekit_amd import _device as dev, _lib

    Xd, od = cuda(X), cuda(np.asarray(offsets, np.int32))
    M, n = Xd.shape
    flag = torch.full((1,), 9, dtype=torch.int32, device="cuda")
    ptr, nbytes = workspace(state.E, n, M, ws)
    _lib.check(_lib.lib.slk_hessian_accumulate_experts(state.h.data_ptr(), state.m.data_ptr(), Xd.data_ptr(), od.data_ptr(), state.E, n, M,
                                                       state.c.data_ptr(), flag.data_ptr(), ptr, nbytes, dev.stream_handle()))
    return int(flag.item())


def accumulate_codes(state, a_codes, a_scales, offsets, activations, ws="full"):
    """slk_hessian_accumulate_experts_mx on device tensors; returns the two flags."""
    from sleekit_amd import _device as dev, _lib, mx

    ac, asc, od = cuda(a_codes), cuda(a_scales), cuda(np.asarray(offsets, np.int32))
    M, n = asc.shape[0], asc.shape[1] * 32
    flag = torch.full((2,), 9, dtype=torch.int32, device="cuda")
    ptr, nbytes = workspace(state.E, 32, M, ws)
    _lib.check(_lib.lib.slk_hessian_accumulate_experts_mx(state.h.data_ptr(), state.m.data_ptr(), ac.data_ptr(), asc.data_ptr(),
                                                          mx._activations(activations).c_fmt, od.data_ptr(), state.E, n, M, state.c.data_ptr(),
                                                          flag.data_ptr(), ptr, nbytes, dev.stream_handle()))
    return tuple(int(v) for v in flag.tolist())


def assert_state(got, want, what):
    for name, g, w in zip(("H", "mean"), got[:2], want[:2]):
        if not sm.same_bits(g, w):
            at = sm.first_difference(g, w)
            raise AssertionError(f"{what}: {name} first differs at {at}: got {float(g[at])!r}, want {float(w[at])!r}; "
                                 f"{int((np.asarray(g).view(np.uint32) != np.asarray(w).view(np.uint32)).sum())} entries differ")
    assert np.array_equal(got[2], want[2]), f"{what}: counts {got[2]} != {want[2]}"


# ------------------------------------------------------------------------------------ 1. float rows, exact inputs, the model
EXACT_CASES = [(n, False, "full") for n in xm.EXACT_F32_N] + [(n, True, "full") for n in xm.EXACT_BF16_N] + \
    [(n, False, None) for n in xm.EXACT_BF16_N]


@pytest.mark.parametrize("n,pieces,ws", EXACT_CASES)
def test_exact_inputs_match_the_model(n, pieces, ws):
    """Counts (0, 1, 17, 33, 0, 64), then other routing in which two experts that had rows have none; n = 130 and 260 on the
    float32 chain, 128 and 256 with a full workspace (bfloat16 x 3, three-piece inputs) and with none; one expert starts from
    a count of 2^31 + 5."""
    E = len(xm.EXACT_COUNTS[0])
    batches = xm.exact_batches(n, pieces)
    start = np.zeros(E, np.int64)
    start[xm.BIG_COUNT_EXPERT] = xm.BIG_COUNT
    state = State(E, n, start)
    want = xm.zero_state(E, n)[:2] + (start,)
    for b, (X, offsets) in enumerate(batches):
        assert accumulate_experts(state, X, offsets, ws) == 0
        want = xm.accumulate_experts_model(*want, X, offsets, pieces=pieces, exact=True)[:3]
        got = state.get()
        assert_state(got, want, f"n = {n}, batch {b}")
        assert xm.bitwise_symmetric(got[0]), f"n = {n}, batch {b}: H is not bit-wise symmetric"
    state.assert_guards(f"n = {n}")


# ------------------------------------------------------------------------------ 2. float rows, random data, the single call
@pytest.mark.parametrize("ws", ["full", None])
def test_random_data_is_the_single_call_on_each_slice(ws):
    from sleekit_amd import _device as dev, _lib

    n, counts = xm.RANDOM_N, xm.RANDOM_COUNTS
    E, M = len(counts), sum(counts)
    offsets = xm.offsets_of(counts)
    state, single = State(E, n), State(E, n)
    before = np.zeros(E, np.int64)
    for b in range(2):
        X = cuda(sm.block_gaussian(M, n, 90 + b))
        assert accumulate_experts(state, X.cpu().numpy(), offsets, ws) == 0
        for e in range(E):
            T = counts[e]
            if T == 0:
                continue
            room = 4096 + 6 * n * ((T + 31) // 32 * 32)  # the single call whose workspace holds all T_e tokens
            scratch, _ = dev.scratch(room, "expert_stats_single")
            H = single.h[e * n * n:(e + 1) * n * n]
            m = single.m[e * n:(e + 1) * n]
            _lib.check(_lib.lib.slk_hessian_accumulate(H.data_ptr(), m.data_ptr(), X[offsets[e]:].data_ptr(), n, T, int(before[e]),
                                                       scratch.data_ptr() if ws else 0, room if ws else 0, dev.stream_handle()))
            before[e] += T
        got, want = state.get(), single.get()
        assert_state(got, (want[0], want[1], before), f"batch {b}, workspace {ws}")
    state.assert_guards("random data")


# --------------------------------------------------------------------------------------------------------- 3. untouched memory
@pytest.mark.parametrize("n,ws", [(130, "full"), (128, "full"), (128, None)])
def test_experts_without_rows_and_guard_bands_keep_their_bits(n, ws):
    counts = xm.EXACT_COUNTS[0]
    E, empty = len(counts), [e for e, c in enumerate(counts) if c == 0]
    X, offsets = xm.exact_batches(n, False)[0]
    state = State(E, n, fill=empty)
    before = state.get()
    assert accumulate_experts(state, X, offsets, ws) == 0
    got = state.get()
    for e in empty:
        assert sm.same_bits(got[0][e], before[0][e]) and sm.same_bits(got[1][e], before[1][e]) and got[2][e] == 0, f"expert {e} has no rows"
    want = xm.accumulate_experts_model(*before, X, offsets, pieces=bool(ws) and n % 128 == 0)[:3]
    assert_state(got, want, f"n = {n}")
    state.assert_guards(f"n = {n}")


# ------------------------------------------------------------------------------------------------ 4. offsets that break the rule
@pytest.mark.parametrize("how", sorted(xm.BROKEN_OFFSETS))
def test_offsets_that_break_the_rule_change_nothing(how):
    import sleekit_amd
    from sleekit_amd import mx

    n = 128
    counts = xm.EXACT_COUNTS[0]
    E = len(counts)
    X, offsets = xm.exact_batches(n, False)[0]
    broken = xm.BROKEN_OFFSETS[how](np.array(offsets))
    assert not xm.offsets_valid(broken, X.shape[0])
    for ws in ("full", None):
        state = State(E, n, start=np.arange(E), fill=range(E))
        before = state.get()
        assert accumulate_experts(state, X, broken, ws) == 1
        assert_state(state.get(), before, f"{how}, workspace {ws}")
        state.assert_guards(how)
    a_codes, a_scales, _ = xm.exact_codes("mxfp8", 32)
    cstate = State(len(xm.CODED_COUNTS), 32, fill=range(len(xm.CODED_COUNTS)))
    before = cstate.get()
    assert accumulate_codes(cstate, a_codes, a_scales, xm.BROKEN_OFFSETS[how](xm.offsets_of(xm.CODED_COUNTS)), "mxfp8") == (1, 0)
    assert_state(cstate.get(), before, f"{how}, coded rows")
    stats = sleekit_amd.ExpertStatistics(E, n)
    with pytest.raises(ValueError) as err:
        stats.add_batch(cuda(X), cuda(broken))
    assert str(err.value) == mx._OFFSETS_RULE
    assert not host(stats.hessian).any() and not host(stats.counts).any()


# ------------------------------------------------------------------------------------------- 5. coded rows, exact inputs, the model
@pytest.mark.parametrize("n", xm.CODED_N)
@pytest.mark.parametrize("activations", xm.FORMATS)
def test_coded_rows_match_the_model(activations, n):
    import sleekit_amd

    a_codes, a_scales, X = xm.exact_codes(activations, n)
    counts = xm.CODED_COUNTS
    E, M, offsets = len(counts), sum(counts), xm.offsets_of(counts)
    for ws in ("full", None):
        state = State(E, n)
        assert accumulate_codes(state, a_codes, a_scales, offsets, activations, ws) == (0, 0)
        want = xm.accumulate_codes_model(*xm.zero_state(E, n), a_codes, a_scales, offsets, activations, exact=True)
        assert want[3] == 0
        got = state.get()
        assert_state(got, want[:3], f"{activations}, n = {n}, workspace {ws}")
        assert xm.bitwise_symmetric(got[0])
        state.assert_guards(activations)
    # E = 1: the dense case, all rows, on top of a count
    dense = sleekit_amd.ExpertStatistics(1, n)
    dense.counts += 3
    dense.add_codes(cuda(a_codes), cuda(a_scales), cuda(np.array([0, M], np.int32)), activations)
    want = xm.accumulate_codes_model(*xm.zero_state(1, n)[:2], np.array([3]), a_codes, a_scales, [0, M], activations, exact=True)
    assert_state((host(dense.hessian), host(dense.mean), host(dense.counts)), want[:3], f"{activations}, n = {n}, E = 1")


@pytest.mark.parametrize("activations", xm.FORMATS)
def test_a_nan_scale_byte_raises_the_flag(activations):
    import sleekit_amd

    a_codes, a_scales, _ = xm.exact_codes(activations, 32)
    a_scales = np.array(a_scales)
    a_scales[20, 0] = 255
    offsets = xm.offsets_of(xm.CODED_COUNTS)
    state = State(len(xm.CODED_COUNTS), 32)
    assert accumulate_codes(state, a_codes, a_scales, offsets, activations) == (0, 1)
    stats = sleekit_amd.ExpertStatistics(len(xm.CODED_COUNTS), 32)
    with pytest.raises(ValueError, match="255"):
        stats.add_codes(cuda(a_codes), cuda(a_scales), cuda(offsets), activations)


# ------------------------------------------------------------------------------------------ 6. coded rows, random codes, the bound
@pytest.mark.parametrize("activations", xm.FORMATS)
def test_random_codes_within_the_summation_bound(activations):
    """First batch, scale bytes 100 .. 150, T_e up to 130: per entry |H - H64| <= T_e 2^-23 (|X|^T |X|) / c'.
    Measured on the MI355X (largest ratio to the bound over the experts): see DESIGN.md section 28."""
    a_codes, a_scales, X = xm.random_codes(activations)
    counts = xm.RANDOM_CODED_COUNTS
    E, n, offsets = len(counts), xm.RANDOM_CODED_N, xm.offsets_of(counts)
    state = State(E, n)
    assert accumulate_codes(state, a_codes, a_scales, offsets, activations) == (0, 0)
    H, mean, got_counts = state.get()
    assert np.array_equal(got_counts, counts)
    worst = 0.0
    for e, T in enumerate(counts):
        Xe = X[offsets[e]:offsets[e + 1]]
        if T == 0:
            assert not H[e].any() and not mean[e].any()
            continue
        ratio = xm.coded_ratio(H[e], Xe, T)
        print(f"{activations}: expert {e}, T = {T}: max |H - H64| / bound = {ratio:.4f}")
        worst = max(worst, ratio)
        m64 = Xe.sum(axis=0) / T
        mb = T * 2.0 ** -23 * np.abs(Xe).sum(axis=0) / T
        assert (np.abs(mean[e] - m64) <= mb).all()
    print(f"{activations}: largest ratio {worst:.4f}")
    assert worst <= 1.0, f"{activations}: |H - H64| is {worst:.3f} of the bound"
    assert xm.bitwise_symmetric(H)


# ------------------------------------------------------------------------------------------------------------- 7. the recipe
def test_the_calibration_recipe_end_to_end():
    """up statistics from routed tokens -> quantize_experts -> MXExperts -> the fused gate/up product's h as codes -> down
    statistics from those codes -> quantize_experts -> MXExpertsMLP.  E = 3 experts of (64, 160) up layers (2 N = 64) and
    (160, 32) down layers, k = 2."""
    import sleekit_amd
    from sleekit_amd import mx

    E, K, N, T, k = 3, 160, 32, 48, 2
    rng = np.random.default_rng(5)
    x = cuda(rng.standard_normal((T, K)).astype(np.float32))
    ids = cuda(np.stack([rng.permutation(E)[:k] for _ in range(T)]).astype(np.int64))
    W_up = [cuda((rng.standard_normal((2 * N, K)) * 0.2).astype(np.float32)) for _ in range(E)]
    W_down = [cuda((rng.standard_normal((K, N)) * 0.2).astype(np.float32)) for _ in range(E)]
    activations = "mxfp4"

    up_stats = sleekit_amd.ExpertStatistics(E, K)
    up_stats.add_tokens(x, ids)
    order, offsets = mx.sort_by_expert(ids, E)
    rows = x[order // k]
    off = host(offsets)
    assert np.array_equal(host(up_stats.counts), np.diff(off))
    model = xm.accumulate_experts_model(*xm.zero_state(E, K), host(rows), off)  # (n = 160: the float32 chain; bit equality is test 2's)
    assert np.array_equal(host(up_stats.counts), model[2])
    assert np.allclose(host(up_stats.hessian), model[0], rtol=1e-5, atol=1e-6)

    up_results = mx.quantize_experts(W_up, up_stats.hessians())
    assert len(up_results) == E
    up = mx.MXExperts.from_results(up_results, activations=activations)
    ac, asc = mx.quantize_mxfp4_act(rows)
    hc, hs = mx.matmul_mx_glu_experts(ac, asc, up.codes, up.scales, offsets, activations=activations)
    gate = (1.0, None, 0.0, False)
    hc2, hs2, bad, flag = mx._matmul_mx_glu_experts(ac, asc, up.codes, up.scales, offsets, None, activations, "mxfp4", *gate, fused=False)
    assert int(bad.item()) == 0 and int(flag.item()) == 0

    down_stats, down_unfused = sleekit_amd.ExpertStatistics(E, N), sleekit_amd.ExpertStatistics(E, N)
    down_stats.add_codes(hc, hs, offsets, activations)
    down_unfused.add_codes(hc2, hs2, offsets, activations)
    got = (host(down_stats.hessian), host(down_stats.mean), host(down_stats.counts))
    assert_state(got, (host(down_unfused.hessian), host(down_unfused.mean), host(down_unfused.counts)), "fused against unfused h")
    h = xm.decode(host(hc), host(hs), activations)
    for e in range(E):
        assert xm.exact_products(h[off[e]:off[e + 1]]), f"expert {e}: the products of this h are not exact in float32"
    want = xm.accumulate_codes_model(*xm.zero_state(E, N), host(hc), host(hs), off, activations, exact=True)
    assert_state(got, want[:3], "down statistics against the model on the decoded h")

    down_results = mx.quantize_experts(W_down, down_stats.hessians())
    assert len(down_results) == E
    mlp = mx.MXExpertsMLP.from_results(up_results, down_results, activations=activations)
    y = mlp.forward_tokens(x, ids)
    assert tuple(y.shape) == (T, K) and bool(torch.isfinite(y).all())

    # an expert never routed to: the identity stands in for its zero matrix, and GPTQ under H = I is round-to-nearest
    partial = sleekit_amd.ExpertStatistics(E, K)
    partial.add_tokens(x, torch.where(ids == 1, torch.full_like(ids, 2), ids)[:, :1])
    assert int(partial.counts[1].item()) == 0 and not host(partial.hessians(fill_unseen=False)[1]).any()
    Hs = partial.hessians()
    assert np.array_equal(host(Hs[1]), np.eye(K, dtype=np.float32)) and sm.same_bits(host(Hs[0]), host(partial.hessian[0]))
    unseen = mx.quantize_experts(W_up, Hs)[1]
    alone = mx.quantize_mxfp4(W_up[1], torch.eye(K, device="cuda"))
    assert np.array_equal(host(unseen.codes), host(alone.codes)) and np.array_equal(host(unseen.scales), host(alone.scales))
