"""Without a GPU: the expert-grouped statistics' entries exist and refuse bad arguments before any launch, the workspace
function follows its documented formula, tests/expert_stats_model.py gives hand-computed tiny cases, and every comparison of
tests/test_gpu_expert_stats.py fails for each mistake it is there to find (the model's mutations)."""

import os

import numpy as np
import pytest

import expert_stats_model as xm
import stats_model as sm


# ------------------------------------------------------------------------------------------------------------- the entries
NEW = ("slk_hessian_experts_workspace_bytes", "slk_hessian_accumulate_experts", "slk_hessian_accumulate_experts_mx")


def test_library_exports_the_entries_and_lib_declares_them():
    import sleekit_amd
    from sleekit_amd import _lib

    for name in NEW:
        assert name in _lib.PROTOTYPES and hasattr(_lib.lib, name), name
    assert len(_lib.PROTOTYPES["slk_hessian_accumulate_experts"][1]) == 12
    assert len(_lib.PROTOTYPES["slk_hessian_accumulate_experts_mx"][1]) == 14
    assert _lib.lib.slk_abi_version() == 8
    assert sleekit_amd.ExpertStatistics is sleekit_amd.statistics.ExpertStatistics
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "sleekit_amd.h")) as f:
        header = f.read()
    for name in NEW:
        assert name + "(" in header, name


def test_workspace_bytes_follow_the_documented_formula():
    from sleekit_amd import _lib

    f = _lib.lib.slk_hessian_experts_workspace_bytes

    def formula(E, n, M):
        table = (32 * (1 + E) + 255) // 256 * 256
        return table + (6 * n * 32 * (M // 32 + min(E, M)) if n % 128 == 0 else 0)

    for E, n, M in ((1, 128, 1), (6, 256, 115), (6, 130, 115), (128, 4096, 32768), (1024, 2880, 64), (7, 32, 1), (1024, 128, 5), (33, 384, 31)):
        assert f(E, n, M) == formula(E, n, M), (E, n, M)
    assert f(1, 128, 1) == 256 + 6 * 128 * 32
    for E, n, M in ((0, 128, 4), (4, 0, 4), (4, 128, 0), (-1, 128, 4), (4, -128, 4), (4, 128, -4)):
        assert f(E, n, M) == 0, (E, n, M)


def test_argument_errors_do_not_touch_the_gpu():
    from sleekit_amd import _lib

    lib, p = _lib.lib, 4096  # (an aligned address that is never followed)
    big = 1 << 20

    def f32(H=p, mean=p, X=p, offsets=p, E=4, n=128, M=8, counts=p, flag=p, ws=p, ws_bytes=big):
        return lib.slk_hessian_accumulate_experts(H, mean, X, offsets, E, n, M, counts, flag, ws, ws_bytes, None)

    def coded(H=p, mean=p, ac=p, asc=p, fmt=_lib.MX_ACT_FP8, offsets=p, E=4, n=128, M=8, counts=p, flag=p, ws=p, ws_bytes=big):
        return lib.slk_hessian_accumulate_experts_mx(H, mean, ac, asc, fmt, offsets, E, n, M, counts, flag, ws, ws_bytes, None)

    for call in (f32, coded):
        for E in (0, -1, _lib.MX_MAX_EXPERTS + 1):
            assert call(E=E) == _lib.E_ARG and b"E must be" in lib.slk_last_error(), E
        for kw in (dict(n=0), dict(n=-32), dict(M=0), dict(M=-1)):
            assert call(**kw) == _lib.E_ARG and b"at least 1" in lib.slk_last_error(), kw
        for name in ("H", "mean", "offsets", "counts", "flag"):
            assert call(**{name: None}) == _lib.E_ARG and b"null" in lib.slk_last_error(), name
        assert call(ws=p + 4) == _lib.E_ARG and b"aligned" in lib.slk_last_error()
        assert call(ws_bytes=32 * 5 - 1) == _lib.E_ARG and b"too small" in lib.slk_last_error()
        assert call(ws_bytes=0) == _lib.E_ARG and b"too small" in lib.slk_last_error()
    assert f32(X=None) == _lib.E_ARG and b"null X" in lib.slk_last_error()
    for name in ("ac", "asc"):
        assert coded(**{name: None}) == _lib.E_ARG and b"null" in lib.slk_last_error(), name
    assert coded(ac=p + 8) == _lib.E_ARG and b"aligned" in lib.slk_last_error()
    for n in (16, 48, 130):
        assert coded(n=n) == _lib.E_ARG and b"32" in lib.slk_last_error(), n
    for fmt in (-1, 3):
        assert coded(fmt=fmt) == _lib.E_ARG and b"a_fmt" in lib.slk_last_error(), fmt


def test_expert_statistics_checks_its_arguments_before_the_gpu():
    import sleekit_amd

    for E in (0, -1, 1025, 2.0, True):
        with pytest.raises(ValueError, match="num_experts"):
            sleekit_amd.ExpertStatistics(E, 32, device="cuda")
    for n in (0, -32, 1.5):
        with pytest.raises(ValueError, match="features"):
            sleekit_amd.ExpertStatistics(4, n, device="cuda")
    with pytest.raises(RuntimeError, match="GPU"):
        sleekit_amd.ExpertStatistics(4, 32, device="cpu")


# --------------------------------------------------------------------------------------------------------------- the model
def test_model_on_hand_computed_cases():
    # two experts of one feature: rows (2), (4, 6); expert 0 had 1 token of mean 1 and H 1
    X = np.array([[2.0], [4.0], [6.0]], np.float32)
    H, mean, counts, flag = xm.accumulate_experts_model(np.array([[[1.0]], [[0.0]]]), np.array([[1.0], [0.0]]), [1, 0], X, [0, 1, 3])
    assert flag == 0 and counts.tolist() == [2, 2]
    assert H[0, 0, 0] == np.float32(1 * 0.5 + 4 / 2) and mean[0, 0] == np.float32(1 * 0.5 + 2 / 2)
    assert H[1, 0, 0] == np.float32((16 + 36) / 2) and mean[1, 0] == np.float32(5.0)
    # an expert without rows keeps its bits, here a NaN's payload
    H0 = np.full((2, 1, 1), xm.SENTINEL, np.float32)
    H, mean, counts, flag = xm.accumulate_experts_model(H0, np.zeros((2, 1)), [7, 0], X, [0, 0, 3])
    assert sm.same_bits(H[0], H0[0]) and counts.tolist() == [7, 3] and mean[1, 0] == np.float32(4.0)
    # two features: the cross term, mirrored
    X2 = np.array([[1.0, 2.0], [3.0, -1.0]], np.float32)
    H, mean, counts, _ = xm.accumulate_experts_model(np.zeros((1, 2, 2)), np.zeros((1, 2)), [0], X2, [0, 2])
    assert H[0].tolist() == [[5.0, -0.5], [-0.5, 2.5]] and mean[0].tolist() == [2.0, 0.5]
    # offsets that break the rule: nothing changes, the flag is 1
    for bad in ([1, 1, 3], [0, 2, 1, 3][:3], [0, 1, 2], [0, 3]):
        H, mean, counts, flag = xm.accumulate_experts_model(H0, np.ones((2, 1)), [7, 9], X, bad)
        assert flag == 1 and sm.same_bits(H, H0) and counts.tolist() == [7, 9] and mean.tolist() == [[1.0], [1.0]]
    # a count past 2^24 rounds in cnt, and f is formed from the quotient in float64
    big = 2 ** 31 + 5
    H, _, counts, _ = xm.accumulate_experts_model(np.ones((1, 1, 1)), np.zeros((1, 1)), [big], X[:1], [0, 1])
    assert counts[0] == big + 1 and H[0, 0, 0] == np.float32(np.float32(1.0) * np.float32(big / (big + 1)) + np.float32(4.0) / np.float32(big + 1))


def test_model_decodes_the_three_formats():
    # one row of one block each: code 1 of every format at scale byte 128 (2^1)
    for activations, smallest in (("mxfp8", 2.0 ** -9), ("mxfp4", 0.5), ("mxfp6_e2m3", 0.125)):
        codes = np.zeros((1, 32), np.uint8)
        codes[0, 0], codes[0, 1] = 1, 1 | xm.SIGN[activations]
        X = xm.decode(xm.PACK[activations](codes), np.array([[128]], np.uint8), activations)
        assert X[0, 0] == 2 * smallest and X[0, 1] == -2 * smallest and not X[0, 2:].any(), activations
        H, mean, counts, flag = xm.accumulate_codes_model(*xm.zero_state(1, 32), xm.PACK[activations](codes), np.array([[128]], np.uint8), [0, 1], activations)
        assert flag == 0 and H[0, 0, 0] == 4 * smallest ** 2 and H[0, 0, 1] == -4 * smallest ** 2 and H[0, 1, 0] == H[0, 0, 1] and counts[0] == 1
        assert xm.accumulate_codes_model(*xm.zero_state(1, 32), xm.PACK[activations](codes), np.array([[255]], np.uint8), [0, 1], activations)[3] == 2
    assert xm.exact_products(np.array([[1.0, 3.0], [0.5, 0.0]])) and not xm.exact_products(np.array([[2.0 ** 13, 1.0], [2.0 ** -13, 1.0]]))


def test_coded_builders_hold_what_they_promise():
    for activations in xm.FORMATS:
        for n in xm.CODED_N:
            a_codes, a_scales, X = xm.exact_codes(activations, n)  # (asserts coverage and exactness)
            assert a_scales.min() == 125 and a_scales.max() == 129 and X.shape == (sum(xm.CODED_COUNTS), n)
            offsets = xm.offsets_of(xm.CODED_COUNTS)
            for e in range(len(xm.CODED_COUNTS)):
                assert xm.exact_products(X[offsets[e]:offsets[e + 1]])
            assert np.array_equal(X.astype(np.float32).astype(np.float64), X)
            assert np.array_equal(sm.bf16_round(X.astype(np.float32)).astype(np.float64), X), "every decoded value is a bfloat16"
        a_codes, a_scales, X = xm.random_codes(activations)
        assert a_scales.min() == 100 and a_scales.max() == 150 and np.isfinite(X).all()
        assert np.array_equal(sm.bf16_round(X.astype(np.float32)).astype(np.float64), X)


# ----------------------------------------------------------------------------------------------------------- the mutations
FLOAT_MUTATIONS = (dict(slice_from_next=True), dict(factor_from="next"), dict(factor_from="M"), dict(scale_empty=True),
                   dict(counts_not_advanced=True), dict(token_past_bound=True))


def differs(a, b):
    return not xm.same_state(a, b)


@pytest.mark.parametrize("n,pieces", [(130, False), (128, True), (128, False)])
def test_every_mutation_changes_the_exact_comparison(n, pieces):
    """test_exact_inputs_match_the_model: the state after the two batches, from the count past 2^31."""
    E = len(xm.EXACT_COUNTS[0])
    start = np.zeros(E, np.int64)
    start[xm.BIG_COUNT_EXPERT] = xm.BIG_COUNT
    batches = xm.exact_batches(n, pieces)
    true = xm.run_batches(batches, E, n, start, pieces, exact=True)
    assert xm.bitwise_symmetric(true[0])
    for mutation in FLOAT_MUTATIONS:
        assert differs(xm.run_batches(batches, E, n, start, pieces, **mutation), true), mutation
    # stats_model's own mutations of one expert's update show through the grouped comparison as well: the second batch on
    # the first batch's state with a wrong first state
    wrong = list(xm.run_batches(batches[:1], E, n, start, pieces))
    wrong[0] = wrong[0].copy()
    wrong[0][3] = np.triu(wrong[0][3])  # (no mirror)
    X, offsets = batches[1]
    assert differs(xm.accumulate_experts_model(*wrong, X, offsets, pieces=pieces)[:3], true)


def test_every_mutation_changes_the_sentinel_comparison():
    """test_experts_without_rows_and_guard_bands_keep_their_bits: sentinel-filled experts without rows."""
    n = 130
    counts = xm.EXACT_COUNTS[0]
    E, empty = len(counts), [e for e, c in enumerate(counts) if c == 0]
    X, offsets = xm.exact_batches(n, False)[0]
    H, mean, c = xm.zero_state(E, n)
    H[empty], mean[empty] = xm.SENTINEL, xm.SENTINEL
    true = xm.accumulate_experts_model(H, mean, c, X, offsets)[:3]
    for e in empty:
        assert sm.same_bits(true[0][e], H[e]) and sm.same_bits(true[1][e], mean[e])
    mutated = xm.accumulate_experts_model(H, mean, c, X, offsets, scale_empty=True)[:3]
    assert differs(mutated, true) and not sm.same_bits(mutated[0][empty[0]], H[empty[0]])
    for mutation in FLOAT_MUTATIONS:
        assert differs(xm.accumulate_experts_model(H, mean, c, X, offsets, **mutation)[:3], true), mutation


@pytest.mark.parametrize("n", xm.CODED_N)
@pytest.mark.parametrize("activations", xm.FORMATS)
def test_every_mutation_changes_the_coded_comparison(activations, n):
    """test_coded_rows_match_the_model: first batch, CODED_COUNTS, and the dense case on top of a count of 3."""
    a_codes, a_scales, _ = xm.exact_codes(activations, n)
    E, offsets = len(xm.CODED_COUNTS), xm.offsets_of(xm.CODED_COUNTS)
    true = xm.accumulate_codes_model(*xm.zero_state(E, n), a_codes, a_scales, offsets, activations, exact=True)[:3]
    mutations = FLOAT_MUTATIONS + ((dict(scale_from_neighbour=True),) if n > 32 else ())  # (one block a row has no neighbour)
    for mutation in mutations:
        if mutation == dict(factor_from="next"):
            continue  # (from zero counts f = 0 for every expert; the exact float comparison's second batch finds this one)
        assert differs(xm.accumulate_codes_model(*xm.zero_state(E, n), a_codes, a_scales, offsets, activations, **mutation)[:3], true), mutation
    M = a_scales.shape[0]
    dense = xm.accumulate_codes_model(*xm.zero_state(1, n)[:2], [3], a_codes, a_scales, [0, M], activations, exact=True)[:3]
    for mutation in (dict(factor_from="M"), dict(counts_not_advanced=True)) + ((dict(scale_from_neighbour=True),) if n > 32 else ()):
        got = xm.accumulate_codes_model(*xm.zero_state(1, n)[:2], [3], a_codes, a_scales, [0, M], activations, **mutation)[:3]
        if mutation == dict(factor_from="M"):
            assert xm.same_state(got, dense)  # (E = 1: M is the expert's own count -- not a mistake there)
        else:
            assert differs(got, dense), mutation


@pytest.mark.parametrize("activations", xm.FORMATS)
def test_mutations_break_the_random_coded_bound(activations):
    """test_random_codes_within_the_summation_bound: the model's own float32 product keeps the bound; a neighbour's scale byte,
    a token past the bound and a slice from the next expert do not."""
    a_codes, a_scales, X = xm.random_codes(activations)
    counts = xm.RANDOM_CODED_COUNTS
    E, n, offsets = len(counts), xm.RANDOM_CODED_N, xm.offsets_of(counts)

    def worst(**mutation):
        H = xm.accumulate_codes_model(*xm.zero_state(E, n), a_codes, a_scales, offsets, activations, **mutation)[0]
        return max(xm.coded_ratio(H[e], X[offsets[e]:offsets[e + 1]], T) for e, T in enumerate(counts) if T)

    assert worst() <= 2.0 ** -1 / 1.0  # (one rounding of the float64 product: half a unit of T 2^-23 |X|^T |X| at T >= 1)
    for mutation in (dict(scale_from_neighbour=True), dict(token_past_bound=True), dict(slice_from_next=True), dict(factor_from="M")):
        assert worst(**mutation) > 1.0, mutation


def test_broken_offsets_are_broken():
    for counts in (xm.EXACT_COUNTS[0], xm.CODED_COUNTS):
        o = xm.offsets_of(counts)
        assert xm.offsets_valid(o, sum(counts))
        for how, f in xm.BROKEN_OFFSETS.items():
            assert not xm.offsets_valid(f(np.array(o)), sum(counts)), how
            assert len(f(np.array(o))) == len(o)
