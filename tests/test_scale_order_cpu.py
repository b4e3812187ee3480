"""No GPU: the cases of tests/test_gpu_scale_order.py are worth running and its comparisons can fail.

The scale search's only output is the chosen grid point, so a case proves NumPy's summation order only if a sum taken in
another order picks another point somewhere.  Every dense-grid case is therefore run here through the oracle beside three
wrong models (tests/scale_order_model.py: search_choices) and must be changed by each of them; the counts are printed
(pytest -s) and recorded in DESIGN.md, "What the scale and order tests hold"."""

import numpy as np
import pytest

import scale_order_model as som
from groups_model import GroupGrid, group_scales_model
from groups_offsets_model import AsymGrid
from oracle import npsum, obq_ref, scaling_ref

BUDGET = 1.05e8  # rows x grid points x row length the oracle may be asked for in one case


# ------------------------------------------------------------------------------------------------ 1. the condition
@pytest.mark.parametrize("case", som.search_cases(), ids=som.case_id)
def test_dense_grid_case_tells_wrong_sums_apart(case):
    """From 64 elements on: float32 sums taken sequentially, the last element of every row left out, and (with a diagonal)
    the diagonal rotated by one column each change the chosen scale of at least one row.  Below 64 the two that leave the
    order of the sum alone must (a one-element row has no rotation); the order mutant is reported."""
    n = case["n"]
    assert case["rows"] * case["points"] * n <= BUDGET
    W, hd = som.search_inputs(case)
    chosen = som.search_choices(W, som.oracle_grid(case["cb"]), hd, **som.search_kwargs(case))
    counts = {k: som.rows_changed(chosen["oracle"], v) for k, v in chosen.items() if k != "oracle"}
    print(f"{som.case_id(case)}: {case['rows']} rows x {case['points']} points, rows changed: {counts}")
    required = set(counts)
    if n < 64:
        required.discard("sequential")
    if n == 1:
        required.discard("hd_shift")
    for k in required:
        assert counts[k] >= 1, (som.case_id(case), k, counts)


@pytest.mark.parametrize("n,cb,hd", [(129, "u4", True), (257, "asym16", False), (576, "nf4", True)])
def test_the_harness_oracle_is_best_grid_scale(n, cb, hd):
    """search_choices walks the grid through the oracle's own pieces: its "oracle" entry is best_grid_scale's result."""
    case = dict(n=n, cb=cb, hd=hd, rows=9, points=300, seed=7000 + n)
    W, h = som.search_inputs(case)
    kw = som.search_kwargs(case)
    chosen = som.search_choices(W, som.oracle_grid(cb), h, **kw)
    assert som.bits_fault(chosen["oracle"], scaling_ref.best_grid_scale(W, som.oracle_grid(cb), H=h, **kw)) is None


def test_a_sequential_oracle_would_fail_the_dense_grids(monkeypatch):
    """The oracle with its row sum replaced by a sequential one no longer gives the dense-grid expectation."""
    case = next(c for c in som.search_cases() if c["n"] == 257 and c["cb"] == "u4" and not c["hd"])
    W, _ = som.search_inputs(case)
    kw = som.search_kwargs(case)
    want = scaling_ref.best_grid_scale(W, som.oracle_grid("u4"), **kw)
    monkeypatch.setattr(scaling_ref, "grid_error", lambda H, D: som.sequential_sum(np.square(D)))
    assert som.rows_changed(scaling_ref.best_grid_scale(W, som.oracle_grid("u4"), **kw), want) >= 1


def test_every_search_kernel_form_is_reached():
    """By slk_scale_search's dispatch arithmetic: every chain length S of the regular kernel the suite did not reach, each
    leaf count, the table branch of both kernels, and the general kernel below, at and past one staged chunk."""
    forms = {(c["n"], c["cb"]): som.search_form(c["n"], c["cb"] == "nf4") for c in som.search_cases()}
    for n in som.GENERAL_LENGTHS:
        assert forms[(n, "u4")][0] == "general", n
    regular = {n: forms[(n, "u4")] for n in som.REGULAR_LENGTHS}
    assert all(f[0] == "regular" for f in regular.values())
    assert {(f[1], f[2]) for f in regular.values()} == {(9, 8), (10, 8), (11, 8), (13, 8), (14, 8), (15, 8), (9, 16), (13, 32)}
    assert forms[(512, "u4")] == ("general", 1, "uniform") and forms[(520, "u4")] == ("general", 1, "uniform")
    assert [forms[(n, "u4")][1] for n in (8191, 8192, 8193)] == [1, 1, 2]
    assert forms[(129, "nf4")] == ("general", 1, "table")
    assert forms[(576, "nf4")] == ("regular", 9, 8, "table") and forms[(1152, "nf4")] == ("regular", 9, 16, "table")
    assert {c["cb"] for c in som.search_cases() if c["n"] == 257} == {c["cb"] for c in som.search_cases() if c["n"] == 640} == {"u4", "u3", "asym16"}
    for n in som.REGULAR_LENGTHS:
        assert som.search_form(n, False, no_regular=True)[0] == "general"
    # the factor groups of the tie cases: 256 / (8 L) lists scanned side by side
    assert [256 // (8 * som.search_form(n, False)[2]) for n in som.TIE_LENGTHS[:2]] == [4, 2]
    assert som.search_form(som.TIE_LENGTHS[2], False)[0] == "general"
    assert som.search_form(som.extreme_rows()[0].shape[1], False)[0] == "general"
    assert {p for p, _, _ in som.TIE_GRIDS} >= {1, 2, 3, 5, 7} and any(lo == hi for _, lo, hi in som.TIE_GRIDS)


def test_other_search_cases_stay_inside_the_budget():
    W, _ = som.extreme_rows()
    assert W.shape == (24, 1000) and W.size * som.EXTREME_POINTS <= BUDGET
    for g, G in som.GROUPED_CASES:
        assert som.GROUPED_ROWS * g * G * som.GROUPED_POINTS <= BUDGET
    for n in som.TIE_LENGTHS:
        assert sum(6 * n * p for p, _, _ in som.TIE_GRIDS) <= BUDGET


@pytest.mark.parametrize("n", som.TIE_LENGTHS)
def test_tie_rows_tie(n):
    """A zero row under the 3-level codebook has error exactly 0 at every factor: the oracle keeps the first one."""
    W, hd = som.tie_rows(n)
    grd = som.oracle_grid("u3")
    base = scaling_ref.no_clip_scale(W, grd, 0)
    assert base[0] == np.float32(1.0e-16)
    for f in (np.float32(0.05), np.float32(0.5), np.float32(1.0)):
        D = scaling_ref.quantize_scaled(W, f * base, grd) - W
        assert scaling_ref.grid_error(hd, D)[0] == 0 and scaling_ref.grid_error(None, D)[0] == 0
    got = scaling_ref.best_grid_scale(W, grd, H=hd, grid_size=7)
    assert got[0] == np.float32(1.0e-16) * np.float32(0.05)


@pytest.mark.parametrize("g,G", som.GROUPED_CASES)
def test_grouped_case_tells_the_neighbours_diagonal_apart(g, G):
    W, H = som.grouped_inputs(g, G)
    kw = dict(min_factor=som.MIN_FACTOR, max_factor=som.MAX_FACTOR, grid_size=som.GROUPED_POINTS)
    for name in ("u4", "nf4"):
        grd = som.oracle_grid(name)
        want = group_scales_model(W, grd, H, g, "diag", **kw)
        wrong = group_scales_model(W, grd, som.neighbour_diagonal(H, g), g, "diag", **kw)
        changed = som.rows_changed(want, wrong)
        print(f"g = {g}, {G} groups, {name}: the neighbouring slice changes {changed} of {want.size} group scales")
        assert changed >= 1


@pytest.mark.parametrize("n", som.NAN_LENGTHS)
def test_the_reference_carries_a_nan(n):
    W, bad = som.nan_rows(n)
    grd = som.oracle_grid("u4")
    with np.errstate(invalid="ignore"):
        for got in (scaling_ref.no_clip_scale(W, grd, 0), scaling_ref.norm_scale(W, 0), scaling_ref.best_grid_scale(W, grd, grid_size=20)):
            assert np.isnan(got[bad]).all() and np.isfinite(np.delete(got, bad)).all()


def test_closed_form_rows_hold_their_edges():
    for n in (1, 9, 520, 8193):
        W = som.closed_form_rows(n)
        assert np.signbit(W[2]).all() and (W[2] == 0).all()
        assert np.square(W[3]).mean() < 1.0e-16
        if n > 1:
            assert W[0].argmax() == 0 and W[1].argmin() == n - 1 and W[4].argmin() == 0 and W[5].argmax() == n - 1


# ------------------------------------------------------------------------------------------------ 2. column statistics
def test_every_column_miss_path_is_reached():
    forms = [som.miss_form(R, n) for R in som.MISS_ROWS for n in som.MISS_COLS]
    assert {f["chunks"] for f in forms} == {1, 2, 3}
    assert {(f["prefetch"], f["ragged_chunk"]) for f in forms} == {(False, True), (False, False), (True, True), (True, False)}
    assert {(f["ragged_block"], f["vector_loads"], f["mixed_loads"]) for f in forms} == {
        (True, False, False),   # n = 1, 31, 33, 130: scalar loads
        (False, True, False),   # n = 32: 16-byte loads throughout
        (True, True, True),     # n = 100: 16-byte loads, the last block's tail by element
    }
    assert som.miss_form(257, 100, aligned=False)["vector_loads"] is False
    W = som.miss_weights(257, 33)
    assert (np.abs(W) > 1).mean() > 0.01 and (np.abs(W) < 1).mean() > 0.5  # some weights clip, most do not


def test_numpy_reduces_a_single_column_pairwise():
    """An (R, 1) array is a contiguous vector to NumPy's axis-0 reduction: its pairwise sum, not the row-after-row order of
    wider matrices (what k_column_miss_single follows at n == 1)."""
    W = som.miss_weights(600, 1)
    terms = np.square(som.oracle_grid("u8")(W) - W)
    assert terms.sum(axis=0)[0] == np.ascontiguousarray(terms[:, 0]).sum()
    assert terms.sum(axis=0)[0] != som.sequential_sum(terms.T)[0]
    wide = np.square(som.miss_weights(600, 2))
    assert np.array_equal(wide.sum(axis=0), som.sequential_sum(np.ascontiguousarray(wide.T)))


@pytest.mark.parametrize("R", som.MISS_LONG_ROWS)
def test_long_single_columns_tell_the_chunked_sum_apart(R):
    """Past 8192 rows NumPy adds the pairwise sums of pieces of 8192 terms (oracle/npsum.py's model with its default chunk);
    one pairwise tree over the whole column gives other bits in at least one of the sums the GPU test compares, for the
    plain, the grouped and the asymmetric quantizer each."""
    assert R > som.NP_CHUNK
    W = som.miss_weights(R, 1)
    S, O = som.single_column_scales(R)
    differ = {"plain": 0, "grouped": 0, "asymmetric": 0}
    for name in ("u8", "nf4"):
        grd = som.oracle_grid(name)
        forms = {"plain": grd, "grouped": GroupGrid(grd, S, 1, None), "asymmetric": AsymGrid(grd, S, O, 1, None)}
        for what, quantize in forms.items():
            for squared in (False, True):
                d = quantize(W) - W
                terms = np.ascontiguousarray((np.square(d) if squared else np.abs(d))[:, 0])
                want = som.miss_reference(W, quantize, squared)[0]
                assert want == npsum.pairwise_sum_f32(terms), (R, name, what, squared)
                differ[what] += int(want != npsum.pairwise_sum_f32(terms, chunk=None))
    print(f"R = {R}: sums of 4 that one unchunked tree changes: {differ}")
    assert all(differ.values()), differ


def test_single_column_groups_quantize_by_their_own_scales():
    """The one-column grouped cases are no multiple of the plain one: the grouped and asymmetric terms differ from the
    codebook's and from each other."""
    W = som.miss_weights(600, 1)
    S, O = som.single_column_scales(600)
    grd = som.oracle_grid("u8")
    sums = [som.miss_reference(W, q, True)[0] for q in (grd, GroupGrid(grd, S, 1, None), AsymGrid(grd, S, O, 1, None))]
    assert len(set(sums)) == 3


# ------------------------------------------------------------------------------------------------ 3. the sort
@pytest.mark.parametrize("kind", som.SORT_KINDS + ("nan",))
def test_sort_keys_tie(kind):
    for n in som.SORT_LENGTHS:
        keys = som.sort_keys(kind, n)
        assert keys.shape == (n,) and keys.dtype == np.float64
        if n >= 15:
            finite = keys[~np.isnan(keys)]
            assert len(np.unique(finite)) < len(finite), (kind, n)
    if kind == "zeros":
        k = som.sort_keys(kind, 257)
        assert (np.signbit(k) & (k == 0)).any() and (~np.signbit(k) & (k == 0)).any()
    if kind == "nan":
        k = som.sort_keys(kind, 257)
        assert (np.isnan(k) & np.signbit(k)).any() and (np.isnan(k) & ~np.signbit(k)).any()
    if kind == "run":
        k = som.sort_keys(kind, 4097)
        s = -(-4097 // som.SORT_SLICES)
        assert k[s - 1] == k[s] and k[255] == k[256] and k[1023] == k[1024]


def test_sort_lengths_reach_both_gathers_and_every_edge():
    assert {n for n in som.SORT_LENGTHS if som.gather_form(n) == "lds"} == {16, 256, 1024, 1100}
    assert {n for n in som.TIED_DIAGONALS + som.KEY_LENGTHS if som.gather_form(n) == "lds"} == {8, 32, 100}
    slices = [-(-n // som.SORT_SLICES) for n in som.SORT_LENGTHS]
    assert slices[:5] == [1, 1, 1, 1, 2] and max(slices) == 257  # n < 16: empty slices; one key a slice; the first two-key slice
    assert {-(-n // 256) for n in som.SORT_LENGTHS} >= {1, 2, 4, 5, 17}  # blocks of 256 threads


def test_sort_comparator_rejects_an_unstable_order():
    keys = som.sort_keys("ints", 257)
    order = np.argsort(keys, kind="stable")
    assert som.sort_fault(order, keys) is None
    i = int(np.flatnonzero(keys[order][:-1] == keys[order][1:])[0])
    wrong = order.copy()
    wrong[[i, i + 1]] = wrong[[i + 1, i]]  # two tied columns swapped: still sorted, no longer stable
    assert som.sort_fault(wrong, keys) is not None
    twice = order.copy()
    twice[0] = twice[1]
    assert som.sort_fault(twice, keys) == "not a permutation"
    zeros = som.sort_keys("zeros", 64)
    assert som.sort_fault(np.argsort(zeros, kind="stable"), zeros) is None
    assert som.sort_fault(np.lexsort((np.arange(64), np.signbit(zeros), zeros)), zeros) is not None  # -0.0 before +0.0: not a tie


def test_sort_comparator_accepts_any_place_for_the_nans():
    keys = som.sort_keys("nan", 257)
    nan = np.flatnonzero(np.isnan(keys))
    rest = np.flatnonzero(~np.isnan(keys))
    rest = rest[np.argsort(keys[rest], kind="stable")]
    assert som.sort_fault(np.concatenate([rest, nan]), keys) is None
    assert som.sort_fault(np.concatenate([nan[::-1], rest]), keys) is None
    mixed = np.insert(rest, np.linspace(0, rest.size, nan.size).astype(int), nan)
    assert som.sort_fault(mixed, keys) is None
    i = int(np.flatnonzero(keys[rest][:-1] == keys[rest][1:])[0])
    rest[[i, i + 1]] = rest[[i + 1, i]]
    assert som.sort_fault(np.concatenate([rest, nan]), keys) is not None


@pytest.mark.parametrize("n", som.TIED_DIAGONALS)
def test_tied_diagonals_are_valid(n):
    for H in som.tied_diagonal_hessians(n):
        assert H.dtype == np.float32 and len(np.unique(H.diagonal())) == 4
        for damp in (0.01, 0.0):
            Hd = som.damped(H, damp)
            np.linalg.cholesky(Hd)
            stable = obq_ref.column_order(None, Hd, None, "diag", ties="stable")
            assert not np.array_equal(stable, np.lexsort((-np.arange(n), -Hd.diagonal())))  # ties the other way: another order


# ------------------------------------------------------------------------------------------------ 4. keys made by kernels
def test_key_hessians_are_positive_definite_and_their_keys_apart():
    """The oracle's neighbouring keys lie further apart than the bound everywhere, so the order check is the whole order."""
    for n in sorted(set(som.KEY_LENGTHS + som.PIVOT_LENGTHS)):
        H = som.key_hessian(n)
        Hd = som.damped(H, som.DAMP)
        np.linalg.cholesky(Hd)
        if n in som.KEY_LENGTHS and n > 1:
            for combined in (0, 1):
                k = np.sort(som.oracle_inverse_keys(Hd, combined))
                gap = (np.diff(k) / np.maximum(np.abs(k[:-1]), np.abs(k[1:]))).min()
                assert gap > 1000 * som.key_bound(n), (n, combined, gap)


def test_inverse_key_comparator_rejects_a_moved_key():
    n = 257
    H = som.key_hessian(n)
    Hd = som.damped(H, som.DAMP)
    U0 = np.triu(obq_ref.inverse_factor_upper(Hd))
    for combined in (0, 1):
        want = som.inverse_key_reference(U0, H, som.DAMP, combined)
        assert som.key_excess(want, want, n) == 0
        assert np.allclose(want, som.oracle_inverse_keys(Hd, combined), rtol=1e-9)
        moved = want.copy()
        moved[100] *= 1 + 1e-12
        assert som.key_excess(moved, want, n) > 1
        order = np.argsort(want, kind="stable")
        assert som.order_fault(order, som.oracle_inverse_keys(Hd, combined), som.key_bound(n)) is None
        order[[3, 4]] = order[[4, 3]]
        assert som.order_fault(order, som.oracle_inverse_keys(Hd, combined), som.key_bound(n)) is not None


def test_pivot_ties_are_decided_by_position():
    H = som.tied_pivot_hessian()
    n = H.shape[0]
    assert np.array_equal(H, H.T) and (H.diagonal() == 4 * n).all() and (np.abs(H).sum(axis=1) < 2 * H.diagonal()).all()
    want = obq_ref.pivot_order(H)
    assert sorted(want.tolist()) == list(range(n))
    assert not np.array_equal(want, som.pivot_order_by_column(H))  # the smallest column index is another rule here
    assert not np.array_equal(want, np.arange(n))
    K = som.key_hessian(300)
    Kd = K + np.float64(som.damp_term(K, som.DAMP)) * np.eye(300)
    assert np.array_equal(obq_ref.pivot_order(Kd), som.pivot_order_by_column(Kd))  # (the restatement is the oracle without ties)


# ------------------------------------------------------------------------------------------------ 5. dead columns, mean removal
def test_dead_column_comparator_tells_negative_zero_from_a_small_diagonal():
    H, W = som.dead_case(3, 257, "negative_zero")
    assert np.signbit(H[128, 128]) and H[128, 128] == 0
    H2, W2 = H.copy(), W.copy()
    H2[128, 128] = np.float32(1e-30)  # alive
    a, b = (H.copy(), W.copy()), (H2, W2)
    obq_ref.patch_dead_columns(*a)
    obq_ref.patch_dead_columns(*b)
    assert a[0][128, 128] == H.diagonal().mean() and (a[1][:, 128] == 0).all()
    assert som.bits_fault(a[0], b[0]) is not None and som.bits_fault(a[1], b[1]) is not None
    assert som.bits_fault(np.float32([0.0]), np.float32([-0.0])) is not None
    assert som.bits_fault(np.float32([np.nan, 1.0]), np.float32([np.nan, 1.0])) is None


def test_dead_and_mean_cases_hold_their_edges():
    for n in som.DEAD_LENGTHS:
        for kind in som.DEAD_KINDS:
            H, W = som.dead_case(1, n, kind)
            dead = H.diagonal() == 0
            assert dead.sum() == {"none": 0, "all": n}.get(kind, dead.sum())
            if kind == "edges":
                assert dead[0] and dead[-1] and (n < 9 or (dead[3:6].all() and dead[n - 2]))
            if kind in ("edges", "negative_zero"):
                assert dead.any() and (n == 1 or not dead.all())
            if kind == "all":
                h = H.copy()
                obq_ref.patch_dead_columns(h, W.copy())
                assert (h.diagonal() == 0).all()
    for n in som.MEAN_LENGTHS:
        H, mean = som.mean_case(n)
        if n > 8:
            with np.errstate(over="ignore", invalid="ignore"):
                out = obq_ref.strip_input_mean(H, mean)
            assert np.isinf(out).any() and np.isfinite(out).any() and (mean == 0).sum() >= 3 and np.signbit(mean[mean == 0]).any()
