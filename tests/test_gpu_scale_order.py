"""The stage that makes every discrete decision ahead of the column loop, held to NumPy where its choices flip: per-row
scales on dense grids (scalesearch.hip), column statistics (k_column_miss), the counting sort and the keys made by kernels
(prepare.hip), dead columns and mean removal.  tests/scale_order_model.py builds the cases; tests/test_scale_order_cpu.py
proves, without a GPU, that each dense-grid case tells NumPy's sum from a sequential one and from a missed element
("What the scale and order tests hold")."""

import numpy as np
import pytest
import torch

import scale_order_model as som
from groups_model import GroupGrid, group_scales_model
from groups_offsets_model import AsymGrid
from oracle import obq_ref, scaling_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def amd():
    assert torch.cuda.is_available(), "these tests need the GPU"
    from sleekit_amd import _lib, codebook, engine, groups, obq, scaling

    class NS:
        pass

    ns = NS()
    ns.lib, ns.codebook, ns.engine, ns.groups, ns.obq, ns.scaling = _lib, codebook, engine, groups, obq, scaling
    return ns


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(got, want, what):
    fault = som.bits_fault(got, want)
    assert fault is None, (what, fault)


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------------ 1. scale search
@pytest.mark.parametrize("case", som.search_cases(), ids=som.case_id)
def test_dense_grid_search_is_numpy(amd, slkopt, case):
    """compute_min_mse_scaling on a grid of thousands of points over the upper part of the range, where a float32 sum taken in
    another order, or one element short, picks another point (counted per case on the CPU): the oracle's scales bit for bit;
    a regular length gives the same bits through the general kernel."""
    W, hd = som.search_inputs(case)
    cb, kw = som.device_codebook(amd.codebook, case["cb"]), som.search_kwargs(case)
    want = scaling_ref.best_grid_scale(W, som.oracle_grid(case["cb"]), H=hd, **kw)
    got = amd.scaling.compute_min_mse_scaling(W, cb, H=hd, **kw)
    print(som.case_id(case), "rows off the oracle:", som.rows_changed(got, want), "of", len(want))
    same_bits(got, want, som.case_id(case))
    if som.search_form(case["n"], case["cb"] == "nf4")[0] == "regular":
        slkopt.setenv("SLK_NO_REGULAR_SEARCH", "1")
        general = amd.scaling.compute_min_mse_scaling(W, cb, H=hd, **kw)
        slkopt.delenv("SLK_NO_REGULAR_SEARCH")
        same_bits(general, want, (som.case_id(case), "general kernel"))


@pytest.mark.parametrize("n", som.TIE_LENGTHS)
def test_search_ties_and_short_factor_lists(amd, n):
    """Errors that tie over the whole grid (a zero row, a row of one value), fewer grid points than factor groups, counts that
    are no multiple of them, min_factor == max_factor: the first smallest error wins, as in the oracle's scan."""
    W, hd = som.tie_rows(n)
    for name in ("u3", "u4"):
        cb, grd = som.device_codebook(amd.codebook, name), som.oracle_grid(name)
        for points, lo, hi in som.TIE_GRIDS:
            kw = dict(min_factor=lo, max_factor=hi, grid_size=points)
            for H in (None, hd):
                got = amd.scaling.compute_min_mse_scaling(W, cb, H=H, **kw)
                same_bits(got, scaling_ref.best_grid_scale(W, grd, H=H, **kw), (n, name, points, lo, hi, H is None))
                if name == "u3":  # 0 is a level: the zero row's error is exactly 0 at every factor
                    factors = np.linspace(lo, hi, points, dtype=np.float32)
                    assert got[0] == np.float32(1.0e-16) * factors[0], (n, points, got[0])


@pytest.mark.parametrize("name", ["u8", "asym16"])
def test_general_kernel_fast_division_on_extreme_rows(amd, slkopt, name):
    """The general kernel's fast division on rows with a wide dynamic range, zeros, denormals, 1e30 entries and divisors with
    an all-ones significand, on a dense grid: NumPy's scales, and those of the true divide."""
    W, hd = som.extreme_rows()
    assert som.search_form(W.shape[1], False)[0] == "general"
    cb, grd = som.device_codebook(amd.codebook, name), som.oracle_grid(name)
    kw = dict(min_factor=som.MIN_FACTOR, max_factor=som.MAX_FACTOR, grid_size=som.EXTREME_POINTS)
    for H in (None, hd):
        got = amd.scaling.compute_min_mse_scaling(W, cb, H=H, **kw)
        slkopt.setenv("SLK_NO_FAST_SEARCH_DIV", "1")
        slow = amd.scaling.compute_min_mse_scaling(W, cb, H=H, **kw)
        slkopt.delenv("SLK_NO_FAST_SEARCH_DIV")
        same_bits(got, slow, (name, H is None, "true divide"))
        with np.errstate(over="ignore", invalid="ignore"):  # the 1e30 entries square to inf, in NumPy as on the GPU
            want = scaling_ref.best_grid_scale(W, grd, H=H, **kw)
        same_bits(got, want, (name, H is None))


@pytest.mark.parametrize("g,G", som.GROUPED_CASES)
def test_grouped_search_on_dense_grids(amd, g, G):
    """slk_scale_search_grouped through groups.compute_group_scaling: every group of every row against the oracle's search
    of that group with its own slice of the diagonal (on the CPU the neighbour's slice changes a scale)."""
    W, H = som.grouped_inputs(g, G)
    kw = dict(min_factor=som.MIN_FACTOR, max_factor=som.MAX_FACTOR, grid_size=som.GROUPED_POINTS)
    for name in ("u4", "nf4"):
        cb, grd = som.device_codebook(amd.codebook, name), som.oracle_grid(name)
        for mode in ("mse", "diag"):
            got = amd.groups.compute_group_scaling(W, cb, g, H, mode, **kw)
            same_bits(got, group_scales_model(W, grd, H, g, mode, **kw), (g, G, name, mode))


@pytest.mark.parametrize("n", som.GENERAL_LENGTHS + som.REGULAR_LENGTHS)
def test_closed_form_scales(amd, n):
    """compute_non_saturating_scaling and compute_norm_scaling at every row length of the search: extremes in the first and
    in the last column, a row of -0.0, a row under the 1e-16 floor."""
    W = som.closed_form_rows(n)
    for name in ("u4", "asym16", "nf4"):
        got = amd.scaling.compute_non_saturating_scaling(W, som.device_codebook(amd.codebook, name), 0)
        same_bits(got, scaling_ref.no_clip_scale(W, som.oracle_grid(name), 0), (n, name))
    same_bits(amd.scaling.compute_norm_scaling(W, 0), scaling_ref.norm_scale(W, 0), (n, "norm"))


@pytest.mark.parametrize("n", som.NAN_LENGTHS)
def test_nan_in_a_row_gives_a_nan_scale(amd, n):
    """NumPy's min, max and maximum carry a NaN, so the reference's three scale functions return NaN for a row that holds
    one (at column 0, in the middle, at the end); the other rows keep the bits they have without those rows."""
    W, bad = som.nan_rows(n)
    good = np.setdiff1d(np.arange(W.shape[0]), bad)
    cb, grd = som.device_codebook(amd.codebook, "u4"), som.oracle_grid("u4")
    hd = (np.abs(W[0]) * 10 + 0.1).astype(np.float32)
    calls = {
        "max": lambda X: amd.scaling.compute_non_saturating_scaling(X, cb, 0),
        "norm": lambda X: amd.scaling.compute_norm_scaling(X, 0),
        "mse": lambda X: amd.scaling.compute_min_mse_scaling(X, cb, grid_size=50),
        "diag": lambda X: amd.scaling.compute_min_mse_scaling(X, cb, H=hd, grid_size=50),
    }
    with np.errstate(invalid="ignore"):
        refs = {"max": scaling_ref.no_clip_scale(W, grd, 0), "norm": scaling_ref.norm_scale(W, 0),
                "mse": scaling_ref.best_grid_scale(W, grd, grid_size=50), "diag": scaling_ref.best_grid_scale(W, grd, H=hd, grid_size=50)}
    for what, call in calls.items():
        got, alone = call(W), call(np.ascontiguousarray(W[good]))
        print(n, what, "scales of the NaN rows:", got[bad])
        assert np.isnan(refs[what][bad]).all(), what  # the reference's rule
        same_bits(got[good], alone, (n, what, "finite rows"))
        same_bits(got[good], refs[what][good], (n, what, "finite rows against the oracle"))
        assert np.isnan(got[bad]).all(), (n, what, got[bad])


# ------------------------------------------------------------------------------------------------ 2. column statistics
@pytest.mark.parametrize("R", som.MISS_ROWS)
def test_column_miss_shapes(amd, R):
    """engine.column_miss against NumPy's float32 axis-0 sums, bit for bit: one row to three 256-row chunks (the prefetch of
    a next chunk, ragged last chunks), one column to five 32-column blocks (ragged blocks, 16-byte loads on, off and mixed)."""
    for n in som.MISS_COLS:
        W = som.miss_weights(R, n)
        Wd = cuda(W)
        for name in ("u8", "nf4"):
            abi, grd = som.device_codebook(amd.codebook, name)._abi(), som.oracle_grid(name)
            for squared in (False, True):
                got = amd.engine.column_miss(Wd, abi, squared).cpu().numpy()
                same_bits(got, som.miss_reference(W, grd, squared), (R, n, name, squared))


def test_column_miss_off_16_byte_alignment(amd):
    """n % 4 == 0 on a contiguous view that starts 4 bytes into a buffer: the 16-byte loads must be off."""
    R, n = 257, 100
    W = som.miss_weights(R, n)
    buf = torch.zeros(R * n + 1, dtype=torch.float32, device="cuda")
    Wd = buf[1:].view(R, n)
    Wd.copy_(torch.from_numpy(W))
    assert Wd.is_contiguous() and Wd.data_ptr() % 16 != 0 and Wd.data_ptr() % 4 == 0
    for name in ("u8", "nf4"):
        abi, grd = som.device_codebook(amd.codebook, name)._abi(), som.oracle_grid(name)
        for squared in (False, True):
            same_bits(amd.engine.column_miss(Wd, abi, squared).cpu().numpy(), som.miss_reference(W, grd, squared), (name, squared))


@pytest.mark.parametrize("R", [257, 600])
@pytest.mark.parametrize("g,n", [(32, 96), (50, 150)])
def test_column_miss_grouped_and_asymmetric(amd, R, g, n):
    """The grouped and the asymmetric forms of the column statistics against the group quantizers of tests/groups_model.py and
    tests/groups_offsets_model.py."""
    W = som.miss_weights(R, n)
    S, O = som.group_scales(W, g)
    Wd, Sd, Od = cuda(W), cuda(S), cuda(O)
    for name in ("u8", "nf4"):
        abi, grd = som.device_codebook(amd.codebook, name)._abi(), som.oracle_grid(name)
        for squared in (False, True):
            got = amd.engine.column_miss(Wd, abi, squared, Sd, g).cpu().numpy()
            same_bits(got, som.miss_reference(W, GroupGrid(grd, S, g, None), squared), (R, g, name, squared, "grouped"))
            got = amd.engine.column_miss(Wd, abi, squared, Sd, g, Od).cpu().numpy()
            same_bits(got, som.miss_reference(W, AsymGrid(grd, S, O, g, None), squared), (R, g, name, squared, "asymmetric"))


@pytest.mark.parametrize("R", som.MISS_ROWS + som.MISS_LONG_ROWS)
def test_column_miss_of_one_column(amd, R):
    """n = 1 (one group of one column): NumPy reduces an (R, 1) array along axis 0 as a contiguous vector, pairwise and in
    pieces of 8192 terms, and so does k_column_miss_single in its plain, grouped and asymmetric forms -- below one chunk of
    the staged column, one term past it, and over three chunks with a ragged last one."""
    W = som.miss_weights(R, 1)
    S, O = som.single_column_scales(R)
    Wd, Sd, Od = cuda(W), cuda(S), cuda(O)
    for name in ("u8", "nf4"):
        abi, grd = som.device_codebook(amd.codebook, name)._abi(), som.oracle_grid(name)
        for squared in (False, True):
            got = amd.engine.column_miss(Wd, abi, squared).cpu().numpy()
            same_bits(got, som.miss_reference(W, grd, squared), (R, name, squared, "plain"))
            got = amd.engine.column_miss(Wd, abi, squared, Sd, 1).cpu().numpy()
            same_bits(got, som.miss_reference(W, GroupGrid(grd, S, 1, None), squared), (R, name, squared, "grouped"))
            got = amd.engine.column_miss(Wd, abi, squared, Sd, 1, Od).cpu().numpy()
            same_bits(got, som.miss_reference(W, AsymGrid(grd, S, O, 1, None), squared), (R, name, squared, "asymmetric"))


# ------------------------------------------------------------------------------------------------ 3. the sort
def device_sort(amd, keys):
    n = keys.size
    H = torch.eye(n, dtype=torch.float32, device="cuda")
    order, _, _ = amd.engine.factorize_order_only(H, n, amd.lib.ORDER_KEYS, cuda(keys))
    return order.cpu().numpy()


@pytest.mark.parametrize("n", som.SORT_LENGTHS)
def test_counting_sort_is_a_stable_argsort(amd, n):
    """Caller-supplied float64 keys through slk_hessian_prepare: repeated small integers, +0.0 against -0.0 (a tie, as in
    NumPy), infinities, denormals and +-1e308, runs of equal keys over a slice boundary, a 256-thread block and index 1024."""
    for kind in som.SORT_KINDS:
        keys = som.sort_keys(kind, n)
        fault = som.sort_fault(device_sort(amd, keys), keys)
        assert fault is None, (n, kind, fault)


@pytest.mark.parametrize("n", som.SORT_LENGTHS)
def test_counting_sort_with_nan_keys(amd, n):
    """NaN keys of both signs among finite ones: the order is a permutation, and the columns without a NaN come in their
    stable sorted order among themselves; where the NaNs land is not prescribed."""
    keys = som.sort_keys("nan", n)
    assert np.isnan(keys).any()
    fault = som.sort_fault(device_sort(amd, keys), keys)
    assert fault is None, (n, fault)


@pytest.mark.parametrize("damp", [0.01, 0.0])
@pytest.mark.parametrize("n", som.TIED_DIAGONALS)
def test_diagonal_order_with_ties(amd, n, damp):
    """Diagonals of four distinct values: the diag order is the stable one, from engine.factorize and, for three different
    matrices at once, from engine.factorize_batch; each matrix of the batch is its single call."""
    Hs = som.tied_diagonal_hessians(n)
    Hd = [cuda(H) for H in Hs]
    border, bU, binfo = amd.engine.factorize_batch(Hd, n, damp, amd.lib.ORDER_DIAG)
    assert binfo.cpu().tolist() == [0, 0, 0]
    for b, H in enumerate(Hs):
        want = obq_ref.column_order(None, som.damped(H, damp), None, "diag", ties="stable")
        order, U, info = amd.engine.factorize(Hd[b], n, damp, amd.lib.ORDER_DIAG)
        assert int(info.item()) == 0
        assert np.array_equal(order.cpu().numpy(), want), (n, damp, b, "single")
        assert np.array_equal(border[b].cpu().numpy(), want), (n, damp, b, "batch")
        assert torch.equal(bU[b], U), (n, damp, b, "factor of the batch")


# ------------------------------------------------------------------------------------------------ 4. keys made by kernels
@pytest.mark.parametrize("n", som.KEY_LENGTHS)
def test_inverse_diagonal_keys(amd, n):
    """engine.inverse_diag_keys against float64 NumPy sums over the device's own first factor, within 2 (n + 2) 2^-53; the
    keys' order is the oracle's inv_diag / combined_diag order wherever the oracle's neighbours are further apart."""
    H = som.key_hessian(n)
    Hd = cuda(H)
    _, U0, info = amd.engine.factorize(Hd, n, som.DAMP, amd.lib.ORDER_NONE)
    assert int(info.item()) == 0
    U0 = U0.cpu().numpy()
    for combined in (0, 1):
        got = amd.engine.inverse_diag_keys(Hd, n, som.DAMP, combined).cpu().numpy()
        want = som.inverse_key_reference(U0, H, som.DAMP, combined)
        excess = som.key_excess(got, want, n)
        print(f"n = {n} combined = {combined}: largest difference is {excess:.3f} of the bound")
        assert excess <= 1.0, (n, combined, excess)
        oracle_keys = som.oracle_inverse_keys(som.damped(H, som.DAMP), combined)
        fault = som.order_fault(np.argsort(got, kind="stable"), oracle_keys, som.key_bound(n))
        assert fault is None, (n, combined, fault)


@pytest.mark.parametrize("n", som.PIVOT_LENGTHS)
def test_pivot_keys_are_the_reference_order(amd, n):
    H = som.key_hessian(n)
    keys = amd.engine.pivot_keys(cuda(H), n, som.DAMP).cpu().numpy()
    Hd = H + np.float64(som.damp_term(H, som.DAMP)) * np.eye(n)
    assert np.array_equal(np.argsort(keys, kind="stable"), obq_ref.pivot_order(Hd)), n
    assert np.array_equal(np.sort(keys), np.arange(n))


def test_pivot_ties_go_to_the_first_position(amd):
    """Small integers, equal diagonal entries: conditional variances tie exactly, and the first POSITION of the reference's
    swapped order wins (the smallest column index gives another order: checked on the CPU)."""
    H = som.tied_pivot_hessian()
    n = H.shape[0]
    keys = amd.engine.pivot_keys(cuda(H), n, 0.0).cpu().numpy()
    assert np.array_equal(np.argsort(keys, kind="stable"), obq_ref.pivot_order(H))


# ------------------------------------------------------------------------------------------------ 5. dead columns, mean removal
@pytest.mark.parametrize("R", som.DEAD_ROWS)
@pytest.mark.parametrize("n", som.DEAD_LENGTHS)
def test_dead_columns(amd, R, n):
    """obq.remove_dead_values against the oracle, H and W bit for bit: dead columns first, last and side by side, a -0.0 on
    the diagonal (dead in NumPy), none dead, all dead (the fill is 0)."""
    for kind in som.DEAD_KINDS:
        H, W = som.dead_case(R, n, kind)
        wantH, wantW = H.copy(), W.copy()
        obq_ref.patch_dead_columns(wantH, wantW)
        amd.obq.remove_dead_values(H, W)
        same_bits(H, wantH, (R, n, kind, "H"))
        same_bits(W, wantW, (R, n, kind, "W"))


@pytest.mark.parametrize("n", som.MEAN_LENGTHS)
def test_mean_removal(amd, n):
    H, mean = som.mean_case(n)
    with np.errstate(over="ignore", invalid="ignore"):
        want = obq_ref.strip_input_mean(H, mean)
    same_bits(amd.obq.remove_input_bias(H, mean), want, n)
