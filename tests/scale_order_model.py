"""Inputs, wrong-on-purpose models and comparators for the stage that makes every discrete decision ahead of the column loop:
the per-row scales (scalesearch.hip), the column statistics (k_column_miss), the sort and its keys (prepare.hip), dead columns
and mean removal.  NumPy only.  tests/test_gpu_scale_order.py runs the cases on the device, tests/test_scale_order_cpu.py
checks without a GPU that every case can tell a right kernel from a subtly wrong one ("What the scale and order
tests hold")."""

import numpy as np

from oracle import grid, scaling_ref
from sleekit_amd import synth

# ------------------------------------------------------------------------------------------------ codebooks
CODEBOOKS = {  # name -> (levels, lo, hi) of a uniform codebook; "nf4" is the NormalFloat4 table
    "u4": (4, -1.0, 1.0),
    "u3": (3, -1.0, 1.0),
    "u8": (8, -1.0, 1.0),
    "asym16": (16, -0.75, 1.25),
}


def oracle_grid(name):
    return grid.TableGrid.nf4() if name == "nf4" else grid.UniformGrid(*CODEBOOKS[name])


def device_codebook(codebook, name):
    """The sleekit_amd.codebook object of a codebook name (`codebook`: that module)."""
    return codebook.Codebook.nf4() if name == "nf4" else codebook.UniformCodebook(*CODEBOOKS[name])


# ------------------------------------------------------------------------------------------------ scale search: dense grids
GENERAL_LENGTHS = (1, 2, 7, 8, 9, 64, 127, 128, 129, 257, 512, 520, 1000, 8191, 8192, 8193)
REGULAR_LENGTHS = (576, 640, 704, 832, 896, 960, 1152, 3328)
NP_CHUNK = 8192  # npsum.h: the general kernel stages a row through LDS in chunks of this many terms


def search_form(n, table, no_regular=False):
    """The kernel slk_scale_search launches for rows of n elements, by its own dispatch arithmetic: ("regular", S, L) for
    k_scale_search_regular<S> over L leaves of 8 S elements, ("general", chunks) for k_scale_search with its row staged in
    `chunks` pieces; then "table" or "uniform" (cb_value's branch; the fast division serves the uniform one only)."""
    m, L, regular = n, 1, True
    while m > 128 and regular:
        regular = m % 2 == 0 and (m // 2) % 8 == 0
        m //= 2
        L *= 2
    regular = regular and m % 8 == 0 and m >= 8 and L in (8, 16, 32) and 9 <= m // 8 <= 16 and not no_regular
    form = ("regular", m // 8, L) if regular else ("general", -(-n // NP_CHUNK))
    return form + ("table" if table else "uniform",)


def search_size(n):
    """(rows, grid points) of the dense-grid case at row length n: rows * points * n stays at or below 1e8, the oracle's budget
    of a few seconds (it needs about 2.6e-8 s per element), and well below it where fewer already discriminate."""
    if n <= 257:
        return 48, 4000
    if n <= 1152:
        return 24, 3000
    if n <= 3328:
        return 12, 2500
    return 6, 2000


MIN_FACTOR, MAX_FACTOR = 0.3, 1.0


def search_cases():
    """Every dense-grid case of the GPU test: dicts n, cb, hd (bool), rows, points, seed."""
    cases = []
    for n in GENERAL_LENGTHS + REGULAR_LENGTHS:
        books = ["u4"]
        if n in (129, 576, 1152):
            books.append("nf4")
        if n in (257, 640):
            books += ["u3", "asym16"]
        for cb in books:
            for hd in (False, True):
                rows, points = search_size(n)
                cases.append(dict(n=n, cb=cb, hd=hd, rows=rows, points=points, seed=SEARCH_SEEDS.get((n, cb, hd), 7000 + n)))
    return cases


# (n, cb, hd) -> seed where 7000 + n does not meet the condition of test_scale_order_cpu.py (one of the wrong models changed no
# row): the next of 8000 + n, 9000 + n, ... that does
SEARCH_SEEDS = {
    (520, "u4", True): 8520, (576, "nf4", False): 8576, (576, "nf4", True): 8576, (640, "asym16", False): 8640,
    (960, "u4", True): 8960, (8191, "u4", False): 17191, (8191, "u4", True): 16191, (8192, "u4", True): 17192,
    (8193, "u4", True): 18193,
}


def case_id(c):
    return f"n{c['n']}-{c['cb']}-{'hd' if c['hd'] else 'plain'}"


def search_inputs(c):
    """(W, hd or None) of a dense-grid case: the weights and the diagonal of test_scale_search_regular_tree."""
    W = synth.make_weights(c["rows"], c["n"], c["seed"])
    hd = (np.abs(synth.normal_grid(c["seed"], 8, 1, c["n"])[0]) * 3 + 0.1).astype(np.float32) if c["hd"] else None
    return W, hd


def search_kwargs(c):
    return dict(min_factor=MIN_FACTOR, max_factor=MAX_FACTOR, grid_size=c["points"])


def sequential_sum(terms):
    """Row sums in float32, one element after the other: what a kernel that ignores NumPy's pairwise tree computes."""
    return np.cumsum(terms, axis=1, dtype=np.float32)[:, -1]


def search_choices(W, grd, hd, min_factor, max_factor, grid_size):
    """The oracle's grid search beside three wrong models, in one pass over the grid.  The oracle's side is the oracle's own
    code (no_clip_scale, quantize_scaled, grid_error, _first_best: what best_grid_scale is made of); the wrong models replace
    its row sum -- "sequential": float32 sums taken in order; "drop_last": the last element of every row left out;
    "hd_shift" (with hd): the diagonal rotated by one column -- and keep the first strict minimum the same way.
    Returns {name: chosen scales}."""
    base = scaling_ref.no_clip_scale(W, grd, 0)
    factors = np.linspace(min_factor, max_factor, grid_size, dtype=np.float32)
    names = ["sequential", "drop_last"] + (["hd_shift"] if hd is not None else [])
    lowest = {k: np.full(base.size, np.inf, dtype=np.float32) for k in names}
    chosen = {k: np.full(base.size, np.inf, dtype=np.float32) for k in names}
    shifted = None if hd is None else np.roll(hd, 1)
    at = [0]

    def row_errors(sc):
        D = scaling_ref.quantize_scaled(W, sc, grd) - W
        sq = np.square(D)
        terms = sq if hd is None else np.expand_dims(hd, 0) * sq
        wrong = {"sequential": sequential_sum(terms), "drop_last": terms[:, :-1].sum(axis=1)}
        if hd is not None:
            wrong["hd_shift"] = (np.expand_dims(shifted, 0) * sq).sum(axis=1)
        f = factors[at[0]]
        at[0] += 1
        for k in names:
            better = wrong[k] < lowest[k]
            lowest[k][better] = wrong[k][better]
            chosen[k][better] = f
        return scaling_ref.grid_error(hd, D)

    with np.errstate(over="ignore", invalid="ignore"):
        out = {"oracle": scaling_ref._first_best(base, factors, row_errors)}
        for k in names:
            out[k] = base * chosen[k]
    return out


def rows_changed(a, b):
    return int((a.view(np.uint32) != b.view(np.uint32)).sum())


# ------------------------------------------------------------------------------------------------ scale search: ties, short lists
TIE_LENGTHS = (576, 1152, 1000)  # four factor groups, two groups, the general kernel
TIE_GRIDS = ((1, 0.05, 1.0), (2, 0.05, 1.0), (3, 0.05, 1.0), (5, 0.05, 1.0), (7, 0.05, 1.0), (6, 0.7, 0.7), (101, 0.05, 1.0))


def tie_rows(n):
    """Rows whose errors tie over the grid: all zero, one repeated value of either sign, beside random rows."""
    W = synth.make_weights(6, n, 7300 + n)
    W[0] = 0.0
    W[1] = np.float32(0.37)
    W[2] = np.float32(-0.011)
    hd = (np.abs(synth.normal_grid(7300 + n, 8, 1, n)[0]) * 3 + 0.1).astype(np.float32)
    return W, hd


def extreme_rows():
    """The rows of test_scale_search_fast_division (wide dynamic range, zeros, denormals, 1e30 entries), cut to 1000 columns:
    the general kernel.  Returns (W, hd)."""
    rng = np.random.default_rng(5)
    R, n = 64, 1024
    W = (rng.standard_normal((R, n)) * np.exp(rng.uniform(-12, 6, (R, 1)))).astype(np.float32)
    W[0, :16] = [0.0, -0.0, 1e-45, -1e-45, 1e-39, 3e-38, 1e-30, -1e-31, 1e30, -3e37, 1.0, -1.0, 0.5, 2.0, 1e-20, 1e20]
    W[1] *= np.float32(1e-25)
    W[2] *= np.float32(1e18)
    hd = (np.abs(rng.standard_normal(n)) + 0.01).astype(np.float32)
    return np.ascontiguousarray(W[:24, :1000]), np.ascontiguousarray(hd[:1000])


EXTREME_POINTS = 1500

# ------------------------------------------------------------------------------------------------ grouped search
GROUPED_CASES = tuple((g, G) for g in (64, 100) for G in (3, 5))
GROUPED_ROWS, GROUPED_POINTS = 8, 3000


def grouped_inputs(g, G):
    """(W, H) of a grouped-search case: H is diagonal (the search reads nothing else of it)."""
    n = g * G
    W = synth.make_weights(GROUPED_ROWS, n, 7600 + n)
    hd = (np.abs(synth.normal_grid(7600 + n, 8, 1, n)[0]) * 3 + 0.1).astype(np.float32)
    return W, np.diag(hd).astype(np.float32)


def neighbour_diagonal(H, g):
    """H with every group's slice of the diagonal replaced by the next group's: the wrong model of the grouped search."""
    return np.diag(np.roll(H.diagonal(), -g)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ closed forms, NaN
def closed_form_rows(n):
    """Rows for the closed-form scales: the extreme in the first column, in the last, a row of -0.0, a row whose mean square
    is below 1e-16, then random rows."""
    W = synth.make_weights(8, n, 7800 + n)
    W[0, 0] = np.float32(1.0)
    W[1, -1] = np.float32(-1.0)
    W[2] = np.float32(-0.0)
    W[3] *= np.float32(1.0e-8)
    W[4, 0] = np.float32(-2.0)
    W[5, -1] = np.float32(3.0)
    return W


NAN_LENGTHS = (129, 576, 1000)


def nan_rows(n):
    """(W, nan_rows): finite rows with three rows that hold one NaN each, at column 0, at the middle and at the last."""
    W = synth.make_weights(7, n, 7900 + n)
    W[1, 0] = np.nan
    W[3, n // 2] = np.nan
    W[5, n - 1] = np.nan
    return W, np.array([1, 3, 5])


# ------------------------------------------------------------------------------------------------ column statistics
MISS_ROWS = (1, 31, 255, 256, 257, 512, 513, 600)
MISS_COLS = (1, 31, 32, 33, 100, 130)
# one column, more rows than NumPy's inner loop takes at once (8192): two chunks, the second of one term, and three with a
# ragged last one -- k_column_miss_single stages the column through row_sum_numpy chunk by chunk
MISS_LONG_ROWS = (8193, 20000)
CM_ROWS, CM_COLS = 256, 32  # elementwise.hip: rows per chunk, columns per workgroup


def miss_form(R, n, aligned=True):
    """The paths k_column_miss takes for an (R, n) matrix, from slk_column_miss's arithmetic."""
    return dict(chunks=-(-R // CM_ROWS), prefetch=R > CM_ROWS, ragged_chunk=R % CM_ROWS != 0, blocks=-(-n // CM_COLS),
                ragged_block=n % CM_COLS != 0, vector_loads=n % 4 == 0 and aligned,
                mixed_loads=n % 4 == 0 and aligned and n % CM_COLS != 0)


def miss_weights(R, n):
    """Scaled weights for the column statistics: most inside the codebook's range, some beyond it."""
    return (synth.make_weights(R, n, 8100 + 7 * R + n) * np.float32(25)).astype(np.float32)


def miss_reference(W, quantize, squared):
    d = quantize(W) - W
    return (np.square(d) if squared else np.abs(d)).sum(axis=0)


def group_scales(W, g):
    """Positive group scales and midpoint offsets (R, n / g) for the grouped statistics."""
    R, n = W.shape
    V = W.reshape(R, n // g, g)
    S = np.maximum(np.abs(V).max(axis=2) * np.float32(0.8), np.float32(1e-6)).astype(np.float32)
    O = (np.float32(0.5) * (V.min(axis=2) + V.max(axis=2))).astype(np.float32)
    return S, O


def single_column_scales(R):
    """(S, O) of shape (R, 1) for a one-column matrix in groups of one column: scales and offsets of their own (a group's
    extremes are the element itself and would leave every term the same multiple of it)."""
    rng = np.random.default_rng(8150 + R)
    return rng.uniform(0.4, 1.6, (R, 1)).astype(np.float32), (rng.standard_normal((R, 1)) * 0.2).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the sort
SORT_LENGTHS = (1, 2, 15, 16, 17, 255, 256, 257, 1023, 1024, 1025, 1100, 4097)
SORT_KINDS = ("ints", "zeros", "extremes", "run")
SORT_SLICES = 16  # prepare.hip: slices of the j range, slice = ceil(n / 16)


def gather_form(n, aligned=True):
    """The gather slk_hessian_prepare runs after the sort, by its own arithmetic: rows staged through LDS with 16-byte loads
    ("lds": n % 4 == 0, n <= 16384, an aligned H), or element by element ("plain")."""
    return "lds" if n % 4 == 0 and n <= 16384 and aligned else "plain"


_NEG_NAN = np.array([0xFFF8000000000001], dtype=np.uint64).view(np.float64)[0]
_POS_NAN = np.array([0x7FF8000000000000], dtype=np.uint64).view(np.float64)[0]


def sort_keys(kind, n):
    """float64 keys for the counting sort."""
    rng = np.random.default_rng(8200 + n)
    if kind == "ints":  # small integers with many repeats
        return rng.integers(-2, 3, n).astype(np.float64)
    if kind == "zeros":  # +0.0 and -0.0 tie
        return rng.choice(np.array([0.0, -0.0, 0.0, -0.0, 1.0, -1.0]), n)
    if kind == "extremes":
        pool = np.array([np.inf, -np.inf, 5e-324, -5e-324, 1e-310, -1e-310, 2.2250738585072014e-308, 1e308, -1e308, 0.0, -0.0, 1.0])
        return rng.choice(pool, n)
    if kind == "run":  # descending keys with runs of equal keys over a slice boundary, a 256-thread block and index 1024
        keys = np.arange(n, 0, -1).astype(np.float64)
        slice_ = -(-n // SORT_SLICES)
        for centre in (slice_, 256, 1024, 5 * slice_):
            lo, hi = max(centre - 3, 0), min(centre + 4, n)
            if lo < hi:
                keys[lo:hi] = keys[lo]
        return keys
    if kind == "nan":  # both signs of the NaN pattern among repeated finite keys
        keys = rng.integers(-2, 3, n).astype(np.float64)
        where = rng.random(n) < 0.2
        where[:: max(n // 3, 1)] = True
        keys[where] = np.where(rng.random(int(where.sum())) < 0.5, _POS_NAN, _NEG_NAN)
        return keys
    raise ValueError(kind)


def sort_fault(order, keys):
    """None when `order` is the stable argsort of `keys`, else what is wrong.  With NaN keys: `order` must be a permutation
    and the other columns must come in their stable sorted order among themselves; where the NaNs land is free."""
    order, n = np.asarray(order), keys.size
    if order.shape != (n,) or not np.array_equal(np.sort(order), np.arange(n)):
        return "not a permutation"
    finite = ~np.isnan(keys)
    if finite.all():
        want = np.argsort(keys, kind="stable")
        return None if np.array_equal(order, want) else f"first difference at position {int(np.flatnonzero(order != want)[0])}"
    got = order[finite[order]]
    want = np.flatnonzero(finite)[np.argsort(keys[finite], kind="stable")]
    return None if np.array_equal(got, want) else "the columns without a NaN key are out of their stable order"


TIED_DIAGONALS = (100, 257)


def tied_diagonal_hessians(n):
    """Three positive definite float32 Hessians whose diagonals take four distinct values: diagonally dominant."""
    out = []
    for b in range(3):
        rng = np.random.default_rng(8300 + 10 * n + b)
        A = rng.uniform(-1, 1, (n, n)) * (0.4 / n)
        H = (A + A.T).astype(np.float32)
        levels = np.array([1.0, 1.5, 2.25, 3.0], dtype=np.float32) * np.float32(1 + b)
        H[np.arange(n), np.arange(n)] = levels[rng.integers(0, 4, n)]
        out.append(H)
    return out


def damped(H, damp):
    """The float64 damped matrix as test_order_and_factor builds it (float32 damping term, NEP 50)."""
    return H + damp * H.diagonal().mean() * np.eye(H.shape[0])


# ------------------------------------------------------------------------------------------------ keys made by kernels
KEY_LENGTHS = (1, 7, 8, 9, 31, 32, 33, 63, 65, 100, 257)
PIVOT_LENGTHS = (1, 2, 255, 256, 257, 300)
DAMP = 0.01


def key_hessian(n):
    return synth.make_hessian(n, 8400 + n)[0]


def damp_term(H, damp):
    """float32(damp) * mean(diag H) in float32: the device's damping term."""
    return np.float32(damp) * H.diagonal().mean()


def inverse_key_reference(U0, H, damp, combined):
    """Float64 sums over a factor U0 (U0^T U0 = Hd^-1): diag(Hd^-1), or -diag(Hd) / diag(Hd^-1)."""
    dinv = np.square(U0.astype(np.float64)).sum(axis=0)
    if not combined:
        return dinv
    return -(H.diagonal().astype(np.float64) + np.float64(damp_term(H, damp))) / dinv


def key_bound(n):
    """2 (n + 2) 2^-53, relative: both sides sum at most n non-negative terms in some order, each within n 2^-53 of the exact
    sum, plus one rounding for the quotient."""
    return 2.0 * (n + 2) * 2.0 ** -53


def key_excess(got, want, n):
    """Largest relative difference of the keys over the bound (<= 1 passes)."""
    return float((np.abs(got - want) / np.abs(want)).max() / key_bound(n))


def order_fault(order, oracle_keys, rel):
    """None when `order` sorts `oracle_keys` ascending wherever neighbouring keys are further apart than rel (relative)."""
    k = oracle_keys[order]
    slack = rel * np.maximum(np.abs(k[:-1]), np.abs(k[1:]))
    bad = np.flatnonzero(k[:-1] > k[1:] + slack)
    return None if bad.size == 0 else f"positions {bad[:5].tolist()} are out of the oracle's order"


def oracle_inverse_keys(Hd, combined):
    inv = np.linalg.inv(Hd).diagonal()
    return -Hd.diagonal() / inv if combined else inv


def tied_pivot_hessian(n=300):
    """A Hessian of small integers, diagonally dominant with equal diagonal entries, float32: column 0 is coupled (2) to
    the first two thirds of the other columns and to nothing else.  Column 0 goes first (all diagonals tie); the uncoupled
    last third keeps the full diagonal and follows, each of its columns swapping one of the columns 1, 2, ... to a far
    position; the coupled columns then tie exactly at every step (equal inputs round equally), and the first POSITION of
    the swapped order -- n / 3, n / 3 + 1, ... before 1, 2, ... -- is not the smallest column index."""
    H = np.zeros((n, n), dtype=np.float32)
    H[0, 1:2 * n // 3 + 1] = H[1:2 * n // 3 + 1, 0] = np.float32(2)
    H[np.arange(n), np.arange(n)] = np.float32(4 * n)
    return H


def pivot_order_by_column(H):
    """obq_ref.pivot_order with ties broken by the smallest COLUMN index instead of the first position: the wrong rule."""
    H = np.asarray(H, dtype=np.float64)
    n = H.shape[0]
    pos, diag, B, d = np.arange(n), H.diagonal().copy(), np.zeros((n, n)), np.zeros(n)
    for k in range(n):
        a = np.abs(diag[pos[k:]])
        tied = np.flatnonzero(a == a.max())
        j = int(tied[np.argmin(pos[k:][tied])]) + k
        pos[[k, j]] = pos[[j, k]]
        p = pos[k]
        d[k] = diag[p]
        rest = pos[k + 1:]
        x = H[p, rest].copy()
        for m in range(k):
            x = x - (B[m, p] * B[m, rest]) / d[m]
        B[k, rest] = x
        diag[rest] = diag[rest] - (x * x) / d[k]
    return pos


# ------------------------------------------------------------------------------------------------ dead columns, mean removal
DEAD_LENGTHS = (1, 255, 257, 1100)
DEAD_ROWS = (1, 2100)
DEAD_KINDS = ("edges", "negative_zero", "none", "all")


def dead_case(R, n, kind):
    """(H, W) float32: a diagonal-heavy H with dead columns (zero diagonal) by `kind`."""
    rng = np.random.default_rng(8600 + n + R)
    H = (rng.standard_normal((n, n)) * 0.01).astype(np.float32)
    H[np.arange(n), np.arange(n)] = (np.abs(rng.standard_normal(n)) + 0.5).astype(np.float32)
    W = synth.make_weights(R, n, 8600 + n + R)
    d = H.diagonal().copy()
    if kind == "edges":  # the first, the last and neighbouring indices
        d[[0, n - 1]] = 0.0
        if n > 8:
            d[[3, 4, 5, n - 2]] = 0.0
    elif kind == "negative_zero":  # counts as dead in NumPy
        d[n // 2] = -0.0
        d[0] = -0.0
    elif kind == "all":
        d[:] = 0.0
    H[np.arange(n), np.arange(n)] = d
    return H, W


def bits_fault(got, want):
    """None when two float32 arrays are equal bit for bit (so -0.0 is not +0.0 and a NaN equals itself)."""
    a, b = np.ascontiguousarray(got, np.float32).view(np.uint32), np.ascontiguousarray(want, np.float32).view(np.uint32)
    if a.shape != b.shape:
        return f"shapes {a.shape} and {b.shape}"
    bad = np.flatnonzero(a.ravel() != b.ravel())
    return None if bad.size == 0 else f"{bad.size} elements differ, the first at flat index {int(bad[0])}"


MEAN_LENGTHS = (1, 257, 1100)


def mean_case(n):
    """(H, mean) float32 for the mean removal: the mean holds +0.0, -0.0 and large entries (products that round, one that
    overflows)."""
    rng = np.random.default_rng(8700 + n)
    H = rng.standard_normal((n, n)).astype(np.float32)
    mean = rng.standard_normal(n).astype(np.float32)
    mean[0] = -0.0 if n > 1 else 3.0e18
    if n > 8:
        mean[1], mean[2], mean[3], mean[n - 1], mean[n // 2] = 0.0, 3.0e18, -1.0e20, 7.0e18, -0.0
    return H, mean
