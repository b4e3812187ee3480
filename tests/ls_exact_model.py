"""Exact ("dyadic") layers for the local search: inputs on which every float32 operation of the search is exact, so the
reference, the oracle (oracle.obq_ref) and the device must agree on every row, every move, every gain bit and every carried
error -- no near-tie allowance -- and on which gains tie constantly, so the tie rule (np.argmax: the first column wins;
down wins when best_up == best_down, obq.py:338-346) is exercised at almost every decision.

Plain NumPy, no GPU.  tests/test_ls_exact_cpu.py checks the input conditions of every case listed here (exactness, the tie
floors, a row that stops early); tests/test_gpu_ls_exact.py runs the same cases on the device.

Why the inputs are exact.  W and every codebook value are multiples of `unit` (a power of two, a quarter of the smallest grid
step), H holds small integers.  Every term of delta @ H is then a multiple of `unit`, every term of a gain or of a row's error
a multiple of unit^2, and while the sum of the terms' magnitudes stays below 2^24 of these units every partial sum in ANY
order is a float32 number: BLAS, NumPy's pairwise sum, the MFMA and the bf16x3 split all give the same bits (assert_exact).
"""

import numpy as np

from oracle import grid as ogrid
from oracle import obq_ref

TABLE = (-1.0, -0.5, -0.25, 0.0, 0.125, 0.5, 1.0)  # dyadic values, uneven gaps (smallest 1/8)
UNIFORM = (2, 3, 5, 9, 17, 129, 257)  # levels on [-1, 1] whose step 2 / (levels - 1) is a power of two
MOVES = 12
BANDS = 3


# ------------------------------------------------------------------------------------------------------------------ grids
def oracle_grid(name):
    """name: "table" or the number of levels of a uniform grid on [-1, 1], as a string."""
    return ogrid.TableGrid(TABLE) if name == "table" else ogrid.UniformGrid(int(name), -1, 1)


def grid_step(name):
    """The smallest gap between two grid values."""
    return 0.125 if name == "table" else 2.0 / (int(name) - 1)


def grid_unit(name):
    """A quarter of the smallest grid step: weights on whole steps would start at their optimum."""
    assert name == "table" or int(name) in UNIFORM
    return grid_step(name) / 4


def device_codebook(name):
    from sleekit_amd.codebook import Codebook, UniformCodebook

    return Codebook(np.array(TABLE, dtype=np.float32)) if name == "table" else UniformCodebook(int(name), -1, 1)


def reference_codebook(ref_codebook, name):
    """The reference's own codebook (ref_codebook: its `sleekit.codebook` module; the fixture generator only)."""
    if name == "table":
        return ref_codebook.Codebook(np.array(TABLE, dtype=np.float32))
    return ref_codebook.UniformCodebook(int(name), -1, 1)


# ------------------------------------------------------------------------------------------------------------------ layers
def dyadic_hessian(n, seed, symmetric=True):
    """(n, n) float32 of small integers: BANDS bands in [-2, 2] next to the diagonal, about n / 2 scattered far couplings in
    [-2, 2], a diagonal in [1, 8].  symmetric=False: the two triangles are drawn independently (row c and column c differ).
    Index assignment into zeros: n = 16384 takes about a second."""
    rng = np.random.default_rng([seed, n, 1])
    H = np.zeros((n, n), dtype=np.float32)
    i = np.arange(n)

    def both(a, b):
        v = rng.integers(-2, 3, len(a))
        H[a, b] = v
        H[b, a] = v if symmetric else rng.integers(-2, 3, len(a))

    for k in range(1, min(BANDS, n - 1) + 1):
        both(i[:-k], i[k:])
    a, b = rng.integers(0, n, n // 2), rng.integers(0, n, n // 2)
    a, b = np.minimum(a, b), np.maximum(a, b)
    far = np.unique(a[b - a > BANDS].astype(np.int64) * n + b[b - a > BANDS])  # (every pair once: no order of assignment)
    both(far // n, far % n)
    H[i, i] = rng.integers(1, 9, n)
    return H


def dyadic_layer(R, n, seed, unit, grid=None, symmetric=True, reach=4, quiet_rows=1, H=None):
    """W (R, n) float32 multiples of `unit` in [-1 - reach unit, 1 + reach unit] and H = dyadic_hessian(n, seed, symmetric)
    (or the H given: the Hessian depends on n and the seed alone, so cases of one length share it).

    reach = 4 units is one step of the uniform grid the unit belongs to: |W| up to 1.25 for 9 levels.  Weights past the ends
    clip, so their candidates saturate at the top / bottom level (D = 0, gain exactly 0: never taken).  A reach of 0.25
    whatever the grid would leave a fifth of the weights of the 257-level layer 128 units off the grid and the error sum of
    a long row past 2^24 units.
    quiet_rows (needs `grid`): the last rows sit ON the grid except at three columns ("pruned" rows): only the few columns
    coupled to those three can gain, so such a row stops before the moves run out (-1 in its trace)."""
    rng = np.random.default_rng([seed, n, R, 2])
    top = int(round(1.0 / unit)) + reach
    W = (rng.integers(-top, top + 1, size=(R, n)).astype(np.float32) * np.float32(unit)).astype(np.float32)
    if grid is not None:
        for r in range(R - quiet_rows, R):
            off = rng.choice(n, size=min(3, n), replace=False)
            keep = W[r, off].copy()
            W[r] = grid(W[r].copy())
            W[r, off] = keep
    if H is None:
        H = dyadic_hessian(n, seed, symmetric)
    return W, H


def start(W, grid):
    """Q0: every weight on its nearest grid value (what the column loop would leave without error propagation)."""
    return np.asarray(grid(W.copy()), dtype=np.float32)


def plateau_layer(n, rows, seed=0):
    """A constructed layer of exact ties on the 9-level grid (step 1/4): H is a positive integer diagonal, so the gain of
    moving column j by D is -h_j D (D + 2 (Q0 - W)_j), a function of that column alone.  One row per entry of `rows`:

      ("down", cols)    W = 1/16 and Q0 = 1/2 at every column of `cols` (h = 8): moving down gains 8 * 5/32, then 8 * 1/32
                        once more -- the same value at all of them, so the search must take them in increasing order, twice;
      ("updown", cols)  W = 1/8, exactly halfway between two levels.  The FIRST column of `cols` starts at Q0 = -1/4 and gains
                        8 * 1/8 by moving up, the others start at Q0 = 1/2 and gain the same by moving down:
                        best_up == best_down, so the down moves come first although an up move has the smaller column.

    Elsewhere: five columns per row with W = 0, Q0 = 1/4 and their own h in [1, 8] (gain h / 16 <= 1/2: strictly smaller
    than the tied columns' first gain, 5/4 or 1), the rest on grid values with Q0 = W (gains -h / 16 or, saturated, 0).
    Returns W, Q0, H."""
    rng = np.random.default_rng([seed, n, len(rows), 3])
    R = len(rows)
    h = rng.integers(1, 9, n).astype(np.float32)
    W = (rng.integers(-4, 5, size=(R, n)).astype(np.float32) * np.float32(0.25)).astype(np.float32)
    Q0 = W.copy()
    tied = sorted({c for _, cols in rows for c in cols})
    free = np.setdiff1d(np.arange(n), tied)
    for r, (kind, cols) in enumerate(rows):
        cols = list(cols)
        assert kind in ("down", "updown") and len(set(cols)) == len(cols) and 0 <= min(cols) and max(cols) < n
        others = rng.choice(free, size=min(5, len(free)), replace=False)
        W[r, others], Q0[r, others] = 0.0, 0.25
        if kind == "down":
            W[r, cols], Q0[r, cols] = 0.0625, 0.5
        else:
            W[r, cols] = 0.125
            Q0[r, cols[0]] = -0.25
            Q0[r, cols[1:]] = 0.5
    h[tied] = 8.0
    H = np.zeros((n, n), dtype=np.float32)
    H[np.arange(n), np.arange(n)] = h
    return W, Q0, H


def plateau_follows_the_rule(trace, rows):
    """The tie rule alone (no arithmetic) on a trace of plateau_layer(n, rows): among a row's moves on its tied columns the
    first ones are the down moves in increasing column order, then (up against down) the up move of the first column."""
    for r, (kind, cols) in enumerate(rows):
        cols = list(cols)
        want = [2 * c for c in sorted(cols)] if kind == "down" else [2 * c for c in sorted(cols[1:])] + [2 * cols[0] + 1]
        got = [int(t) for t in trace[r] if t >= 0 and t // 2 in cols]
        if got[:len(want)] != want:
            return False
    return True


# ------------------------------------------------------------------------------------------------------------------ the run
def decision(gain_up, gain_down, Q, Q_up, Q_down):
    """The move every row is about to take (obq.py:338-346), read off the search's arrays (the oracle's or the reference's
    own: this only inspects them).  Returns (code, go_up, stays): code = 2 * column + up, or -1 where no gain is positive
    or the "move" is one onto the value the weight already has (`stays`).
    Such a candidate (the up-candidate of the top level) has D = 0.  With a symmetric H its gain is exactly 0 on exact
    inputs and it is never taken.  A non-symmetric H leaves it a residue (the initial gains read column c of H, the updates
    row c): the reference then "moves" onto the same value, which changes neither Q nor any gain, and repeats that until
    the moves run out -- "stay" in the device's trace, as oracle.obq_ref.move_record counts it."""
    rows = np.arange(Q.shape[0])
    bu, bd = gain_up.max(axis=1), gain_down.max(axis=1)
    go_up = (bu > bd) & (bu > 0)
    go_down = ~go_up & (bd > 0)
    col = np.where(go_up, gain_up.argmax(axis=1), gain_down.argmax(axis=1))
    step = np.where(go_up, Q_up[rows, col], Q_down[rows, col]) - Q[rows, col]
    live = go_up | go_down
    stays = live & (step == 0)
    return np.where(live & ~stays, 2 * col + go_up, -1).astype(np.int32), go_up, stays


def run_state(state, moves):
    """Drive an obq_ref._SearchState `moves` moves.  Returns dict(Q, trace, gain_up, gain_down, err, tied_argmax, tied_taken,
    up_equals_down, decisions, non_moves): the trace in the device's convention (2 * column + up; -1 from the first move at which the
    row's best gain is not positive) and the tie census over the decisions whose best gain is positive:
      tied_argmax     the maximum of gain_up or of gain_down is attained at more than one column
      tied_taken      ... of the plane the move is taken from
      up_equals_down  best_up == best_down."""
    R = state.W.shape[0]
    trace = np.full((R, moves), -1, dtype=np.int32)
    tied_argmax = tied_taken = up_equals_down = decisions = non_moves = 0
    for m in range(moves):
        gu, gd = state.gain[+1], state.gain[-1]
        bu, bd = gu.max(axis=1), gd.max(axis=1)
        code, go_up, stays = decision(gu, gd, state.Q, state.cand[+1], state.cand[-1])
        live = code >= 0
        non_moves += int(stays.sum())
        trace[:, m] = code
        if m:
            assert (trace[trace[:, m - 1] < 0, m] < 0).all()  # a row that stopped stays stopped
        many_u, many_d = (gu == bu[:, None]).sum(axis=1) > 1, (gd == bd[:, None]).sum(axis=1) > 1
        decisions += int(live.sum())
        tied_argmax += int(((many_u | many_d) & live).sum())
        tied_taken += int((np.where(go_up, many_u, many_d) & live).sum())
        up_equals_down += int(((bu == bd) & live).sum())
        state.move()
    return dict(Q=state.Q, trace=trace, gain_up=state.gain[+1], gain_down=state.gain[-1], err=state.err,
                tied_argmax=tied_argmax, tied_taken=tied_taken, up_equals_down=up_equals_down, decisions=decisions,
                non_moves=non_moves)


def reference_run(W, Q0, H, grid, moves):
    """(Q, trace, gain_up, gain_down, err) of oracle.obq_ref's search state after `moves` moves from Q0."""
    r = run_state(obq_ref._SearchState(W, Q0, H, grid), moves)
    return r["Q"], r["trace"], r["gain_up"], r["gain_down"], r["err"]


def tie_census(W, Q0, H, grid, moves):
    """dict(decisions, tied_argmax, tied_taken, up_equals_down, stopped_rows) of a case (see run_state)."""
    r = run_state(obq_ref._SearchState(W, Q0, H, grid), moves)
    out = {k: r[k] for k in ("decisions", "tied_argmax", "tied_taken", "up_equals_down")}
    out["stopped_rows"] = int((r["trace"] < 0).any(axis=1).sum())
    return out


# ------------------------------------------------------------------------------------------------------------------ validity
def _whole(x, unit):
    y = np.asarray(x) / np.float32(unit)  # (a power of two: the quotient is exact in the array's own type)
    return bool((y == np.rint(y)).all())


def is_symmetric(H):
    """np.array_equal(H, H.T) of a sparse H, by its non-zeros (the transposed read of 16384 x 16384 is slow)."""
    a, b = np.nonzero(H)
    return bool((H[a, b] == H[b, a]).all())


def exact_bounds(W, Q, A, unit):
    """For A = |H|: (max_j sum_k |d_k| |H_kj| / unit over H and over its transpose, max_r sum_j |d_j| (|d| @ |H|)_j / unit^2) for d = Q - W.
    The sums are of non-negative whole numbers, so float32 products are exact while they stay below 2^24, and a sum that
    would pass 2^24 still comes out at least 2^24: the comparison with the bound is right either way."""
    d = (np.abs(Q.astype(np.float64) - W) / unit).astype(np.float32)
    cols, rows = d @ A, d @ A.T
    return float(max(cols.max(), rows.max())), float((cols.astype(np.float64) * d).sum(axis=1).max())


def assert_exact(W, Q0, H, unit, grid, moves, check_rows=None, make_state=None, H64=None, absH=None):
    """What makes a case valid: W, Q0 and the grid are whole multiples of `unit`, H of 1; the magnitude sums of delta @ H (by
    columns and, for the search's row sums, by rows of H) and of the rows' errors stay below 2^24 units -- at the start and at
    the end of the search; and the oracle's search run in float32 and in float64 (the latter on `check_rows`, default all) agrees
    exactly on Q, both gain planes and err.  make_state(rows, dtype): the search state of these rows with every input as `dtype`
    (default: obq_ref._SearchState on `grid`).  H64, absH: H as float64 and |H| where the caller keeps them.
    Returns the float32 run (run_state's dict) of all rows."""
    assert _whole(W, unit) and _whole(Q0, unit) and _whole(H, 1.0)
    values = grid.values if hasattr(grid, "values") else None
    assert values is None or _whole(values, unit)
    rows = np.arange(W.shape[0]) if check_rows is None else np.asarray(check_rows)
    if make_state is None:
        def make_state(rows, dtype):
            h = H if dtype == np.float32 else (H.astype(np.float64) if H64 is None else H64)
            return obq_ref._SearchState(W[rows].astype(dtype), Q0[rows].astype(dtype), h, grid)
    r32 = run_state(make_state(np.arange(W.shape[0]), np.float32), moves)
    assert r32["non_moves"] == 0 or not is_symmetric(H)
    A = np.abs(H) if absH is None else absH
    for Q in (Q0, r32["Q"]):
        b1, b2 = exact_bounds(W, Q, A, unit)
        assert b1 < 2.0 ** 24 and b2 < 2.0 ** 24, (b1, b2)
    r64 = run_state(make_state(rows, np.float64), moves)
    for k in ("Q", "gain_up", "gain_down", "err"):
        assert r32[k].dtype == np.float32 and r64[k].dtype == np.float64, k
        assert np.array_equal(r32[k][rows].astype(np.float64), r64[k]), k
    assert np.array_equal(r32["trace"][rows], r64["trace"])
    assert _whole(r32["Q"], unit)
    return r32


# ------------------------------------------------------------------------------------------------------------------ the cases
# the general-kernel lengths: none halves to multiples of 8 down to 128 with 8, 16, 32 or 64 leaves, so no wave form takes them
GENERAL_N = (7, 96, 300, 1000, 1100, 2056, 4104, 8200, 12296, 16380, 16384)
WAVE_N = (768, 1024, 1536, 2048, 3072, 4096, 6144, 8192)
SEED = 9000


def ept_class(n):
    """EPT of the k_local_search instantiation that `local_search_impl` launches for a row of n columns (search.hip): the
    slots per thread (n + 255) / 256 of a 256-thread workgroup, in the first class that holds them."""
    slots = (n + 255) // 256
    return next(e for e in (4, 8, 16, 32, 48, 64) if slots <= e)


def wave_shape(n):
    """(M8, S, WAVES) of the k_local_search_wave instantiation for a row of n columns, or None where there is none: n halved
    while above 128 must stay a multiple of 16 (even halves of multiples of 8), giving 8, 16, 32 or 64 leaves of m = 96 or 128."""
    m, leaves = n, 1
    while m > 128:
        if m % 2 or (m // 2) % 8:
            return None
        m, leaves = m // 2, leaves * 2
    if m % 8 or m < 8 or (m // 8, leaves) not in {(a, b) for a in (12, 16) for b in (8, 16, 32, 64)}:
        return None
    return m // 8, 2 if leaves in (16, 64) else 1, 4 if leaves >= 32 else 1


def cand_kind(n, name):
    """How the general kernel keeps the candidate steps for (n, grid): 1 floats (EPT <= 8), 2 packed levels (a uniform grid
    of at most 256 levels), 0 recomputed."""
    return 1 if ept_class(n) <= 8 else 2 if name != "table" and int(name) <= 256 else 0


def general_cases():
    """(n, grid name) of the general-kernel cases: 9 levels, the table and 257 levels per length; 129 levels wherever the
    levels are packed (EPT >= 16: from n = 2056; the top byte values); 2, 3, 5 and 17 levels at n = 4104 (packed levels of
    the shortest grids: with 2 levels every down-candidate and every up-candidate of the top level saturates)."""
    out = []
    for n in GENERAL_N:
        out += [(n, g) for g in ("9", "table", "257") + (("129",) if ept_class(n) >= 16 else ()) + (("2", "3", "5", "17") if n == 4104 else ())]
    return out


def wave_cases():
    return [(n, g) for n in WAVE_N for g in ("9", "table", "257")]


def rows_of(n):
    return 5 if n % 2 else 6


# seeds that meet the input floors of tests/test_ls_exact_cpu.py where SEED + n does not (the reference alone decides)
SEEDS = {(7, "257", True): 32007, (7, "9", True): 12007, (7, "table", True): 313007, (96, "9", True): 10096,
         (96, "table", True): 160096, (300, "9", True): 10300, (300, "table", True): 14300, (1024, "257", True): 11024,
         (1024, "table", True): 13024, (1100, "257", True): 11100, (1100, "table", True): 21100, (1536, "257", True): 11536,
         (1536, "table", True): 12536, (2048, "table", True): 12048, (2056, "table", True): 16056, (3072, "257", True): 13072,
         (3072, "table", True): 14072, (4096, "table", True): 14096, (6144, "table", True): 16144, (8200, "9", True): 18200,
         (8200, "table", True): 19200, (12296, "table", True): 26296, (16380, "257", True): 26380}


def case(n, name, symmetric=True, R=None, H=None, seed=None, quiet_rows=1):
    """W, Q0, H, grid, unit of the random case (n, grid name).  The Hessian follows n alone (pass it to share it)."""
    grid, unit = oracle_grid(name), grid_unit(name)
    seed = SEEDS.get((n, name, symmetric), SEED + n) if seed is None else seed
    H = dyadic_hessian(n, SEED + n, symmetric) if H is None else H
    W, H = dyadic_layer(rows_of(n) if R is None else R, n, seed, unit, grid, symmetric, quiet_rows=quiet_rows, H=H)
    return W, start(W, grid), H, grid, unit


_fixture = []


def fixture():
    """(arrays, cases) of tests/golden/ls_exact.npz (tests/golden/make_golden_ls_exact.py), loaded once."""
    if not _fixture:
        import json
        import os

        fix = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ls_exact.npz"))
        _fixture.extend([fix, json.loads(str(fix["meta"]))["cases"]])
    return _fixture[0], _fixture[1]


def check_against_fixture(i, trace, Q):
    """The moves and the final values of fixture case i against the reference's own."""
    fix, cases = fixture()
    c = cases[i]
    assert np.array_equal(trace, fix[f"trace_{i}"]), c
    if f"idx_{i}" in fix:
        assert np.array_equal(oracle_grid(c["grid"]).index(Q.copy()), fix[f"idx_{i}"]), c
    else:
        assert np.array_equal(Q.view(np.uint32), fix[f"Q_{i}"].view(np.uint32)), c


def fixture_inputs(c):
    """W, Q0, H of a case of tests/golden/ls_exact.npz (c: its entry of the fixture's meta)."""
    if "plateau" in c:
        return plateau_layer(c["n"], [(k, tuple(cols)) for k, cols in c["plateau"]])
    W, Q0, H, _, _ = case(c["n"], c["grid"], c["symmetric"], R=c["R"], seed=c["seed"])
    return W, Q0, H


def batch_case(n, b, R=128):
    """Layer b of the batch cases: its own Hessian and weights, the 9-level grid."""
    return case(n, "9", R=R, H=dyadic_hessian(n, SEED + n + 1 + b), seed=SEED + n + 1 + b, quiet_rows=8)


# ------------------------------------------------------------------------------------------------------------------ groups
GROUPED = ((96, 32), (1100, 4), (4104, 8), (1024, 128))
SCALE_SEEDS = {(96, 32): 6, (1100, 4): 3, (4104, 8): 1, (1024, 128): 1}  # (chosen like SEEDS: the input floors)
GROUPED_PLATEAU = (1024, 128, (("down", (5, 300)), ("updown", (130, 700)), ("down", (3, 259, 700)), ("updown", (1023, 0, 640))))


def _scales(rng, R, n, g):
    return rng.choice(np.array([0.5, 1.0, 2.0], dtype=np.float32), size=(R, n // g))


def grouped_case(n, g, H=None):
    """W, Q0, S, H, grid, unit: the 9-level case of length n with a scale from {1/2, 1, 2} per row and group of g columns.
    The group quantizer codebook(x / s) / (1 / s) is the grid scaled by s, exactly for a power of two: W and Q0 are the
    per-row case's, times the scales; the common unit is half the per-row one."""
    W, Q0, H, grid, unit = case(n, "9", H=H)
    S = _scales(np.random.default_rng([SEED, n, g, 4 + 10 * SCALE_SEEDS[(n, g)]]), W.shape[0], n, g)
    s = np.repeat(S, g, axis=1)
    return (W * s).astype(np.float32), (Q0 * s).astype(np.float32), S, H, grid, unit / 2


def grouped_plateau():
    """W, Q0, S, H, grid, unit, rows: plateau_layer whose tied columns sit in different groups with equal scales."""
    n, g, rows = GROUPED_PLATEAU
    W, Q0, H = plateau_layer(n, rows)
    S = _scales(np.random.default_rng([SEED, n, g, 5]), len(rows), n, g)
    for r, (_, cols) in enumerate(rows):
        assert len({c // g for c in cols}) == len(cols)
        S[r, [c // g for c in cols]] = S[r, cols[0] // g]
    s = np.repeat(S, g, axis=1)
    return (W * s).astype(np.float32), (Q0 * s).astype(np.float32), S, H, oracle_grid("9"), grid_unit("9") / 2, rows


def grouped_state(W, Q0, S, H, grid, g, rows=None, dtype=np.float32):
    """tests/groups_ls_model.py's search state (the oracle's, with the group quantizer's candidates) of the given rows."""
    from groups_ls_model import GroupCandidates, _GroupedState

    rows = np.arange(W.shape[0]) if rows is None else rows
    return _GroupedState(W[rows].astype(dtype), Q0[rows].astype(dtype), H.astype(dtype), GroupCandidates(grid, S[rows], g))


# ------------------------------------------------------------------------------------------------------------------ plateaus
def leaf_width(n):
    """m of the chain-per-lane kernels: n halved until it is at most 128 (their column j sits in thread
    8 * ((j / m) % (8 WAVES)) + (j % m) % 8)."""
    m = n
    while m > 128:
        m //= 2
    return m


def plateau_rows(n):
    """The tied sets of the plateau case of length n: both columns in one thread of the general kernel (j, j + 256); in
    neighbouring lanes; in different waves; the first and the last column; in the chain-per-lane layout, the smaller column
    in the higher lane -- inside a leaf (2 in lane 2, 9 in lane 1) and, where the row has them, across register sets or
    waves (5 against the first column of leaf 8); a three-way tie; up against down in both column orders."""
    m = leaf_width(n)
    rows = [("down", (37, 37 + 256)), ("down", (100, 101)), ("down", (10, 74)), ("down", (20, 720)), ("down", (0, n - 1)),
            ("down", (2, 9)), ("down", (3, 259, 700)), ("updown", (2, 9)), ("updown", (9, 2)), ("updown", (0, n - 1, 5))]
    if 8 * m < n:
        rows += [("down", (5, 8 * m)), ("updown", (5, 8 * m)), ("updown", (8 * m, 5))]
    return rows
