"""The exact ("dyadic") local-search layers without a GPU (tests/ls_exact_model.py): every case the GPU tests run
(tests/test_gpu_ls_exact.py) is held to the conditions that make it valid -- whole multiples of the unit, magnitude sums below
2^24 units, the oracle's float32 run equal to its float64 run -- and to the input floors that make it worth running: ties at
the argmax, best_up == best_down, a row that stops early.  The floors are conditions on the inputs (the seeds in
ls_exact_model.SEEDS were chosen to meet them; the oracle alone decides), not measurements of any kernel.  The oracle itself
is held to the real reference's moves on these inputs (tests/golden/ls_exact.npz)."""

import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import ls_exact_model as M  # noqa: E402
from oracle import obq_ref  # noqa: E402

FIX, CASES = M.fixture()

RANDOM = sorted({(n, g, True) for n, g in M.general_cases() + M.wave_cases()} | {(300, "9", False), (1024, "9", False)})
# at most 12 rows x 12 moves: at least this many tied-argmax and best_up == best_down decisions (n = 7 has 7 columns to tie)
FLOORS = {7: (5, 2)}
FLOOR = (20, 5)

_hessian = {}


def hessian(n, symmetric):
    """(H, H as float64, |H|) of the random cases of length n: built once per length (the cases come sorted by it)."""
    if (n, symmetric) not in _hessian:
        _hessian.clear()
        H = M.dyadic_hessian(n, M.SEED + n, symmetric)
        assert symmetric == M.is_symmetric(H)
        _hessian[(n, symmetric)] = (H, H.astype(np.float64), np.abs(H))
    return _hessian[(n, symmetric)]


def meets_floors(n, census):
    tied, updown = FLOORS.get(n, FLOOR)
    return census["tied_argmax"] >= tied and census["up_equals_down"] >= updown and census["stopped_rows"] >= 1


@pytest.mark.parametrize("n,name,symmetric", RANDOM)
def test_random_case_is_exact_and_ties(n, name, symmetric):
    H, H64, absH = hessian(n, symmetric)
    W, Q0, H, grid, unit = M.case(n, name, symmetric, H=H)
    assert W.shape[0] <= 12 and (np.abs(W) > 1).any() and (W != Q0).any()
    few = None if n <= 4096 else [0, W.shape[0] - 1]  # (the bounds carry the guarantee; the float64 run is a second witness)
    r = M.assert_exact(W, Q0, H, unit, grid, M.MOVES, check_rows=few, H64=H64, absH=absH)
    census = dict(r, stopped_rows=int((r["trace"] < 0).any(axis=1).sum()))
    print(n, name, symmetric, {k: census[k] for k in ("decisions", "tied_argmax", "tied_taken", "up_equals_down", "stopped_rows")})
    assert meets_floors(n, census), census
    assert census["tied_taken"] >= 1 or n == 7  # a tie in the plane the move is taken from: the tie rule decided a move


@pytest.mark.parametrize("n", [320, 1024])
def test_batch_layers_are_exact(n):
    hs = []
    for b in range(3):
        W, Q0, H, grid, unit = M.batch_case(n, b)
        r = M.assert_exact(W, Q0, H, unit, grid, M.MOVES)
        assert r["tied_argmax"] >= 20 and r["up_equals_down"] >= 5 and (r["trace"] < 0).any()
        hs.append(H)
    assert not np.array_equal(hs[0], hs[1]) and not np.array_equal(hs[1], hs[2])


@pytest.mark.parametrize("n", [1024, 2048, 4096, 1100])
def test_plateau_ties_go_to_the_first_column_and_down(n):
    rows = M.plateau_rows(n)
    W, Q0, H = M.plateau_layer(n, rows)
    r = M.assert_exact(W, Q0, H, M.grid_unit("9"), M.oracle_grid("9"), M.MOVES)
    assert M.plateau_follows_the_rule(r["trace"], rows)
    assert r["tied_taken"] >= 2 * len(rows) and r["up_equals_down"] >= sum(k == "updown" for k, _ in rows)
    # the rule check can fail: the same trace with the first two moves of a row exchanged
    wrong = r["trace"].copy()
    wrong[0, [0, 1]] = wrong[0, [1, 0]]
    assert not M.plateau_follows_the_rule(wrong, rows)


@pytest.mark.parametrize("n,g", M.GROUPED)
def test_grouped_cases_are_exact(n, g):
    W, Q0, S, H, grid, unit = M.grouped_case(n, g)
    assert set(np.unique(S)) <= {0.5, 1.0, 2.0} and len(np.unique(S)) == 3
    s = np.repeat(S, g, axis=1)
    assert np.array_equal(Q0, (grid(W / s) / (np.float32(1) / s)).astype(np.float32))  # the group quantizer's own values
    few = None if n <= 4096 else np.array([0, W.shape[0] - 1])
    r = M.assert_exact(W, Q0, H, unit, grid, M.MOVES, check_rows=few,
                       make_state=lambda rows, dtype: M.grouped_state(W, Q0, S, H, grid, g, rows, dtype))
    assert r["tied_argmax"] >= 20 and r["up_equals_down"] >= 5 and (r["trace"] < 0).any(), {k: v for k, v in r.items() if np.isscalar(v)}


def test_grouped_plateau_is_exact_and_follows_the_rule():
    W, Q0, S, H, grid, unit, rows = M.grouped_plateau()
    n, g, _ = M.GROUPED_PLATEAU
    r = M.assert_exact(W, Q0, H, unit, grid, M.MOVES,
                       make_state=lambda rr, dtype: M.grouped_state(W, Q0, S, H, grid, g, rr, dtype))
    assert M.plateau_follows_the_rule(r["trace"], rows)
    for row, (_, cols) in enumerate(rows):
        assert len({c // g for c in cols}) == len(cols) and len({S[row, c // g] for c in cols}) == 1


# ------------------------------------------------------------------------------------------------------------------ the comparisons can fail
class WrongTies(obq_ref._SearchState):
    """The oracle's search with one of the mistakes the exact layers are there to find: `last` -- the LAST column wins among
    equal gains (a reduction that keeps the later of two equal values); `up_on_tie` -- up wins when best_up == best_down
    (`>=` in the decision line).  Records its own trace."""

    def __init__(self, W, Q, H, grid, last=False, up_on_tie=False):
        super().__init__(W, Q, H, grid)
        self.last, self.up_on_tie, self.codes = last, up_on_tie, []

    def _apply(self, sign, mask):
        gains, n = self.gain[sign], self.W.shape[1]
        cols = (n - 1 - gains[:, ::-1].argmax(axis=1)) if self.last else gains.argmax(axis=1)
        self.codes[-1][mask] = 2 * cols[mask] + (sign > 0)
        if self.last:
            rows = np.arange(len(cols))[mask]
            kept = gains[rows, cols[mask]].copy()
            self._apply_marked(sign, mask, rows, cols[mask], kept)
        else:
            super()._apply(sign, mask)

    def _apply_marked(self, sign, mask, rows, cols, kept):
        # obq_ref._SearchState._apply with the column given: the gain it subtracts and updates is the kept one
        new = self.cand[sign][rows, cols]
        q_old = self.Q[rows, cols].copy()
        self.Q[rows, cols] = new
        up_old = self.cand[+1][rows, cols].copy()
        self.cand[+1][rows, cols] = self.grid.quantize_up(new)
        down_old = self.cand[-1][rows, cols].copy()
        self.cand[-1][rows, cols] = self.grid.quantize_down(new)
        self.err[rows] -= kept
        self._refresh(+1, rows, cols, q_old, up_old)
        self._refresh(-1, rows, cols, q_old, down_old)

    def move(self):
        bu, bd = self.gain[+1].max(axis=1), self.gain[-1].max(axis=1)
        go_up = ((bu >= bd) if self.up_on_tie else (bu > bd)) & (bu > 0)
        go_down = ~go_up & (bd > 0)
        self.codes.append(np.full(len(bu), -1, dtype=np.int32))
        self._apply(+1, go_up)
        self._apply(-1, go_down)


def wrong_trace(W, Q0, H, grid, **mistake):
    state = WrongTies(W, Q0, H, grid, **mistake)
    for _ in range(M.MOVES):
        state.move()
    return np.stack(state.codes, axis=1)


def test_the_mistaken_search_without_a_mistake_is_the_oracle():
    W, Q0, H, grid, _ = M.case(300, "9")
    assert np.array_equal(wrong_trace(W, Q0, H, grid), M.reference_run(W, Q0, H, grid, M.MOVES)[1])


@pytest.mark.parametrize("n,name,symmetric", [c for c in RANDOM if c[0] <= 4104])
def test_a_wrong_tie_rule_shows_on_every_case(n, name, symmetric):
    """Either mistake changes the moves of every random case (lengths up to 4104 here: the longer ones meet the same floors)."""
    H = hessian(n, symmetric)[0]
    W, Q0, H, grid, _ = M.case(n, name, symmetric, H=H)
    want = M.reference_run(W, Q0, H, grid, M.MOVES)[1]
    assert not np.array_equal(wrong_trace(W, Q0, H, grid, up_on_tie=True), want)
    if n > 7:  # (7 columns: ties at the argmax, but none in the plane a move is taken from)
        assert not np.array_equal(wrong_trace(W, Q0, H, grid, last=True), want)


@pytest.mark.parametrize("n", [1024, 2048, 4096, 1100])
def test_a_wrong_tie_rule_shows_on_every_plateau_row(n):
    rows = M.plateau_rows(n)
    W, Q0, H = M.plateau_layer(n, rows)
    grid = M.oracle_grid("9")
    want = M.reference_run(W, Q0, H, grid, M.MOVES)[1]
    last, up = wrong_trace(W, Q0, H, grid, last=True), wrong_trace(W, Q0, H, grid, up_on_tie=True)
    for r, (kind, cols) in enumerate(rows):  # (one up against one down column: no tie inside a plane)
        assert (kind == "updown" and len(cols) == 2) or not np.array_equal(last[r], want[r]), r
        assert kind == "down" or not np.array_equal(up[r], want[r]), r


# ------------------------------------------------------------------------------------------------------------------ fixture
def test_every_instantiation_is_reached():
    """The general kernel's classes by the dispatch's own arithmetic (ls_exact_model.ept_class), not by a list: every EPT
    with a table, with packed levels (129 among them) and recomputing on more than 256 levels, each at a ragged length."""
    assert [M.ept_class(n) for n in (1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193, 12288, 12289, 16384)] == \
        [4, 8, 8, 16, 16, 32, 32, 48, 48, 64, 64]
    assert all(M.wave_shape(n) is None for n in M.GENERAL_N) and M.wave_shape(320) is None
    assert {M.wave_shape(n) for n in M.WAVE_N} == {(a, b, c) for a in (12, 16) for b in (1, 2) for c in (1, 4)}
    ragged = {(M.ept_class(n), name) for n, name in M.general_cases() if n % 256}
    for ept in (4, 8, 16, 32, 48, 64):
        assert {(ept, "9"), (ept, "table"), (ept, "257")} <= ragged
        assert ept < 16 or (ept, "129") in ragged
    assert {(M.ept_class(n), M.cand_kind(n, g)) for n, g in M.general_cases()} == \
        {(4, 1), (8, 1)} | {(e, k) for e in (16, 32, 48, 64) for k in (0, 2)}


def test_fixture_cover():
    plain = {(c["n"], c["grid"], c["symmetric"]) for c in CASES if "plateau" not in c}
    assert plain == {(7, "9", True), (96, "9", True), (300, "9", True), (1100, "9", True), (1100, "table", True),
                     (1100, "257", True), (300, "9", False)}
    assert any("updown" in [k for k, _ in c.get("plateau", [])] for c in CASES)
    assert all(c["moves"] == M.MOVES and c.get("R", 4) <= 12 for c in CASES)


@pytest.mark.parametrize("i", range(len(CASES)))
def test_oracle_follows_the_reference(i):
    c = CASES[i]
    W, Q0, H = M.fixture_inputs(c)
    Q, trace, _, _, _ = M.reference_run(W, Q0, H, M.oracle_grid(c["grid"]), c["moves"])
    M.check_against_fixture(i, trace, Q)
    if "plateau" in c:
        assert M.plateau_follows_the_rule(FIX[f"trace_{i}"], c["plateau"])  # the reference's own behaviour at exact ties
    else:  # the fixture's seeds are the cases' own
        assert c["seed"] == M.SEEDS.get((c["n"], c["grid"], c["symmetric"]), M.SEED + c["n"]) and c["R"] == M.rows_of(c["n"])
