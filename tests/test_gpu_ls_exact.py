"""The local search on the MI355X against the oracle on exact ("dyadic") layers (tests/ls_exact_model.py): every row, every
move, every gain and every carried error must be the oracle's -- no near-tie evidence, no allowance by count, no tolerance.
On these inputs no float32 operation rounds, so the summation order of the initial product cannot excuse a departure, and
gains tie at most decisions, so the tie rule (the first column; down when best_up == best_down) decides moves all the time.
tests/test_ls_exact_cpu.py holds every case used here to the conditions that make it valid.

Every comparison is on the bits, with one exception that is stated here once: a gain that is ZERO may carry either sign
(the oracle forms -D^2 h - 2 x D, the device (-D^2) h + 2 (-x) D: for D = 0 and x = +0 these are -0 and +0).  The sign of a
zero gain decides nothing -- every use of a gain is a comparison -- so `same` accepts a zero for a zero and nothing else.

Run on the GPU box:  python -m pytest tests/test_gpu_ls_exact.py -m gpu -q
"""

import numpy as np
import pytest
import torch

import ls_exact_model as M
from oracle import obq_ref

pytestmark = pytest.mark.gpu
MOVES = M.MOVES
CASES = M.fixture()[1]


@pytest.fixture(scope="module", autouse=True)
def gpu():
    assert torch.cuda.is_available(), "these tests need the GPU"
    torch.cuda.set_device(0)


@pytest.fixture(scope="module")
def hessians():
    """(n, symmetric) -> (H, H on the device): built and uploaded once per length (n >= 8200: hundreds of megabytes each)."""
    cache = {}

    def get(n, symmetric=True):
        if (n, symmetric) not in cache:
            H = M.dyadic_hessian(n, M.SEED + n, symmetric)
            cache[(n, symmetric)] = (H, torch.from_numpy(H).cuda())
        return cache[(n, symmetric)]

    yield get
    cache.clear()
    torch.cuda.empty_cache()


_references = {}


def reference(key, W, Q0, H, name, moves=MOVES):
    """M.reference_run of a case, computed once and shared (never written to)."""
    if key not in _references:
        _references[key] = M.reference_run(W, Q0, H, M.oracle_grid(name), moves)
    return _references[key]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(got, want):
    """Bit for bit; a zero for a zero of either sign (module docstring)."""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    return got.shape == want.shape and bool(((bits(got) == bits(want)) | ((got == 0) & (want == 0))).all())


def device_search(W, Q0, Hd, name, moves=MOVES, general=None, want_err=True):
    """engine.local_search on device copies: dict(Q, idx, trace, gain_up, gain_down, err) as NumPy arrays.
    general: the `no_wave_search` option for the call (None: as it is)."""
    from sleekit_amd import _lib, engine

    cb = M.device_codebook(name)
    abi = engine.require_uniform(cb)
    Wd, Qd = torch.from_numpy(W).cuda(), torch.from_numpy(Q0).cuda().clone()
    R, n = W.shape
    idx = torch.empty((R, n), dtype=torch.uint8, device="cuda") if len(cb) <= 256 else None
    gains = torch.empty((R, 2, n), dtype=torch.float32, device="cuda")
    err = torch.empty(R, dtype=torch.float32, device="cuda") if want_err else None
    if general is None:
        trace = engine.local_search(Wd, Qd, Hd, abi, moves, idx, want_trace=True, gains=gains, gains_mode=1, row_err=err)
    else:
        with _lib.option("no_wave_search", general):
            trace = engine.local_search(Wd, Qd, Hd, abi, moves, idx, want_trace=True, gains=gains, gains_mode=1, row_err=err)
    torch.cuda.synchronize()
    return dict(Q=Qd.cpu().numpy(), idx=None if idx is None else idx.cpu().numpy(), trace=trace.cpu().numpy(),
                gain_up=gains[:, 0].cpu().numpy(), gain_down=gains[:, 1].cpu().numpy(),
                err=None if err is None else err.cpu().numpy())


def holds(got, want, W, H, name, with_err=True):
    """A device result against M.reference_run's: Q, indices, trace, both gain planes and the carried error."""
    Q, trace, gain_up, gain_down, err = want
    assert np.array_equal(got["trace"], trace), np.argwhere(got["trace"] != trace)[:4]
    assert np.array_equal(bits(got["Q"]), bits(Q))
    if got["idx"] is not None:
        assert np.array_equal(got["idx"], M.oracle_grid(name).index(Q.copy()))
    assert same(got["gain_up"], gain_up) and same(got["gain_down"], gain_down)
    if with_err:
        assert np.array_equal(bits(got["err"]), bits(err))
        # on these inputs the carried error IS the error of the final Q: nothing rounds in either
        assert np.array_equal(bits(got["err"]), bits(obq_ref.row_errors(W, Q, H)))


# ------------------------------------------------------------------------------------------------- a. the general kernel
@pytest.mark.parametrize("n,name", M.general_cases())
def test_general_kernel_is_the_oracle(n, name, hessians):
    """k_local_search<EPT, TABLE, CAND, false> at every EPT on irregular lengths (ls_exact_model.ept_class: 7 .. 1000 run EPT
    4, 1100 EPT 8, 2056 EPT 16, 4104 EPT 32, 8200 EPT 48, 12296 .. 16384 EPT 64): steps kept as floats (EPT <= 8), as packed
    levels (9 and 129 levels from EPT 16), recomputed (the table and 257 levels from EPT 16), with a ragged tail of padded
    slots at every length but 16384."""
    H, Hd = hessians(n)
    W, Q0, _, _, _ = M.case(n, name, H=H)
    got = device_search(W, Q0, Hd, name)
    holds(got, reference((n, name, True), W, Q0, H, name), W, H, name)
    assert (got["trace"] >= 0).sum() >= (4 if n == 7 else 40)  # (the search moved)


# ------------------------------------------------------------------------------------------------- b. the wave kernels
# (a uniform grid of more than 256 levels has no chain-per-lane form: 257 levels with the option at 1 only)
@pytest.mark.parametrize("n,name,general", [(n, name, g) for n, name in M.wave_cases() for g in (-1, 1) if name != "257" or g == 1])
def test_wave_and_general_kernels_are_the_oracle(n, name, general, hessians):
    """The eight chain-per-lane shapes (R = 6: a partial workgroup of the four-rows-per-workgroup form) and the general
    kernel on the same regular rows, each against the oracle rather than against each other."""
    H, Hd = hessians(n)
    W, Q0, _, _, _ = M.case(n, name, H=H)
    assert W.shape[0] == 6
    got = device_search(W, Q0, Hd, name, general=general)
    holds(got, reference((n, name, True), W, Q0, H, name), W, H, name)


# ------------------------------------------------------------------------------------------------- c. plateaus
# (1100 has no chain-per-lane form: one launch)
@pytest.mark.parametrize("n,general", [(1024, -1), (1024, 1), (2048, -1), (2048, 1), (4096, -1), (4096, 1), (1100, 0)])
def test_plateaus_go_to_the_first_column_and_down(n, general):
    rows = M.plateau_rows(n)
    W, Q0, H = M.plateau_layer(n, rows)
    got = device_search(W, Q0, torch.from_numpy(H).cuda(), "9", general=general)
    assert M.plateau_follows_the_rule(got["trace"], rows), got["trace"]
    holds(got, reference(("plateau", n), W, Q0, H, "9"), W, H, "9")


# ------------------------------------------------------------------------------------------------- d. carried gains
@pytest.mark.parametrize("n,general", [(1100, 0), (1024, -1), (1024, 1)])
def test_carried_gains_are_the_oracles(n, general, hessians):
    """5 moves storing the gains, then three calls of one move from the stored gains == 8 moves at once == the oracle's state
    after 8 moves, gains included; obq.quantize_local_search and LocalSearchQuantizer.do_move() k times agree with it."""
    from sleekit_amd import _lib, engine, obq

    H, Hd = hessians(n)
    W, Q0, _, grid, _ = M.case(n, "9", H=H)
    want = reference((n, "9", True, 8), W, Q0, H, "9", 8)
    cb = M.device_codebook("9")
    abi = engine.require_uniform(cb)
    R = W.shape[0]
    with _lib.option("no_wave_search", general):
        once = device_search(W, Q0, Hd, "9", 8)
        Wd, Qd = torch.from_numpy(W).cuda(), torch.from_numpy(Q0).cuda().clone()
        idx = torch.empty((R, n), dtype=torch.uint8, device="cuda")
        gains = torch.empty((R, 2, n), dtype=torch.float32, device="cuda")
        traces = [engine.local_search(Wd, Qd, Hd, abi, 5, idx, want_trace=True, gains=gains, gains_mode=1)]
        for _ in range(3):
            traces.append(engine.local_search(Wd, Qd, Hd, abi, 1, idx, want_trace=True, gains=gains, gains_mode=2))
        torch.cuda.synchronize()
        steps = dict(Q=Qd.cpu().numpy(), idx=idx.cpu().numpy(), trace=torch.cat(traces, dim=1).cpu().numpy(),
                     gain_up=gains[:, 0].cpu().numpy(), gain_down=gains[:, 1].cpu().numpy())
        holds(once, want, W, H, "9")
        holds(steps, want, W, H, "9", with_err=False)
        assert np.array_equal(bits(obq.quantize_local_search(W, Q0, H, cb, 8)), bits(want[0]))
        ls = obq.LocalSearchQuantizer(W, Q0, H, cb)
        state = obq_ref._SearchState(W, Q0, H, grid)
        assert same(ls.gain_up, state.gain[+1]) and same(ls.gain_down, state.gain[-1])
        for k in range(8):
            ls.do_move()
            state.move()
            assert np.array_equal(bits(ls.Q), bits(state.Q)), k
            assert same(ls.gain_up, state.gain[+1]) and same(ls.gain_down, state.gain[-1]), k
        assert np.array_equal(bits(ls.Q), bits(want[0])) and np.array_equal(bits(ls.err), bits(want[4]))


# ------------------------------------------------------------------------------------------------- e. batch
@pytest.mark.parametrize("vouch", [True, False])
@pytest.mark.parametrize("n", [320, 1024])
def test_batch_layers_are_their_own_searches(n, vouch):
    from sleekit_amd import engine

    B, R = 3, 128
    layers = [M.batch_case(n, b, R) for b in range(B)]
    W = torch.from_numpy(np.stack([l[0] for l in layers])).cuda()
    Q = torch.from_numpy(np.stack([l[1] for l in layers])).cuda()
    Hs = [torch.from_numpy(l[2]).cuda() for l in layers]
    idx = torch.empty((B, R, n), dtype=torch.uint8, device="cuda")
    err = torch.empty((B, R), dtype=torch.float32, device="cuda")
    sym = torch.ones(B, dtype=torch.int32, device="cuda") if vouch else None
    engine.local_search_batch(W, Q, Hs, engine.require_uniform(M.device_codebook("9")), MOVES, idx, sym, err)
    torch.cuda.synchronize()
    for b, (w, q0, h, grid, _) in enumerate(layers):
        want_Q, _, _, _, want_err = reference(("batch", n, b), w, q0, h, "9")
        assert np.array_equal(bits(Q[b].cpu().numpy()), bits(want_Q)), b
        assert np.array_equal(idx[b].cpu().numpy(), grid.index(want_Q.copy())), b
        assert np.array_equal(bits(err[b].cpu().numpy()), bits(want_err)), b


# ------------------------------------------------------------------------------------------------- f. a non-symmetric H
@pytest.mark.parametrize("n,general", [(300, 0), (1024, -1), (1024, 1)])
def test_non_symmetric_hessian_reads_columns_then_rows(n, general, hessians):
    """The reference reads COLUMN j of H for the initial gains (delta @ H) and ROW c for the updates of a move on c; a
    non-symmetric integer H tells the two apart.  (No row_err: it is the reference's error for a symmetric H only.)"""
    H, Hd = hessians(n, False)
    assert not M.is_symmetric(H)
    W, Q0, _, _, _ = M.case(n, "9", False, H=H)
    got = device_search(W, Q0, Hd, "9", general=general, want_err=False)
    holds(got, reference((n, "9", False), W, Q0, H, "9"), W, H, "9", with_err=False)


# ------------------------------------------------------------------------------------------------- g. group scales
def grouped_search(W, Q0, S, H, g):
    from sleekit_amd import engine, groups

    Wd, Qd, Sd, Hd = (torch.from_numpy(x).cuda() for x in (W, Q0.copy(), S, H))
    R, n = W.shape
    idx = torch.empty((R, n), dtype=torch.uint8, device="cuda")
    err = torch.empty(R, dtype=torch.float32, device="cuda")
    abi = engine.require_uniform(M.device_codebook("9"))
    trace = groups.run_search_grouped(Wd, Qd, Sd, Hd, abi, g, MOVES, idx, want_trace=True, row_err=err)
    torch.cuda.synchronize()
    return Qd.cpu().numpy(), idx.cpu().numpy(), trace.cpu().numpy(), err.cpu().numpy()


def holds_grouped(got, W, Q0, S, H, grid, g):
    """groups.run_search_grouped against tests/groups_ls_model.py's state, exactly (no follows_model allowance)."""
    want = M.run_state(M.grouped_state(W, Q0, S, H, grid, g), MOVES)
    Q, idx, trace, err = got
    assert np.array_equal(trace, want["trace"])
    assert np.array_equal(bits(Q), bits(want["Q"]))
    assert np.array_equal(idx, grid.index(want["Q"] / np.repeat(S, g, axis=1)))
    assert np.array_equal(bits(err), bits(want["err"]))
    return want


@pytest.mark.parametrize("n,g", M.GROUPED)
def test_grouped_search_is_the_model(n, g, hessians):
    W, Q0, S, H, grid, _ = M.grouped_case(n, g, H=hessians(n)[0])
    holds_grouped(grouped_search(W, Q0, S, H, g), W, Q0, S, H, grid, g)


def test_grouped_plateau_across_groups():
    W, Q0, S, H, grid, _, rows = M.grouped_plateau()
    got = grouped_search(W, Q0, S, H, M.GROUPED_PLATEAU[1])
    assert M.plateau_follows_the_rule(got[2], rows)
    holds_grouped(got, W, Q0, S, H, grid, M.GROUPED_PLATEAU[1])


# ------------------------------------------------------------------------------------------------- the reference's own moves
@pytest.mark.parametrize("i", range(len(CASES)))
def test_device_follows_the_reference(i):
    c = CASES[i]
    W, Q0, H = M.fixture_inputs(c)
    got = device_search(W, Q0, torch.from_numpy(H).cuda(), c["grid"], c["moves"], want_err=c["symmetric"])
    M.check_against_fixture(i, got["trace"], got["Q"])
