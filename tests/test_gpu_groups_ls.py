"""Local search on group-scaled layers on the MI355X (sleekit_amd.groups.local_search_grouped, slk_local_search_grouped)
against the reference's own moves (tests/golden/groups_ls.npz), the NumPy model (tests/groups_ls_model.py) and itself.

Row-by-row parity: a row may end differently from the reference or the model only where one of its decisions was a
proven near-tie (tests/ls_evidence.py) -- no allowance by count.

Run on the GPU box:  python -m pytest tests/test_gpu_groups_ls.py -m gpu -q
"""

import numpy as np
import pytest
import torch

from groups_ls_model import local_search_grouped as model_search, trace_of
from groups_model import oracle_grid
from ls_evidence import explain_rows
from oracle import obq_ref
from sleekit_amd import synth
from test_groups_ls_cpu import CASES, case_inputs, check_against_fixture

pytestmark = pytest.mark.gpu
NEAR_LIMIT = 64.0


@pytest.fixture(scope="module", autouse=True)
def gpu():
    assert torch.cuda.is_available(), "these tests need the GPU"
    torch.cuda.set_device(0)


def codebook(name):
    from sleekit_amd.codebook import Codebook, UniformCodebook

    return Codebook.nf4() if name == "nf4" else UniformCodebook(int(name), -1, 1)


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def device_search(W, Q0, S, cb, H, g, moves, want_idx=True):
    """(Q, idx, trace, row_err) of slk_local_search_grouped on device copies of NumPy / device inputs."""
    from sleekit_amd import _device as dev, engine, groups

    Wd, Sd, Hd = dev.to_device(W), dev.to_device(S), dev.to_device(H)
    Qd = dev.to_device(Q0).clone()
    R, n = Wd.shape
    idx = torch.empty((R, n), dtype=torch.uint8, device=Wd.device) if want_idx else None
    err = torch.empty(R, dtype=torch.float32, device=Wd.device)
    trace = groups.run_search_grouped(Wd, Qd, Sd, Hd, engine.require_uniform(cb), g, moves, idx, want_trace=True, row_err=err)
    torch.cuda.synchronize()
    return Qd.cpu().numpy(), None if idx is None else idx.cpu().numpy(), trace.cpu().numpy(), err.cpu().numpy()


def grouped_start(R, n, g, cbn, seed, device_layer=False, mode="mse"):
    """W, H (float32 NumPy), S and Q0 = quantize_grouped(W, S, cb, H, g) (0 moves) for a synthetic layer."""
    from sleekit_amd import groups

    if device_layer:
        L = synth.make_layer_device(R, n, seed, "cuda")
        Wd, Hd = L["W"], L["H"]
    else:
        L = synth.make_layer(R, n, seed)
        Wd, Hd = torch.from_numpy(L["W"]).cuda(), torch.from_numpy(L["H"].astype(np.float32)).cuda()
    cb = codebook(cbn)
    S = groups.compute_group_scaling(Wd, cb, g, Hd, mode=mode)
    Q0 = groups.quantize_grouped(Wd, S, cb, Hd, g)
    return Wd.cpu().numpy(), Hd.cpu().numpy(), S.cpu().numpy(), Q0.cpu().numpy()


def follows_model(W, Q0, S, cbn, H, g, moves, got_Q, got_trace, rows=None):
    """The device's rows against the model's: equal bit for bit, or departing at a proven near-tie of the model's."""
    rows = np.arange(W.shape[0]) if rows is None else rows
    records = []
    want = model_search(W[rows], Q0[rows], S[rows], oracle_grid(cbn), H, g, moves, records)
    bad = np.flatnonzero((bits(got_Q[rows]) != bits(want)).any(axis=1))
    near = obq_ref.near_tie_summary(records, NEAR_LIMIT)
    explain_rows(bad, got_trace[rows], near)
    good = np.setdiff1d(np.arange(len(rows)), bad)
    assert np.array_equal(got_trace[rows][good], trace_of(records)[good])
    return len(bad)


# ---------------------------------------------------------------------------------------------------------------- fixtures
@pytest.mark.parametrize("i", range(len(CASES)))
def test_fixture_matches_the_reference(i):
    c = CASES[i]
    W, H, S, Q0 = case_inputs(i)
    Q, idx, trace, _ = device_search(W, Q0, S, codebook(c["codebook"]), H, c["g"], c["moves"])
    check_against_fixture(i, idx, trace)


# ---------------------------------------------------------------------------------------------------------------- model
@pytest.mark.parametrize("R,n,g,cbn,moves,seed", [
    (64, 96, 32, "8", 25, 7101), (64, 96, 1, "3", 10, 7102), (64, 96, 96, "nf4", 10, 7103), (33, 172, 43, "16", 40, 7104),
    (17, 768, 3, "4", 30, 7105), (40, 1024, 128, "8", 10, 7106),
])
def test_small_layers_follow_the_model(R, n, g, cbn, moves, seed):
    W, H, S, Q0 = grouped_start(R, n, g, cbn, seed)
    Q, idx, trace, _ = device_search(W, Q0, S, codebook(cbn), H, g, moves)
    assert follows_model(W, Q0, S, cbn, H, g, moves, Q, trace) == 0 or n > 96  # 64 x 96: bit for bit


# ---------------------------------------------------------------------------------------------------------------- kernel forms
@pytest.mark.parametrize("n", [768, 1024, 1536, 2048, 3072, 4096, 6144, 8192])
def test_wave_and_general_kernels_agree(n, slkopt):
    R, g = 12, 128
    W, H, S, Q0 = grouped_start(R, n, g, "8", 7200 + n // 256, device_layer=n > 2048)
    for cbn in ("8", "nf4"):
        cb = codebook(cbn)
        slkopt.setenv("no_wave_search", 0)
        a = device_search(W, Q0, S, cb, H, g, 20)
        slkopt.setenv("no_wave_search", 1)
        b = device_search(W, Q0, S, cb, H, g, 20)
        for x, y in zip(a, b):
            assert np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8)), (n, cbn)
        assert (a[2][:, 0] >= 0).any()  # (the search moved)


@pytest.mark.parametrize("n,g", [(96, 3), (1000, 8), (5000, 1000), (11008, 128), (16384, 1)])
def test_ragged_lengths_follow_the_model(n, g):
    R = 6
    W, H, S, Q0 = grouped_start(R, n, g, "8", 7300 + n % 97, device_layer=n > 1000)
    if g == 1:  # (a scale of its own per weight leaves nothing to search: vary a row scale by column instead)
        S = (S.max(axis=1, keepdims=True) * (1 + (np.arange(n, dtype=np.float32) % 5) / 16)).astype(np.float32)
    Q, idx, trace, _ = device_search(W, Q0, S, codebook("8"), H, g, 12)
    follows_model(W, Q0, S, "8", H, g, 12, Q, trace)


# ---------------------------------------------------------------------------------------------------------------- codebooks
def test_wide_uniform_codebook_without_indices_and_nf4():
    W, H, S, Q0 = grouped_start(16, 1024, 64, "512", 7401)
    Q, idx, trace, _ = device_search(W, Q0, S, codebook("512"), H, 64, 15, want_idx=False)
    follows_model(W, Q0, S, "512", H, 64, 15, Q, trace)
    from sleekit_amd import groups

    with pytest.raises(ValueError):
        groups.local_search_grouped(W, Q0, S, codebook("512"), H, 64, 5, return_indices=True)
    W, H, S, Q0 = grouped_start(16, 3072, 128, "nf4", 7402, device_layer=True)
    Q, idx, trace, _ = device_search(W, Q0, S, codebook("nf4"), H, 128, 15)
    follows_model(W, Q0, S, "nf4", H, 128, 15, Q, trace)


# ---------------------------------------------------------------------------------------------------------------- consistency
def test_indices_errors_and_the_layer_path():
    from sleekit_amd import groups

    R, n, g, cbn = 64, 1024, 128, "8"
    cb = codebook(cbn)
    W, H, S, Q0 = grouped_start(R, n, g, cbn, 7501)
    errs = [obq_ref.row_errors(W.astype(np.float64), Q0.astype(np.float64), H.astype(np.float64)).mean()]
    for moves in (1, 10, 100):
        Q, idx = groups.local_search_grouped(W, Q0, S, cb, H, g, moves, return_indices=True)
        assert np.array_equal(bits(groups.dequantize_grouped(idx, S, cb, g)), bits(Q))
        _, _, _, carried = device_search(W, Q0, S, cb, H, g, moves)
        exact = obq_ref.row_errors(W.astype(np.float64), Q.astype(np.float64), H.astype(np.float64))
        # the carried error: the initial product's float32 roundings (at most n of the magnitude of its terms) and a few
        # per move, each of the magnitude of the terms behind a gain
        D0 = np.abs(W - Q0).astype(np.float64)
        terms = ((D0 @ np.abs(H).astype(np.float64)) * D0).sum(axis=1)
        assert (np.abs(carried - exact) <= 2.0 ** -24 * (n + 8 * moves) * terms).all(), moves
        errs.append(exact.mean())
    assert all(b <= a for a, b in zip(errs, errs[1:])), errs
    # the layer path: 0 moves is today's quantize_grouped; k moves is the loop then the search
    Wd, Sd, Hd = (torch.from_numpy(x).cuda() for x in (W, S, H))
    q0, i0 = groups.quantize_grouped(Wd, Sd, cb, Hd, g, "diag", 0.01, 32, 8, True)
    q1, i1 = groups.quantize_grouped(Wd, Sd, cb, Hd, g, return_indices=True, nb_ls_moves=0)
    assert np.array_equal(bits(q0), bits(q1)) and torch.equal(i0, i1)
    qk, ik = groups.quantize_grouped(Wd, Sd, cb, Hd, g, return_indices=True, nb_ls_moves=10)
    qs, is_ = groups.local_search_grouped(q0.new_tensor(W), q0, Sd, cb, Hd, g, 10, return_indices=True)
    assert np.array_equal(bits(qk), bits(qs)) and torch.equal(ik, is_)
    res = groups.quantize_layer_grouped(Wd, Sd, cb, Hd, g, nb_ls_moves=10, want_ls_trace=True)
    assert res.ls_trace.shape == (R, 10) and res.ls_error.shape == (R,)
    assert np.array_equal(bits(res.Q), bits(qk)) and torch.equal(res.idx, ik)
    assert groups.local_search_grouped(W, Q0, S, cb, H, g, 0) is Q0


def test_too_wide_is_refused_before_any_launch():
    from sleekit_amd import _lib

    buf = torch.zeros(16, device="cuda")
    p = buf.data_ptr()
    rc = _lib.lib.slk_local_search_grouped(p, p, p, p, 16512, 1, 16512, 8, -1.0, 1.0, None, 5, None, None, None, p, 64, None)
    assert rc != 0 and b"16384" in _lib.lib.slk_last_error()
    rc = _lib.lib.slk_local_search_grouped(p, p, p, p, 7, 1, 96, 8, -1.0, 1.0, None, 5, None, None, None, p, 64, None)
    assert rc != 0 and b"group_size" in _lib.lib.slk_last_error()


# ---------------------------------------------------------------------------------------------------------------- scale
def test_4096_layer_follows_the_model():
    R = n = 4096
    g, moves = 128, 100
    W, H, S, Q0 = grouped_start(R, n, g, "8", 7601, device_layer=True)
    Q, idx, trace, _ = device_search(W, Q0, S, codebook("8"), H, g, moves)
    rows = np.arange(0, R, 16)  # (rows are independent: the model follows a sample of 256 of them)
    follows_model(W, Q0, S, "8", H, g, moves, Q, trace, rows)
