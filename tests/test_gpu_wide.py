"""Layers wider than 16384 columns and factors past 4 GiB ("Width limits").

Two width boundaries switch paths:
  * past 16384 columns the loop leaves the standard-schedule window kernel (window2) for the general one, the permutes
    leave LDS (PERM_MAX) and the local search refuses;
  * past 4 GiB of one float64 factor (ld * ld * 8 > 2^32, ld >= 23232) the chain factorisation's 32-bit buffer offsets
    would wrap: those factorisations take the panel kernels.
Everything here is held to a float64 computation or to the reference (tests/golden/wide_cases.json), never only to
another form of the same kernel.  Inputs come from synth.make_layer_device (the host generator's bytes, in seconds);
the workspaces are released between widths so that the process stays well under 64 GB of device memory.
"""

import hashlib
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from oracle import grid, npsum, obq_ref, scaling_ref
from sleekit_amd import synth

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
BOUNDARY = (23168, 23232, 28672)  # ld * ld * 8 just under 2^32, just over, a 70B-class down-projection


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.fixture(scope="module")
def amd():
    assert torch.cuda.is_available(), "these tests need the GPU"
    from sleekit_amd import _device, _lib, codebook, engine, obq, scaling, statistics

    class NS:
        pass

    ns = NS()
    ns.dev, ns.lib, ns.codebook, ns.engine, ns.obq, ns.scaling, ns.statistics = _device, _lib, codebook, engine, obq, scaling, statistics
    yield ns
    _release(ns)
    print(f"\npeak device memory of test_gpu_wide: {torch.cuda.max_memory_reserved() / 2**30:.1f} GiB reserved")


def _release(amd):
    torch.cuda.synchronize()
    amd.dev.release_workspaces()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def wide_cases():
    with open(os.path.join(GOLDEN, "wide_cases.json")) as f:
        return json.load(f)["cases"]


def hessian(n, seed):
    """float32 device Hessian of the synthetic generator (T = 2 n tokens)."""
    return synth.make_layer_device(8, n, seed, DEV, keep=("H",))["H"]


def check_columns(H, order, U, damp=0.01, count=32):
    """max |U^T (U P[:, J]) - I[:, J]| in float64 for P = Hd[order][:, order] and 32 columns J spread over the factor:
    the first, middle and last 128 rows of outer blocks (512 columns) from first to last, and the last tile.  U^T U = P^-1
    is the factor's defining property; this check does not use any factorisation kernel."""
    n = H.shape[0]
    blocks = (n + 511) // 512
    J = []
    for b in np.linspace(0, blocks - 1, 10).round().astype(int):
        lo, hi = 512 * b, min(512 * (b + 1), n)
        J += [lo + 5, (lo + hi) // 2 + 17, hi - 3]
    J += [n - 64 + 11, n - 1]
    J = torch.tensor(sorted(set(J))[:count], dtype=torch.int64, device=DEV)
    d = H.diagonal().cpu().numpy()
    damp_value = float(damp * npsum.mean_f32(d))  # the damping the device applies (slk_diag_mean: NumPy's order)
    assert np.float32(npsum.mean_f32(d)) == d.mean()
    cols = H[order[:, None], order[J][None, :]].double()  # P[:, J] without the damping
    cols[J, torch.arange(len(J), device=DEV)] += damp_value
    Z = U.T @ (U @ cols)
    Z[J, torch.arange(len(J), device=DEV)] -= 1.0
    return float(Z.abs().max())


# --------------------------------------------------------------------------- factor at the 4 GiB boundary
@pytest.mark.parametrize("n", BOUNDARY)
def test_factor_past_4gib_is_the_panel_form_and_inverts(amd, n):
    """Default form (the chain up to 4 GiB of factor, the panel kernels past it) against panel_split = 1, bit for bit, and
    each against the float64 property U^T U P = I on 32 columns (bound of test_order_and_factor)."""
    H = hessian(n, 4400 + n % 97)
    o1, U1, i1 = amd.engine.factorize(H, n, 0.01, amd.lib.ORDER_DIAG)
    with amd.lib.option("panel_split", 1):
        o2, U2, i2 = amd.engine.factorize(H, n, 0.01, amd.lib.ORDER_DIAG)
    torch.cuda.synchronize()
    err1, err2 = check_columns(H, o1, U1), check_columns(H, o2, U2)
    same = torch.equal(o1, o2) and torch.equal(U1, U2)
    print(f"n={n}: status {int(i1.item())} / {int(i2.item())}, U equal: {same}, "
          f"max |U^T U P - I| on 32 columns: default {err1:.3g}, panel_split=1 {err2:.3g}")
    assert int(i2.item()) == 0 and err2 < 1e-8, (int(i2.item()), err2)
    assert int(i1.item()) == 0 and err1 < 1e-8 and same, (int(i1.item()), err1, same)
    del U1, U2
    _release(amd)


def test_factor_past_4gib_lookahead_and_batch(amd):
    """23232 columns (just past 4 GiB): the factor that looks ahead, and a batch of two, are the single call's bit for bit."""
    n = 23232
    Hs = [hessian(n, 4500), hessian(n, 4501)]
    alone = []
    for H in Hs:
        o, U, i = amd.engine.factorize(H, n, 0.01, amd.lib.ORDER_DIAG)
        torch.cuda.synchronize()
        assert int(i.item()) == 0
        alone.append((o, U))
    oa, Ua, ia = amd.engine.factorize(Hs[0], n, 0.01, amd.lib.ORDER_DIAG, lookahead=True)
    torch.cuda.synchronize()
    assert int(ia.item()) == 0 and torch.equal(oa, alone[0][0]) and torch.equal(Ua, alone[0][1])
    del oa, Ua
    _release(amd)
    ob, Ub, ib = amd.engine.factorize_batch(Hs, n, 0.01, amd.lib.ORDER_DIAG)
    torch.cuda.synchronize()
    assert int(ib.abs().sum().item()) == 0
    for b in range(2):
        assert torch.equal(ob[b], alone[b][0]) and torch.equal(Ub[b], alone[b][1]), b
    assert check_columns(Hs[1], ob[1], Ub[1]) < 1e-8
    del ob, Ub, alone
    _release(amd)


# --------------------------------------------------------------------------- whole layers against the reference
@pytest.mark.parametrize("case", range(3))
def test_wide_layers_against_reference_hashes(amd, wide_cases, case):
    """64 x 16512 (diag and sqerr: general window kernel, permutes in global memory, the column-miss keys) and 64 x 24576
    (a factor past 4 GiB) through quantize_with_scaling, against the hash of the real reference's indices.  The rules of
    test_gpu_parity._large: bit-exact, with the layer error within 1e-5 relative of the reference's; or, when the ordering
    key has exact ties (NumPy's argsort is unstable, the device sort stable), bit-exact against the oracle run with stable
    ties, with the layer error within 1e-5 relative of THAT run's.  (64 x 16512 diag has 8 tied keys: one row of 64 takes
    the other tied column first, which moves the layer's mean error by 1.07e-5 relative -- the reference's rows, not the
    device's error product, are what differ.)"""
    c = wide_cases[case]
    assert c["moves"] == 0 and not c["strip_mean"]
    L = synth.make_layer_device(c["R"], c["n"], c["seed"], DEV, T=c["T"])
    W, H, sc = (L[k].cpu().numpy() for k in ("W", "H", "scale"))
    assert sha(W) == c["sha_W"] and sha(H) == c["sha_H"] and sha(sc) == c["sha_scale"]
    cb = amd.codebook.UniformCodebook(c["levels"], -1, 1)
    out = amd.scaling.quantize_with_scaling(L["W"], L["scale"], cb, L["H"], c["order"], c["damp"], c["moves"])
    err = float(amd.obq.quantization_error(L["W"], out, L["H"]))
    out = out.cpu().numpy()
    idx = cb.quantize_index(amd.scaling.apply_scaling(out, sc, 0))
    del L
    _release(amd)
    if sha(idx) == c["sha_idx"]:
        assert abs(err - c["err"]) <= 1e-5 * abs(c["err"]), (err, c["err"])
        return
    Hd_diag = H.diagonal().astype(np.float64) + np.float64(np.float32(c["damp"]) * H.diagonal().mean())
    assert len(np.unique(Hd_diag)) < len(Hd_diag), "no ties and no local search: indices must match the reference bit for bit"
    g = grid.UniformGrid(c["levels"], -1, 1)
    want = scaling_ref.quantize_scaled(W, sc, g, H, c["order"], c["damp"], 0, ties="stable")
    bad_rows = int((idx != g.index(scaling_ref.divide_rows(want, sc, 0))).any(axis=1).sum())
    want_err = float(obq_ref.mean_error(W, want, H))
    assert abs(err - want_err) <= 1e-5 * abs(want_err), (err, want_err)
    assert bad_rows == 0, f"{bad_rows} rows differ from the oracle with stable tie-breaking"


# --------------------------------------------------------------------------- stages at 23232 and 28672 columns
@pytest.mark.parametrize("n", [23232, 28672])
def test_hessian_accumulate_wide(amd, n):
    """X^T X on the bfloat16 MFMA past 4 GiB of float64 H: a ragged token count, two batches (running mean) and a workspace
    that takes 32 tokens at a time, against float64 (the tolerance of test_hessian_accumulate_bf16_path)."""
    g = torch.Generator(device=DEV).manual_seed(n)
    scale = 0.5 + torch.rand(n, device=DEV, generator=g)
    X1 = (torch.randn((200, n), device=DEV, generator=g) * scale).float().contiguous()
    X2 = (torch.randn((75, n), device=DEV, generator=g) + 0.3).float().contiguous()
    ws, full = amd.dev.workspace(0, n)
    want_m = (X1.double().sum(0) + X2.double().sum(0)) / 275.0
    for ws_bytes in (full, 4096 + 6 * n * 40):
        H = torch.zeros((n, n), dtype=torch.float32, device=DEV)
        m = torch.zeros(n, dtype=torch.float32, device=DEV)
        count = 0
        for X in (X1, X2):
            amd.lib.check(amd.lib.lib.slk_hessian_accumulate(H.data_ptr(), m.data_ptr(), X.data_ptr(), n, X.shape[0], count,
                                                             ws.data_ptr(), ws_bytes, None))
            count += X.shape[0]
        torch.cuda.synchronize()
        assert torch.equal(H, H.T)
        # float64 in row strips of 2048 (a whole float64 H and its temporaries would be 30 GB at 28672 columns)
        excess, peak = [], 0.0
        for r0 in range(0, n, 2048):
            r1 = min(r0 + 2048, n)
            want = (X1[:, r0:r1].double().T @ X1.double() + X2[:, r0:r1].double().T @ X2.double()) / 275.0
            peak = max(peak, float(want.abs().max()))
            excess.append(((H[r0:r1].double() - want).abs() - 2e-5 * want.abs()).max().item())
        assert max(excess) <= 2e-6 * peak, (ws_bytes, max(excess), peak)
        assert torch.allclose(m.double(), want_m, rtol=1e-5, atol=1e-6)
        del H
    _release(amd)


@pytest.mark.parametrize("n", [23232, 28672])
def test_layer_error_wide(amd, n):
    """channelwise_error on the bfloat16 path (a symmetric H) past 4 GiB: every row within 1e-5 of float64."""
    g = torch.Generator(device=DEV).manual_seed(n + 1)
    R = 64
    W = torch.randn((R, n), device=DEV, generator=g)
    Q = (W + 0.2 * torch.randn((R, n), device=DEV, generator=g)).contiguous()
    X = torch.randn((256, n), device=DEV, generator=g)
    H = (X.T @ X) / 256.0 + torch.diag(torch.rand(n, device=DEV, generator=g))
    H = ((H + H.T) * 0.5).contiguous()
    del X
    assert torch.equal(H, H.T)
    got = amd.engine.row_errors(W, Q, H)
    D = (W - Q).double()
    want = ((D @ H.double()) * D).sum(dim=1)
    rel = ((got.double() - want).abs() / want.abs()).max()
    assert float(rel) <= 1e-5, float(rel)
    del H
    _release(amd)


@pytest.mark.parametrize("n", [23232, 28672])
def test_diag_mean_wide(amd, n):
    rng = np.random.default_rng(n)
    d = (np.square(rng.standard_normal(n)) * 3).astype(np.float32)
    H = torch.zeros((n, n), dtype=torch.float32, device=DEV)
    H.diagonal().copy_(torch.from_numpy(d))
    out = torch.empty(1, dtype=torch.float32, device=DEV)
    amd.lib.check(amd.lib.lib.slk_diag_mean(H.data_ptr(), n, out.data_ptr(), None, 0, None))
    assert np.float32(out.item()) == npsum.mean_f32(d) == d.mean()
    del H
    _release(amd)


@pytest.mark.parametrize("n", [23232, 28672])
def test_scale_search_wide(amd, n):
    """The per-row scale search on 8 rows of 23232 / 28672 columns: the NumPy-order oracle's sums and choices, bit for bit."""
    g = grid.UniformGrid(4, -1, 1)
    cb = amd.codebook.UniformCodebook(4, -1, 1)
    W = synth.make_weights(8, n, 4000 + n)
    hd = (np.abs(synth.normal_grid(4000 + n, 8, 1, n)[0]) * 3 + 0.1).astype(np.float32)
    assert np.array_equal(amd.scaling.compute_norm_scaling(W, 0), scaling_ref.norm_scale(W, 0))
    assert np.array_equal(amd.scaling.compute_non_saturating_scaling(W, cb, 0), scaling_ref.no_clip_scale(W, g, 0))
    assert np.array_equal(amd.scaling.compute_min_mse_scaling(W, cb, grid_size=30), scaling_ref.best_grid_scale(W, g, grid_size=30))
    assert np.array_equal(amd.scaling.compute_min_mse_scaling(W, cb, H=hd, grid_size=30),
                          scaling_ref.best_grid_scale(W, g, H=hd, grid_size=30))


@pytest.mark.parametrize("n", [16512, 24576])
def test_window_kernel_wide(amd, n):
    """Past 16384 columns only the general window kernel and the global-memory permutes serve: against the oracle's
    schedule on a synthetic U, 40 rows (a ragged last row tile)."""
    rng = np.random.default_rng(n)
    R = 40
    W = (rng.standard_normal((R, n)) * 0.6).astype(np.float32)
    U = np.triu(rng.standard_normal((n, n), dtype=np.float32).astype(np.float64) * (0.3 / np.sqrt(n)))
    U[np.diag_indices(n)] = 1.0 + rng.random(n)
    cb = amd.codebook.UniformCodebook(8, -1, 1)
    Q, E = W.copy(), np.zeros_like(W)
    amd.obq._quantize_opt_block(Q, E, U, cb, 32, 8)
    _release(amd)
    Q0, E0 = W.copy(), np.zeros_like(W)
    obq_ref.run_schedule(Q0, E0, U, grid.UniformGrid(8, -1, 1), obq_ref.block_schedule(n, 32, 8))
    assert np.array_equal(Q, Q0)
    np.testing.assert_allclose(E, E0, rtol=1e-6, atol=1e-7)


# --------------------------------------------------------------------------- refusals
def test_local_search_past_16384_columns_is_refused(amd):
    """The local search supports n <= 16384: a wider layer with moves is refused with the library's error, from
    engine.quantize_layer and from Sleekit.quantize alike, and the process goes on working."""
    n = 16512
    L = synth.make_layer_device(16, n, 4600, DEV)
    cb = amd.codebook.UniformCodebook(16, -1, 1)
    with pytest.raises(RuntimeError, match=r"n <= 16384"):
        amd.engine.quantize_layer(L["W"], L["H"], cb, L["scale"], "diag", 0.01, 4)
    layer = torch.nn.Linear(n, 16).to(DEV)
    sk = amd.statistics.Sleekit(layer)
    g = torch.Generator(device=DEV).manual_seed(5)
    sk.add_batch(torch.randn((300, n), device=DEV, generator=g))
    before = layer.weight.detach().clone()
    with pytest.raises(RuntimeError, match=r"n <= 16384"):
        sk.quantize(4, nb_ls_moves=3)
    torch.cuda.synchronize()
    # a refusal, not a crash: the layer is as it was, and the same layer without moves still quantizes
    assert torch.equal(layer.weight, before)
    res = sk.quantize(4, nb_ls_moves=0)
    torch.cuda.synchronize()
    assert res.Q.shape == (16, n) and bool(torch.isfinite(layer.weight).all())
    del L, sk, layer
    _release(amd)
