"""Group-wise scales (sleekit_amd.groups) at the shapes where kernels break, against the NumPy model of tests/groups_model.py
(pinned to the reference by tests/test_groups_cpu.py) and against the reference's own edge cases (tests/golden/groups_edges.npz):
ragged row tiles, groups of 1 to 8200 columns that start inside a leaf or a 4-column load, widths that are not a multiple of
4, leaves of 1 to 768 columns, both leaf kernels, layers past 16384 columns, the per-group scale search at the boundaries of
NumPy's pairwise sum, the grouped column miss, and scales from 5e-18 to 1e10.

Run on the GPU box:  python -m pytest tests/test_gpu_groups_fuzz.py -m gpu -q
"""

import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from groups_model import GroupGrid, group_scales_model, indices, model_grouped
from oracle import grid, obq_ref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
ORDERS = ("none", "diag", "err", "sqerr", "pivot", "inv_diag", "combined_diag")


@pytest.fixture(scope="module")
def amd():
    assert torch.cuda.is_available(), "these tests need the GPU"
    from sleekit_amd import _device, _lib, codebook, engine, groups, synth

    class NS:
        pass

    ns = NS()
    ns.dev, ns.lib, ns.codebook, ns.engine, ns.groups, ns.synth = _device, _lib, codebook, engine, groups, synth
    torch.cuda.reset_peak_memory_stats()
    yield ns
    print(f"\npeak device memory of test_gpu_groups_fuzz: {torch.cuda.max_memory_reserved() / 2**30:.2f} GiB reserved")


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def host(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a


def codebooks(amd, name, levels=None, values=None):
    """(device codebook, oracle grid) of one codebook: uniform on [-1, 1], nf4, or a table of sorted values."""
    if name == "nf4":
        return amd.codebook.Codebook.nf4(), grid.TableGrid.nf4()
    if name == "table":
        return amd.codebook.Codebook(values), grid.TableGrid(values)
    return amd.codebook.UniformCodebook(levels, -1, 1), grid.UniformGrid(levels, -1, 1)


def describe(c):
    return {k: v for k, v in c.items() if not isinstance(v, np.ndarray)}


# ---------------------------------------------------------------------------------------------------- 1. the edge fixtures
@pytest.fixture(scope="module")
def edges():
    data = np.load(os.path.join(GOLDEN, "groups_edges.npz"))
    return data, json.loads(str(data["meta"]))


def edge_layer(amd, c):
    L = amd.synth.make_layer(c["R"], c["n"], c["seed"])
    if c["zero_group"] is not None:
        k, g = c["zero_group"], c["g"]
        L["W"][:, k * g:(k + 1) * g] = 0
    return L


def fixture_codebook(amd, name):
    return amd.codebook.Codebook.nf4() if name == "nf4" else amd.codebook.UniformCodebook(int(name), -1, 1)


def test_edge_fixtures_match_the_reference(amd, edges):
    """Every edge case through quantize_grouped on NumPy arrays and on device tensors: Q to the reference's SHA-256, the
    indices to the reference's where kept, dequantize_grouped back to Q bit for bit, and the device scale search to the
    reference's S."""
    import hashlib

    data, meta = edges
    for i, c in enumerate(meta["cases"]):
        L = edge_layer(amd, c)
        S = data[f"S_{i}"]
        cb = fixture_codebook(amd, c["codebook"])
        args = (c["g"], c["act_order"], c["damp"], c["min_block_size"], c["num_blocks"])
        Q, idx = amd.groups.quantize_grouped(L["W"], S, cb, L["H"], *args, return_indices=True)
        assert isinstance(Q, np.ndarray) and hashlib.sha256(Q.tobytes()).hexdigest() == c["sha256_Q"], f"case {i}: {c}"
        if f"idx_{i}" in data.files:
            assert np.array_equal(idx, data[f"idx_{i}"]), f"case {i}: indices"
        Wd, Hd, Sd = (torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in (L["W"], L["H"], S))
        Qd, idxd = amd.groups.quantize_grouped(Wd, Sd, cb, Hd, *args, return_indices=True)
        assert Qd.is_cuda and np.array_equal(bits(Qd), bits(Q)) and np.array_equal(host(idxd), idx), f"case {i}: device tensors"
        back = amd.groups.dequantize_grouped(idxd, Sd, cb, c["g"])
        assert np.array_equal(bits(back), bits(Q)), f"case {i}: dequantize"
        got_S = amd.groups.compute_group_scaling(L["W"], cb, c["g"], L["H"], c["mode"])
        assert np.array_equal(bits(got_S), bits(S)), f"case {i}: scales"


# ---------------------------------------------------------------------------------------------------- 2. random layers
def _divisors(n):
    return [d for d in range(1, n + 1) if n % d == 0]


def _case(seed):
    rng = np.random.default_rng(7100 + seed)
    R = int(rng.choice([1, 2, 3, 15, 16, 17, 31, 33, 48, 70]))
    n = int(rng.choice([1, 2, 5, 16, 31, 33, 47, 64, 65, 96, 100, 105, 130, 172, 200, 258, 300]))
    divs = _divisors(n)
    odd = [d for d in divs if d % 2 == 1 and d not in (1, n)]
    g = int(rng.choice([1, n] + 2 * odd + divs))  # 1, n and the odd divisors more often than the others
    T = 2 * n + 8
    X = rng.standard_normal((T, n)) * (0.5 + 2.0 * rng.random(n))
    X[:, : min(n, 3)] += rng.standard_normal((T, 1)) * 3.0
    H = (X.T @ X / T).astype(np.float32)
    H = ((H + H.T) * np.float32(0.5)).astype(np.float32)
    W = (rng.standard_normal((R, n)) * 0.05).astype(np.float32)
    kind = str(rng.choice(["uniform", "uniform", "table", "nf4"]))
    levels = int(rng.choice([2, 3, 4, 5, 8, 16, 17, 64, 255, 256])) if kind == "uniform" else int(rng.choice([2, 3, 5, 16, 37]))
    values = None
    if kind == "table":
        values = np.sort(rng.uniform(-1, 1, levels)).astype(np.float32)
        values[0], values[-1] = -1.0, 1.0
        if (np.diff(values) <= 0).any():
            values = np.linspace(-1, 1, levels).astype(np.float32)
    c = dict(seed=seed, R=R, n=n, g=g, W=W, H=H, kind=kind, levels=levels, values=values, act_order=str(rng.choice(ORDERS)),
             damp=float(rng.choice([0.01, 0.03, 0.1])), scales=str(rng.choice(["search", "random", "pow2", "zero"])),
             mode=str(rng.choice(["max", "mse", "diag"])), blocking=[(32, 8), (32, 8), (16, 4), (48, 4), (1, 2)][int(rng.integers(5))])
    c["zero"] = int(rng.integers(n // g)) if c["scales"] == "zero" else None
    return c, rng


def _scales(c, rng, grd):
    R, n, g, W, H = c["R"], c["n"], c["g"], c["W"], c["H"]
    G = n // g
    if c["scales"] == "random":
        return rng.uniform(0.005, 0.3, (R, G)).astype(np.float32)
    if c["scales"] == "pow2":
        return np.ldexp(np.float32(1), rng.integers(-9, -1, (R, G))).astype(np.float32)
    if c["scales"] == "zero":  # a group of zero weights: its scale is the search's floor, 1e-16 (max) or 5e-18 (searched)
        W[:, c["zero"] * g:(c["zero"] + 1) * g] = 0
    return group_scales_model(W, grd, H, g, c["mode"])


@pytest.mark.parametrize("seed", range(40))
def test_grouped_layer_against_model(amd, seed):
    """A random grouped layer through quantize_grouped (device factor and order) against the model with stable ties: Q bit
    for bit, the model's indices, and dequantize_grouped(idx, S) back to Q's bits."""
    c, rng = _case(seed)
    cb, grd = codebooks(amd, c["kind"], c["levels"], c["values"])
    S = _scales(c, rng, grd)
    mb, nb = c["blocking"]
    want = model_grouped(c["W"], S, grd, c["H"], c["g"], c["act_order"], c["damp"], mb, nb, ties="stable")
    Q, idx = amd.groups.quantize_grouped(c["W"], S, cb, c["H"], c["g"], c["act_order"], c["damp"], mb, nb, return_indices=True)
    case = describe(c)
    assert np.array_equal(bits(Q), bits(want)), (case, np.argwhere(bits(Q) != bits(want))[:5])
    assert np.array_equal(idx, indices(want, S, grd, c["g"])), case
    back = amd.groups.dequantize_grouped(idx, S, cb, c["g"])
    assert np.array_equal(bits(back), bits(Q)), case


# ---------------------------------------------------------------------------------------------------- 3. a given factor
def _synthetic_u(n, seed, odd_diagonal):
    """An upper-triangular float64 factor in processing order (as test_window_kernels_agree): small off-diagonal entries,
    a diagonal in [1, 2); odd_diagonal: one entry 1.111...1b, which defeats the leaf's exact-division shortcut."""
    rng = np.random.default_rng(seed)
    U = np.triu(rng.standard_normal((n, n), dtype=np.float32).astype(np.float64) * (0.3 / np.sqrt(n)))
    U[np.diag_indices(n)] = 1.0 + rng.random(n)
    if odd_diagonal:
        U[n // 3, n // 3] = np.nextafter(2.0, 0.0)
    return U


def unused_hessian(n):
    """An (n, n) stand-in for H where the factor is given (quantize_layer_grouped then reads only its shape)."""
    return torch.zeros((1, 1), device=DEV).expand(n, n)


def _loop(amd, W, S, g, order, U, cb_abi, mb, nb):
    """One raw call of slk_gptq_quantize_grouped with E_out (errors in processing order)."""
    R, n = W.shape
    levels, lo, hi, table = cb_abi
    ws, ws_bytes = amd.dev.workspace(R, n)
    Q = torch.full((R, n), float("nan"), device=DEV)
    idx = torch.full((R, n), 255, dtype=torch.uint8, device=DEV)
    E = torch.full((R, n), float("nan"), device=DEV)
    p = amd.dev.ptr
    amd.lib.check(amd.lib.lib.slk_gptq_quantize_grouped(p(W), p(S), g, p(order), p(U), R, n, levels, lo, hi, p(table), mb, nb, 0,
                                                        p(Q), p(idx), p(E), p(ws), ws_bytes, amd.dev.stream_handle()))
    return Q, idx, E


# (n, R, g, odd diagonal, min_block, num_blocks, order): g a multiple of 16 and not; leaves of 32, 33-48 and 550-768 columns
# (global-memory window); 109 rows leave a ragged last tile of 13, 17 and 40 of 1 and 8.
FACTOR_CASES = [
    (96, 17, 3, False, 32, 8, "identity"),
    (96, 40, 32, True, 48, 4, "random"),
    (768, 109, 48, True, 32, 8, "random"),
    (768, 40, 12, False, 768, 1, "identity"),
    (1024, 109, 8, True, 32, 8, "random"),
    (1024, 17, 128, False, 48, 4, "identity"),
    (1100, 40, 55, True, 640, 2, "random"),
    (1100, 17, 100, False, 32, 8, "identity"),
    (1376, 109, 43, False, 48, 4, "random"),
    (1376, 40, 32, True, 32, 8, "random"),
    (3072, 40, 96, True, 32, 8, "random"),
    (3072, 17, 3, False, 48, 4, "identity"),
    (4096, 109, 128, True, 32, 8, "random"),
    (4096, 17, 8, False, 48, 4, "random"),
]


@pytest.mark.parametrize("case", FACTOR_CASES, ids=lambda c: "n{}-r{}-g{}-{}-mb{}x{}-{}".format(c[0], c[1], c[2], "odd" if c[3] else "plain",
                                                                                                  c[4], c[5], c[6]))
def test_grouped_loop_on_a_given_factor(amd, case, slkopt):
    """The grouped loop on a synthetic factor, through quantize_layer_grouped(factor=...) and the raw entry with E_out:
    Q equal to obq_ref.run_schedule with GroupGrid bit for bit, E to rtol 1e-6, idx the model's; then the same calls with
    the register leaf switched off (SLK_NO_FAST_LEAF: the generic leaf everywhere) give identical bits."""
    n, R, g, odd, mb, nb, order_kind = case
    rng = np.random.default_rng(n * 7 + R)
    W = (rng.standard_normal((R, n)) * 0.6).astype(np.float32)
    S = rng.uniform(0.8, 2.0, (R, n // g)).astype(np.float32)  # W / s mostly inside the codebook's range
    order = np.arange(n) if order_kind == "identity" else rng.permutation(n)
    U = _synthetic_u(n, n + R, odd)
    cb, grd = codebooks(amd, "uniform", 8)
    cb_abi = amd.engine.require_uniform(cb)
    Q0 = W[:, order].copy()
    E0 = np.zeros_like(Q0)
    Z = GroupGrid(grd, S, g, order)
    obq_ref.run_schedule(Q0, E0, U, Z, obq_ref.block_schedule(n, mb, nb))
    assert Z.i == n
    want = Q0[:, np.argsort(order)]
    Wd, Sd = torch.from_numpy(W).to(DEV), torch.from_numpy(S).to(DEV)
    od, Ud = torch.from_numpy(order.astype(np.int64)).to(DEV), torch.from_numpy(U).to(DEV)
    info = torch.zeros(1, dtype=torch.int32, device=DEV)
    runs = []
    for generic in (False, True):
        slkopt.setenv("SLK_NO_FAST_LEAF", "1" if generic else "0")
        res = amd.groups.quantize_layer_grouped(Wd, Sd, cb, unused_hessian(n), g, "none", 0.01, mb, nb, factor=(od, Ud, info))
        Q, idx, E = _loop(amd, Wd, Sd, g, od, Ud, cb_abi, mb, nb)
        torch.cuda.synchronize()
        runs.append((bits(res.Q), host(res.idx), bits(Q), host(idx), bits(E)))
    slkopt.delenv("SLK_NO_FAST_LEAF")
    q_res, i_res, q_raw, i_raw, e_raw = runs[0]
    assert np.array_equal(q_res, bits(want)), (case, np.argwhere(q_res != bits(want))[:5])
    assert np.array_equal(q_raw, q_res) and np.array_equal(i_raw, i_res), case
    assert np.array_equal(i_res, indices(want, S, grd, g)), case
    np.testing.assert_allclose(e_raw.view(np.float32), E0, rtol=1e-6, atol=1e-7, err_msg=str(case))
    for a, b in zip(runs[0], runs[1]):
        assert np.array_equal(a, b), (case, "generic leaf")


def test_grouped_loop_wide(amd):
    """Past 16384 columns (general window kernel, global-memory permutes) with group scales: 16512 columns, 40 rows (a
    ragged last row tile), g = 128 and g = 129 (groups that start inside leaves and 4-column loads), a random order, against
    the oracle's schedule on a synthetic factor."""
    n, R = 16512, 40
    rng = np.random.default_rng(16512)
    W = (rng.standard_normal((R, n)) * 0.6).astype(np.float32)
    U = _synthetic_u(n, 16513, False)
    order = rng.permutation(n)
    cb, grd = codebooks(amd, "uniform", 8)
    Wd, od = torch.from_numpy(W).to(DEV), torch.from_numpy(order.astype(np.int64)).to(DEV)
    Ud = torch.from_numpy(U).to(DEV)
    info = torch.zeros(1, dtype=torch.int32, device=DEV)
    try:
        for g in (128, 129):
            S = rng.uniform(0.8, 2.0, (R, n // g)).astype(np.float32)  # W / s mostly inside the codebook's range
            res = amd.groups.quantize_layer_grouped(Wd, torch.from_numpy(S).to(DEV), cb, unused_hessian(n), g, "none", 0.01, 32, 8,
                                                    factor=(od, Ud, info))
            Q, idx = bits(res.Q), host(res.idx)
            del res
            want = model_grouped(W, S, grd, None, g, None, None, 32, 8, factor=(order, U))
            assert np.array_equal(Q, bits(want)), (g, np.argwhere(Q != bits(want))[:5])
            assert np.array_equal(idx, indices(want, S, grd, g)), g
    finally:
        del Ud
        torch.cuda.synchronize()
        amd.dev.release_workspaces()
        torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------- 4. the scale search
SEARCH_CASES = [  # (g, groups per row, R)
    (1, 3, 17), (2, 2, 33), (7, 3, 1), (8, 1, 17), (9, 2, 33), (16, 3, 1), (100, 2, 17), (127, 3, 33), (128, 1, 1),
    (129, 2, 17), (1100, 3, 1), (8200, 2, 17),
]


@pytest.mark.parametrize("case", SEARCH_CASES, ids=lambda c: "g{}-G{}-r{}".format(*c))
def test_group_scale_search_edges(amd, case):
    """compute_group_scaling in modes max, mse, diag, diag3, and with grid_size=30 and min_factor=0.2, against pick_scale per
    group bit for bit: group lengths below 8, off a multiple of 8 and past NumPy's 8192-element chunk; a zero group (the
    1e-16 floor), a group of equal weights, and a Hessian with a zero diagonal entry inside a group."""
    g, G, R = case
    n = g * G
    rng = np.random.default_rng(g * 31 + G)
    W = (rng.standard_normal((R, n)) * 0.05).astype(np.float32)
    W[:, :g] = 0  # group 0 of every row: zero weights
    if G > 1:
        W[:, g:2 * g] = np.float32(0.03)  # group 1: equal weights
    else:
        W[0] = 0
    d = (0.5 + rng.random(n)).astype(np.float32)
    d[min(n - 1, g + g // 2)] = 0  # a zero diagonal entry inside a group
    H = np.diag(d).astype(np.float32)
    for cb_name, levels in (("uniform", 8), ("uniform", 3), ("nf4", None)):
        cb, grd = codebooks(amd, cb_name, levels)
        for mode, kw in (("max", {}), ("mse", {}), ("diag", {}), ("diag3", {}), ("mse", dict(grid_size=30)),
                         ("diag", dict(min_factor=0.2))):
            want = group_scales_model(W, grd, H, g, mode, **kw)
            got = amd.groups.compute_group_scaling(W, cb, g, H, mode, **kw)
            assert np.array_equal(bits(got), bits(want)), (case, cb_name, levels, mode, kw, np.argwhere(bits(got) != bits(want))[:5])


# ---------------------------------------------------------------------------------------------------- 5. the column miss
@pytest.mark.parametrize("R", [1, 255, 256, 257, 600])
def test_column_miss_grouped_edges(amd, R):
    """err / sqerr keys from the grouped miss kernel against NumPy float32 column sums of |Z(W) - W| (or its square) added
    row after row, bit for bit: a 256-row pass that turns over, widths off a multiple of 4 (scalar loads), odd groups that
    start inside a 4-column load, and a W one float off 16-byte alignment."""
    rng = np.random.default_rng(R)
    for n, g in ((5, 5), (5, 1), (33, 3), (33, 11), (1100, 55), (1100, 275)):
        W = (rng.standard_normal((R, n)) * 0.05).astype(np.float32)
        S = rng.uniform(0.01, 0.1, (R, n // g)).astype(np.float32)
        for cb_name, levels in (("uniform", 8), ("nf4", None)):
            cb, grd = codebooks(amd, cb_name, levels)
            cb_abi = amd.engine.require_uniform(cb)
            D = GroupGrid(grd, S, g, None)(W) - W
            Sd = torch.from_numpy(S).to(DEV)
            buf = torch.zeros(R * n + 1, device=DEV)
            for aligned in (True, False):
                Wd = buf[:R * n].view(R, n) if aligned else buf[1:].view(R, n)
                Wd.copy_(torch.from_numpy(W))
                for squared in (False, True):
                    terms = np.square(D) if squared else np.abs(D)
                    want = np.zeros(n, np.float32)
                    for r in range(R):
                        want += terms[r]
                    got = amd.groups.column_miss_grouped(Wd, Sd, g, cb_abi, squared)
                    case = (R, n, g, cb_name, aligned, squared)
                    assert np.array_equal(bits(got), bits(want)), (case, np.argwhere(bits(got) != bits(want))[:5])


# ---------------------------------------------------------------------------------------------------- 6. extreme scales
@pytest.mark.parametrize("value", [5e-18, 1e-16, 2.0 ** -60, 2.0 ** 40, 1e10], ids=lambda v: f"{v:g}")
def test_indices_at_extreme_scales(amd, value):
    """Every scale set to one value, from the smallest the search makes (5e-18, a zero group) through what a caller may pass
    to Sleekit.quantize(scale=...) to large ones: Q against the model, the indices the model's, and the indices back to Q's
    bits (k_permute_out_grouped's claim that they come back exactly)."""
    L = amd.synth.make_layer(33, 172, 7300)
    g = 43
    S = np.full((33, 172 // g), np.float32(value), np.float32)
    for name, levels in (("uniform", 8), ("uniform", 3), ("uniform", 256), ("nf4", None)):
        cb, grd = codebooks(amd, name, levels)
        for act_order in ("diag", "sqerr"):
            want = model_grouped(L["W"], S, grd, L["H"], g, act_order, 0.01, 32, 8, ties="stable")
            Q, idx = amd.groups.quantize_grouped(L["W"], S, cb, L["H"], g, act_order, 0.01, return_indices=True)
            case = (value, name, levels, act_order)
            assert np.array_equal(bits(Q), bits(want)), (case, np.argwhere(bits(Q) != bits(want))[:5])
            assert np.array_equal(idx, indices(want, S, grd, g)), case
            back = amd.groups.dequantize_grouped(idx, S, cb, g)
            assert np.array_equal(bits(back), bits(Q)), case
