"""Asymmetric group quantization on the MI355X (sleekit_amd.groups with `offsets`) against the reference's own results
(tests/golden/groups_offsets.npz, made by tests/golden/make_golden_offsets.py), the NumPy model of
tests/groups_offsets_model.py and the symmetric grouped path already pinned.

Run on the GPU box:  python -m pytest tests/test_gpu_groups_offsets.py -m gpu -q
"""

import hashlib
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from groups_model import group_scales_model, oracle_grid
from groups_offsets_model import centred, midpoints, model_asym, rebuild, shaped_layer

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx():
    assert torch.cuda.is_available(), "these tests need the GPU"
    data = np.load(os.path.join(GOLDEN, "groups_offsets.npz"))
    return data, json.loads(str(data["meta"]))


def codebook(name):
    from sleekit_amd.codebook import Codebook, UniformCodebook

    return Codebook.nf4() if name == "nf4" else UniformCodebook(int(name), -1, 1)


def host(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(host(a)).tobytes()).hexdigest()


def bits(a):
    return np.ascontiguousarray(host(a), dtype=np.float32).view(np.uint32)


def device_case(W, H, cbn, g, act_order, mode, damp, mb, nb, **kw):
    """O, S, Q (and idx) of one layer, every step on the device."""
    from sleekit_amd import groups

    cb = codebook(cbn)
    O = groups.compute_group_offsets(W, g)
    S = groups.compute_group_scaling(W, cb, g, H, mode=mode, offsets=O)
    out = groups.quantize_grouped_asym(W, S, O, cb, H, g, act_order, damp, mb, nb, **kw)
    return (O, S) + (out if isinstance(out, tuple) else (out,))


def test_fixtures_bit_for_bit(fx):
    from sleekit_amd import groups

    data, meta = fx
    for i, c in enumerate(meta["cases"]):
        L = shaped_layer(c["R"], c["n"], c["g"], c["seed"], c["variant"])
        want = 256 >= len(codebook(c["codebook"]))
        O, S, Q, *rest = device_case(L["W"], L["H"], c["codebook"], c["g"], c["act_order"], c["mode"], c["damp"],
                                     c["min_block_size"], c["num_blocks"], return_indices=want)
        assert np.array_equal(bits(O), bits(data[f"O_{i}"])), f"case {i}: O {c}"
        assert np.array_equal(bits(S), bits(data[f"S_{i}"])), f"case {i}: S {c}"
        assert sha(Q) == c["sha256_Q"], f"case {i}: Q {c}"
        if want:
            idx = rest[0]
            back = groups.dequantize_grouped(idx, S, codebook(c["codebook"]), c["g"], offsets=O)
            assert np.array_equal(bits(back), bits(Q)), f"case {i}: dequantize"
            if f"idx_{i}" in data:
                assert np.array_equal(idx, data[f"idx_{i}"]), f"case {i}: idx"


def test_fixtures_on_device_tensors(fx):
    from sleekit_amd import groups

    data, meta = fx
    for i, c in enumerate(meta["cases"][:6]):
        L = shaped_layer(c["R"], c["n"], c["g"], c["seed"], c["variant"])
        W, H, S, O = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (L["W"], L["H"], data[f"S_{i}"], data[f"O_{i}"]))
        Q = groups.quantize_grouped_asym(W, S, O, codebook(c["codebook"]), H, c["g"], c["act_order"], c["damp"],
                                         c["min_block_size"], c["num_blocks"])
        assert isinstance(Q, torch.Tensor) and Q.is_cuda and sha(Q) == c["sha256_Q"], f"case {i}"


def test_large_layer_hashes(fx):
    from sleekit_amd import synth

    _, meta = fx
    c = meta["large"]
    L = synth.make_layer_device(c["R"], c["n"], c["seed"], "cuda")
    O, S, Q = device_case(L["W"], L["H"], c["codebook"], c["g"], c["act_order"], c["mode"], c["damp"], 32, 8)
    assert sha(O) == c["sha256_O"] and sha(S) == c["sha256_S"]
    assert sha(Q) == c["sha256_Q"]


FUZZ = [  # (R, n, g, codebook, act_order, mode, min_block_size, num_blocks)
    (48, 4096, 64, "8", "diag", "max", 32, 8),
    (40, 4096, 8, "4", "sqerr", "max", 32, 8),       # 512 groups: the leaves read S and O from memory
    (16, 4096, 2048, "16", "none", "mse", 32, 8),
    (21, 1376, 1, "8", "err", "max", 48, 4),         # g = 1
    (64, 2048, 128, "nf4", "inv_diag", "max", 32, 8),
    (19, 1200, 75, "8", "diag", "max", 600, 2),      # 600-column leaves: the window from memory
    (64, 768, 384, "256", "pivot", "max", 32, 8),
]


def fuzz_layer(R, n, seed, hessian=True):
    rng = np.random.default_rng(seed)
    W = rng.standard_normal((R, n)).astype(np.float32)
    W *= np.float32(10.0) ** rng.integers(-17, 10, (R, 1)).astype(np.float32)   # scales from ~5e-18 to 1e10
    W += rng.standard_normal((R, 1)).astype(np.float32) * np.abs(W).max(axis=1, keepdims=True)
    if not hessian:
        return np.ascontiguousarray(W), None
    X = rng.standard_normal((512, n)).astype(np.float32)
    H = (X.T.astype(np.float64) @ X / 512).astype(np.float32)  # rank 512: the damping makes it definite
    return np.ascontiguousarray(W), H


@pytest.mark.parametrize("case", range(len(FUZZ)))
def test_fuzz_against_the_model(case):
    from sleekit_amd import groups

    R, n, g, cbn, order, mode, mb, nb = FUZZ[case]
    W, H = fuzz_layer(R, n, 9100 + case)
    grd = oracle_grid(cbn)
    O = groups.compute_group_offsets(W, g)
    assert np.array_equal(bits(O), bits(midpoints(W, g)))
    S = groups.compute_group_scaling(W, codebook(cbn), g, H, mode=mode, offsets=O)
    assert np.array_equal(bits(S), bits(group_scales_model(centred(W, O, g), grd, H, g, mode)))
    Q, idx = groups.quantize_grouped_asym(W, S, O, codebook(cbn), H, g, order, 0.01, mb, nb, return_indices=True)
    want = model_asym(W, S, O, grd, H, g, order, 0.01, mb, nb, ties="stable")
    assert np.array_equal(bits(Q), bits(want))
    back = groups.dequantize_grouped(idx, S, codebook(cbn), g, offsets=O)
    assert np.array_equal(bits(back), bits(Q))
    if cbn != "nf4":
        assert np.array_equal(bits(rebuild(idx, S, O, cbn, g)), bits(Q))


@pytest.mark.parametrize("g", [1, 3, 64, 100, 8200])
def test_offsets_and_scale_kernels_at_every_group_size(g):
    from sleekit_amd import groups

    n = 16400 if g == 8200 else 4200 if g != 64 else 4096
    W, H = fuzz_layer(24, n, 9300 + g, hessian=g != 8200)
    O = groups.compute_group_offsets(W, g)
    assert np.array_equal(bits(O), bits(midpoints(W, g)))
    for mode in ("max", "mse", "diag") if H is not None else ("max", "mse"):
        S = groups.compute_group_scaling(W, codebook("8"), g, H, mode=mode, offsets=O)
        assert np.array_equal(bits(S), bits(group_scales_model(centred(W, O, g), oracle_grid("8"), H, g, mode))), mode


def test_zero_offsets_equal_the_symmetric_path(fx):
    from sleekit_amd import groups, synth

    for R, n, g, order in ((64, 512, 64, "sqerr"), (17, 1100, 55, "diag"), (33, 4096, 8, "err")):
        L = synth.make_layer(R, n, 9400 + g)
        cb = codebook("4")
        S = groups.compute_group_scaling(L["W"], cb, g, L["H"], mode="mse")
        Qs, ids = groups.quantize_grouped(L["W"], S, cb, L["H"], g, order, return_indices=True)
        Qa, ida = groups.quantize_grouped_asym(L["W"], S, np.zeros_like(S), cb, L["H"], g, order, return_indices=True)
        assert np.array_equal(Qs, Qa)  # values equal; only the sign of a zero may differ
        assert np.array_equal(ids, ida)


def test_batch_equals_separate_calls():
    from sleekit_amd import codebook as cbm
    from sleekit_amd import engine, groups, synth

    B, R, n, g = 3, 64, 512, 32
    cb = cbm.UniformCodebook(8, -1, 1)
    Ws, Ss, Os, orders, Us, singles = [], [], [], [], [], []
    for b in range(B):
        L = synth.make_layer(R, n, 9500 + b)
        W = torch.from_numpy(L["W"]).cuda()
        H = torch.from_numpy(L["H"]).cuda()
        O = groups.compute_group_offsets(W, g)
        S = groups.compute_group_scaling(W, cb, g, H, mode="mse", offsets=O)
        res = groups.quantize_layer_grouped(W, S, cb, H, g, "diag", offsets=O)
        Ws.append(W), Ss.append(S), Os.append(O), orders.append(res.order), Us.append(res.U), singles.append((res.Q, res.idx))
    U = torch.stack(Us).contiguous()
    Q, idx = groups.run_loop_batch_grouped(torch.stack(Ws).contiguous(), torch.stack(Ss).contiguous(), torch.stack(orders).contiguous(),
                                           U, engine.require_uniform(cb), g, 32, 8, offsets=torch.stack(Os).contiguous())
    for b in range(B):
        assert np.array_equal(bits(Q[b]), bits(singles[b][0])), b
        assert torch.equal(idx[b], singles[b][1]), b


def test_sleekit_quantize_with_offsets_equals_the_groups_path():
    import torch.nn as nn

    from sleekit_amd import Sleekit, groups, synth
    from sleekit_amd.codebook import UniformCodebook

    torch.manual_seed(0)
    lay = nn.Linear(256, 96).cuda()
    with torch.no_grad():
        lay.weight.copy_(torch.from_numpy(synth.make_layer(96, 256, 9601)["W"]) + 0.05)
    st = Sleekit(lay)
    for _ in range(3):
        st.add_batch(torch.randn(64, 256, device="cuda") + 0.3)
    W0 = lay.weight.detach().clone()
    b0 = lay.bias.detach().clone()
    res = st.quantize(3, group_size=64, offsets="mid", bias_correction=True, scaling_mode="diag", order_mode="sqerr")
    # the same steps through sleekit_amd.groups
    from sleekit_amd import _device as dev
    from sleekit_amd import _lib

    H = torch.empty_like(st.hessian)
    _lib.check(_lib.lib.slk_hessian_strip_mean(dev.ptr(st.hessian), dev.ptr(st.mean), 256, dev.ptr(H), dev.stream_handle()))
    cb = UniformCodebook(8, -1, 1)
    O = groups.compute_group_offsets(W0, 64)
    S = groups.compute_group_scaling(W0, cb, 64, H, mode="diag", offsets=O)
    Q, idx = groups.quantize_grouped_asym(W0, S, O, cb, H, 64, "sqerr", return_indices=True)
    assert torch.equal(lay.weight.data, Q)
    assert torch.equal(res.O, O) and torch.equal(res.S, S) and torch.equal(res.idx, idx)
    shift = ((W0 - Q) * st.mean).sum(dim=1)
    assert torch.equal(lay.bias.data, b0 + shift)
    assert torch.equal(groups.dequantize_grouped(res.idx, res.S, cb, 64, offsets=res.O), Q)


def test_refusals():
    import torch.nn as nn

    from sleekit_amd import Sleekit, groups, synth

    L = synth.make_layer(32, 128, 9701)
    cb = codebook("8")
    O = groups.compute_group_offsets(L["W"], 32)
    S = groups.compute_group_scaling(L["W"], cb, 32, L["H"], mode="max", offsets=O)
    with pytest.raises(NotImplementedError):
        groups.quantize_layer_grouped(torch.from_numpy(L["W"]).cuda(), torch.from_numpy(S).cuda(), cb, torch.from_numpy(L["H"]).cuda(),
                                      32, nb_ls_moves=5, offsets=O)
    with pytest.raises(ValueError):
        groups.quantize_grouped_asym(L["W"], S, O[:, :2], cb, L["H"], 32)
    with pytest.raises(ValueError):
        groups.dequantize_grouped(np.zeros((32, 128), np.uint8), S, cb, 32, offsets=O[:5])
    lay = nn.Linear(128, 32).cuda()
    st = Sleekit(lay)
    st.add_batch(torch.randn(16, 128, device="cuda"))
    with pytest.raises(ValueError):
        st.quantize(3, offsets="mid")
    with pytest.raises(NotImplementedError):
        st.quantize(3, group_size=32, offsets="mid", nb_ls_moves=5)
    with pytest.raises(NotImplementedError):
        st.quantize(3, group_size=32, offsets="mid", scaling_mode="obq")
    with pytest.raises(ValueError):
        st.quantize(3, group_size=32, offsets="low")


def test_centred_copy_of_the_midpoint_pass():
    """compute_group_offsets(centred=True): O and W - O from one pass, bit for bit NumPy's, at groups of 1 to 4100."""
    from sleekit_amd import groups

    for g, n in ((1, 300), (7, 700), (64, 4096), (100, 4200), (4100, 8200)):
        W, _ = fuzz_layer(19, n, 9800 + g, hessian=False)
        O, Wc = groups.compute_group_offsets(W, g, centred=True)
        assert np.array_equal(bits(O), bits(midpoints(W, g))), g
        assert np.array_equal(bits(Wc), bits(centred(W, midpoints(W, g), g))), g


# ---------------------------------------------------------------------------------------------------- the loop on a given factor
def synthetic_u(n, seed):
    """An upper-triangular float64 factor in processing order: small off-diagonal entries, a diagonal in [1, 2)."""
    rng = np.random.default_rng(seed)
    U = np.triu(rng.standard_normal((n, n), dtype=np.float32).astype(np.float64) * (0.3 / np.sqrt(n)))
    U[np.diag_indices(n)] = 1.0 + rng.random(n)
    return U


def given_factor_layer(R, n, g, seed):
    rng = np.random.default_rng(seed)
    W = (rng.standard_normal((R, n)) * 0.6 + rng.standard_normal((R, 1))).astype(np.float32)
    O = midpoints(W, g)
    S = rng.uniform(0.3, 1.0, (R, n // g)).astype(np.float32)
    return W, S, O, rng.permutation(n)


# (n, R, g, min_block, num_blocks): G = 384 and 385 on either side of the staged slots, groups past them with ragged last row
# tiles (the leaves read S and O from memory), leaves of 550 and 768 columns (the window from memory)
FACTOR_CASES = [
    (3072, 33, 8, 32, 8),     # G = 384: every group staged
    (3080, 33, 8, 32, 8),     # G = 385: the generic leaf from memory
    (3080, 1, 8, 48, 4),
    (1100, 17, 55, 640, 2),
    (768, 40, 1, 768, 1),
    (4096, 109, 2, 32, 8),
]


@pytest.mark.parametrize("case", FACTOR_CASES, ids=lambda c: "n{}-r{}-g{}-mb{}x{}".format(*c))
def test_loop_on_a_given_factor(case, slkopt):
    """quantize_layer_grouped(factor=..., offsets=O) against the model's schedule on the same factor, bit for bit, with the
    register leaf and with the generic leaf everywhere."""
    from sleekit_amd import groups

    n, R, g, mb, nb = case
    W, S, O, order = given_factor_layer(R, n, g, n * 3 + R)
    U = synthetic_u(n, n + g)
    want = model_asym(W, S, O, oracle_grid("8"), None, g, None, None, mb, nb, factor=(order, U))
    Wd, Sd, Od = (torch.from_numpy(x).cuda() for x in (W, S, O))
    od, Ud = torch.from_numpy(order.astype(np.int64)).cuda(), torch.from_numpy(U).cuda()
    info = torch.zeros(1, dtype=torch.int32, device="cuda")
    H = torch.zeros((1, 1), device="cuda").expand(n, n)  # only its shape is read with a given factor
    for generic in ("0", "1"):
        slkopt.setenv("SLK_NO_FAST_LEAF", generic)
        res = groups.quantize_layer_grouped(Wd, Sd, codebook("8"), H, g, "none", 0.01, mb, nb, factor=(od, Ud, info), offsets=Od)
        assert np.array_equal(bits(res.Q), bits(want)), (case, generic)
        back = groups.dequantize_grouped(res.idx, Sd, codebook("8"), g, offsets=Od)
        assert torch.equal(back.view(torch.int32), res.Q.view(torch.int32)), case
    slkopt.delenv("SLK_NO_FAST_LEAF")


def test_loop_wide():
    """Past 16384 columns: 16512 columns, 40 rows (a ragged last tile), g = 129 (129 groups, staged) and g = 16 (1032 groups,
    from memory), a random order, against the model's schedule on a synthetic factor."""
    from sleekit_amd import _device as dev
    from sleekit_amd import groups

    n, R = 16512, 40
    U = synthetic_u(n, 16514)
    Ud = torch.from_numpy(U).cuda()
    info = torch.zeros(1, dtype=torch.int32, device="cuda")
    H = torch.zeros((1, 1), device="cuda").expand(n, n)
    try:
        for g in (129, 16):
            W, S, O, order = given_factor_layer(R, n, g, 16512 + g)
            od = torch.from_numpy(order.astype(np.int64)).cuda()
            res = groups.quantize_layer_grouped(torch.from_numpy(W).cuda(), torch.from_numpy(S).cuda(), codebook("8"), H, g, "none",
                                                0.01, 32, 8, factor=(od, Ud, info), offsets=torch.from_numpy(O).cuda())
            Q, idx = bits(res.Q), host(res.idx)
            del res
            want = model_asym(W, S, O, oracle_grid("8"), None, g, None, None, 32, 8, factor=(order, U))
            assert np.array_equal(Q, bits(want)), (g, np.argwhere(Q != bits(want))[:5])
            assert np.array_equal(bits(rebuild(idx, S, O, "8", g)), Q), g
    finally:
        del Ud
        torch.cuda.synchronize()
        dev.release_workspaces()
        torch.cuda.empty_cache()


def _hip_runtime():
    """The HIP runtime this process already uses (the one libsleekit_amd.so resolved), for exact-size device buffers."""
    import ctypes

    with open("/proc/self/maps") as f:
        paths = [line.split()[-1] for line in f if "libamdhip64" in line]
    hip = ctypes.CDLL(paths[0])
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    hip.hipFree.argtypes = [ctypes.c_void_p]
    return hip


@pytest.mark.parametrize("R, n, g", [(1, 16384, 1), (17, 4096, 2)])
def test_ragged_rows_with_exact_size_scales_and_offsets(R, n, g):
    """R % 16 != 0 and more than 384 groups: the in-LDS window's padding rows past R read nothing of S and O.  S and O sit
    in hipMalloc buffers of exactly R * G floats (no allocator slack behind them) and go through the C entry point."""
    import ctypes

    from sleekit_amd import _device as dev
    from sleekit_amd import _lib, engine, groups

    W, S, O, order = given_factor_layer(R, n, g, 9900 + R)
    U = synthetic_u(n, 9901 + R)
    want = model_asym(W, S, O, oracle_grid("8"), None, g, None, None, 32, 8, factor=(order, U))
    hip = _hip_runtime()
    torch.cuda.synchronize()
    bufs = []
    try:
        for a in (S, O):
            p = ctypes.c_void_p()
            assert hip.hipMalloc(ctypes.byref(p), a.nbytes) == 0
            bufs.append(p)
            assert hip.hipMemcpy(p, a.ctypes.data, a.nbytes, 1) == 0  # host to device
        Wd = torch.from_numpy(W).cuda()
        od, Ud = torch.from_numpy(order.astype(np.int64)).cuda(), torch.from_numpy(U).cuda()
        levels, lo, hi, table = engine.require_uniform(codebook("8"))
        ws, ws_bytes = dev.workspace(R, n)
        Q = torch.empty((R, n), device="cuda")
        idx = torch.empty((R, n), dtype=torch.uint8, device="cuda")
        _lib.check(_lib.lib.slk_gptq_quantize_grouped_asym(dev.ptr(Wd), bufs[0].value, bufs[1].value, g, dev.ptr(od), dev.ptr(Ud), R, n,
                                                           levels, lo, hi, dev.ptr(table), 32, 8, 0, dev.ptr(Q), dev.ptr(idx), None,
                                                           dev.ptr(ws), ws_bytes, dev.stream_handle()))
        torch.cuda.synchronize()
    finally:
        for p in bufs:
            hip.hipFree(p)
    assert np.array_equal(bits(Q), bits(want))
    assert np.array_equal(bits(groups.dequantize_grouped(idx, S, codebook("8"), g, offsets=O)), bits(Q))
