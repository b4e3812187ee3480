"""Group scales over a batch of layers (slk_gptq_quantize_grouped_batch) and through the layer stream of sleekit_amd.dist,
on the MI355X: the batch entry against single grouped calls and against the reference's own grouped results
(tests/golden/groups.npz), the stream's local, stacked and row-shard routes against sleekit_amd.groups one layer at a time,
two ranks on one GPU, and a factorisation failure inside a batched round.

Run on the GPU box:  python -m pytest tests/test_gpu_groups_batch.py -m gpu -q
"""

import hashlib
import json
import os
import socket

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from sleekit_amd import synth

pytestmark = pytest.mark.gpu


def codebook(name):
    from sleekit_amd.codebook import Codebook, UniformCodebook

    return Codebook.nf4() if name == "nf4" else UniformCodebook(int(name), -1, 1)


def sha(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def group_scales(W, g):
    """Positive (R, n / g) float32 scales, a function of W alone (the same in every process): max |w| of the group, floored."""
    R, n = W.shape
    return (W.abs().reshape(R, n // g, g).amax(dim=2) + 0.05).contiguous()


def layer(R, n, seed, g=None, kind="group", dev=None):
    """A synthetic layer dict on `dev`: kind "group" (gscale / group_size), "row" (scale) or "unscaled"."""
    dev = dev or torch.device("cuda", 0)
    if R * n >= 1 << 22:
        L = synth.make_layer_device(R, n, seed, dev, keep=("W", "H", "scale"))
    else:
        made = synth.make_layer(R, n, seed, device=dev if n >= 1024 else None)  # (wide Hessians: their products on the GPU)
        L = {k: torch.from_numpy(made[k]).to(dev) for k in ("W", "H", "scale")}
    lay = dict(W=L["W"], H=L["H"])
    if kind == "group":
        lay["gscale"], lay["group_size"] = group_scales(L["W"], g), g
    elif kind == "row":
        lay["scale"] = L["scale"]
    return lay


# ---------------------------------------------------------------------------------------------------- 1. the batch entry
def _loop(W, S, g, order, U, B, rpl, n, cb_abi, min_block, num_blocks):
    """One raw call of the grouped loop (batched when B > 1, the single-layer entry otherwise), with E_out."""
    from sleekit_amd import _device as sdev
    from sleekit_amd import _lib

    levels, lo, hi, table = cb_abi
    ws, ws_bytes = sdev.workspace(rpl, n, batch=B, grouped=True)
    Q = torch.full((B * rpl, n), float("nan"), device=W.device)
    idx = torch.full((B * rpl, n), 255, dtype=torch.uint8, device=W.device)
    E = torch.full((B * rpl, n), float("nan"), device=W.device)
    p = sdev.ptr
    if B == 1:
        code = _lib.lib.slk_gptq_quantize_grouped(p(W), p(S), g, p(order), p(U), rpl, n, levels, lo, hi, p(table), min_block, num_blocks,
                                                  0, p(Q), p(idx), p(E), p(ws), ws_bytes, sdev.stream_handle())
    else:
        code = _lib.lib.slk_gptq_quantize_grouped_batch(p(W), p(S), g, p(order), p(U), B, rpl, n, levels, lo, hi, p(table), min_block,
                                                        num_blocks, 0, p(Q), p(idx), p(E), p(ws), ws_bytes, sdev.stream_handle())
    _lib.check(code)
    return Q, idx, E


def _factor(W, S, g, H, cb, act_order, damp=0.01):
    from sleekit_amd import engine, groups

    miss = groups.grouped_keys(W, S, g, engine.require_uniform(cb), act_order, H, damp)
    order, U, info = engine.factorize(H, H.shape[0], damp, engine.order_mode_code(act_order), miss)
    assert int(info.item()) == 0
    return order, U


# (batch, rows per layer, n, g, codebook, act_order, min_block, num_blocks).  Leaves wider than 512 columns run on global
# memory in a kernel of their own (k_gptq_wide_leaf): 768 columns in one leaf, and 550-column leaves of 1100.
BATCH_CASES = [
    (2, 64, 128, 32, "8", "none", 32, 8),
    (5, 320, 128, 128, "nf4", "diag", 32, 8),
    (8, 64, 128, 128, "8", "pivot", 16, 4),
    (8, 64, 768, 128, "8", "sqerr", 32, 8),
    (2, 320, 768, 768, "nf4", "pivot", 32, 8),
    (5, 64, 768, 32, "8", "diag", 768, 1),
    (8, 320, 1100, 1100, "8", "diag", 32, 8),
    (2, 64, 1100, 100, "nf4", "sqerr", 640, 2),
    (5, 64, 1100, 1100, "8", "none", 640, 2),
    (5, 64, 3072, 128, "8", "pivot", 32, 8),
    (2, 320, 3072, 32, "nf4", "none", 32, 8),
    (8, 64, 3072, 3072, "8", "sqerr", 32, 8),
    (2, 64, 3072, 128, "nf4", "diag", 32, 8),
]


@pytest.mark.parametrize("case", BATCH_CASES, ids=lambda c: "B{}-r{}-n{}-g{}-{}-{}-mb{}".format(*c[:7]))
def test_batch_equals_single_calls(case):
    from sleekit_amd import engine

    B, rpl, n, g, cb_name, act_order, mb, nb = case
    cb = codebook(cb_name)
    cb_abi = engine.require_uniform(cb)
    lays = [layer(rpl, n, 7000 + 31 * n + b, g) for b in range(B)]
    facs = [_factor(l["W"], l["gscale"], g, l["H"], cb, act_order) for l in lays]
    singles = [_loop(l["W"], l["gscale"], g, f[0], f[1], 1, rpl, n, cb_abi, mb, nb) for l, f in zip(lays, facs)]
    W = torch.stack([l["W"] for l in lays]).contiguous()
    S = torch.stack([l["gscale"] for l in lays]).contiguous()
    order = torch.stack([f[0] for f in facs]).contiguous()
    U = torch.stack([f[1] for f in facs]).contiguous()
    Q, idx, E = _loop(W, S, g, order, U, B, rpl, n, cb_abi, mb, nb)
    for b, (q1, i1, e1) in enumerate(singles):
        rows = slice(b * rpl, (b + 1) * rpl)
        assert torch.equal(Q[rows].view(torch.int32), q1.view(torch.int32)), (case, b)
        assert torch.equal(idx[rows], i1), (case, b)
        assert torch.equal(E[rows].view(torch.int32), e1.view(torch.int32)), (case, b)
    # and the Python wrapper, shaped (B, R, n)
    from sleekit_amd import groups

    Qw, iw = groups.run_loop_batch_grouped(W.view(B, rpl, n), S.view(B, rpl, n // g), order, U, cb_abi, g, mb, nb)
    assert torch.equal(Qw.view(B * rpl, n), Q) and torch.equal(iw.view(B * rpl, n), idx)


# ---------------------------------------------------------------------------------------------------- 2. the reference
def test_batch_middle_layer_matches_the_reference():
    """Every small case of groups.npz in the middle of a batch of three same-shaped layers (rows padded to a multiple of 64
    with zero weights and unit scales): its rows of Q hit the reference's SHA-256, its indices equal the reference's."""
    from sleekit_amd import engine, groups

    data = np.load(os.path.join(GOLDEN, "groups.npz"))
    meta = json.loads(str(data["meta"]))
    dev = torch.device("cuda", 0)
    for i, c in enumerate(meta["cases"]):
        R, n, g = c["R"], c["n"], c["g"]
        cb = codebook(c["codebook"])
        cb_abi = engine.require_uniform(cb)
        rpl = (R + 63) // 64 * 64
        Ws, Ss, orders, Us = [], [], [], []
        for b in range(3):
            if b == 1:
                L = synth.make_layer(R, n, c["seed"])
                W, H, S = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (L["W"], L["H"], data[f"S_{i}"]))
            else:
                L = synth.make_layer(R, n, 9000 + 3 * i + b)
                W, H = torch.from_numpy(L["W"]).to(dev), torch.from_numpy(L["H"]).to(dev)
                S = group_scales(W, g)
            order, U = _factor(W, S, g, H, cb, c["act_order"], c["damp"])
            Ws.append(torch.cat([W, torch.zeros(rpl - R, n, device=dev)]))
            Ss.append(torch.cat([S, torch.ones(rpl - R, n // g, device=dev)]))
            orders.append(order)
            Us.append(U)
        Q, idx = groups.run_loop_batch_grouped(torch.stack(Ws), torch.stack(Ss), torch.stack(orders), torch.stack(Us), cb_abi, g,
                                               c["min_block_size"], c["num_blocks"])
        assert sha(Q[1, :R]) == c["sha256_Q"], f"case {i}: {c}"
        if f"idx_{i}" in data.files:
            assert np.array_equal(idx[1, :R].cpu().numpy(), data[f"idx_{i}"]), f"case {i}: {c}"


# ---------------------------------------------------------------------------------------------------- 3. the stream, one rank
def _alone(lay, cb, act_order="diag"):
    """What the layer gives one by one: sleekit_amd.groups for grouped layers, engine.quantize_layer for the others."""
    from sleekit_amd import engine, groups

    if lay.get("gscale") is not None:
        res = groups.quantize_layer_grouped(lay["W"], lay["gscale"], cb, lay["H"], lay["group_size"], act_order)
    else:
        res = engine.quantize_layer(lay["W"], lay["H"], cb, lay.get("scale"), act_order)
    return res.Q, res.idx, engine.row_errors(lay["W"], res.Q, lay["H"])


def _model_order_stream():
    spec = [((256, 256), 64)] * 3 + [((256, 256), 128)] * 2 + [((256, 256), "row")] * 2 + [((256, 256), "unscaled")] + \
           [((100, 384), 128)] * 3 + [((1100, 1600), 64)] * 3 + [((1100, 1600), "row")] * 2 + [((4096, 4096), 128)]
    order = list(range(0, len(spec), 3)) + list(range(1, len(spec), 3)) + list(range(2, len(spec), 3))  # shapes interleaved
    out = []
    for i in order:
        (R, n), kind = spec[i]
        if isinstance(kind, int):
            out.append(layer(R, n, 7400 + i, kind))
        else:
            out.append(layer(R, n, 7400 + i, kind=kind))
    return out


def test_stream_on_one_rank_matches_one_by_one():
    from sleekit_amd import codebook as cbm
    from sleekit_amd import dist as sdist

    cb = cbm.UniformCodebook(8, -1, 1)
    layers = _model_order_stream()
    be = sdist.HipBackend(cb, "diag", 0.01, 0, with_error=True)
    calls = {"local": [], "stacked": []}
    run_local, run_stacked = be.run_round_local, be.run_round_stacked
    be.run_round_local = lambda m: (calls["local"].append([sdist._layer_kind(x) for x in m]), run_local(m))[1]
    be.run_round_stacked = lambda m, f: (calls["stacked"].append([sdist._layer_kind(x) for x in m]), run_stacked(m, f))[1]
    shards = sdist.quantize_stream(layers, be)
    torch.cuda.synchronize()
    # local rounds: 256 x 256 with g = 64 (3), g = 128 (2), per-row (2); 100 x 384 with g = 128 (3, ragged: padded to 128 rows).
    # The lone unscaled 256 x 256 layer goes alone.  Stacked: 1100 x 1600 with g = 64 (3) and per-row (2).
    assert sorted(map(str, calls["local"])) == sorted(map(str, [[("group", 64)] * 3, [("group", 128)] * 2, ["row"] * 2,
                                                                  [("group", 128)] * 3]))
    assert sorted(map(str, calls["stacked"])) == sorted(map(str, [[("group", 64)] * 3, ["row"] * 2]))
    for l, (lay, sh) in enumerate(zip(layers, shards)):
        Q, idx, err = _alone(lay, cb)
        assert torch.equal(sh["Q"], Q) and torch.equal(sh["idx"], idx) and int(sh["info"].item()) == 0, l
        assert sh["rows"] == (0, lay["W"].shape[0])
        np.testing.assert_allclose(sh["row_err"].cpu().numpy(), err.cpu().numpy(), rtol=1e-5)
        if lay.get("gscale") is not None:  # idx is the codebook index of Q / s
            from sleekit_amd import groups

            assert torch.equal(groups.dequantize_grouped(sh["idx"], lay["gscale"], cb, lay["group_size"]), sh["Q"])
    plain = sdist.quantize_stream(layers, sdist.HipBackend(cb, "diag", 0.01, 0, with_error=True, overlap=False))
    torch.cuda.synchronize()
    for a, b in zip(shards, plain):
        assert torch.equal(a["Q"], b["Q"]) and torch.equal(a["idx"], b["idx"]) and torch.equal(a["row_err"], b["row_err"])


# ---------------------------------------------------------------------------------------------------- 4. err / sqerr keys
@pytest.mark.parametrize("act_order", ["sqerr", "err"])
def test_stream_orders_from_the_grouped_miss(act_order):
    from sleekit_amd import codebook as cbm
    from sleekit_amd import dist as sdist

    cb = cbm.UniformCodebook(4, -1, 1)
    layers = [layer(256, 512, 7600, 128), layer(130, 768, 7601, 64), layer(256, 512, 7602, 32)]
    shards = sdist.quantize_stream(layers, sdist.HipBackend(cb, act_order, 0.01, 0, with_error=True))
    torch.cuda.synchronize()
    for lay, sh in zip(layers, shards):
        Q, idx, err = _alone(lay, cb, act_order)
        assert torch.equal(sh["Q"], Q) and torch.equal(sh["idx"], idx) and int(sh["info"].item()) == 0
        np.testing.assert_allclose(sh["row_err"].cpu().numpy(), err.cpu().numpy(), rtol=1e-5)


# ---------------------------------------------------------------------------------------------------- 5. two ranks
def _rank_layers(dev):
    spec = [(97, 256, 64), (97, 256, 64), (97, 256, 128), (130, 512, 128), (97, 256, "row"), (130, 512, 128), (65, 768, 768),
            (97, 256, 64)]
    return [layer(R, n, 7700 + i, k) if isinstance(k, int) else layer(R, n, 7700 + i, kind=k, dev=dev) for i, (R, n, k) in
            enumerate(spec)]


def _rank_worker(rank, size, port, q):
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=size)
    try:
        from sleekit_amd import codebook as cbm
        from sleekit_amd import dist as sdist

        layers = _rank_layers(torch.device("cuda", 0))
        shards = sdist.quantize_stream(layers, sdist.HipBackend(cbm.UniformCodebook(8, -1, 1), "diag", 0.01, 0, with_error=True))
        torch.cuda.synchronize()
        errs = [float(sdist.layer_error(s["row_err"], layers[i]["W"].shape[0])) for i, s in enumerate(shards)]
        q.put((rank, [(s["rows"], s["idx"].cpu().numpy(), s["Q"].cpu().numpy(), int(s["info"].item())) for s in shards], errs))
    finally:
        dist.destroy_process_group()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.timeout(300)
def test_two_ranks_one_gpu_grouped_stream():
    import torch.multiprocessing as mp

    from sleekit_amd import codebook as cbm
    from sleekit_amd import dist as sdist

    layers = _rank_layers(torch.device("cuda", 0))
    single = sdist.quantize_stream(layers, sdist.HipBackend(cbm.UniformCodebook(8, -1, 1), "diag", 0.01, 0, with_error=True))
    torch.cuda.synchronize()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = sorted([q.get(timeout=240) for _ in procs], key=lambda x: x[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for l, lay in enumerate(layers):
        R = lay["W"].shape[0]
        (lo0, hi0), idx0, q0, info0 = got[0][1][l]
        (lo1, hi1), idx1, q1, info1 = got[1][1][l]
        assert (lo0, hi1) == (0, R) and hi0 == lo1 and info0 == 0 and info1 == 0
        assert np.array_equal(np.concatenate([idx0, idx1]), single[l]["idx"].cpu().numpy()), l
        assert np.array_equal(np.concatenate([q0, q1]).view(np.uint32), single[l]["Q"].cpu().numpy().view(np.uint32)), l
        want = float(single[l]["row_err"].double().sum() / R)
        assert abs(got[0][2][l] - want) <= 1e-6 * abs(want)


# ---------------------------------------------------------------------------------------------------- 6. a failing factor
def test_indefinite_hessian_in_a_grouped_round_names_the_layer():
    from sleekit_amd import _device as sdev
    from sleekit_amd import codebook as cbm
    from sleekit_amd import dist as sdist

    cb = cbm.UniformCodebook(8, -1, 1)
    layers = [layer(128, 192, 7800 + i, 64) for i in range(8)]
    layers[5]["H"] = layers[5]["H"].clone()
    layers[5]["H"][17, 17] = -1.0
    be = sdist.HipBackend(cb, "diag", 0.01, 0, with_error=True)
    calls = []
    run_local = be.run_round_local
    be.run_round_local = lambda members: (calls.append(len(members)), run_local(members))[1]
    with pytest.raises(np.linalg.LinAlgError, match=r"layer 5 \(128 x 192\)"):
        sdist.quantize_stream(layers, be)
    assert calls == [8]  # one batched round
    sdev.raise_pending()
    try:
        sdev.lazy_errors = True
        shards = sdist.quantize_stream(layers, be, join=False)
        torch.cuda.synchronize()
        for l, (lay, sh) in enumerate(zip(layers, shards)):
            if l != 5:  # the rest of the round comes out right
                Q, idx, _ = _alone(lay, cb)
                assert torch.equal(sh["Q"], Q) and torch.equal(sh["idx"], idx), l
        with pytest.raises(np.linalg.LinAlgError, match=r"layer 5 "):
            sdev.raise_pending()
    finally:
        sdev.lazy_errors = False
        sdev._pending_info.clear()
