#!/usr/bin/env python3
"""Micro-benchmark (GPU box): the grouped local search (slk_local_search_grouped) next to the per-row search
(slk_local_search, as tools/micro_ls.py times it) on the same layer shapes and moves, 8 levels, group size 128.
Per kernel: average time per launch from the library's profile (the initial product, the diagonal and the moves).
SHAPES=4096x4096,... MOVES=0,10,100 G=128 choose other cases (moves = 0: the fixed part of the search kernel)."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from sleekit_amd import _lib, codebook, engine, groups, synth

cb = codebook.UniformCodebook(8, -1, 1)
SHAPES = [tuple(int(x) for x in sh.split("x")) for sh in os.environ.get("SHAPES", "4096x4096,1024x4096,4096x1024,4096x11008").split(",")]
MOVES = [int(x) for x in os.environ.get("MOVES", "0,10,100").split(",")]
G = int(os.environ.get("G", "128"))


def timed(run):
    for _ in range(2):
        run()
    torch.cuda.synchronize()
    _lib.lib.slk_profile_reset(); _lib.lib.slk_profile_enable(1)
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    _lib.lib.slk_profile_enable(0)
    rows = {k["kernel"]: 1e3 * k["total_ms"] / k["launches"] for k in _lib.profile_report()}
    _lib.lib.slk_profile_reset()
    return rows


abi = cb._abi()
for R, n in SHAPES:
    L = synth.make_layer_device(R, n, 1006, torch.device("cuda"))
    # per-row: the scaled layer as engine.quantize_layer searches it
    res = engine.quantize_layer(L["W"], L["H"], cb, L["scale"], unscale=False)
    Ws = engine.rows_divide(L["W"], L["scale"])
    # grouped: mse group scales, the grouped loop's de-scaled output
    S = groups.compute_group_scaling(L["W"], cb, G, L["H"], mode="mse")
    Q0 = groups.quantize_grouped(L["W"], S, cb, L["H"], G)
    for moves in MOVES:
        row = timed(lambda: engine.local_search(Ws, res.Q.clone(), L["H"], abi, moves))
        grp = timed(lambda: groups.run_search_grouped(L["W"], Q0.clone(), S, L["H"], abi, G, moves))
        a, b = row.get("local_search", 0.0), grp.get("local_search_grouped", 0.0)
        rest_a = sum(v for k, v in row.items() if k != "local_search")
        rest_b = sum(v for k, v in grp.items() if k != "local_search_grouped")
        print(f"{R} x {n}, g = {G}, {moves:3d} moves:  moves kernel per-row {a:9.2f} us  grouped {b:9.2f} us  "
              f"({b / max(a, 1e-9):.2f}x);  product + diagonal {rest_a:8.2f} / {rest_b:8.2f} us", flush=True)
