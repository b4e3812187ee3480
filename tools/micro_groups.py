#!/usr/bin/env python3
"""Group-wise scales: ms per layer of the grouped loop against the per-row path, on the MI355X.

    python tools/micro_groups.py [--reps 10] [--shapes 4096x4096,4096x11008] [--groups 64,128,0]   (0 = g = n)

single:     one layer at a time, each waited for (the single-layer API: factor, loop, status read back)
pipelined:  `reps` layers enqueued back to back, status words checked once at the end (sleekit_amd._device.lazy_errors)
Both time the whole layer from W, S, H on the device: damping + order + factor + loop (+ err/sqerr keys), not the scale
search.  The per-row row is engine.quantize_layer with a per-row scale (quantize_with_scaling without local search).

--offsets: after each group size's row, the asymmetric loop (offsets = the groups' midpoints) with its ratio to the
symmetric grouped row of the same g, and the midpoint kernel's read bandwidth (compute_group_offsets, W read once).
"""

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from sleekit_amd import _device as dev  # noqa: E402
from sleekit_amd import engine, groups, synth  # noqa: E402
from sleekit_amd.codebook import UniformCodebook  # noqa: E402


def timed(fn, reps, pipelined):
    fn()  # warm-up: workspaces, LDS opt-ins, helper streams
    torch.cuda.synchronize()
    if pipelined:
        dev.lazy_errors = True
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        t = time.perf_counter() - t0
        dev.raise_pending()
        dev.lazy_errors = False
        return 1e3 * t / reps
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    ts.sort()
    return 1e3 * ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shapes", default="4096x4096,4096x11008")
    ap.add_argument("--groups", default="64,128,0")
    ap.add_argument("--order", default="diag")
    ap.add_argument("--offsets", action="store_true", help="also time the asymmetric loop and the midpoint kernel")
    ap.add_argument("--out", default=None, help="also write the rows as JSON here")
    args = ap.parse_args()
    cb = UniformCodebook(8, -1, 1)
    rows = []
    for shape in args.shapes.split(","):
        R, n = (int(x) for x in shape.split("x"))
        L = synth.make_layer_device(R, n, 4242, torch.device("cuda"))
        W, H, s = L["W"], L["H"], L["scale"]
        for pipelined in (False, True):
            first = len(rows)
            base = timed(lambda: engine.quantize_layer(W, H, cb, s, args.order, 0.01, want_idx=False), args.reps, pipelined)
            rows.append(dict(shape=shape, path="pipelined" if pipelined else "single", g="per-row", ms=round(base, 3), ratio=1.0))
            for g in (int(x) for x in args.groups.split(",")):
                g = g or n
                S = (s[:, None] * torch.ones(1, n // g, device=W.device)).contiguous()
                ms = timed(lambda: groups.quantize_layer_grouped(W, S, cb, H, g, args.order, 0.01, want_idx=False), args.reps, pipelined)
                rows.append(dict(shape=shape, path="pipelined" if pipelined else "single", g=g, ms=round(ms, 3), ratio=round(ms / base, 2)))
                if args.offsets:
                    O = groups.compute_group_offsets(W, g)
                    ma = timed(lambda: groups.quantize_layer_grouped(W, S, cb, H, g, args.order, 0.01, want_idx=False, offsets=O),
                               args.reps, pipelined)
                    rows.append(dict(shape=shape, path="pipelined" if pipelined else "single", g=f"{g} asym", ms=round(ma, 3),
                                     ratio=round(ma / ms, 3)))
                    if not pipelined:
                        mo = timed(lambda: groups.compute_group_offsets(W, g), args.reps, True)
                        rows.append(dict(shape=shape, path="midpoints", g=g, ms=round(mo, 4), ratio=round(4e-6 * R * n / mo, 1)))
            for r in rows[first:]:
                print(f"{r['shape']:>10} {r['path']:>9} g={str(r['g']):>8}  {r['ms']:8.3f} ms  x{r['ratio']:.2f}", flush=True)
        del W, H, s, L
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
