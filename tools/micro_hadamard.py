#!/usr/bin/env python3
"""Micro-benchmark (GPU box): the block Hadamard rotation (slk_hadamard_rows through Rotation.apply).

  1. Rotation.apply on bfloat16 (M, K) beside torch.clone of the same tensor -- the yardstick for bytes in plus bytes
     out -- at M = 1, 16, 256, 4096 and K = 4096 (block 4096), K = 11008 (block 256);
  2. RotatedLinear beside its bare PackedLinear at M = 1 and 16 on 4096 x 4096, 3 bits, g = 128: what a rotated layer adds
     at decode.
Device events around every call, the two sides alternating call by call, median of --reps with [min, max]; one JSON line
per row.  Numbers: DESIGN.md section 16."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from sleekit_amd import PackedLinear, RotatedLinear, Rotation
from sleekit_amd.codebook import UniformCodebook

HBM = 6.3e12  # bytes / s, the figure the other micro-benchmarks use


def alternate(sides, reps, warmup=5):
    """{name: [us, ...]} of callables timed in turn, call by call."""
    times = {name: [] for name in sides}
    for i in range(warmup + reps):
        for name, call in sides.items():
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            call()
            end.record()
            end.synchronize()
            if i >= warmup:
                times[name].append(1e3 * start.elapsed_time(end))
    return times


def summary(us):
    return dict(median_us=round(statistics.median(us), 2), min_us=round(min(us), 2), max_us=round(max(us), 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--m", default="1,16,256,4096")
    args = ap.parse_args()
    torch.manual_seed(0)
    for K in (4096, 11008):
        rot = Rotation(K, seed=1)
        for M in (int(m) for m in args.m.split(",")):
            x = torch.randn(M, K, device="cuda").bfloat16()
            t = alternate({"apply": lambda: rot.apply(x), "clone": lambda: torch.clone(x)}, args.reps)
            a, c = summary(t["apply"]), summary(t["clone"])
            traffic = 2 * 2 * M * K
            print(json.dumps(dict(what="apply_vs_clone", M=M, K=K, block=rot.block, apply=a, clone=c,
                                  ratio=round(a["median_us"] / c["median_us"], 3),
                                  apply_share_of_hbm=round(traffic / (a["median_us"] * 1e-6) / HBM, 4))))
    K = N = 4096
    cb = UniformCodebook(8, -1, 1)
    inner = PackedLinear(K, N, cb, group_size=128, device="cuda")
    inner.words.copy_(torch.randint(-2**31, 2**31 - 1, inner.words.shape, dtype=torch.int64, device="cuda").to(torch.int32))
    inner.group_scales.copy_(torch.rand(inner.group_scales.shape, device="cuda") * 0.05 + 0.01)
    layer = RotatedLinear(inner, Rotation(K, seed=1))
    for M in (1, 16):
        x = torch.randn(M, K, device="cuda").bfloat16()
        t = alternate({"rotated": lambda: layer(x), "bare": lambda: inner(x)}, args.reps)
        r, b = summary(t["rotated"]), summary(t["bare"])
        print(json.dumps(dict(what="rotated_vs_packed_linear", M=M, K=K, N=N, bits=3, g=128, rotated=r, bare=b,
                              added_us=round(r["median_us"] - b["median_us"], 2))))


if __name__ == "__main__":
    main()
