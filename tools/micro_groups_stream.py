#!/usr/bin/env python3
"""Group-wise scales through the layer stream (sleekit_amd.dist.quantize_stream) against one layer at a time
(groups.quantize_layer_grouped), on the MI355X.  Prints one JSON line.

    python tools/micro_groups_stream.py [--reps 10] [--warmup 3] [--repeats 3] [--g 128]

opt125m:    OPT-125M-shaped grouped stream (12 x {4 x 768^2, 3072 x 768, 768 x 3072}, 8 levels, diag order):
            quantize_stream on one rank against a loop of quantize_layer_grouped.
big:        8 grouped 4096 x 4096 layers, the same two ways.
rank_of_8:  one rank of 8 on the OPT-125M-shaped stream, REHEARSED on this GPU (sleekit_amd.dist.rehearse: the rank's rounds,
            roots, streams and kernels, with the all-gather replaced by a local hand-over) -- not a measurement of 8 GPUs.
Every number is ms per pass over the stream, from device events around `reps` passes after `warmup` passes, the median of
`repeats` such runs (all runs listed).  Neither side computes layer errors (HipBackend(with_error=False)); status words are
checked once per run (sleekit_amd._device.lazy_errors).  The group scales come from the diag search, outside the timing.
"""

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from sleekit_amd import _device as dev  # noqa: E402
from sleekit_amd import dist as sdist  # noqa: E402
from sleekit_amd import groups, synth  # noqa: E402
from sleekit_amd.codebook import UniformCodebook  # noqa: E402

OPT125M = ([(768, 768)] * 4 + [(3072, 768), (768, 3072)]) * 12


def make_layers(shapes, g, cb, seed0):
    device = torch.device("cuda", 0)
    out = []
    for i, (R, n) in enumerate(shapes):
        L = synth.make_layer_device(R, n, seed0 + i, device, keep=("W", "H"))
        S = groups.compute_group_scaling(L["W"], cb, g, L["H"], "diag")
        out.append(dict(W=L["W"], H=L["H"], gscale=S, group_size=g))
    torch.cuda.synchronize()
    return out


def timed(fn, reps, warmup, repeats):
    """ms per call: device events around `reps` calls, after `warmup`; the median of `repeats` runs, and every run."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    dev.raise_pending()
    runs = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        torch.cuda.synchronize()
        dev.raise_pending()
        runs.append(e0.elapsed_time(e1) / reps)
    return round(statistics.median(runs), 3), [round(r, 3) for r in runs]


def compare(layers, cb, args):
    be = sdist.HipBackend(cb, "diag", 0.01, 0, with_error=False)

    def stream():
        sdist.quantize_stream(layers, be)

    def one_by_one():
        for lay in layers:
            groups.quantize_layer_grouped(lay["W"], lay["gscale"], cb, lay["H"], lay["group_size"], "diag")

    s_ms, s_runs = timed(stream, args.reps, args.warmup, args.repeats)
    o_ms, o_runs = timed(one_by_one, args.reps, args.warmup, args.repeats)
    return dict(layers=len(layers), stream_ms=s_ms, one_by_one_ms=o_ms, speedup=round(o_ms / s_ms, 3), stream_runs=s_runs,
                one_by_one_runs=o_runs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--g", type=int, default=128)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    dev.lazy_errors = True
    cb = UniformCodebook(8, -1, 1)
    out = dict(tool="micro_groups_stream", group_size=args.g, levels=8, act_order="diag", reps=args.reps, warmup=args.warmup,
               repeats=args.repeats, gpu_max_hw_queues=os.environ.get("GPU_MAX_HW_QUEUES"))

    small = make_layers(OPT125M, args.g, cb, 8100)
    out["opt125m"] = compare(small, cb, args)
    big = make_layers([(4096, 4096)] * 8, args.g, cb, 8300)
    out["big_4096x4096x8"] = compare(big, cb, args)
    del big
    torch.cuda.empty_cache()

    be = sdist.HipBackend(cb, "diag", 0.01, 0, with_error=False)
    sdist.rehearse = (0, 8)
    try:
        ms, runs = timed(lambda: sdist.quantize_stream(small, be), args.reps, args.warmup, args.repeats)
    finally:
        sdist.rehearse = None
    out["opt125m_rank_of_8_rehearsed"] = dict(stream_ms=ms, stream_runs=runs, note="one rank of 8 rehearsed on one GPU")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
