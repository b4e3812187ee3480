#!/usr/bin/env python3
"""The weight-only MX product (activations="bfloat16") against what a user ran before it, on the MI355X.

    python tools/micro_mx_a16.py [--reps 30] [--shapes 4096x4096,5760x2880] [--m 1,16,64,256,4096] [--weights mxfp4,mxfp6_e2m3]
                                 [--experts 32] [--tokens 16,64]

A layer N x K of random codes under scale bytes 118 .. 123 and a bfloat16 x (M, K), both resident on the device; bfloat16
out.  Every leg runs through its public Python call, is warmed up, and is timed with device events around ONE call (median
of `reps`, with [min, max]); the legs alternate call by call in one process, and the new call is in the rotation twice: the
difference of its two medians is the run-to-run spread.

  new  mx.linear_mxfp4 / linear_mxfp6 (activations="bfloat16"): slk_mx_gemm_a16, one launch
  (a)  the same call with activations="mxfp8": the activation quantizer, the block-scaled product and the flag's read
  (b)  packing.linear_packed at 4 bits with the E2M1 table and group_size = 32 over the same indices and scales (MXFP4 only:
       the packed layer stores float32 group scales, 5 bits a weight)
  (c)  torch.nn.functional.linear on mx.dequantize_mxfp4 / _mxfp6(..., dtype=bfloat16), de-quantized beforehand (not timed)

and for a mixture-of-experts layer, top-4 of E experts at T tokens (M = 4 T rows sorted by expert):

  new  mx.linear_mx_experts (activations="bfloat16"): slk_mx_gemm_experts_a16, its flag's read included
  (a)  the same call with activations="mxfp8"
  (d)  the loop of dense new calls over the experts that have rows, on slices made beforehand with the counts known to the host

`floor_us` is the layer's bytes (codes and scale bytes; for the experts, of the experts that have rows) over the HBM rate
of 8 TB/s: the least time of a call that reads the weights once, which is what M <= 64 should approach.  The clock the device
reports before and after the run (rocm-smi, read only) is printed where the tool is there.  One JSON line per row.
"""

import argparse
import json
import os
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from sleekit_amd import mx, packing  # noqa: E402

HBM_BYTES_PER_US = 8.0e6  # 8 TB/s (MI355X_MICROARCH)
K_TOP = 4


def timed(fns, reps):
    """Median, min and max (us) of each of `fns`, called in turn `reps` times."""
    for _ in range(3):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts[k].append(a.elapsed_time(b) * 1e3)
    return [[round(v, 1) for v in (sorted(t)[len(t) // 2], min(t), max(t))] for t in ts]


def clocks():
    """The device's own report of its clocks (read only), or None where the tool is missing."""
    tool = shutil.which("rocm-smi") or "/opt/rocm/bin/rocm-smi"
    if not os.path.exists(tool):
        return None
    try:
        out = subprocess.run([tool, "-d", "0", "--showclocks"], capture_output=True, text=True, timeout=60).stdout
    except (OSError, subprocess.SubprocessError):
        return None
    return [line.strip() for line in out.splitlines() if "sclk" in line or "mclk" in line]


def random_layer(E, N, K, weights, gen):
    """(idx (E N, K) table indices, S (E N, K / 32) float32 powers of two, codes, scale bytes) on the device."""
    levels = 15 if weights == "mxfp4" else 63
    idx = torch.randint(0, levels, (E * N, K), dtype=torch.uint8, device="cuda", generator=gen)
    S = torch.exp2(torch.randint(-9, -3, (E * N, K // 32), device="cuda", generator=gen).float())
    codes, scales = (mx.pack_mxfp4 if weights == "mxfp4" else mx.pack_mxfp6)(idx, S)
    return idx, S, codes, scales


def dense_rows(N, K, weights, ms, reps):
    gen = torch.Generator(device="cuda").manual_seed(N + K)
    idx, S, codes, scales = random_layer(1, N, K, weights, gen)
    linear = mx.linear_mxfp4 if weights == "mxfp4" else mx.linear_mxfp6
    Wd = (mx.dequantize_mxfp4 if weights == "mxfp4" else mx.dequantize_mxfp6)(codes, scales, dtype=torch.bfloat16)
    words = packing.pack_indices(idx, 4) if weights == "mxfp4" else None
    layer_bytes = codes.numel() + scales.numel()
    for M in ms:
        x = torch.randn((M, K), device="cuda", generator=gen).bfloat16()
        legs = {"new": lambda: linear(x, codes, scales, activations="bfloat16"),
                "a_mxfp8": lambda: linear(x, codes, scales, activations="mxfp8"),
                "c_torch_bf16": lambda: F.linear(x, Wd)}
        if words is not None:
            legs["b_packed"] = lambda: packing.linear_packed(x, words, mx.E2M1, 4, group_scales=S, group_size=32)
        legs["new_again"] = legs["new"]
        # the legs compute the same layer: (b) and (c) on the same operands up to the order of float32 sums
        y, yc = legs["new"]().float(), legs["c_torch_bf16"]().float()
        err = float((y - yc).abs().max() / yc.abs().max())
        assert err < 2e-2, f"the new call and torch disagree: {err}"
        if words is not None:
            yb = legs["b_packed"]().float()
            assert float((y - yb).abs().max() / yb.abs().max()) < 2e-2, "the new call and the packed layer disagree"
        t = dict(zip(legs, timed(list(legs.values()), reps)))
        new = min(t["new"][0], t["new_again"][0])
        print(json.dumps(dict(kind="dense", weights=weights, size=f"{N}x{K}", M=M, **{f"{k}_us": v for k, v in t.items()},
                              spread_us=round(abs(t["new"][0] - t["new_again"][0]), 1), floor_us=round(layer_bytes / HBM_BYTES_PER_US, 2),
                              a_over_new=round(t["a_mxfp8"][0] / new, 2), c_over_new=round(t["c_torch_bf16"][0] / new, 2),
                              b_over_new=round(t["b_packed"][0] / new, 2) if words is not None else None,
                              tflops=round(2.0 * M * N * K / new * 1e-6, 1), weights_gb_s=round(layer_bytes / new * 1e-3, 1),
                              max_rel_diff_to_torch=round(err, 5))), flush=True)


def expert_rows(E, N, K, weights, tokens, reps):
    gen = torch.Generator(device="cuda").manual_seed(E + N + K)
    _, _, codes, scales = random_layer(E, N, K, weights, gen)
    codes, scales = codes.reshape(E, N, -1), scales.reshape(E, N, -1)
    linear = mx.linear_mxfp4 if weights == "mxfp4" else mx.linear_mxfp6
    for T in tokens:
        M = K_TOP * T
        counts = np.random.default_rng(E + T).multinomial(M, np.full(E, 1.0 / E))
        host_offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        offsets = torch.from_numpy(host_offsets).cuda()
        x = torch.randn((M, K), device="cuda", generator=gen).bfloat16()
        live = [e for e in range(E) if counts[e] > 0]
        pieces = [(x[host_offsets[e]:host_offsets[e + 1]], codes[e], scales[e]) for e in live]

        def loop():
            return [linear(xe, c, s, activations="bfloat16") for xe, c, s in pieces]

        legs = {"new": lambda: mx.linear_mx_experts(x, codes, scales, offsets, activations="bfloat16", weights=weights),
                "a_mxfp8": lambda: mx.linear_mx_experts(x, codes, scales, offsets, activations="mxfp8", weights=weights),
                "d_loop": loop}
        legs["new_again"] = legs["new"]
        assert torch.equal(legs["new"]().view(torch.int16), torch.cat(loop()).view(torch.int16)), "the grouped call and the loop disagree"
        t = dict(zip(legs, timed(list(legs.values()), reps)))
        new = min(t["new"][0], t["new_again"][0])
        read = len(live) * (codes[0].numel() + scales[0].numel())
        print(json.dumps(dict(kind="experts", weights=weights, E=E, size=f"{N}x{K}", T=T, M=M, experts_with_rows=len(live),
                              largest_expert=int(counts.max()), **{f"{k}_us": v for k, v in t.items()},
                              spread_us=round(abs(t["new"][0] - t["new_again"][0]), 1), floor_us=round(read / HBM_BYTES_PER_US, 2),
                              a_over_new=round(t["a_mxfp8"][0] / new, 2), d_over_new=round(t["d_loop"][0] / new, 2),
                              weights_gb_s=round(read / new * 1e-3, 1))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--shapes", default="4096x4096,5760x2880")
    ap.add_argument("--m", default="1,16,64,256,4096")
    ap.add_argument("--weights", default="mxfp4,mxfp6_e2m3")
    ap.add_argument("--experts", type=int, default=32)
    ap.add_argument("--tokens", default="16,64")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "micro_mx_a16 measures the MI355X; there is no CPU path"
    torch.cuda.set_device(0)
    print(json.dumps(dict(kind="clocks", when="before", report=clocks())), flush=True)
    shapes = [tuple(int(v) for v in shape.split("x")) for shape in args.shapes.split(",")]
    for weights in args.weights.split(","):
        for N, K in shapes:
            dense_rows(N, K, weights, [int(m) for m in args.m.split(",")], args.reps)
            torch.cuda.empty_cache()
        if args.experts:
            N, K = shapes[-1]
            expert_rows(args.experts, N, K, weights, [int(t) for t in args.tokens.split(",")], args.reps)
            torch.cuda.empty_cache()
    print(json.dumps(dict(kind="clocks", when="after", report=clocks())), flush=True)


if __name__ == "__main__":
    main()
