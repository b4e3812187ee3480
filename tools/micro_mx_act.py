#!/usr/bin/env python3
"""MXFP4 activations against MXFP8 ones, and the rotation fused into the quantizer against the two steps, on the MI355X.

    python tools/micro_mx_act.py [--reps 20] [--m 1,16,256,4096] [--only linear|fused]

Every side runs on preallocated outputs and is timed with device events (median of `reps` after a warm-up, with
[min, max]); the sides of a row alternate call by call in one process.

  linear  layers N x K = 4096 x 4096 and 4096 x 11008, M rows of bfloat16 activations, bfloat16 output:
          (a8) slk_mx_quantize_act  + slk_mx_gemm      what linear_mxfp4 launches by default (W4A8)
          (a4) slk_mx_quantize_act4 + slk_mx_gemm_a4   what activations="mxfp4" launches (W4A4)
          each in the rotation twice: the difference of the two medians of one side is the run-to-run spread.
          M <= 16 moves the weights once and is held against HBM (6.3 TB/s); M >= 256 against the block-scaled MFMA
          peak of its format (5 PFLOP/s E4M3, 10 PFLOP/s E2M1).
  fused   rows x n = 4096 x 4096, block 4096, bfloat16 x, for both formats:
          (two) slk_hadamard_rows to float32 + slk_mx_quantize_act / _act4
          (one) slk_mx_rotate_quantize_act
          with the bytes each must move as a share of HBM.
One JSON line per row and side.
"""

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from sleekit_amd import _device as dev, _lib, rotation  # noqa: E402

HBM = 6.3e12  # bytes/s
PEAK = {"a8": 5.0e15, "a4": 10.0e15}  # FLOP/s on the block-scaled MFMA
L = _lib.lib


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
    return [(sorted(t)[len(t) // 2], min(t), max(t)) for t in ts]


def stats(t):
    return dict(us=round(t[0], 1), min_us=round(t[1], 1), max_us=round(t[2], 1))


def linear_rows(N, K, M, reps):
    s = dev.stream_handle
    gen = torch.Generator(device="cuda").manual_seed(N + K + M)
    codes = torch.randint(0, 256, (N, K // 2), dtype=torch.uint8, device="cuda", generator=gen)
    codes &= 0x77  # (no -0: every nibble is one of the codes the packer writes)
    scales = torch.randint(118, 124, (N, K // 32), dtype=torch.uint8, device="cuda", generator=gen)
    x = torch.randn((M, K), device="cuda", generator=gen).to(torch.bfloat16)
    a8 = torch.empty((M, K), dtype=torch.uint8, device="cuda")
    a4 = torch.empty((M, K // 2), dtype=torch.uint8, device="cuda")
    asc = torch.empty((M, K // 32), dtype=torch.uint8, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    y = torch.empty((M, N), dtype=torch.bfloat16, device="cuda")

    def w4a8():
        _lib.check(L.slk_mx_quantize_act(dev.ptr(x), _lib.DTYPE_BF16, M, K, dev.ptr(a8), dev.ptr(asc), dev.ptr(flag), s()))
        _lib.check(L.slk_mx_gemm(dev.ptr(a8), dev.ptr(asc), dev.ptr(codes), dev.ptr(scales), None, M, N, K, _lib.DTYPE_BF16, dev.ptr(y), s()))

    def w4a4():
        _lib.check(L.slk_mx_quantize_act4(dev.ptr(x), _lib.DTYPE_BF16, M, K, dev.ptr(a4), dev.ptr(asc), dev.ptr(flag), s()))
        _lib.check(L.slk_mx_gemm_a4(dev.ptr(a4), dev.ptr(asc), dev.ptr(codes), dev.ptr(scales), None, M, N, K, _lib.DTYPE_BF16, dev.ptr(y), s()))

    sides = [("a8", w4a8), ("a4", w4a4)]
    ts = timed([fn for _, fn in sides] * 2, reps)
    first, second = ts[:len(sides)], ts[len(sides):]
    w_bytes = N * K // 2 + N * K // 32
    flops = 2.0 * M * N * K
    out = {}
    for (name, _), t, t2 in zip(sides, first, second):
        # x read, codes and scale bytes written and read again, the layer, y
        nbytes = w_bytes + 2 * M * K + 2 * (M * K * (8 if name == "a8" else 4) // 8 + M * K // 32) + 2 * M * N
        t_hbm, t_mfma = nbytes / HBM * 1e6, flops / PEAK[name] * 1e6
        out[name] = (t, t2)
        print(json.dumps(dict(bench="linear", size=f"{N}x{K}", M=M, side="W4A8: quantize_act + mx_gemm" if name == "a8" else
                              "W4A4: quantize_act4 + mx_gemm_a4", **stats(t), repeat_us=round(t2[0], 1), bytes=int(nbytes),
                              share_of_hbm=round(t_hbm / t[0], 3), tflops=round(flops / t[0] * 1e-6, 1),
                              share_of_mfma_peak=round(t_mfma / t[0], 4), bound="hbm" if t_hbm >= t_mfma else "mfma")), flush=True)
    (t8, t8b), (t4, t4b) = out["a8"], out["a4"]
    print(json.dumps(dict(bench="linear", size=f"{N}x{K}", M=M, side="W4A4 against W4A8", a8_over_a4=round(t8[0] / t4[0], 3),
                          a4_median_within_a8_range=bool(max(t4[0], t4b[0]) <= max(t8[2], t8b[2])),
                          spread_us=round(max(abs(t8[0] - t8b[0]), abs(t4[0] - t4b[0])), 1))), flush=True)


def fused_rows(rows, n, block, reps):
    s = dev.stream_handle
    gen = torch.Generator(device="cuda").manual_seed(rows + n)
    x = torch.randn((rows, n), device="cuda", generator=gen).to(torch.bfloat16)
    rot = rotation.Rotation(n, block=block, seed=1)
    yf = torch.empty((rows, n), dtype=torch.float32, device="cuda")
    c8 = torch.empty((rows, n), dtype=torch.uint8, device="cuda")
    c4 = torch.empty((rows, n // 2), dtype=torch.uint8, device="cuda")
    sc = torch.empty((rows, n // 32), dtype=torch.uint8, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")

    def two(fp4):
        def run():
            _lib.check(L.slk_hadamard_rows(dev.ptr(x), _lib.DTYPE_BF16, dev.ptr(yf), _lib.DTYPE_F32, rows, n, block, dev.ptr(rot.signs), 0, s()))
            if fp4:
                _lib.check(L.slk_mx_quantize_act4(dev.ptr(yf), _lib.DTYPE_F32, rows, n, dev.ptr(c4), dev.ptr(sc), dev.ptr(flag), s()))
            else:
                _lib.check(L.slk_mx_quantize_act(dev.ptr(yf), _lib.DTYPE_F32, rows, n, dev.ptr(c8), dev.ptr(sc), dev.ptr(flag), s()))
        return run

    def one(fp4):
        def run():
            _lib.check(L.slk_mx_rotate_quantize_act(dev.ptr(x), _lib.DTYPE_BF16, rows, n, block, dev.ptr(rot.signs),
                                                    _lib.MX_ACT_FP4 if fp4 else _lib.MX_ACT_FP8, dev.ptr(c4 if fp4 else c8), dev.ptr(sc),
                                                    dev.ptr(flag), s()))
        return run

    for fp4 in (False, True):
        t_two, t_one, t_two2, t_one2 = timed([two(fp4), one(fp4)] * 2, reps)
        e = rows * n
        code_bytes = e // 2 if fp4 else e
        b_two = 2 * e + 4 * e + 4 * e + code_bytes + e // 32
        b_one = 2 * e + code_bytes + e // 32
        fmt = "mxfp4" if fp4 else "mxfp8"
        print(json.dumps(dict(bench="fused", shape=f"{rows}x{n}", block=block, fmt=fmt, side="two steps: hadamard_rows float32 + quantize",
                              **stats(t_two), repeat_us=round(t_two2[0], 1), bytes=b_two, share_of_hbm=round(b_two / HBM * 1e6 / t_two[0], 3))), flush=True)
        print(json.dumps(dict(bench="fused", shape=f"{rows}x{n}", block=block, fmt=fmt, side="fused: mx_rotate_quantize_act",
                              **stats(t_one), repeat_us=round(t_one2[0], 1), bytes=b_one, share_of_hbm=round(b_one / HBM * 1e6 / t_one[0], 3),
                              two_over_one=round(t_two[0] / t_one[0], 2),
                              median_below_two_steps_min=bool(max(t_one[0], t_one2[0]) < min(t_two[1], t_two2[1])))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--m", default="1,16,256,4096")
    ap.add_argument("--only", choices=("linear", "fused"), default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "micro_mx_act measures the MI355X; there is no CPU path"
    torch.cuda.set_device(0)
    if args.only != "fused":
        for N, K in ((4096, 4096), (4096, 11008)):
            for M in (int(m) for m in args.m.split(",")):
                linear_rows(N, K, M, args.reps)
                torch.cuda.empty_cache()
    if args.only != "linear":
        fused_rows(4096, 4096, 4096, args.reps)


if __name__ == "__main__":
    main()
