#!/usr/bin/env python3
"""The packed MXFP4 linear layer against the routes a user had before it, on the MI355X.

    python tools/micro_mx_gemm.py [--reps 20] [--m 1,16,256,4096] [--w6]

Layers N x K = 4096 x 4096 and 4096 x 11008, M rows of bfloat16 activations, bfloat16 output.  Every side runs on
preallocated outputs and is timed with device events (median of `reps` after a warm-up, with [min, max]); the sides of a
row alternate call by call in one process, and (b) and (c) are in the rotation twice: the difference of the two medians of
one side is the run-to-run spread the verdict allows for.

  (a) slk_mx_gemm on activations quantized beforehand
  (b) slk_mx_quantize_act + slk_mx_gemm: what linear_mxfp4 launches
  (c) slk_mx_dequantize to bfloat16 + torch.matmul: the route there was before
  (d) torch.matmul alone on a resident bfloat16 copy of the layer (16 times the packed layer's bytes)
  and mx.linear_mxfp4 / mx.dequantize_mxfp4 + matmul as Python calls (allocations and the flag's read included).

M <= 16 moves the weights once and is held against HBM: bytes the algorithm must move over 6.3 TB/s.  M >= 256 is held
against the E4M3 block-scaled MFMA peak (5 PFLOP/s dense).  `bound` names the larger of the two shares' times.
--w6: the MXFP6 layer instead -- slk_mx_gemm_w6 with MXFP8 and MXFP6 activations (W6A8, W6A6) against slk_mx_gemm and
slk_mx_gemm_a6 on an MXFP4 layer of the same shape (W4A8, W4A6), activations quantized beforehand, the four sides alternating.
One JSON line per row.
"""

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from sleekit_amd import _device as dev, _lib, mx  # noqa: E402

HBM = 6.3e12  # bytes/s
PEAK = 5.0e15  # FLOP/s, E4M3 operands on the block-scaled MFMA
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


def rows(N, K, M, reps):
    s = dev.stream_handle
    gen = torch.Generator(device="cuda").manual_seed(N + K + M)
    codes = torch.randint(0, 256, (N, K // 2), dtype=torch.uint8, device="cuda", generator=gen)
    codes &= 0x77  # (no -0: every nibble is one of the codes the packer writes)
    scales = torch.randint(118, 124, (N, K // 32), dtype=torch.uint8, device="cuda", generator=gen)
    x = torch.randn((M, K), device="cuda", generator=gen).to(torch.bfloat16)
    ac = torch.empty((M, K), dtype=torch.uint8, device="cuda")
    asc = torch.empty((M, K // 32), dtype=torch.uint8, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    y = torch.empty((M, N), dtype=torch.bfloat16, device="cuda")
    y2 = torch.empty((M, N), dtype=torch.bfloat16, device="cuda")
    Wd = torch.empty((N, K), dtype=torch.bfloat16, device="cuda")
    Wres = mx.dequantize_mxfp4(codes, scales, dtype=torch.bfloat16)

    def quant():
        _lib.check(L.slk_mx_quantize_act(dev.ptr(x), _lib.DTYPE_BF16, M, K, dev.ptr(ac), dev.ptr(asc), dev.ptr(flag), s()))

    def gemm():
        _lib.check(L.slk_mx_gemm(dev.ptr(ac), dev.ptr(asc), dev.ptr(codes), dev.ptr(scales), None, M, N, K, _lib.DTYPE_BF16, dev.ptr(y), s()))

    def b():
        quant()
        gemm()

    def c():
        _lib.check(L.slk_mx_dequantize(dev.ptr(codes), dev.ptr(scales), N, K, _lib.DTYPE_BF16, dev.ptr(Wd), None, s()))
        torch.matmul(x, Wd.T, out=y2)

    def d():
        torch.matmul(x, Wres.T, out=y2)

    def b_py():
        mx.linear_mxfp4(x, codes, scales)

    def c_py():
        torch.matmul(x, mx.dequantize_mxfp4(codes, scales, dtype=torch.bfloat16).T)

    quant()
    t_a, t_b, t_c, t_d, t_b2, t_c2, t_bpy, t_cpy = timed([gemm, b, c, d, b, c, b_py, c_py], reps)
    w_bytes = N * K // 2 + N * K // 32
    flops = 2.0 * M * N * K
    size = f"{N}x{K}"
    spread = max(abs(t_b[0] - t_b2[0]), abs(t_c[0] - t_c2[0]))

    def emit(side, t, nbytes, **extra):
        us, lo, hi = t
        t_hbm, t_mfma = nbytes / HBM * 1e6, flops / PEAK * 1e6
        out = dict(size=size, M=M, side=side, us=round(us, 1), min_us=round(lo, 1), max_us=round(hi, 1), bytes=int(nbytes),
                   share_of_hbm=round(t_hbm / us, 3), tflops=round(flops / us * 1e-6, 1), share_of_mfma_peak=round(t_mfma / us, 4),
                   bound="hbm" if t_hbm >= t_mfma else "mfma", **extra)
        print(json.dumps(out), flush=True)

    emit("a: mx_gemm, activations quantized before", t_a, w_bytes + M * K * 33 // 32 + 2 * M * N)
    emit("b: quantize_act + mx_gemm", t_b, w_bytes + 2 * M * K + 2 * M * N, repeat_us=round(t_b2[0], 1), spread_us=round(spread, 1),
         faster_than_c=bool(max(t_b[0], t_b2[0]) + spread < min(t_c[0], t_c2[0])), c_over_b=round(t_c[0] / t_b[0], 2))
    emit("c: mx_dequantize bfloat16 + torch.matmul", t_c, w_bytes + 4 * N * K + 2 * M * K + 2 * M * N, repeat_us=round(t_c2[0], 1))
    emit("d: torch.matmul on a resident bfloat16 layer", t_d, 2 * N * K + 2 * M * K + 2 * M * N)
    emit("b as mx.linear_mxfp4", t_bpy, w_bytes + 2 * M * K + 2 * M * N)
    emit("c as mx.dequantize_mxfp4 + torch.matmul", t_cpy, w_bytes + 4 * N * K + 2 * M * K + 2 * M * N)


def rows_w6(N, K, M, reps):
    s = dev.stream_handle
    gen = torch.Generator(device="cuda").manual_seed(N + K + M)
    w4 = torch.randint(0, 256, (N, K // 2), dtype=torch.uint8, device="cuda", generator=gen) & 0x77
    idx6 = torch.randint(0, 63, (N, K), dtype=torch.uint8, device="cuda", generator=gen)
    scales = torch.randint(118, 124, (N, K // 32), dtype=torch.uint8, device="cuda", generator=gen)
    w6 = mx.pack_mxfp6(idx6, mx.decode_scales(scales))[0]
    del idx6
    x = torch.randn((M, K), device="cuda", generator=gen).to(torch.bfloat16)
    a8, a8s = mx.quantize_mxfp8(x)
    a6, a6s = mx.quantize_mxfp6_act(x)
    y = torch.empty((M, N), dtype=torch.bfloat16, device="cuda")
    P = dev.ptr

    def w4a8():
        _lib.check(L.slk_mx_gemm(P(a8), P(a8s), P(w4), P(scales), None, M, N, K, _lib.DTYPE_BF16, P(y), s()))

    def w6a8():
        _lib.check(L.slk_mx_gemm_w6(P(a8), P(a8s), P(w6), P(scales), None, M, N, K, _lib.MX_ACT_FP8, _lib.DTYPE_BF16, P(y), s()))

    def w4a6():
        _lib.check(L.slk_mx_gemm_a6(P(a6), P(a6s), P(w4), P(scales), None, M, N, K, _lib.DTYPE_BF16, P(y), s()))

    def w6a6():
        _lib.check(L.slk_mx_gemm_w6(P(a6), P(a6s), P(w6), P(scales), None, M, N, K, _lib.MX_ACT_FP6, _lib.DTYPE_BF16, P(y), s()))

    sides = (("W4A8 slk_mx_gemm", w4a8, 4, 8), ("W6A8 slk_mx_gemm_w6", w6a8, 6, 8), ("W4A6 slk_mx_gemm_a6", w4a6, 4, 6),
             ("W6A6 slk_mx_gemm_w6", w6a6, 6, 6), ("W4A8 again", w4a8, 4, 8))
    ts = timed([fn for _, fn, _, _ in sides], reps)
    flops = 2.0 * M * N * K
    for (name, _, wb, ab), (us, lo, hi) in zip(sides, ts):
        nbytes = (N * wb + M * ab) * K // 8 + (N + M) * K // 32 + 2 * M * N
        t_hbm, t_mfma = nbytes / HBM * 1e6, flops / PEAK * 1e6
        print(json.dumps(dict(size=f"{N}x{K}", M=M, side=name, us=round(us, 1), min_us=round(lo, 1), max_us=round(hi, 1), bytes=int(nbytes),
                              share_of_hbm=round(t_hbm / us, 3), tflops=round(flops / us * 1e-6, 1), over_w4a8=round(us / ts[0][0], 3))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--m", default="1,16,256,4096")
    ap.add_argument("--w6", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "micro_mx_gemm measures the MI355X; there is no CPU path"
    torch.cuda.set_device(0)
    for N, K in ((4096, 4096), (4096, 11008)):
        for M in (int(m) for m in args.m.split(",")):
            (rows_w6 if args.w6 else rows)(N, K, M, args.reps)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
