#!/usr/bin/env python3
"""The packed-index linear layer against the routes a user had before it, on the MI355X.

    python tools/micro_packed_gemm.py [--reps 20] [--m 1,16,256,4096] [--bits 3] [--g 128]

Layers N x K = 4096 x 4096 and 4096 x 11008 at `bits` bits with group scales and offsets (groups of `g`), M rows of
bfloat16 activations, bfloat16 output.  Every side runs on preallocated outputs and is timed with device events (median
of `reps` after a warm-up, with [min, max]); the sides of a row alternate call by call in one process.

  (a) slk_packed_gemm
  (b) slk_dequantize_packed to bfloat16 + torch.nn.functional.linear on the result, timed together: the route there was
  (c) torch.nn.functional.linear alone on a layer de-quantized beforehand: the resident 16-bit alternative

M <= 16 moves the weights once and is held against HBM: the bytes (a) must move (4 * words + scales + offsets, x and y)
over 6.3 TB/s.  M >= 256 is held against the bfloat16 MFMA peak (2.5 PFLOP/s dense).  One JSON line per side and row.
"""

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from sleekit_amd import _device as dev, _lib, packing  # noqa: E402
from sleekit_amd.codebook import UniformCodebook  # noqa: E402

HBM = 6.3e12  # bytes/s
PEAK = 2.5e15  # FLOP/s, bfloat16 MFMA, dense
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


def rows(N, K, M, bits, g, reps):
    s = dev.stream_handle
    gen = torch.Generator(device="cuda").manual_seed(N + K + M)
    levels = 1 << bits
    cb = UniformCodebook(levels, -1, 1)
    idx = torch.randint(0, levels, (N, K), dtype=torch.uint8, device="cuda", generator=gen)
    P = packing.pack_indices(idx, bits)
    S = torch.rand((N, K // g), device="cuda", generator=gen) * 0.09 + 0.01
    O = torch.rand((N, K // g), device="cuda", generator=gen) * 0.1 - 0.05
    x = torch.randn((M, K), device="cuda", generator=gen).to(torch.bfloat16)
    y = torch.empty((M, N), dtype=torch.bfloat16, device="cuda")
    y2 = torch.empty((M, N), dtype=torch.bfloat16, device="cuda")
    Wd = torch.empty((N, K), dtype=torch.bfloat16, device="cuda")
    Wres = packing.dequantize_packed(P, K, cb, group_scales=S, offsets=O, dtype=torch.bfloat16)
    BF16 = _lib.DTYPE_BF16

    def a():
        _lib.check(L.slk_packed_gemm(dev.ptr(x), BF16, dev.ptr(P), bits, levels, -1.0, 1.0, None, None, dev.ptr(S), dev.ptr(O), g, None,
                                     M, N, K, BF16, BF16, dev.ptr(y), s()))

    def b():
        _lib.check(L.slk_dequantize_packed(dev.ptr(P), N, K, bits, levels, -1.0, 1.0, None, None, dev.ptr(S), dev.ptr(O), g, BF16,
                                           dev.ptr(Wd), s()))
        torch.matmul(x, Wd.T, out=y2)  # (F.linear without an allocation)

    def c():
        torch.matmul(x, Wres.T, out=y2)

    def a_py():
        packing.linear_packed(x, P, cb, group_scales=S, offsets=O)

    def b_py():
        F.linear(x, packing.dequantize_packed(P, K, cb, group_scales=S, offsets=O, dtype=torch.bfloat16))

    t_a, t_b, t_c, t_a2, t_b2, t_apy, t_bpy = timed([a, b, c, a, b, a_py, b_py], reps)
    w_bytes = 4 * P.numel() + 4 * S.numel() + 4 * O.numel()
    io = 2 * M * K + 2 * M * N
    flops = 2.0 * M * N * K
    size = f"{N}x{K}"
    spread = max(abs(t_a[0] - t_a2[0]), abs(t_b[0] - t_b2[0]))

    def emit(side, t, nbytes, **extra):
        us, lo, hi = t
        t_hbm, t_mfma = nbytes / HBM * 1e6, flops / PEAK * 1e6
        out = dict(size=size, M=M, bits=bits, g=g, side=side, us=round(us, 1), min_us=round(lo, 1), max_us=round(hi, 1), bytes=int(nbytes),
                   share_of_hbm=round(t_hbm / us, 3), tflops=round(flops / us * 1e-6, 1), share_of_mfma_peak=round(t_mfma / us, 4),
                   bound="hbm" if t_hbm >= t_mfma else "mfma", **extra)
        print(json.dumps(out), flush=True)

    emit("a: slk_packed_gemm", t_a, w_bytes + io, repeat_us=round(t_a2[0], 1), spread_us=round(spread, 1),
         faster_than_b=bool(max(t_a[0], t_a2[0]) + spread < min(t_b[0], t_b2[0])), b_over_a=round(t_b[0] / t_a[0], 2),
         c_over_a=round(t_c[0] / t_a[0], 2))
    emit("b: slk_dequantize_packed bfloat16 + linear", t_b, w_bytes + 4 * N * K + io, repeat_us=round(t_b2[0], 1))
    emit("c: linear on a resident bfloat16 layer", t_c, 2 * N * K + io)
    emit("a as packing.linear_packed", t_apy, w_bytes + io)
    emit("b as packing.dequantize_packed + F.linear", t_bpy, w_bytes + 4 * N * K + io)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--m", default="1,16,256,4096")
    ap.add_argument("--bits", type=int, default=3)
    ap.add_argument("--g", type=int, default=128)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "micro_packed_gemm measures the MI355X; there is no CPU path"
    torch.cuda.set_device(0)
    for N, K in ((4096, 4096), (4096, 11008)):
        for M in (int(m) for m in args.m.split(",")):
            rows(N, K, M, args.bits, args.g, args.reps)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
