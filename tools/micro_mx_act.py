#!/usr/bin/env python3
"""MXFP4 and MXFP6 activations against MXFP8 ones, and the rotation fused into the quantizer against the two steps, on the
MI355X.

    python tools/micro_mx_act.py [--reps 20] [--m 1,16,256,4096] [--only linear|fused|quantize] [--parent-lib libsleekit_amd.so]

Every side runs on preallocated outputs and is timed with device events (median of `reps` after a warm-up, with
[min, max]); the sides of a row alternate call by call in one process.

  linear  layers N x K = 4096 x 4096 and 4096 x 11008, M rows of bfloat16 activations, bfloat16 output:
          (a8) slk_mx_quantize_act  + slk_mx_gemm      what linear_mxfp4 launches by default (W4A8)
          (a6) slk_mx_quantize_act6 + slk_mx_gemm_a6   what activations="mxfp6_e2m3" launches (W4A6)
          (a4) slk_mx_quantize_act4 + slk_mx_gemm_a4   what activations="mxfp4" launches (W4A4)
          and, with --parent-lib (a library built from another commit), (p8), (p6) and (p4): W4A8, W4A6 and W4A4 through
          that library, in the same rotation.  Each side is in the rotation twice: the difference of the two medians of one
          side is the run-to-run spread.
          M <= 16 moves the weights once and is held against HBM (6.3 TB/s); M >= 256 against the block-scaled MFMA
          peak of its format (5 PFLOP/s E4M3, 10 PFLOP/s E2M3 and E2M1).
  fused   rows x n = 4096 x 4096, block 4096, bfloat16 x, for the three formats:
          (two) slk_hadamard_rows to float32 + slk_mx_quantize_act / _act6 / _act4
          (one) slk_mx_rotate_quantize_act / _act6
          with the bytes each must move as a share of HBM; with --parent-lib also the fused kernel of this library and of
          that one alternating, each side twice, as in the quantize rows.
  quantize  4096 x 11008 bfloat16: each plain quantizer (slk_mx_quantize_act, _act6, _act4) and each activation
          de-quantizer (slk_mx_dequantize_act, _act6, to bfloat16) alone, this library and --parent-lib (required) alternating,
          each side twice; the spread is the difference of the parent's own two medians.
One JSON line per row and side.
"""

import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from sleekit_amd import _device as dev, _lib, rotation  # noqa: E402

HBM = 6.3e12  # bytes/s
PEAK = {"a8": 5.0e15, "a6": 10.0e15, "a4": 10.0e15}  # FLOP/s on the block-scaled MFMA
L = _lib.lib


def load_library(path):
    """Another build of the library (a parent commit's), with the prototypes of the entries it has."""
    other = ctypes.CDLL(os.path.abspath(path))
    for name, (res, args) in _lib.PROTOTYPES.items():
        fn = getattr(other, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, args
    return other


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


BITS = {"a8": 8, "a6": 6, "a4": 4}
NAMES = {"a8": "W4A8: quantize_act + mx_gemm", "a6": "W4A6: quantize_act6 + mx_gemm_a6", "a4": "W4A4: quantize_act4 + mx_gemm_a4",
         "p8": "parent W4A8: quantize_act + mx_gemm", "p6": "parent W4A6: quantize_act6 + mx_gemm_a6",
         "p4": "parent W4A4: quantize_act4 + mx_gemm_a4"}


def linear_rows(N, K, M, reps, parent=None):
    s = dev.stream_handle
    gen = torch.Generator(device="cuda").manual_seed(N + K + M)
    codes = torch.randint(0, 256, (N, K // 2), dtype=torch.uint8, device="cuda", generator=gen)
    codes &= 0x77  # (no -0: every nibble is one of the codes the packer writes)
    scales = torch.randint(118, 124, (N, K // 32), dtype=torch.uint8, device="cuda", generator=gen)
    x = torch.randn((M, K), device="cuda", generator=gen).to(torch.bfloat16)
    ac = {name: torch.empty((M, K * bits // 8), dtype=torch.uint8, device="cuda") for name, bits in BITS.items()}
    asc = torch.empty((M, K // 32), dtype=torch.uint8, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    y = torch.empty((M, N), dtype=torch.bfloat16, device="cuda")

    def side(lib, quantize, gemm, a):
        quantize, gemm = getattr(lib, quantize), getattr(lib, gemm)

        def run():
            _lib.check(quantize(dev.ptr(x), _lib.DTYPE_BF16, M, K, dev.ptr(a), dev.ptr(asc), dev.ptr(flag), s()))
            _lib.check(gemm(dev.ptr(a), dev.ptr(asc), dev.ptr(codes), dev.ptr(scales), None, M, N, K, _lib.DTYPE_BF16, dev.ptr(y), s()))
        return run

    sides = [("a8", side(L, "slk_mx_quantize_act", "slk_mx_gemm", ac["a8"])),
             ("a6", side(L, "slk_mx_quantize_act6", "slk_mx_gemm_a6", ac["a6"])),
             ("a4", side(L, "slk_mx_quantize_act4", "slk_mx_gemm_a4", ac["a4"]))]
    if parent is not None:
        sides += [("p8", side(parent, "slk_mx_quantize_act", "slk_mx_gemm", ac["a8"])),
                  ("p6", side(parent, "slk_mx_quantize_act6", "slk_mx_gemm_a6", ac["a6"])),
                  ("p4", side(parent, "slk_mx_quantize_act4", "slk_mx_gemm_a4", ac["a4"]))]
    ts = timed([fn for _, fn in sides] * 2, reps)
    first, second = ts[:len(sides)], ts[len(sides):]
    w_bytes = N * K // 2 + N * K // 32
    flops = 2.0 * M * N * K
    out = {}
    for (name, _), t, t2 in zip(sides, first, second):
        fmt = "a" + name[1]
        # x read, codes and scale bytes written and read again, the layer, y
        nbytes = w_bytes + 2 * M * K + 2 * (M * K * BITS[fmt] // 8 + M * K // 32) + 2 * M * N
        t_hbm, t_mfma = nbytes / HBM * 1e6, flops / PEAK[fmt] * 1e6
        out[name] = (t, t2)
        print(json.dumps(dict(bench="linear", size=f"{N}x{K}", M=M, side=NAMES[name], **stats(t), repeat_us=round(t2[0], 1), bytes=int(nbytes),
                              share_of_hbm=round(t_hbm / t[0], 3), tflops=round(flops / t[0] * 1e-6, 1),
                              share_of_mfma_peak=round(t_mfma / t[0], 4), bound="hbm" if t_hbm >= t_mfma else "mfma")), flush=True)
    (t8, t8b), (t6, t6b), (t4, t4b) = out["a8"], out["a6"], out["a4"]
    spread = max(abs(a[0] - b[0]) for a, b in out.values())
    print(json.dumps(dict(bench="linear", size=f"{N}x{K}", M=M, side="W4A4 against W4A8", a8_over_a4=round(t8[0] / t4[0], 3),
                          a4_median_within_a8_range=bool(max(t4[0], t4b[0]) <= max(t8[2], t8b[2])), spread_us=round(spread, 1))), flush=True)
    print(json.dumps(dict(bench="linear", size=f"{N}x{K}", M=M, side="W4A6 against W4A8 and W4A4", a8_over_a6=round(t8[0] / t6[0], 3),
                          a6_over_a4=round(t6[0] / t4[0], 3), a6_median_at_or_below_a8=bool(max(t6[0], t6b[0]) <= min(t8[0], t8b[0])),
                          a6_median_within_a8_range=bool(min(t8[1], t8b[1]) <= min(t6[0], t6b[0]) and max(t6[0], t6b[0]) <= max(t8[2], t8b[2])),
                          spread_us=round(spread, 1))), flush=True)
    for here, there in (("a8", "p8"), ("a6", "p6"), ("a4", "p4")):
        if there in out:
            print(json.dumps(dict(bench="linear", size=f"{N}x{K}", M=M, side=f"{NAMES[here][:4]} against the parent's",
                                  **against_parent(out[here], out[there]))), flush=True)


def against_parent(this, parent):
    """This library's two (median, min, max) against the parent's two, as the fields of a comparison row."""
    (t, tb), (p, pb) = this, parent
    lo, hi = min(p[1], pb[1]), max(p[2], pb[2])
    return dict(this_us=round(t[0], 1), this_repeat_us=round(tb[0], 1), parent_us=round(p[0], 1), parent_repeat_us=round(pb[0], 1),
                parent_min_us=round(lo, 1), parent_max_us=round(hi, 1), this_over_parent=round(t[0] / p[0], 3),
                parent_spread=round(abs(p[0] - pb[0]) / p[0], 3),
                this_median_within_parent_range=bool(lo <= min(t[0], tb[0]) and max(t[0], tb[0]) <= hi))


def quantize_rows(M, K, reps, parent):
    """Each plain quantizer and each activation de-quantizer alone, this library against the parent's."""
    s = dev.stream_handle
    gen = torch.Generator(device="cuda").manual_seed(M + K)
    x = torch.randn((M, K), device="cuda", generator=gen).to(torch.bfloat16)
    asc = torch.empty((M, K // 32), dtype=torch.uint8, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    back = torch.empty((M, K), dtype=torch.bfloat16, device="cuda")
    for what, bits, quantize, dequantize in (("mxfp8", 8, "slk_mx_quantize_act", "slk_mx_dequantize_act"),
                                             ("mxfp6_e2m3", 6, "slk_mx_quantize_act6", "slk_mx_dequantize_act6"),
                                             ("mxfp4", 4, "slk_mx_quantize_act4", None)):
        a = torch.empty((M, K * bits // 8), dtype=torch.uint8, device="cuda")

        def forth(lib):
            return lambda: _lib.check(getattr(lib, quantize)(dev.ptr(x), _lib.DTYPE_BF16, M, K, dev.ptr(a), dev.ptr(asc), dev.ptr(flag), s()))

        def and_back(lib):
            return lambda: _lib.check(getattr(lib, dequantize)(dev.ptr(a), dev.ptr(asc), M, K, _lib.DTYPE_BF16, dev.ptr(back), dev.ptr(flag), s()))

        for entry, side in ((quantize, forth), (dequantize, and_back)):
            if entry is None:  # (MXFP4 activations are de-quantized by the layer's own slk_mx_dequantize)
                continue
            this, there, this2, there2 = timed([side(L), side(parent)] * 2, reps)
            nbytes = 2 * M * K + M * K * bits // 8 + M * K // 32
            print(json.dumps(dict(bench="quantize", shape=f"{M}x{K}", fmt=what, side=f"{entry} against the parent's", **stats(this), bytes=nbytes,
                                  share_of_hbm=round(nbytes / HBM * 1e6 / this[0], 3), **against_parent((this, this2), (there, there2)))),
                  flush=True)


def fused_rows(rows, n, block, reps, parent=None):
    s = dev.stream_handle
    gen = torch.Generator(device="cuda").manual_seed(rows + n)
    x = torch.randn((rows, n), device="cuda", generator=gen).to(torch.bfloat16)
    rot = rotation.Rotation(n, block=block, seed=1)
    yf = torch.empty((rows, n), dtype=torch.float32, device="cuda")
    c8 = torch.empty((rows, n), dtype=torch.uint8, device="cuda")
    c4 = torch.empty((rows, n // 2), dtype=torch.uint8, device="cuda")
    c6 = torch.empty((rows, 3 * n // 4), dtype=torch.uint8, device="cuda")
    sc = torch.empty((rows, n // 32), dtype=torch.uint8, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")

    plain = {"mxfp8": (L.slk_mx_quantize_act, c8), "mxfp6_e2m3": (L.slk_mx_quantize_act6, c6), "mxfp4": (L.slk_mx_quantize_act4, c4)}

    def two(fmt):
        quantize, c = plain[fmt]

        def run():
            _lib.check(L.slk_hadamard_rows(dev.ptr(x), _lib.DTYPE_BF16, dev.ptr(yf), _lib.DTYPE_F32, rows, n, block, dev.ptr(rot.signs), 0, s()))
            _lib.check(quantize(dev.ptr(yf), _lib.DTYPE_F32, rows, n, dev.ptr(c), dev.ptr(sc), dev.ptr(flag), s()))
        return run

    def one(fmt, lib=L):
        def run():
            if fmt == "mxfp6_e2m3":
                _lib.check(lib.slk_mx_rotate_quantize_act6(dev.ptr(x), _lib.DTYPE_BF16, rows, n, block, dev.ptr(rot.signs), dev.ptr(c6), dev.ptr(sc),
                                                         dev.ptr(flag), s()))
            else:
                fp4 = fmt == "mxfp4"
                _lib.check(lib.slk_mx_rotate_quantize_act(dev.ptr(x), _lib.DTYPE_BF16, rows, n, block, dev.ptr(rot.signs),
                                                          _lib.MX_ACT_FP4 if fp4 else _lib.MX_ACT_FP8, dev.ptr(c4 if fp4 else c8), dev.ptr(sc),
                                                          dev.ptr(flag), s()))
        return run

    for fmt, bits in (("mxfp8", 8), ("mxfp6_e2m3", 6), ("mxfp4", 4)):
        t_two, t_one, t_two2, t_one2 = timed([two(fmt), one(fmt)] * 2, reps)
        e = rows * n
        code_bytes = e * bits // 8
        b_two = 2 * e + 4 * e + 4 * e + code_bytes + e // 32
        b_one = 2 * e + code_bytes + e // 32
        print(json.dumps(dict(bench="fused", shape=f"{rows}x{n}", block=block, fmt=fmt, side="two steps: hadamard_rows float32 + quantize",
                              **stats(t_two), repeat_us=round(t_two2[0], 1), bytes=b_two, share_of_hbm=round(b_two / HBM * 1e6 / t_two[0], 3))), flush=True)
        print(json.dumps(dict(bench="fused", shape=f"{rows}x{n}", block=block, fmt=fmt, side="fused: mx_rotate_quantize_act" + ("6" if bits == 6 else ""),
                              **stats(t_one), repeat_us=round(t_one2[0], 1), bytes=b_one, share_of_hbm=round(b_one / HBM * 1e6 / t_one[0], 3),
                              two_over_one=round(t_two[0] / t_one[0], 2),
                              median_below_two_steps_min=bool(max(t_one[0], t_one2[0]) < min(t_two[1], t_two2[1])))), flush=True)
        if parent is not None:  # the fused kernel alone, this library and the parent's alternating, each side twice
            this, there, this2, there2 = timed([one(fmt), one(fmt, parent)] * 2, reps)
            print(json.dumps(dict(bench="fused", shape=f"{rows}x{n}", block=block, fmt=fmt, side="fused against the parent's",
                                  **against_parent((this, this2), (there, there2)))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--m", default="1,16,256,4096")
    ap.add_argument("--only", choices=("linear", "fused", "quantize"), default=None)
    ap.add_argument("--parent-lib", default=None, help="a libsleekit_amd.so built from another commit: its W4A8, W4A6 and W4A4 join the rotation")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "micro_mx_act measures the MI355X; there is no CPU path"
    torch.cuda.set_device(0)
    parent = load_library(args.parent_lib) if args.parent_lib else None
    if args.only in (None, "linear"):
        for N, K in ((4096, 4096), (4096, 11008)):
            for M in (int(m) for m in args.m.split(",")):
                linear_rows(N, K, M, args.reps, parent)
                torch.cuda.empty_cache()
    if args.only in (None, "fused"):
        fused_rows(4096, 4096, 4096, args.reps, parent)
    if args.only == "quantize" or (args.only is None and parent is not None):
        assert parent is not None, "--only quantize compares against --parent-lib"
        quantize_rows(4096, 11008, args.reps, parent)


if __name__ == "__main__":
    main()
