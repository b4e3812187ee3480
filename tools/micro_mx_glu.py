#!/usr/bin/env python3
"""The fused gated MX MLP against the five-step route it replaces, on the MI355X.

    python tools/micro_mx_glu.py [--reps 20] [--models gpt-oss,llama-7b] [--m 1,16,256,4096] [--t 16,64,8192] [--e 32,128] [--pair a8w4]
                                 [--down-block 32]

A gated MLP down(act(gate(x)) * up(x)): gpt-oss (K = 2880, N = 2880 hidden columns, gate and up interleaved, alpha = 1.702,
limit = 7, shift = 1), dense at M rows and as E experts with T tokens routed uniformly to k = 4 experts each (M = 4 T sorted
rows), and Llama-7B (K = 4096, N = 11008, SwiGLU, not interleaved), dense.  x and the result are bfloat16.  Every side is a
Python call, timed with device events (median of `reps` after a warm-up, with [min, max]); the sides alternate call by call in
one process, and the five-step route is in the rotation twice: the difference of its two medians is the run-to-run spread.

  (a) fused:     mx.gated_mlp_mx / MXExpertsMLP.forward -- the quantizer, the fused gate/up product, the down product
  (b) five-step: linear_mx* to bfloat16, the gate as torch operations on the (M, 2 N) matrix, linear_mx* again (its quantizer
                 inside): what a user ran before
  (c) unfused:   (a) with fused=False -- the up product to float32, slk_mx_glu, the plain quantizer, the down product

(b) rounds the hidden activations twice (to bfloat16, then onto the MX grid), so its result is not (a)'s bit for bit; (a) and
(c) are checked to agree before anything is timed.  One JSON line per row.

--down-block B puts the down layer behind a Rotation of the N hidden features with that block (down_rotation=).  Up to 32 the
fused product rotates h in its epilogue (slk_mx_gemm_glu_rot), and (c), fused=False, is the route such a call took before
that kernel: the up product to float32, slk_mx_glu, the rotating quantizer.  The rows then time (a) against (c), with (c) in
the rotation twice for the spread; (b) has no rotation to compare and is left out.
"""

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from sleekit_amd import mx  # noqa: E402
from sleekit_amd.rotation import Rotation  # noqa: E402

K_TOP = 4
MODELS = {"gpt-oss": dict(K=2880, N=2880, out=2880, gate=dict(alpha=1.702, limit=7.0, shift=1.0, interleaved=True)),
          "llama-7b": dict(K=4096, N=11008, out=4096, gate=dict(alpha=1.0, limit=None, shift=0.0, interleaved=False))}
PAIRS = {"a8w4": "mxfp8", "a4w4": "mxfp4", "a6w4": "mxfp6_e2m3"}


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


def layer(lead, rows, K, gen):
    codes = torch.randint(0, 256, lead + (rows, K // 2), dtype=torch.uint8, device="cuda", generator=gen)
    codes &= 0x77  # (no -0: every nibble is one of the codes the packer writes)
    return codes, torch.randint(118, 124, lead + (rows, K // 32), dtype=torch.uint8, device="cuda", generator=gen)


def torch_gate(y, alpha, limit, shift, interleaved):
    """The gate as a user writes it in torch, on the bfloat16 (M, 2 N) matrix."""
    N = y.shape[-1] // 2
    g, u = (y[..., 0::2], y[..., 1::2]) if interleaved else (y[..., :N], y[..., N:])
    if limit is not None:
        g, u = g.clamp(max=limit), u.clamp(-limit, limit)
    return (u + shift) * (g * torch.sigmoid(alpha * g))


def report(what, M, pair, ts, flops, **more):
    (a, b, c, b2) = ts
    spread = abs(b[0] - b2[0])
    us = lambda t: [round(v, 1) for v in t]  # noqa: E731
    print(json.dumps(dict(model=what, M=M, pair=pair, **more, fused_us=us(a), five_step_us=us(b), five_step_again_us=us(b2), unfused_us=us(c),
                          spread_us=round(spread, 1), five_step_over_fused=round(b[0] / a[0], 2), unfused_over_fused=round(c[0] / a[0], 2),
                          faster=bool(a[0] + spread < min(b[0], b2[0])), tflops=round(flops / a[0] * 1e-6, 1))), flush=True)


def report_rotated(what, M, pair, block, ts, flops, **more):
    (a, c, c2) = ts
    spread = abs(c[0] - c2[0])
    us = lambda t: [round(v, 1) for v in t]  # noqa: E731
    print(json.dumps(dict(model=what, M=M, pair=pair, down_block=block, **more, fused_us=us(a), unfused_us=us(c), unfused_again_us=us(c2),
                          spread_us=round(spread, 1), unfused_over_fused=round(min(c[0], c2[0]) / a[0], 2),
                          faster=bool(a[0] + spread < min(c[0], c2[0])), tflops=round(flops / a[0] * 1e-6, 1))), flush=True)


def dense(name, M, pair, reps, block=0):
    spec, act = MODELS[name], PAIRS[pair]
    K, N, out, gate = spec["K"], spec["N"], spec["out"], spec["gate"]
    gen = torch.Generator(device="cuda").manual_seed(M + K + N)
    (uc, us), (dc, ds) = layer((), 2 * N, K, gen), layer((), out, N, gen)
    x = torch.randn((M, K), device="cuda", generator=gen).bfloat16()
    kw = dict(activations=act, **gate)

    def fused():
        return mx.gated_mlp_mx(x, uc, us, dc, ds, **kw)

    def unfused():
        return mx.gated_mlp_mx(x, uc, us, dc, ds, fused=False, **kw)

    def five_step():
        y = mx.linear_mxfp4(x, uc, us, activations=act)
        return mx.linear_mxfp4(torch_gate(y, **gate), dc, ds, activations=act)

    if block:
        kw["down_rotation"] = Rotation(N, block=block, seed=1)
    assert torch.equal(fused().view(torch.int16), unfused().view(torch.int16)), "fused and unfused disagree"
    flops = 2.0 * M * K * 2 * N + 2.0 * M * N * out
    if block:
        report_rotated(name, M, pair, block, timed([fused, unfused, unfused], reps), flops)
    else:
        report(name, M, pair, timed([fused, five_step, unfused, five_step], reps), flops)


def experts(name, E, T, pair, reps, layers, block=0):
    spec, act = MODELS[name], PAIRS[pair]
    K, N, out, gate = spec["K"], spec["N"], spec["out"], spec["gate"]
    M = K_TOP * T
    (uc, us), (dc, ds) = layers
    counts = np.random.default_rng(E + T).multinomial(M, np.full(E, 1.0 / E))
    offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)).cuda()
    x = torch.randn((M, K), device="cuda", generator=torch.Generator(device="cuda").manual_seed(E + T)).bfloat16()
    up, down = mx.MXExperts(E, K, 2 * N, bias=False, device="cuda", activations=act), mx.MXExperts(E, N, out, bias=False, device="cuda", activations=act)
    up.codes, up.scales, down.codes, down.scales = uc, us, dc, ds
    mlp = mx.MXExpertsMLP(up, down, **gate)
    rot = Rotation(N, block=block, seed=1) if block else None

    def fused():
        return mlp(x, offsets, down_rotation=rot)

    def unfused():
        return mlp(x, offsets, fused=False, down_rotation=rot)

    def five_step():
        y = mx.linear_mx_experts(x, uc, us, offsets, activations=act)
        return mx.linear_mx_experts(torch_gate(y, **gate), dc, ds, offsets, activations=act)

    assert torch.equal(fused().view(torch.int16), unfused().view(torch.int16)), "fused and unfused disagree"
    flops, more = 2.0 * M * K * 2 * N + 2.0 * M * N * out, dict(E=E, T=T, largest_expert=int(counts.max()))
    if block:
        report_rotated(name, M, pair, block, timed([fused, unfused, unfused], reps), flops, **more)
    else:
        report(name, M, pair, timed([fused, five_step, unfused, five_step], reps), flops, **more)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--models", default="gpt-oss,llama-7b")
    ap.add_argument("--m", default="1,16,256,4096")
    ap.add_argument("--t", default="16,64,8192")
    ap.add_argument("--e", default="32,128")
    ap.add_argument("--pair", default="a8w4")
    ap.add_argument("--down-block", type=int, default=0, help="the block of a down rotation (0: none)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "micro_mx_glu measures the MI355X; there is no CPU path"
    torch.cuda.set_device(0)
    ints = lambda s: [int(v) for v in s.split(",") if v]  # noqa: E731
    for name in args.models.split(","):
        for M in ints(args.m):
            dense(name, M, args.pair, args.reps, args.down_block)
        torch.cuda.empty_cache()
    if "gpt-oss" in args.models.split(","):
        spec = MODELS["gpt-oss"]
        for E in ints(args.e):
            gen = torch.Generator(device="cuda").manual_seed(E)
            layers = layer((E,), 2 * spec["N"], spec["K"], gen), layer((E,), spec["out"], spec["N"], gen)
            for T in ints(args.t):
                experts("gpt-oss", E, T, args.pair, args.reps, layers, args.down_block)
            del layers
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
