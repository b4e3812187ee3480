#!/usr/bin/env python3
"""The expert-grouped MX product against the loop over experts a user ran before it, on the MI355X.

    python tools/micro_mx_experts.py [--reps 20] [--e 32,128] [--t 16,64,1024,8192] [--pairs a8w4,a4w4] [--shapes 5760x2880,2880x2880]

A mixture-of-experts layer of E experts N x K (K % 128 != 0 on purpose), T tokens routed to k = 4 experts each: M = 4 T rows,
sorted by expert, activations quantized beforehand, bfloat16 out.  Routing "uniform" draws every row's expert uniformly;
"skewed" puts half the rows on four experts and the rest uniformly on the others.  Every side runs on preallocated outputs
and is timed with device events (median of `reps` after a warm-up, with [min, max]); the sides alternate call by call in
one process, and the loop is in the rotation twice: the difference of its two medians is the run-to-run spread the verdict
allows for.

  (a) slk_mx_gemm_experts: one call -- the prologue and one or two products; the offsets stay on the device
  (b) a loop of slk_mx_gemm (or _a4) over the experts that have rows, on operands sliced beforehand with the counts known to
      the host: the parent's way, not even charged the device-to-host read a real router's counts would cost it
  and both as Python calls: mx.matmul_mx_experts (its flag's read included) and a loop of mx.matmul_mx.

One JSON line per row; `faster` says whether (a) is below (b) by more than the spread of (b)'s two runs.
"""

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from sleekit_amd import _device as dev, _lib, mx  # noqa: E402

L = _lib.lib
K_TOP = 4
PAIRS = {"a8w4": ("mxfp8", 8, "slk_mx_gemm", _lib.MX_ACT_FP8), "a4w4": ("mxfp4", 4, "slk_mx_gemm_a4", _lib.MX_ACT_FP4)}


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


def counts_of(rng, E, M, routing):
    if routing == "uniform":
        return rng.multinomial(M, np.full(E, 1.0 / E))
    counts = np.zeros(E, np.int64)
    counts[:4] = rng.multinomial(M // 2, np.full(4, 0.25))
    counts[4:] = rng.multinomial(M - M // 2, np.full(E - 4, 1.0 / (E - 4)))
    return counts


def layer(E, N, K, gen):
    codes = torch.randint(0, 256, (E, N, K // 2), dtype=torch.uint8, device="cuda", generator=gen)
    codes &= 0x77  # (no -0: every nibble is one of the codes the packer writes)
    return codes, torch.randint(118, 124, (E, N, K // 32), dtype=torch.uint8, device="cuda", generator=gen)


def row(E, N, K, T, routing, pair, codes, scales, reps):
    name, a_bits, entry, a_fmt = PAIRS[pair]
    s, P = dev.stream_handle, dev.ptr
    M = K_TOP * T
    counts = counts_of(np.random.default_rng(E + N + T), E, M, routing)
    host_offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    offsets = torch.from_numpy(host_offsets).cuda()
    gen = torch.Generator(device="cuda").manual_seed(E + N + K + T)
    ac = torch.randint(0, 256, (M, K * a_bits // 8), dtype=torch.uint8, device="cuda", generator=gen) & 0x77  # (no NaN, no -0)
    asc = torch.randint(118, 124, (M, K // 32), dtype=torch.uint8, device="cuda", generator=gen)
    y = torch.empty((M, N), dtype=torch.bfloat16, device="cuda")
    y2 = torch.empty((M, N), dtype=torch.bfloat16, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    ws_bytes = L.slk_mx_experts_workspace_bytes(E, M)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    # the loop's operands, sliced beforehand (views: no copies)
    live = [e for e in range(E) if counts[e] > 0]
    pieces = [(ac[host_offsets[e]:host_offsets[e + 1]], asc[host_offsets[e]:host_offsets[e + 1]], codes[e], scales[e],
               y2[host_offsets[e]:host_offsets[e + 1]], int(counts[e])) for e in live]
    loop_fn = getattr(L, entry)

    def experts_c():
        _lib.check(L.slk_mx_gemm_experts(P(ac), P(asc), P(codes), P(scales), None, P(offsets), E, M, N, K, a_fmt, _lib.MX_W_FP4, _lib.DTYPE_BF16,
                                         P(y), P(flag), P(ws), ws_bytes, s()))

    def loop_c():
        for a, asl, c, sc, out, m in pieces:
            _lib.check(loop_fn(P(a), P(asl), P(c), P(sc), None, m, N, K, _lib.DTYPE_BF16, P(out), s()))

    def experts_py():
        mx.matmul_mx_experts(ac, asc, codes, scales, offsets, dtype=torch.bfloat16, activations=name)

    def loop_py():
        for a, asl, c, sc, _, _ in pieces:
            mx.matmul_mx(a, asl, c, sc, dtype=torch.bfloat16, activations=name)

    experts_c()
    loop_c()
    torch.cuda.synchronize()
    assert int(flag.item()) == 0 and torch.equal(y.view(torch.int16), y2.view(torch.int16)), "the two sides disagree"
    t_a, t_b, t_apy, t_bpy, t_b2, t_bpy2 = timed([experts_c, loop_c, experts_py, loop_py, loop_c, loop_py], reps)
    spread, spread_py = abs(t_b[0] - t_b2[0]), abs(t_bpy[0] - t_bpy2[0])

    def us(t):
        return [round(v, 1) for v in t]

    print(json.dumps(dict(
        E=E, size=f"{N}x{K}", T=T, M=M, routing=routing, pair=pair, experts_with_rows=len(live), largest_expert=int(counts.max()),
        experts_us=us(t_a), loop_us=us(t_b), loop_again_us=us(t_b2), spread_us=round(spread, 1), loop_over_experts=round(t_b[0] / t_a[0], 2),
        faster=bool(t_a[0] + spread < min(t_b[0], t_b2[0])),
        py_experts_us=us(t_apy), py_loop_us=us(t_bpy), py_loop_again_us=us(t_bpy2), py_spread_us=round(spread_py, 1),
        py_loop_over_experts=round(t_bpy[0] / t_apy[0], 2), py_faster=bool(t_apy[0] + spread_py < min(t_bpy[0], t_bpy2[0])),
        tflops=round(2.0 * M * N * K / t_a[0] * 1e-6, 1))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--e", default="32,128")
    ap.add_argument("--t", default="16,64,1024,8192")
    ap.add_argument("--pairs", default="a8w4,a4w4")
    ap.add_argument("--shapes", default="5760x2880,2880x2880")
    ap.add_argument("--routing", default="uniform,skewed")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "micro_mx_experts measures the MI355X; there is no CPU path"
    torch.cuda.set_device(0)
    for E in (int(e) for e in args.e.split(",")):
        for N, K in (tuple(int(v) for v in shape.split("x")) for shape in args.shapes.split(",")):
            codes, scales = layer(E, N, K, torch.Generator(device="cuda").manual_seed(E + N + K))
            for T in (int(t) for t in args.t.split(",")):
                for routing in args.routing.split(","):
                    for pair in args.pairs.split(","):
                        row(E, N, K, T, routing, pair, codes, scales, args.reps)
            del codes, scales
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
