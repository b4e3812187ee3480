#!/usr/bin/env python3
"""The expert-grouped Hessian accumulation against the loop over experts it replaces, on the MI355X.

    python tools/micro_expert_stats.py [--reps 10] [--e 32,128] [--n 2880,4096] [--t 64,1024,8192] [--routing uniform,skewed]

The statistics of E experts of n features, T tokens routed to k = 4 experts each: M = 4 T rows sorted by expert.  Routing
"uniform" draws every row's expert uniformly; "skewed" puts half the rows on four experts and the rest uniformly on the
others.  Every side is timed with device events (median of `reps` after a warm-up, with [min, max]); the sides alternate call
by call in one process, and the loop is in the rotation twice: the difference of its two medians is the run-to-run spread.

  (a) slk_hessian_accumulate_experts: one call -- the prologue, the means, the split and the products
  (b) a loop of slk_hessian_accumulate over the experts that have rows, on slices made beforehand with the counts known to
      the host (not charged the device-to-host read a real router's counts would cost it), each with a workspace for all
      its tokens
  (c) slk_hessian_accumulate_experts_mx on the same rows as MXFP8 codes
  (d) what stood in for (c) before it: slk_mx_dequantize_act to float32, then (a)

Before timing, (a) and (b) from zero statistics are asserted equal bit for bit.  One JSON line per row; floor_us is the
traffic floor -- 8 n^2 bytes per expert with rows, plus the bytes of X -- at `--hbm` TB/s.
"""

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from sleekit_amd import _device as dev, _lib  # noqa: E402

L = _lib.lib
K_TOP = 4


def timed(fns, reps):
    """Median, min and max (us) of each of `fns`, called in turn `reps` times."""
    for _ in range(2):
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


def row(E, n, T, routing, H, H2, reps, hbm):
    s, P = dev.stream_handle, dev.ptr
    M = K_TOP * T
    counts = counts_of(np.random.default_rng(E + n + T), E, M, routing)
    host_offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    offsets = torch.from_numpy(host_offsets).cuda()
    gen = torch.Generator(device="cuda").manual_seed(E + n + T)
    X = torch.randn((M, n), dtype=torch.float32, device="cuda", generator=gen)
    ac = torch.randint(0, 256, (M, n), dtype=torch.uint8, device="cuda", generator=gen) & 0x77  # (no NaN, no -0)
    asc = torch.randint(118, 124, (M, n // 32), dtype=torch.uint8, device="cuda", generator=gen)
    Xd = torch.empty((M, n), dtype=torch.float32, device="cuda")
    mean, mean2 = torch.zeros((E, n), device="cuda"), torch.zeros((E, n), device="cuda")
    cnt, flag = torch.zeros(E, dtype=torch.int64, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda")
    ws_bytes = L.slk_hessian_experts_workspace_bytes(E, n, M)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    live = [e for e in range(E) if counts[e] > 0]
    one_bytes = 4096 + 6 * n * ((int(counts.max()) + 31) // 32 * 32)
    one_ws = torch.empty(one_bytes, dtype=torch.uint8, device="cuda")
    pieces = [(H2[e], mean2[e], X[host_offsets[e]:host_offsets[e + 1]], int(counts[e])) for e in live]
    seen = [0]

    def grouped():
        _lib.check(L.slk_hessian_accumulate_experts(P(H), P(mean), P(X), P(offsets), E, n, M, P(cnt), P(flag), P(ws), ws_bytes, s()))

    def loop():
        for h, m, x, t in pieces:
            _lib.check(L.slk_hessian_accumulate(P(h), P(m), P(x), n, t, seen[0] * t, P(one_ws), one_bytes, s()))
        seen[0] += 1

    def coded():
        _lib.check(L.slk_hessian_accumulate_experts_mx(P(H), P(mean), P(ac), P(asc), _lib.MX_ACT_FP8, P(offsets), E, n, M, P(cnt), P(flag), P(ws),
                                                       ws_bytes, s()))

    def decoded():
        _lib.check(L.slk_mx_dequantize_act(P(ac), P(asc), M, n, _lib.DTYPE_F32, P(Xd), None, s()))
        _lib.check(L.slk_hessian_accumulate_experts(P(H), P(mean), P(Xd), P(offsets), E, n, M, P(cnt), P(flag), P(ws), ws_bytes, s()))

    H.zero_(), H2.zero_()
    grouped()
    loop()
    torch.cuda.synchronize()
    assert flag.tolist() == [0, 0] and cnt.tolist() == counts.tolist(), "the prologue disagrees with the host's counts"
    assert torch.equal(H.view(torch.int32), H2.view(torch.int32)) and torch.equal(mean.view(torch.int32), mean2.view(torch.int32)), \
        "the grouped call and the loop disagree"
    t_a, t_b, t_c, t_d, t_b2 = timed([grouped, loop, coded, decoded, loop], reps)
    spread = abs(t_b[0] - t_b2[0])
    floor_bytes = 8.0 * n * n * len(live) + 4.0 * M * n
    floor_coded = 8.0 * n * n * len(live) + 33.0 / 32.0 * M * n

    def us(t):
        return [round(v, 1) for v in t]

    print(json.dumps(dict(
        E=E, n=n, T=T, M=M, routing=routing, experts_with_rows=len(live), largest_expert=int(counts.max()),
        path="bf16x3" if n % 128 == 0 else "f32", grouped_us=us(t_a), loop_us=us(t_b), loop_again_us=us(t_b2), spread_us=round(spread, 1),
        loop_over_grouped=round(t_b[0] / t_a[0], 2), faster=bool(t_a[0] + spread < min(t_b[0], t_b2[0])),
        coded_us=us(t_c), decoded_us=us(t_d), decoded_over_coded=round(t_d[0] / t_c[0], 2),
        floor_us=round(floor_bytes / hbm * 1e6, 1), coded_floor_us=round(floor_coded / hbm * 1e6, 1))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--e", default="32,128")
    ap.add_argument("--n", default="2880,4096")
    ap.add_argument("--t", default="64,1024,8192")
    ap.add_argument("--routing", default="uniform,skewed")
    ap.add_argument("--hbm", type=float, default=8.0, help="TB/s the traffic floor is taken at (MI355X: 8 TB/s peak)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "micro_expert_stats measures the MI355X; there is no CPU path"
    torch.cuda.set_device(0)
    for E in (int(e) for e in args.e.split(",")):
        for n in (int(v) for v in args.n.split(",")):
            H = torch.zeros((E, n, n), dtype=torch.float32, device="cuda")
            H2 = torch.zeros((E, n, n), dtype=torch.float32, device="cuda")
            for T in (int(t) for t in args.t.split(",")):
                for routing in args.routing.split(","):
                    row(E, n, T, routing, H, H2, args.reps, args.hbm * 1e12)
            del H, H2
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
