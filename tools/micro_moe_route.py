#!/usr/bin/env python3
"""The MoE route in HIP (forward_logits) against the route a user ran before it, written out in torch ops, on the MI355X.

    python tools/micro_moe_route.py [--reps 20] [--e 32,128] [--t 1,16,64,1024,8192] [--pairs a4w4,a8w4] [--shapes 2880x2880,5760x2880]

A mixture-of-experts layer of E experts N x K in MXFP4, T tokens (bfloat16) routed to k = 4 experts each by float32 router
logits.  The two sides alternate call by call in one process and are timed with device events (median of `reps` after a
warm-up, with [min, max]); before any timing the new route's output is held to the old route's bit for bit, on the new
route's ids and gates.

  new:  MXExperts.forward_logits -- slk_moe_topk, slk_moe_sort, slk_mx_quantize_act_rows, slk_mx_gemm_experts, slk_moe_combine
  old:  torch.topk and a softmax over the selected logits, then what MXExperts.forward_tokens did with them before the
        routing kernels existed, inlined here: any / clamp / stable sort / searchsorted, x[order // k], the plain quantizer,
        the grouped product, the inverse permutation by an index-put, y[back].float() and k multiplies and adds
  and three pieces of each side alone, on preallocated inputs and with no flag read:
  routing  logits -> ids, gates, order, (pos,) offsets
  quantize the routed rows of x -> a_codes, a_scales (old: gather, then quantize)
  combine  y (T k, N) -> out (T, N)
  `py_*` is the whole call as Python sees it: host clock around the call, which ends in the read of its flags.

One JSON line per row.  Nothing here is a pass condition but the equality of the bits.
"""

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from sleekit_amd import mx, routing  # noqa: E402

K_TOP = 4
PAIRS = {"a8w4": "mxfp8", "a4w4": "mxfp4"}


def timed(fns, reps):
    """Median, min and max (us) of each of `fns`, called in turn `reps` times: device events."""
    for _ in range(3):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts[i].append(a.elapsed_time(b) * 1e3)
    return [[round(v, 1) for v in (sorted(t)[len(t) // 2], min(t), max(t))] for t in ts]


def wall(fns, reps):
    """Median host time (us) of each of `fns` as a call that ends synchronised."""
    ts = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts[i].append((time.perf_counter() - t0) * 1e6)
    return [round(sorted(t)[len(t) // 2], 1) for t in ts]


def old_routing(logits, E):
    top = torch.topk(logits, K_TOP, dim=1)
    gates = torch.softmax(top.values, dim=1)
    return (top.indices, gates) + mx._sorted_by_expert(top.indices.reshape(-1), E)


def old_combine(y, order, gates, T):
    back = torch.empty_like(order)
    back[order] = torch.arange(order.numel(), device=order.device)
    y = y[back].reshape(T, K_TOP, -1).float()
    total = y[:, 0] * gates[:, 0:1]
    for j in range(1, K_TOP):
        total = total + y[:, j] * gates[:, j:j + 1]
    return total.to(torch.bfloat16)


def old_route(experts, x, ids, gates):
    """MXExperts.forward_tokens before the routing kernels: torch ops around the quantizer and the grouped product."""
    E, T = experts.num_experts, x.shape[0]
    order, offsets, bad = mx._sorted_by_expert(ids.reshape(-1).long(), E)
    y = mx._linear_experts(x[order // K_TOP], experts.codes, experts.scales, offsets, experts.bias, None, experts.activations, None,
                           mx._WEIGHTS[experts.weights], also=((bad, mx._ids_message(E)),))
    return old_combine(y, order, gates, T)


def row(experts, E, N, K, T, pair, reps):
    fmt = mx._FORMATS[PAIRS[pair]]
    gen = torch.Generator(device="cuda").manual_seed(E + N + K + T)
    x = torch.randn((T, K), device="cuda", generator=gen).to(torch.bfloat16)
    logits = torch.randn((T, E), device="cuda", generator=gen)
    n = T * K_TOP
    r = routing.route_topk(logits, K_TOP)
    new = experts.forward_logits(x, logits, K_TOP)
    assert torch.equal(new.view(torch.int16), old_route(experts, x, r.expert_ids, r.gates).view(torch.int16)), "the two routes disagree"
    ids_as_torch = torch.equal(r.expert_ids.long(), torch.topk(logits, K_TOP, dim=1).indices)  # (False only on a tie among random floats)
    order64 = r.order.long()
    y = torch.randn((n, N), device="cuda", generator=gen).to(torch.bfloat16)

    def whole_new():
        experts.forward_logits(x, logits, K_TOP)

    def whole_old():
        ids, gates, _, _, _ = old_routing(logits, E)
        old_route(experts, x, ids, gates)

    def routing_new():
        ids, _, _ = routing._topk(logits, T, E, K_TOP, "selected")
        routing._sort(ids.reshape(-1), n, E)

    def quantize_new():
        routing._quantize_rows(x, T, K, r.order, K_TOP, n, fmt.c_fmt, fmt.bits)

    def quantize_old():
        mx._quantize_act(x[order64 // K_TOP], n, K, fmt)

    def combine_new():
        routing._combine(y, r.pos, r.gates, T, K_TOP, N, torch.bfloat16)

    names = ["whole_new", "whole_old", "routing_new", "routing_old", "quantize_new", "quantize_old", "combine_new", "combine_old", "whole_old_again"]
    fns = [whole_new, whole_old, routing_new, lambda: old_routing(logits, E), quantize_new, quantize_old, combine_new,
           lambda: old_combine(y, order64, r.gates, T), whole_old]
    out = dict(zip((f"{name}_us" for name in names), timed(fns, reps)))
    py_new, py_old = wall([whole_new, whole_old], reps)
    print(json.dumps(dict(E=E, size=f"{N}x{K}", T=T, rows=n, pair=pair, ids_as_torch=ids_as_torch, **out, py_new_us=py_new, py_old_us=py_old,
                          old_over_new=round(out["whole_old_us"][0] / out["whole_new_us"][0], 2),
                          spread_us=round(abs(out["whole_old_us"][0] - out["whole_old_again_us"][0]), 1))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--e", default="32,128")
    ap.add_argument("--t", default="1,16,64,1024,8192")
    ap.add_argument("--pairs", default="a4w4,a8w4")
    ap.add_argument("--shapes", default="2880x2880,5760x2880")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "micro_moe_route measures the MI355X; there is no CPU path"
    torch.cuda.set_device(0)
    for E in (int(e) for e in args.e.split(",")):
        for N, K in (tuple(int(v) for v in shape.split("x")) for shape in args.shapes.split(",")):
            for pair in args.pairs.split(","):
                gen = torch.Generator(device="cuda").manual_seed(E + N + K)
                experts = mx.MXExperts(E, K, N, bias=False, device="cuda", activations=PAIRS[pair])
                experts.codes.copy_(torch.randint(0, 256, experts.codes.shape, dtype=torch.uint8, device="cuda", generator=gen) & 0x77)  # (no -0)
                experts.scales.copy_(torch.randint(118, 124, experts.scales.shape, dtype=torch.uint8, device="cuda", generator=gen))
                for T in (int(t) for t in args.t.split(",")):
                    row(experts, E, N, K, T, pair, args.reps)
                del experts
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
