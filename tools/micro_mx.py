#!/usr/bin/env python3
"""MXFP4: kernel times and HBM rates of the scale search, pack, unpack and dequantize, on the MI355X.

    python tools/micro_mx.py [--reps 20] [--no-layer] [--fp6] [--parent-lib libsleekit_amd.so]

Sizes: 4096 x 4096 and 4096 x 11008.  Each C entry is timed alone on preallocated outputs with device events (median of
`reps` after a warm-up; min and max are printed as the spread), the two sides of a comparison alternating call by call.
Bytes are what the call must move, computed from the shapes.  Share of peak: the rate over the 6.3 TB/s that
MI355X_MICROARCH.md measured as achievable for HBM.

  scale search   slk_mx_scale_search (mse, diag) against the route that was there before it -- slk_scale_search_grouped with
                 the same power-of-two base and the four factors -- results compared bit for bit first; and against its own
                 "max" mode, which reads W once and computes next to nothing: one streaming read of W.
  dequantize     slk_mx_dequantize against slk_dequantize_packed at 4 bits with float32 scales of group 32 (NF4 table).
  pack / unpack  slk_mx_pack / slk_mx_unpack against slk_pack_indices / slk_unpack_indices at 4 bits.
  layer          quantize_mxfp4 (scales, loop, pack) against groups.quantize_grouped with NF4, g = 32, given S, at 4096 x 4096
                 (host clock around a device synchronise), and its parts.
--fp6: the MXFP6 (E2M3) entries against their MXFP4 twins instead, alternating call by call -- slk_mx_scale_search6 against
slk_mx_scale_search (mse, diag), slk_mx_pack6 / slk_mx_unpack6 against slk_mx_pack / slk_mx_unpack, and at 4096 x 4096 a
whole quantize_mxfp6 against quantize_mxfp4 (the loop's search over 63 entries is two levels deeper than over 15).
--parent-lib (a library built from another commit): only the converters, each against that library's -- slk_mx_pack, _unpack,
_pack6, _unpack6, slk_mx_dequantize to float32, bfloat16 and float16, slk_mx_dequantize_act6 and _act to bfloat16 -- the two
libraries alternating call by call, each side twice (micro_mx_act.py's loader and comparison row).  `passes`: both medians of
this library at or below the parent's largest time, or the ratio of the first medians at most 1 + the parent's own spread.
One JSON line per row.
"""

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from sleekit_amd import _device as dev, _lib, engine, groups, mx, packing, synth  # noqa: E402
from sleekit_amd.codebook import Codebook  # noqa: E402

from micro_mx_act import against_parent, load_library, timed  # noqa: E402

HBM = 6.3e12  # bytes/s
L = _lib.lib


def timed_pair(fns, reps):
    """Median, min and max (us) of each of `fns`, called in turn `reps` times."""
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


def row(size, what, t, nbytes, **extra):
    us, lo, hi = t
    rate = nbytes / (us * 1e-6)
    out = dict(size=size, kernel=what, us=round(us, 1), min_us=round(lo, 1), max_us=round(hi, 1), bytes=int(nbytes),
               tb_s=round(rate / 1e12, 3), share_of_hbm=round(rate / HBM, 3), **extra)
    print(json.dumps(out), flush=True)
    return out


def scale_rows(size, W, H, reps):
    R, n = W.shape
    G = n // 32
    s = dev.stream_handle
    hd = H.diagonal().contiguous()
    E = torch.empty((R, G), dtype=torch.uint8, device="cuda")
    S = torch.empty((R, G), dtype=torch.float32, device="cuda")
    base = torch.empty((R, G), dtype=torch.float32, device="cuda")
    old = torch.empty((R, G), dtype=torch.float32, device="cuda")
    levels, lo, hi, table = engine.require_uniform(mx.E2M1)
    factors = torch.tensor([0.125, 0.25, 0.5, 1.0], device="cuda")
    run_max = lambda: _lib.check(L.slk_mx_scale_search(dev.ptr(W), None, _lib.MX_MAX, R, n, dev.ptr(E), dev.ptr(base), s()))  # noqa: E731
    run_max()
    nbytes = 4 * R * n + 5 * R * G
    t_max = None
    for mode, code, h in (("mse", _lib.MX_MSE, None), ("diag", _lib.MX_DIAG, hd)):
        new = lambda: _lib.check(L.slk_mx_scale_search(dev.ptr(W), dev.ptr(h), code, R, n, dev.ptr(E), dev.ptr(S), s()))  # noqa: E731
        was = lambda: _lib.check(L.slk_scale_search_grouped(dev.ptr(W), dev.ptr(base), dev.ptr(factors), 4, dev.ptr(h), 32, R, n,  # noqa: E731
                                                            levels, lo, hi, dev.ptr(table), dev.ptr(old), s()))
        new()
        was()
        same = bool(torch.equal(S.view(torch.int32), old.view(torch.int32)))
        t_new, t_was, t_max = timed_pair([new, was, run_max], reps)
        row(size, f"mx_scale_search {mode}", t_new, nbytes, equals_existing=same, speedup=round(t_was[0] / t_new[0], 1),
            times_one_read=round(t_new[0] / t_max[0], 2))
        row(size, f"scale_search_grouped {mode} (4 factors, base given)", t_was, 4 * R * n + 8 * R * G)
    row(size, "mx_scale_search max (one read of W)", t_max, nbytes)


def pack_rows(size, R, n, reps):
    G = n // 32
    s = dev.stream_handle
    gen = torch.Generator(device="cuda").manual_seed(0)
    idx = torch.randint(0, 15, (R, n), dtype=torch.uint8, device="cuda", generator=gen)
    Eb = torch.randint(100, 140, (R, G), dtype=torch.uint8, device="cuda", generator=gen)
    S = mx.decode_scales(Eb)
    codes, scales = mx.pack_mxfp4(idx, S)
    nf4 = Codebook.nf4()
    levels, lo, hi, table = engine.require_uniform(nf4)
    P = packing.pack_indices(idx, 4)
    idx_out = torch.empty_like(idx)
    S_out = torch.empty_like(S)
    for dtype, code, osz in ((torch.float32, _lib.DTYPE_F32, 4), (torch.bfloat16, _lib.DTYPE_BF16, 2)):
        out = torch.empty((R, n), dtype=dtype, device="cuda")
        new = lambda: _lib.check(L.slk_mx_dequantize(dev.ptr(codes), dev.ptr(scales), R, n, code, dev.ptr(out), None, s()))  # noqa: E731
        was = lambda: _lib.check(L.slk_dequantize_packed(dev.ptr(P), R, n, 4, levels, lo, hi, dev.ptr(table), None, dev.ptr(S), None, 32,  # noqa: E731
                                                         code, dev.ptr(out), s()))
        t_new, t_was = timed_pair([new, was], reps)
        name = str(dtype)[6:]
        row(size, f"mx_dequantize {name}", t_new, R * n // 2 + R * G + osz * R * n, speedup=round(t_was[0] / t_new[0], 2))
        row(size, f"dequantize_packed {name} 4 bits, float32 scales g=32", t_was, R * n // 2 + 4 * R * G + osz * R * n)
        del out
    new = lambda: _lib.check(L.slk_mx_pack(dev.ptr(idx), dev.ptr(S), R, n, dev.ptr(codes), dev.ptr(scales), None, s()))  # noqa: E731
    was = lambda: _lib.check(L.slk_pack_indices(dev.ptr(idx), R, n, 4, dev.ptr(P), s()))  # noqa: E731
    t_new, t_was = timed_pair([new, was], reps)
    row(size, "mx_pack (codes and scale bytes)", t_new, R * n + R * n // 2 + 5 * R * G, speedup=round(t_was[0] / t_new[0], 2))
    row(size, "pack_indices 4 bits", t_was, R * n + R * n // 2)
    new = lambda: _lib.check(L.slk_mx_unpack(dev.ptr(codes), dev.ptr(scales), R, n, dev.ptr(idx_out), dev.ptr(S_out), None, s()))  # noqa: E731
    was = lambda: _lib.check(L.slk_unpack_indices(dev.ptr(P), R, n, 4, dev.ptr(idx_out), s()))  # noqa: E731
    t_new, t_was = timed_pair([new, was], reps)
    row(size, "mx_unpack (indices and float32 scales)", t_new, R * n + R * n // 2 + 5 * R * G, speedup=round(t_was[0] / t_new[0], 2))
    row(size, "unpack_indices 4 bits", t_was, R * n + R * n // 2)


def wall(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return dict(ms=round(ts[len(ts) // 2], 3), min_ms=round(ts[0], 3), max_ms=round(ts[-1], 3))


def layer_rows(W, H, reps):
    nf4 = Codebook.nf4()
    S_nf4 = groups.compute_group_scaling(W, nf4, 32, H, mode="max")
    S_mx = mx.compute_mx_scales(W, H, "mse")[0]
    rows = [
        ("quantize_mxfp4 (mse scales, loop, pack)", lambda: mx.quantize_mxfp4(W, H)),
        ("quantize_mxfp4 given scales (loop, pack)", lambda: mx.quantize_mxfp4(W, H, scales=S_mx)),
        ("quantize_grouped E2M1 g=32 given S (the loop alone)", lambda: groups.quantize_grouped(W, S_mx, mx.E2M1, H, 32, return_indices=True)),
        ("quantize_grouped NF4 g=32 given S", lambda: groups.quantize_grouped(W, S_nf4, nf4, H, 32, return_indices=True)),
        ("compute_mx_scales mse", lambda: mx.compute_mx_scales(W, H, "mse")),
    ]
    for name, fn in rows:
        print(json.dumps(dict(size="4096x4096", call=name, **wall(fn, reps))), flush=True)


def fp6_rows(size, W, H, reps, layer):
    R, n = W.shape
    G = n // 32
    s = dev.stream_handle
    hd = H.diagonal().contiguous()
    E = torch.empty((R, G), dtype=torch.uint8, device="cuda")
    S = torch.empty((R, G), dtype=torch.float32, device="cuda")
    for mode, code, h in (("mse", _lib.MX_MSE, None), ("diag", _lib.MX_DIAG, hd)):
        fp6 = lambda: _lib.check(L.slk_mx_scale_search6(dev.ptr(W), dev.ptr(h), code, R, n, dev.ptr(E), dev.ptr(S), s()))  # noqa: E731
        fp4 = lambda: _lib.check(L.slk_mx_scale_search(dev.ptr(W), dev.ptr(h), code, R, n, dev.ptr(E), dev.ptr(S), s()))  # noqa: E731
        t6, t4 = timed_pair([fp6, fp4], reps)
        row(size, f"mx_scale_search6 {mode}", t6, 4 * R * n + 5 * R * G, over_fp4=round(t6[0] / t4[0], 3))
        row(size, f"mx_scale_search {mode}", t4, 4 * R * n + 5 * R * G)
    gen = torch.Generator(device="cuda").manual_seed(0)
    idx = torch.randint(0, 15, (R, n), dtype=torch.uint8, device="cuda", generator=gen)
    Sb = mx.decode_scales(torch.randint(100, 140, (R, G), dtype=torch.uint8, device="cuda", generator=gen))
    c4, e4 = mx.pack_mxfp4(idx, Sb)
    c6, e6 = mx.pack_mxfp6(idx, Sb)
    idx_out, S_out = torch.empty_like(idx), torch.empty_like(Sb)
    P = dev.ptr
    sides = (("pack", lambda: L.slk_mx_pack6(P(idx), P(Sb), R, n, P(c6), P(e6), None, s()),
              lambda: L.slk_mx_pack(P(idx), P(Sb), R, n, P(c4), P(e4), None, s())),
             ("unpack", lambda: L.slk_mx_unpack6(P(c6), P(e6), R, n, P(idx_out), P(S_out), None, s()),
              lambda: L.slk_mx_unpack(P(c4), P(e4), R, n, P(idx_out), P(S_out), None, s())))
    for what, fp6, fp4 in sides:
        t6, t4 = timed_pair([lambda: _lib.check(fp6()), lambda: _lib.check(fp4())], reps)
        row(size, f"mx_{what}6", t6, R * n + 3 * R * n // 4 + 5 * R * G, over_fp4=round(t6[0] / t4[0], 3))
        row(size, f"mx_{what}", t4, R * n + R * n // 2 + 5 * R * G)
    if layer:
        S4, S6 = mx.compute_mx_scales(W, H, "mse")[0], mx.compute_mx_scales(W, H, "mse", weights="mxfp6_e2m3")[0]
        for name, fn in (("quantize_mxfp6 (mse scales, loop, pack)", lambda: mx.quantize_mxfp6(W, H)),
                         ("quantize_mxfp4 (mse scales, loop, pack)", lambda: mx.quantize_mxfp4(W, H)),
                         ("quantize_mxfp6 given scales (loop, pack)", lambda: mx.quantize_mxfp6(W, H, scales=S6)),
                         ("quantize_mxfp4 given scales (loop, pack)", lambda: mx.quantize_mxfp4(W, H, scales=S4)),
                         ("quantize_mxfp6 (mse scales, loop, pack) again", lambda: mx.quantize_mxfp6(W, H)),
                         ("quantize_mxfp4 (mse scales, loop, pack) again", lambda: mx.quantize_mxfp4(W, H))):
            print(json.dumps(dict(size=size, call=name, **wall(fn, max(3, reps // 4)))), flush=True)


def parent_rows(size, R, n, reps, parent):
    """Every converter of this library against the parent's, on the same buffers."""
    G = n // 32
    P, s = dev.ptr, dev.stream_handle
    gen = torch.Generator(device="cuda").manual_seed(R + n)
    Eb = torch.randint(100, 140, (R, G), dtype=torch.uint8, device="cuda", generator=gen)
    S = mx.decode_scales(Eb)
    S_out, e_out = torch.empty_like(S), torch.empty_like(Eb)
    out = torch.empty((R, n), dtype=torch.float32, device="cuda")  # (every dtype's result: the 16-bit ones fill half of it)
    rows = []
    for six, bits, entries in (("", 4, 15), ("6", 6, 63)):
        idx = torch.randint(0, entries, (R, n), dtype=torch.uint8, device="cuda", generator=gen)
        codes = (mx.pack_mxfp6 if six else mx.pack_mxfp4)(idx, S)[0]
        c_out, idx_out = torch.empty_like(codes), torch.empty_like(idx)
        moved = R * n + R * n * bits // 8 + 5 * R * G
        rows.append((f"slk_mx_pack{six}", moved, lambda lib, six=six, idx=idx, c_out=c_out: getattr(lib, "slk_mx_pack" + six)(
            P(idx), P(S), R, n, P(c_out), P(e_out), None, s())))
        rows.append((f"slk_mx_unpack{six}", moved, lambda lib, six=six, codes=codes, idx_out=idx_out: getattr(lib, "slk_mx_unpack" + six)(
            P(codes), P(Eb), R, n, P(idx_out), P(S_out), None, s())))
        if six:
            rows.append(("slk_mx_dequantize_act6 bfloat16", R * n * bits // 8 + R * G + 2 * R * n, lambda lib, codes=codes: lib.slk_mx_dequantize_act6(
                P(codes), P(Eb), R, n, _lib.DTYPE_BF16, P(out), None, s())))
            continue
        for name, code, osz in (("float32", _lib.DTYPE_F32, 4), ("bfloat16", _lib.DTYPE_BF16, 2), ("float16", _lib.DTYPE_F16, 2)):
            rows.append((f"slk_mx_dequantize {name}", R * n // 2 + R * G + osz * R * n, lambda lib, codes=codes, code=code: lib.slk_mx_dequantize(
                P(codes), P(Eb), R, n, code, P(out), None, s())))
    c8 = torch.randint(0, 0x7F, (R, n), dtype=torch.uint8, device="cuda", generator=gen)  # (E4M3 codes, no NaN)
    rows.append(("slk_mx_dequantize_act bfloat16", R * n + R * G + 2 * R * n, lambda lib: lib.slk_mx_dequantize_act(
        P(c8), P(Eb), R, n, _lib.DTYPE_BF16, P(out), None, s())))
    for entry, nbytes, call in rows:
        this, there, this2, there2 = timed([lambda: _lib.check(call(L)), lambda: _lib.check(call(parent))] * 2, reps)
        cmp = against_parent((this, this2), (there, there2))
        passes = max(this[0], this2[0]) <= cmp["parent_max_us"] or this[0] / there[0] <= 1.0 + abs(there[0] - there2[0]) / there[0]
        row(size, f"{entry} against the parent's", this, nbytes, passes=bool(passes), **cmp)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="a libsleekit_amd.so built from another commit: only the converters, against its")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-layer", action="store_true")
    ap.add_argument("--fp6", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "micro_mx measures the MI355X; there is no CPU path"
    torch.cuda.set_device(0)
    for size, (R, n) in (("4096x4096", (4096, 4096)), ("4096x11008", (4096, 11008))):
        if args.parent_lib:
            parent_rows(size, R, n, args.reps, load_library(args.parent_lib))
            torch.cuda.empty_cache()
            continue
        layer = synth.make_layer_device(R, n, 31, "cuda")
        if args.fp6:
            fp6_rows(size, layer["W"], layer["H"], args.reps, n == 4096 and not args.no_layer)
            del layer
            torch.cuda.empty_cache()
            continue
        scale_rows(size, layer["W"], layer["H"], args.reps)
        pack_rows(size, R, n, args.reps)
        if n == 4096 and not args.no_layer:
            layer_rows(layer["W"], layer["H"], max(3, args.reps // 4))
        del layer
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
