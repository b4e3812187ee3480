#!/usr/bin/env python3
"""Bit-packed indices: kernel times and HBM rates of pack, unpack and dequantize_packed, on the MI355X.

    python tools/micro_packing.py [--reps 20] [--bits 3] [--g 128]

Two sizes: 8 stacked 4096 x 4096 layers (32768 x 4096) and the BASELINE set, all 32 layers of 4096 x 11008 stacked by
rows (131072 x 11008).  Each call is timed alone with device events (median of `reps`, after a warm-up).  Bytes are
what the call must move, computed from the shapes: pack / unpack read or write R n index bytes and 4 W words;
dequantize_packed reads the words and the (R, n / g) scales and offsets and writes R n values (4 or 2 bytes).  The
baseline row is unpack_indices followed by groups.dequantize_grouped (uint8 idx written and read again).  Share of peak:
the rate over the 6.3 TB/s that MI355X_MICROARCH.md measured as achievable for HBM.  One JSON line per row.
"""

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from sleekit_amd import groups, packing  # noqa: E402
from sleekit_amd.codebook import UniformCodebook  # noqa: E402

HBM = 6.3e12  # bytes/s


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)  # us
    ts.sort()
    return ts[len(ts) // 2]


def row(size, what, us, nbytes):
    rate = nbytes / (us * 1e-6)
    out = dict(size=size, kernel=what, us=round(us, 1), bytes=int(nbytes), tb_s=round(rate / 1e12, 3),
               share_of_hbm=round(rate / HBM, 3))
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--bits", type=int, default=3)
    ap.add_argument("--g", type=int, default=128)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "micro_packing measures the MI355X; there is no CPU path"
    torch.cuda.set_device(0)
    b, g = args.bits, args.g
    cb = UniformCodebook(1 << b, -1, 1)
    gen = torch.Generator(device="cuda").manual_seed(0)
    for size, (R, n) in (("8x4096x4096", (8 * 4096, 4096)), ("32x4096x11008", (32 * 4096, 11008))):
        idx = torch.randint(0, 1 << b, (R, n), dtype=torch.uint8, device="cuda", generator=gen)
        S = torch.rand((R, n // g), device="cuda", generator=gen) * 0.1 + 0.01
        O = torch.rand((R, n // g), device="cuda", generator=gen) * 0.1 - 0.05
        P = packing.pack_indices(idx, b)
        words = 4 * P.numel()
        side = 8 * S.numel()
        row(size, f"pack b={b}", timed(lambda: packing.pack_indices(idx, b), args.reps), R * n + words)
        row(size, f"unpack b={b}", timed(lambda: packing.unpack_indices(P, n, b), args.reps), R * n + words)
        for dtype, osz in ((torch.float32, 4), (torch.bfloat16, 2)):
            fn = lambda: packing.dequantize_packed(P, n, cb, group_scales=S, offsets=O, dtype=dtype)  # noqa: E731
            ref = packing.dequantize_packed(P, n, cb, group_scales=S, offsets=O, dtype=dtype)
            row(size, f"dequantize_packed {str(dtype)[6:]} g={g} offsets", timed(fn, args.reps), words + side + osz * R * n)
            del ref
            torch.cuda.empty_cache()

        def two_step():
            return groups.dequantize_grouped(packing.unpack_indices(P, n, b), S, cb, g, offsets=O)

        row(size, f"unpack + dequantize_grouped g={g} offsets", timed(two_step, args.reps),
            (R * n + words) + (R * n + side + 4 * R * n))
        row(size, f"dequantize_grouped alone g={g} offsets", timed(lambda: groups.dequantize_grouped(idx, S, cb, g, offsets=O), args.reps),
            R * n + side + 4 * R * n)
        del idx, S, O, P
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
