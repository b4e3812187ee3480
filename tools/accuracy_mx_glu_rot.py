#!/usr/bin/env python3
"""Output error of the gated MX MLP with the down layer behind a rotation of the hidden features, on the MI355X.

    python tools/accuracy_mx_glu_rot.py [--seeds 4242,7,19,101,2024,31337] [--k 256] [--n 256] [--out 64] [--tokens 128]

The synthetic layer of DESIGN.md sections 18 and 20, as a gated MLP: x = synth.make_activations(tokens, K) (20 channels
with 8 times the gain), an up layer of 2 N rows and a down layer of `out` rows over the N hidden features from
synth.make_weights, SwiGLU.  Both layers are rounded to nearest MXFP4 under the non-saturating scale (the E2M1 activation
quantizer applied to the weight matrix: the same codes and packing), the down layer in the basis it is used in: W_down R
behind a rotation R of the hidden features.  The error is |y - y_ref| / |y_ref| (Frobenius) of mx.gated_mlp_mx against the
float64 MLP of the unquantized x and weights, for MXFP8, MXFP6 and MXFP4 activations (W4A8, W4A6, W4A4) under three
conditions: no down rotation; a block of 32 (one rotation per MX block of h, inside the fused product's epilogue); the
default block (the largest power of two that divides N, on the three-step route).  Each is measured twice: with x as it is
(the keys W4A*_<condition>), and with x behind a rotation of the K input features at its default block and the up layer
quantized in that basis (xrot_W4A*_<condition>), so that the hidden side shows once the input side is at its best.  One JSON
line per seed, then the means.
"""

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from sleekit_amd import mx, synth  # noqa: E402
from sleekit_amd.rotation import Rotation  # noqa: E402

ACTS = {"W4A8": "mxfp8", "W4A6": "mxfp6_e2m3", "W4A4": "mxfp4"}


def errors(seed, K, N, out, tokens):
    x = synth.make_activations(tokens, K, seed).astype(np.float32)
    Wu, Wd = synth.make_weights(2 * N, K, seed), synth.make_weights(out, N, seed + 1)
    y = x.astype(np.float64) @ Wu.astype(np.float64).T
    g, u = y[:, :N], y[:, N:]
    want = (u * (g / (1.0 + np.exp(-g)))) @ Wd.astype(np.float64).T
    xd, Wd_d = torch.from_numpy(x).cuda(), torch.from_numpy(Wd).cuda()
    Wu_d = torch.from_numpy(Wu).cuda()
    rots = {"none": None, "block32": Rotation(N, block=32, seed=seed), "default": Rotation(N, seed=seed)}
    row = dict(seed=seed, default_block=rots["default"].block)
    for prefix, xrot in (("", None), ("xrot_", Rotation(K, seed=seed + 2))):
        uc, us = mx.quantize_mxfp4_act(Wu_d if xrot is None else xrot.apply(Wu_d, dtype=torch.float32))
        for name, act in ACTS.items():
            for cond, rot in rots.items():
                dc, ds = mx.quantize_mxfp4_act(Wd_d if rot is None else rot.apply(Wd_d, dtype=torch.float32))
                got = mx.gated_mlp_mx(xd, uc, us, dc, ds, activations=act, rotation=xrot, down_rotation=rot).double().cpu().numpy()
                row[f"{prefix}{name}_{cond}"] = round(float(np.linalg.norm(got - want) / np.linalg.norm(want)), 4)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", default="4242,7,19,101,2024,31337")
    ap.add_argument("--k", type=int, default=256)
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--out", type=int, default=64)
    ap.add_argument("--tokens", type=int, default=128)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "accuracy_mx_glu_rot runs the MI355X kernels; there is no CPU path"
    torch.cuda.set_device(0)
    rows = [errors(int(s), args.k, args.n, args.out, args.tokens) for s in args.seeds.split(",") if s]
    for r in rows:
        print(json.dumps(r), flush=True)
    keys = [k for k in rows[0] if k not in ("seed", "default_block")]
    print(json.dumps(dict(mean={k: round(float(np.mean([r[k] for r in rows])), 4) for k in keys},
                          low={k: min(r[k] for r in rows) for k in keys}, high={k: max(r[k] for r in rows) for k in keys})), flush=True)


if __name__ == "__main__":
    main()
