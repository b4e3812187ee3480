#!/usr/bin/env python3
"""Generate tests/golden/groups_offsets.npz -- asymmetric group quantization -- by running the REAL reference
(Coloquinte/sleekit).

Run only where the reference is available (same pattern as make_golden_groups.py; SLEEKIT_REF overrides its location):

    python tests/golden/make_golden_offsets.py [--no-large]

Inputs come from the build's own generator (sleekit_amd.synth, keyed by the seeds stored here), shaped by the variants
below; only outputs are written.  For every case, with Z the asymmetric group quantizer of (S, O)

    Z(x) = cb.quantize_value((x - o) / s) / (np.float32(1) / s) + o,   s = S[r, c // g], o = O[r, c // g]

(applied to the whole matrix for the err / sqerr orders, to column order[i] on the i-th leaf column):

    O  = np.float32(0.5) * (min + max) of each group (float32)
    S  = column k: sleekit.scaling.compute_scaling(Wc[:, k g:(k+1) g], cb, H[k g:(k+1) g, k g:(k+1) g], mode), Wc = W - O
    Q  = sleekit.obq.quantize_opt(W, H, Z, act_order, damp, 0, min_block_size, num_blocks)

Stored: O, S and the SHA-256 of Q for every case; for the cases of at most SMALL_IDX elements also uint8 codebook indices
from which Q = value(idx) / (1 / S) + O is rebuilt bit for bit (checked here).  The large case (4096 x 4096, g = 128,
8 levels, diag order, mse) is stored as the SHA-256 of O, S and Q.

Variants: "pos" makes every group one-signed (|W| + 0.01), "shift" moves the layer off centre (W + 3 max |W|), "const"
makes group k of every row one repeated value (its scale sits at the floor), "huge" puts group k near 2^22 with unit
noise (|o| / s >= 2^20: `+ o` absorbs most of the codebook term).  No case has exactly tied order keys (checked), so the
reference's argsort and the device's stable order agree.

No reference source text is copied.
"""

import argparse
import hashlib
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))  # tests/, for groups_offsets_model
sys.path.insert(0, os.environ.get("SLEEKIT_REF", "/root/reference"))

import numpy as np  # noqa: E402

from groups_offsets_model import offsets_model, shaped_layer  # noqa: E402

import sleekit.obq as ref_obq  # noqa: E402
import sleekit.scaling as ref_scaling  # noqa: E402
from sleekit.codebook import Codebook, UniformCodebook  # noqa: E402

NF4 = [-1.0, -0.6961928009986877, -0.5250730514526367, -0.39491748809814453, -0.28444138169288635, -0.18477343022823334,
       -0.09105003625154495, 0.0, 0.07958029955625534, 0.16093020141124725, 0.24611230194568634, 0.33791524171829224,
       0.44070982933044434, 0.5626170039176941, 0.7229568362236023, 1.0]
SMALL_IDX = 8192


def make_codebook(name):
    return Codebook(NF4) if name == "nf4" else UniformCodebook(int(name), -1, 1)


class AsymQuantizer:
    """The asymmetric group quantizer of (S, O) as a callable for quantize_opt (see the module docstring)."""

    def __init__(self, cb, S, O, g, order):
        self.cb, self.S, self.O, self.g, self.order, self.i = cb, S, O, g, order, 0

    def __call__(self, x):
        if x.ndim == 2:
            s, o = np.repeat(self.S, self.g, axis=1), np.repeat(self.O, self.g, axis=1)
        else:
            k = self.order[self.i] // self.g
            s, o = self.S[:, k], self.O[:, k]
            self.i += 1
        return (self.cb.quantize_value((x - o) / s) / (np.float32(1) / s) + o).astype(np.float32)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def values(cb, idx):
    if isinstance(cb, UniformCodebook):
        vals = idx.astype(np.float32)
        vals *= cb.scale
        vals += cb.zero
        return vals
    return np.asarray(cb.values, np.float32)[idx]


def indices(cb, Q, S, O, g):
    """uint8 indices of (Q - o) / s, replaced where they do not rebuild Q by the first index that does; checked."""
    s, o = np.repeat(S, g, axis=1), np.repeat(O, g, axis=1)
    idx = cb.quantize_index((Q - o) / s).astype(np.uint8)
    back = lambda i: (values(cb, i) / (np.float32(1) / s) + o).astype(np.float32)
    bad = back(idx).view(np.uint32) != Q.view(np.uint32)
    for t in reversed(range(len(cb))):
        cand = np.full_like(idx, t)
        hit = bad & (back(cand).view(np.uint32) == Q.view(np.uint32))
        idx[hit] = t
    bad = back(idx).view(np.uint32) != Q.view(np.uint32)
    assert not bad.any(), "indices do not rebuild Q"
    return idx


def midpoints(W, g):
    R, n = W.shape
    V = W.reshape(R, n // g, g)
    return (np.float32(0.5) * (V.min(axis=2) + V.max(axis=2))).astype(np.float32)


def group_scales(Wc, cb, H, g, mode):
    n = Wc.shape[1]
    cols = [ref_scaling.compute_scaling(Wc[:, k:k + g], cb, H[k:k + g, k:k + g], mode) for k in range(0, n, g)]
    return np.stack(cols, axis=1).astype(np.float32)


def reference_case(W, H, cbn, g, order, mode, damp, mb, nb):
    cb = make_codebook(cbn)
    O = midpoints(W, g)
    Wc = (W - np.repeat(O, g, axis=1)).astype(np.float32)
    S = group_scales(Wc, cb, H, g, mode)
    H_opt = H + damp * H.diagonal().mean() * np.eye(H.shape[0])
    order_cols = ref_obq.compute_hessian_order(W, H_opt, AsymQuantizer(cb, S, O, g, None), order)
    Z = AsymQuantizer(cb, S, O, g, order_cols)
    Q = ref_obq.quantize_opt(W, H, Z, order, damp, 0, mb, nb).astype(np.float32)
    assert Z.i == W.shape[1], "the leaves did not visit every column once"
    return cb, O, S, Q


# (R, n, g, codebook, act_order, scale mode, damp, min_block_size, num_blocks, seed, variant)
CASES = [
    (64, 128, 32, "8", "none", "max", 0.01, 32, 8, 6101, None),
    (64, 128, 64, "8", "diag", "mse", 0.01, 32, 8, 6102, "pos"),
    (128, 256, 128, "4", "err", "diag", 0.01, 32, 8, 6103, None),
    (96, 192, 64, "16", "sqerr", "mse", 0.03, 32, 8, 6104, "shift"),
    (96, 256, 32, "3", "pivot", "max", 0.01, 32, 8, 6105, "pos"),
    (128, 256, 128, "8", "inv_diag", "diag", 0.01, 32, 8, 6106, None),
    (64, 256, 256, "8", "diag", "mse", 0.01, 32, 8, 6107, "shift"),
    (64, 256, 64, "nf4", "diag", "max", 0.01, 32, 8, 6108, None),
    (128, 512, 64, "3", "none", "diag", 0.01, 32, 8, 6109, "pos"),
    (96, 512, 512, "16", "pivot", "mse", 0.01, 32, 8, 6110, None),
    (64, 128, 32, "8", "diag", "mse", 0.01, 128, 1, 6111, None),      # one leaf as wide as the layer
    (64, 640, 128, "8", "diag", "mse", 0.01, 640, 1, 6112, "pos"),    # one leaf wider than a window
    (64, 512, 64, "8", "err", "diag5", 0.01, 32, 8, 6113, None),
    (96, 256, 64, "8", "diag", "hessian", 0.01, 32, 8, 6114, None),
    (64, 128, 64, "4", "sqerr", "hessian10", 0.01, 32, 8, 6115, "shift"),
    (1, 105, 1, "3", "none", "max", 0.01, 32, 8, 6201, None),
    (5, 105, 7, "2", "diag", "mse", 0.01, 48, 4, 6202, None),
    (17, 192, 24, "256", "sqerr", "diag3", 0.03, 1, 2, 6203, None),   # one-column leaves
    (33, 172, 43, "nf4", "pivot", "mse", 0.01, 33, 4, 6204, "pos"),
    (109, 105, 7, "3", "combined_diag", "diag", 0.1, 32, 8, 6205, None),
    (70, 1100, 100, "8", "diag", "mse", 0.01, 32, 8, 6206, None),
    (5, 1100, 55, "16", "err", "diag2", 0.01, 640, 2, 6207, None),    # two 550-column leaves
    (17, 344, 43, "8", "diag", "max", 0.01, 32, 8, 6208, "const"),    # a group of one repeated value
    (33, 192, 32, "8", "diag", "mse", 0.01, 48, 4, 6209, "huge"),     # a group with |o| / s >= 2^20
    (128, 320, 5, "4", "inv_diag", "mse", 0.01, 40, 8, 6210, "shift"),
]

LARGE = dict(R=4096, n=4096, g=128, codebook="8", act_order="diag", mode="mse", damp=0.01, seed=6199, variant=None)


def assert_no_tied_keys(W, S, O, H, g, cbn, act_order, damp):
    from groups_model import oracle_grid
    from groups_offsets_model import AsymGrid
    from oracle import obq_ref

    Hd = H + damp * H.diagonal().mean() * np.eye(H.shape[0])
    Z = AsymGrid(oracle_grid(cbn), S, O, g, None)
    a = obq_ref.column_order(W, Hd, Z, act_order, "numpy")
    b = obq_ref.column_order(W, Hd, Z, act_order, "stable")
    assert np.array_equal(a, b), "tied order keys: the reference's order is not the device's"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-large", action="store_true")
    args = ap.parse_args()
    out = {}
    meta = []
    for i, (R, n, g, cbn, order, mode, damp, mb, nb, seed, variant) in enumerate(CASES):
        t0 = time.time()
        L = shaped_layer(R, n, g, seed, variant)
        cb, O, S, Q = reference_case(L["W"], L["H"], cbn, g, order, mode, damp, mb, nb)
        assert_no_tied_keys(L["W"], S, O, L["H"], g, cbn, order, damp)
        # the NumPy model of tests/groups_offsets_model.py agrees before anything is written
        Om, Sm, Qm = offsets_model(L["W"], L["H"], cbn, g, order, mode, damp, mb, nb)
        assert np.array_equal(Om.view(np.uint32), O.view(np.uint32)) and np.array_equal(Sm.view(np.uint32), S.view(np.uint32))
        assert sha(Qm) == sha(Q), f"case {i}: the model's Q differs from the reference's"
        out[f"O_{i}"] = O
        out[f"S_{i}"] = S
        idx = indices(cb, Q, S, O, g)
        if R * n <= SMALL_IDX:
            out[f"idx_{i}"] = idx
        meta.append(dict(R=R, n=n, g=g, codebook=cbn, act_order=order, mode=mode, damp=damp, min_block_size=mb, num_blocks=nb,
                         seed=seed, variant=variant, sha256_Q=sha(Q)))
        print(f"case {i}: {R}x{n} g={g} cb={cbn} {order} {mode} {variant}: {time.time() - t0:.1f} s", flush=True)
    large = None
    if not args.no_large:
        t0 = time.time()
        L = shaped_layer(LARGE["R"], LARGE["n"], LARGE["g"], LARGE["seed"], LARGE["variant"])
        cb, O, S, Q = reference_case(L["W"], L["H"], LARGE["codebook"], LARGE["g"], LARGE["act_order"], LARGE["mode"],
                                     LARGE["damp"], 32, 8)
        large = dict(LARGE, sha256_O=sha(O), sha256_S=sha(S), sha256_Q=sha(Q))
        print(f"large: {time.time() - t0:.1f} s", flush=True)
    out["meta"] = np.array(json.dumps(dict(cases=meta, large=large, numpy=np.__version__)))
    np.savez_compressed(os.path.join(HERE, "groups_offsets.npz"), **out)


if __name__ == "__main__":
    main()
