#!/usr/bin/env python3
"""Generate tests/golden/groups.npz -- group-wise scales -- by running the REAL reference (Coloquinte/sleekit).

Run only where the reference is available (same pattern as make_golden.py; SLEEKIT_REF overrides its location):

    python tests/golden/make_golden_groups.py [--no-large]
    python tests/golden/make_golden_groups.py --edges      # tests/golden/groups_edges.npz only

Inputs come from the build's own generator (sleekit_amd.synth, keyed by the seeds stored here); only outputs are
written.  For every small case:

    S  = column k: sleekit.scaling.compute_scaling(W[:, k g:(k+1) g], cb, H[k g:(k+1) g, k g:(k+1) g], mode)
    Q  = sleekit.obq.quantize_opt(W, H, Z, act_order, damp, 0, min_block_size, num_blocks)

with Z the group quantizer of S: on the whole matrix (the err / sqerr orders) every element by its own column, on the
i-th leaf column the column order[i] -- the reference calls it once per column, in processing order.

Stored: S (float32) and the SHA-256 of Q for every case; for the cases of at most SMALL_IDX elements also the uint8
codebook indices of Q / S, from which Q = value(idx) / (1 / S) is rebuilt bit for bit (checked here before writing).
Q itself is not stored: as float32 it is most of the bytes and compresses poorly.  The large case (4096 x 4096,
g = 128, 8 levels, diag order, mse group scales) is stored as the SHA-256 of S and of Q.

--edges writes tests/golden/groups_edges.npz in the same format from EDGE_CASES: the shapes where kernels break (ragged
row tiles, odd group sizes, widths that are not a multiple of 4, leaves of 1 to 48 and of 550 columns), every act_order,
codebooks of 2 to 256 levels and nf4, and layers with one whole group of zero weights (their scales sit at the floor).
Those cases have no exactly tied order keys (checked here), so the reference's unstable argsort and the device's
stable-tie order agree on them.

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
sys.path.insert(0, os.environ.get("SLEEKIT_REF", "/root/reference"))

import numpy as np  # noqa: E402

from sleekit_amd import synth  # noqa: E402

import sleekit.obq as ref_obq  # noqa: E402
import sleekit.scaling as ref_scaling  # noqa: E402
from sleekit.codebook import Codebook, UniformCodebook  # noqa: E402

NF4 = [-1.0, -0.6961928009986877, -0.5250730514526367, -0.39491748809814453, -0.28444138169288635, -0.18477343022823334,
       -0.09105003625154495, 0.0, 0.07958029955625534, 0.16093020141124725, 0.24611230194568634, 0.33791524171829224,
       0.44070982933044434, 0.5626170039176941, 0.7229568362236023, 1.0]


def make_codebook(name):
    return Codebook(NF4) if name == "nf4" else UniformCodebook(int(name), -1, 1)


class GroupQuantizer:
    """The group quantizer of S as a callable for quantize_opt (see the module docstring)."""

    def __init__(self, cb, S, g, order):
        self.cb, self.S, self.g, self.order, self.i = cb, S, g, order, 0

    def __call__(self, x):
        if x.ndim == 2:
            s = np.repeat(self.S, self.g, axis=1)
        else:
            s = self.S[:, self.order[self.i] // self.g]
            self.i += 1
        return (self.cb.quantize_value(x / s) / (np.float32(1) / s)).astype(np.float32)


SMALL_IDX = 16384


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def indices(cb, Q, S, g):
    """uint8 codebook indices of Q / S, checked to rebuild Q exactly: value(idx) / (1 / s), value formed like quantize_value."""
    s = np.repeat(S, g, axis=1)
    idx = cb.quantize_index(Q / s).astype(np.uint8)
    if isinstance(cb, UniformCodebook):
        vals = idx.astype(np.float32)
        vals *= cb.scale
        vals += cb.zero
    else:
        vals = cb.values[idx]
    back = (vals / (np.float32(1) / s)).astype(np.float32)
    assert np.array_equal(back.view(np.uint32), Q.view(np.uint32)), "indices do not rebuild Q"
    return idx


def group_scales(W, cb, H, g, mode):
    n = W.shape[1]
    cols = [ref_scaling.compute_scaling(W[:, k:k + g], cb, H[k:k + g, k:k + g], mode) for k in range(0, n, g)]
    return np.stack(cols, axis=1).astype(np.float32)


def quantize_grouped_ref(W, S, cb, H, g, act_order, damp, mb, nb):
    W = W.astype(np.float32)
    H = H.astype(np.float32)
    H_opt = H + damp * H.diagonal().mean() * np.eye(H.shape[0])
    order = ref_obq.compute_hessian_order(W, H_opt, GroupQuantizer(cb, S, g, None), act_order)
    Z = GroupQuantizer(cb, S, g, order)
    Q = ref_obq.quantize_opt(W, H, Z, act_order, damp, 0, mb, nb)
    assert Z.i == W.shape[1], "the leaves did not visit every column once"
    return Q.astype(np.float32)


# (R, n, g, codebook, act_order, scale mode, damp, min_block_size, num_blocks, seed)
CASES = [
    (64, 128, 32, "8", "none", "max", 0.01, 32, 8, 5101),
    (64, 128, 64, "8", "diag", "mse", 0.01, 32, 8, 5102),
    (64, 128, 128, "4", "err", "diag", 0.01, 32, 8, 5103),
    (96, 192, 64, "16", "sqerr", "mse", 0.03, 32, 8, 5104),
    (96, 256, 32, "3", "pivot", "max", 0.01, 32, 8, 5105),
    (128, 256, 128, "8", "inv_diag", "diag", 0.01, 32, 8, 5106),
    (128, 256, 256, "8", "diag", "mse", 0.01, 32, 8, 5107),
    (64, 256, 64, "nf4", "diag", "max", 0.01, 32, 8, 5108),
    (96, 384, 128, "4", "sqerr", "diag", 0.03, 32, 8, 5109),
    (128, 384, 32, "16", "err", "mse", 0.01, 16, 4, 5110),
    (64, 512, 128, "8", "diag", "mse", 0.01, 32, 8, 5111),
    (128, 512, 64, "3", "none", "diag", 0.01, 32, 8, 5112),
    (96, 512, 512, "16", "pivot", "mse", 0.01, 32, 8, 5113),
    (128, 512, 32, "8", "sqerr", "max", 0.01, 64, 4, 5114),
    (64, 128, 32, "8", "diag", "mse", 0.01, 128, 1, 5115),      # one leaf as wide as the layer
    (64, 256, 64, "4", "none", "diag", 0.01, 256, 1, 5116),     # one wide leaf, no reordering
    (96, 128, 64, "nf4", "sqerr", "mse", 0.01, 16, 2, 5117),
    (128, 192, 32, "8", "inv_diag", "max", 0.01, 8, 4, 5118),
    (64, 384, 384, "3", "diag", "diag", 0.01, 32, 8, 5119),
    (96, 256, 128, "16", "err", "max", 0.01, 32, 8, 5120),
    (128, 128, 32, "4", "pivot", "diag", 0.01, 32, 8, 5121),
    (64, 512, 64, "8", "err", "diag5", 0.01, 32, 8, 5122),
    (96, 256, 64, "8", "diag", "hessian", 0.01, 32, 8, 5123),
    (64, 128, 64, "4", "sqerr", "hessian10", 0.01, 32, 8, 5124),
    (128, 256, 32, "nf4", "none", "mse", 0.01, 32, 8, 5125),
    (64, 640, 128, "8", "diag", "mse", 0.01, 640, 1, 5126),     # one leaf wider than a window
    (96, 512, 128, "3", "sqerr", "mse", 0.03, 32, 8, 5127),
    (128, 384, 64, "16", "diag", "diag2", 0.01, 32, 8, 5128),
    (64, 256, 256, "8", "inv_diag", "mse", 0.01, 32, 8, 5129),
    (96, 192, 32, "4", "diag", "max", 0.01, 32, 8, 5130),
]

# (R, n, g, codebook, act_order, scale mode, damp, min_block_size, num_blocks, seed, zero group or None)
EDGE_CASES = [
    (1, 96, 1, "3", "none", "max", 0.01, 32, 8, 5201, None),
    (5, 96, 3, "16", "diag", "mse", 0.01, 48, 4, 5202, None),
    (17, 192, 24, "2", "err", "diag", 0.01, 32, 8, 5203, None),
    (33, 172, 4, "256", "sqerr", "diag3", 0.03, 1, 2, 5204, None),
    (17, 172, 43, "nf4", "pivot", "mse", 0.01, 32, 8, 5205, None),
    (1, 100, 25, "8", "inv_diag", "max", 0.01, 48, 4, 5206, None),
    (109, 105, 7, "3", "combined_diag", "diag", 0.1, 32, 8, 5207, None),
    (33, 258, 43, "16", "sqerr", "mse", 0.01, 48, 4, 5208, None),
    (70, 1100, 100, "8", "diag", "mse", 0.01, 32, 8, 5209, None),
    (5, 1100, 55, "nf4", "err", "diag2", 0.01, 640, 2, 5210, None),     # two 550-column leaves (global-memory window)
    (17, 1376, 43, "4", "inv_diag", "mse", 0.01, 32, 8, 5211, None),
    (70, 172, 43, "8", "sqerr", "max", 0.01, 32, 8, 5212, 2),           # a zero group: its scale is the floor, 1e-16
    (33, 96, 3, "3", "diag", "mse", 0.01, 1, 2, 5213, 5),               # a zero group: 5e-18 after the search
    (5, 105, 7, "2", "pivot", "diag", 0.01, 48, 4, 5214, None),
    (70, 1100, 55, "256", "combined_diag", "max", 0.01, 640, 2, 5215, None),
    (17, 100, 25, "16", "none", "diag5", 0.03, 1, 2, 5216, None),
    (109, 192, 24, "nf4", "err", "mse", 0.01, 48, 4, 5217, None),
]


def edge_layer(R, n, g, seed, zero):
    L = synth.make_layer(R, n, seed)
    if zero is not None:
        L["W"][:, zero * g:(zero + 1) * g] = 0
    return L


def assert_no_tied_keys(W, S, H, g, cbn, act_order, damp):
    """The order with NumPy's tie-breaking equals the stable-tie order: no two order keys are exactly equal."""
    from groups_model import GroupGrid, oracle_grid
    from oracle import obq_ref

    Hd = H + damp * H.diagonal().mean() * np.eye(H.shape[0])
    Z = GroupGrid(oracle_grid(cbn), S, g, None)
    a = obq_ref.column_order(W, Hd, Z, act_order, "numpy")
    b = obq_ref.column_order(W, Hd, Z, act_order, "stable")
    assert np.array_equal(a, b), "tied order keys: the reference's order is not the device's"


def edges():
    sys.path.insert(0, os.path.dirname(HERE))  # tests/, for groups_model
    out = {}
    meta = []
    for i, (R, n, g, cbn, order, mode, damp, mb, nb, seed, zero) in enumerate(EDGE_CASES):
        t0 = time.time()
        L = edge_layer(R, n, g, seed, zero)
        cb = make_codebook(cbn)
        S = group_scales(L["W"], cb, L["H"], g, mode)
        assert_no_tied_keys(L["W"], S, L["H"], g, cbn, order, damp)
        Q = quantize_grouped_ref(L["W"], S, cb, L["H"], g, order, damp, mb, nb)
        out[f"S_{i}"] = S
        idx = indices(cb, Q, S, g)
        if R * n <= SMALL_IDX:
            out[f"idx_{i}"] = idx
        meta.append(dict(R=R, n=n, g=g, codebook=cbn, act_order=order, mode=mode, damp=damp, min_block_size=mb, num_blocks=nb,
                         seed=seed, zero_group=zero, sha256_Q=sha(Q)))
        print(f"edge {i}: {R}x{n} g={g} cb={cbn} {order} {mode}: {time.time() - t0:.1f} s", flush=True)
    out["meta"] = np.array(json.dumps(dict(cases=meta, numpy=np.__version__)))
    np.savez_compressed(os.path.join(HERE, "groups_edges.npz"), **out)


LARGE = dict(R=4096, n=4096, g=128, codebook="8", act_order="diag", mode="mse", damp=0.01, seed=5199)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-large", action="store_true")
    ap.add_argument("--edges", action="store_true", help="write groups_edges.npz only")
    args = ap.parse_args()
    if args.edges:
        return edges()
    out = {}
    meta = []
    for i, (R, n, g, cbn, order, mode, damp, mb, nb, seed) in enumerate(CASES):
        t0 = time.time()
        L = synth.make_layer(R, n, seed)
        cb = make_codebook(cbn)
        S = group_scales(L["W"], cb, L["H"], g, mode)
        Q = quantize_grouped_ref(L["W"], S, cb, L["H"], g, order, damp, mb, nb)
        out[f"S_{i}"] = S
        idx = indices(cb, Q, S, g)  # (checks the rebuild for every case, stores the small ones)
        if R * n <= SMALL_IDX:
            out[f"idx_{i}"] = idx
        meta.append(dict(R=R, n=n, g=g, codebook=cbn, act_order=order, mode=mode, damp=damp, min_block_size=mb, num_blocks=nb,
                         seed=seed, sha256_Q=sha(Q)))
        print(f"case {i}: {R}x{n} g={g} cb={cbn} {order} {mode}: {time.time() - t0:.1f} s", flush=True)
    if not args.no_large:
        t0 = time.time()
        L = synth.make_layer(LARGE["R"], LARGE["n"], LARGE["seed"])
        cb = make_codebook(LARGE["codebook"])
        S = group_scales(L["W"], cb, L["H"], LARGE["g"], LARGE["mode"])
        Q = quantize_grouped_ref(L["W"], S, cb, L["H"], LARGE["g"], LARGE["act_order"], LARGE["damp"], 32, 8)
        large = dict(LARGE, sha256_S=sha(S), sha256_Q=sha(Q))
        print(f"large: {time.time() - t0:.1f} s", flush=True)
    else:
        large = None
    out["meta"] = np.array(json.dumps(dict(cases=meta, large=large, numpy=np.__version__)))
    np.savez_compressed(os.path.join(HERE, "groups.npz"), **out)


if __name__ == "__main__":
    main()
