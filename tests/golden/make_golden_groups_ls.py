#!/usr/bin/env python3
"""Generate tests/golden/groups_ls.npz -- local search on group-scaled layers -- by running the REAL reference.

Run only where the reference is available (same pattern as make_golden_groups.py; SLEEKIT_REF overrides its location):

    python tests/golden/make_golden_groups_ls.py

Inputs come from the build's own generator (sleekit_amd.synth, keyed by the seeds stored here, with one group of zero
weights where a case says so); only outputs are written.  For every case:

    S  = column k: sleekit.scaling.compute_scaling(W[:, k g:(k+1) g], cb, H[k g:(k+1) g, k g:(k+1) g], mode)
         ("rowvar", for g = 1, where every weight would otherwise sit on a level of its own scale: the scale of the whole
         row, compute_scaling(W, cb, H, "mse"), times 1 + (c % 5) / 16 in column c -- any positive S is a valid input)
    Q0 = sleekit.obq.quantize_opt(W, H, Z, act_order, 0.01, 0) with Z the group quantizer of S (make_golden_groups.py)
    Q  = the reference's own LocalSearchQuantizer(W, Q0, H, GroupCandidates(cb, S, g)), driven move by move as
         quantize_local_search drives it

GroupCandidates applies S by column: on whole matrices (the initial candidates) every element by its own column; on the
1-D arrays that do_change hands it (the new candidates of the moved entries) the scales of the entries being changed,
which a subclass of LocalSearchQuantizer notes before calling the inherited do_change.  Before every move the gains are
read into oracle.obq_ref.move_record (it only inspects arrays), and the rows whose decision came within NEAR_TIE_LIMIT
roundings are kept with their full records -- the evidence tests/ls_evidence.py reads.

Stored per case: S (float32), idx0 (uint8 codebook indices of Q0 / S: Q0 = value(idx0) / (1 / S) bit for bit, checked
here), the SHA-256 of the final indices and one 64-bit hash per row of them, the final indices themselves for cases of at
most SMALL_IDX elements, and the near-tie records.

No reference source text is copied.
"""

import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.environ.get("SLEEKIT_REF", "/root/reference"))

import numpy as np  # noqa: E402

from make_golden import NEAR_TIE_LIMIT, row_hashes, sha  # noqa: E402
from make_golden_groups import edge_layer, group_scales, indices, make_codebook, quantize_grouped_ref  # noqa: E402

import sleekit.obq as ref_obq  # noqa: E402
import sleekit.scaling as ref_scaling  # noqa: E402

SMALL_IDX = 16384


class GroupCandidates:
    """quantize_up / quantize_down of the group quantizer of S (see the module docstring)."""

    def __init__(self, cb, S, g):
        self.cb, self.S, self.g, self.at = cb, S, g, None

    def _scales(self, x):
        if x.ndim == 2:
            return np.repeat(self.S, self.g, axis=1)
        rows, cols = self.at
        assert x.shape == rows.shape
        return self.S[rows, cols // self.g]

    def quantize_up(self, x):
        s = self._scales(x)
        return (self.cb.quantize_up(x / s) / (np.float32(1) / s)).astype(np.float32)

    def quantize_down(self, x):
        s = self._scales(x)
        return (self.cb.quantize_down(x / s) / (np.float32(1) / s)).astype(np.float32)


class NotingSearch(ref_obq.LocalSearchQuantizer):
    """The reference's search; notes which entries a do_change is about to change (for their scales)."""

    def do_change(self, gains, filter, candidates):
        self.quantizer.at = (np.arange(self.nchannels)[filter], gains.argmax(axis=1)[filter])
        super().do_change(gains, filter, candidates)


def scales(W, cb, H, g, mode):
    if mode != "rowvar":
        return group_scales(W, cb, H, g, mode)
    row = np.asarray(ref_scaling.compute_scaling(W, cb, H, "mse"), np.float32).reshape(-1, 1)
    return (row * (np.float32(1) + np.arange(W.shape[1] // g, dtype=np.float32) % 5 / np.float32(16))).astype(np.float32)


def search_records(W, Q0, H, cb, S, g, moves):
    from oracle import obq_ref  # move_record only inspects arrays: no oracle arithmetic enters the fixture's moves

    ls = NotingSearch(W, Q0, H, GroupCandidates(cb, S, g))
    noise = obq_ref.gain_noise_scale(W, Q0, H)
    records = []
    for _ in range(moves):
        records.append(obq_ref.move_record(ls.gain_up, ls.gain_down, ls.Q_up - ls.Q, ls.Q_down - ls.Q, noise))
        ls.do_move()
    return ls.Q, obq_ref.near_tie_summary(records, NEAR_TIE_LIMIT)


# (R, n, g, codebook, act_order, scale mode, moves, seed, zero group or None)
CASES = [
    (64, 96, 1, "8", "diag", "rowvar", 10, 6101, None),
    (64, 96, 3, "3", "none", "max", 100, 6102, None),
    (64, 96, 32, "2", "sqerr", "mse", 10, 6103, None),
    (64, 96, 96, "16", "diag", "diag", 1, 6104, None),
    (96, 172, 43, "nf4", "diag", "mse", 10, 6105, None),
    (96, 172, 4, "8", "sqerr", "max", 100, 6106, 5),        # a zero group: its scales sit at the floor
    (96, 172, 1, "3", "none", "rowvar", 10, 6107, None),
    (128, 768, 128, "8", "diag", "mse", 10, 6108, None),    # a wave per row
    (8, 768, 3, "16", "diag", "max", 100, 6109, None),
    (32, 1024, 32, "nf4", "diag", "mse", 10, 6110, None),
    (32, 1024, 1024, "3", "sqerr", "mse", 100, 6111, None),
    (16, 1024, 128, "8", "diag", "mse", 1, 6112, 2),        # a zero group
    (8, 1024, 1, "3", "diag", "rowvar", 10, 6116, None),
    (32, 3072, 128, "8", "diag", "mse", 10, 6113, None),    # a workgroup per row
    (32, 3072, 32, "16", "none", "max", 100, 6114, None),
    (16, 3072, 3072, "2", "diag", "diag", 10, 6115, None),
]


def main():
    out = {}
    meta = []
    for i, (R, n, g, cbn, order, mode, moves, seed, zero) in enumerate(CASES):
        t0 = time.time()
        L = edge_layer(R, n, g, seed, zero)
        cb = make_codebook(cbn)
        W, H = L["W"].astype(np.float32), L["H"].astype(np.float32)  # what quantize_opt hands to the search (obq.py:195-196, 216)
        S = scales(L["W"], cb, L["H"], g, mode)
        Q0 = quantize_grouped_ref(L["W"], S, cb, L["H"], g, order, 0.01, 32, 8)
        Q, near = search_records(W, Q0, H, cb, S, g, moves)
        idx0 = indices(cb, Q0, S, g)  # (both checked to rebuild their Q bit for bit)
        idx = indices(cb, Q, S, g)
        out[f"S_{i}"] = S
        out[f"idx0_{i}"] = idx0
        out[f"row_hash_{i}"] = row_hashes(idx)
        if R * n <= SMALL_IDX:
            out[f"idx_{i}"] = idx
        for k, v in near.items():
            out[f"near_{i}/{k}"] = v
        meta.append(dict(R=R, n=n, g=g, codebook=cbn, act_order=order, mode=mode, moves=moves, seed=seed, zero_group=zero,
                         sha256_idx=sha(idx), changed=int((idx != idx0).sum())))
        print(f"case {i}: {R}x{n} g={g} cb={cbn} {moves} moves: {meta[-1]['changed']} indices changed, "
              f"{len(near['rows'])} near-tie rows, {time.time() - t0:.1f} s", flush=True)
    out["meta"] = np.array(json.dumps(dict(cases=meta, near_tie_limit=NEAR_TIE_LIMIT, numpy=np.__version__)))
    np.savez_compressed(os.path.join(HERE, "groups_ls.npz"), **out)


if __name__ == "__main__":
    main()
