#!/usr/bin/env python3
"""Generate tests/golden/mx.npz -- MXFP4 output (sleekit_amd.mx) -- by running the REAL reference.

Run only where the reference is available (same pattern as make_golden_groups_ls.py; SLEEKIT_REF gives its location,
by default a `reference` directory beside this repository):

    python tests/golden/make_golden_mx.py

Inputs come from the build's own generator (tests/mx_model.py: case_layer, keyed by the seeds and the `special` stored
here); only outputs are written.  For every case, with cb = sleekit.codebook.Codebook of the 15 E2M1 values:

    E  = per (row, block of 32 columns) the reference's loop body (sleekit/scaling.py:127-134) over power-of-two candidates:
         b0 = sleekit.scaling.compute_non_saturating_scaling(block, cb); base = the smallest power of two >= b0; "max" gives
         base; "mse" and "diag" walk f = 0.125, 0.25, 0.5, 1: sleekit.scaling.quantize_with_scaling(block, f * base, cb),
         sleekit.scaling._compute_mse(None or diag(H) of the block's columns, quant - block), strictly better kept.
         Stored as the E8M0 byte log2(scale) + 127.
    Q0 = sleekit.obq.quantize_opt(W, H, Z, act_order, 0.01, 0) with Z the group quantizer of S = 2^(E - 127), g = 32
         (make_golden_groups.py: quantize_grouped_ref)
    Q  = the reference's LocalSearchQuantizer driven move by move with that quantizer's candidates
         (make_golden_groups_ls.py: NotingSearch, GroupCandidates)

Checked here before writing: Q0 and Q are values[idx] / (1 / s) bit for bit (make_golden_groups.indices) AND
+-magnitude[code & 7] * 2^(E - 127) bit for bit; no two order keys tie exactly; each of the four factors is chosen somewhere.

Stored per case: E (uint8), the SHA-256 of the indices after the loop and after the moves, one 64-bit hash per row of the
final indices, the final indices themselves for cases of at most SMALL_IDX elements, the SHA-256 of the final codes bytes
(two codes a byte, even column in the low nibble), and the near-tie records of the search cases.

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
sys.path.insert(0, os.path.dirname(HERE))  # tests/, for mx_model
sys.path.insert(0, os.environ.get("SLEEKIT_REF", os.path.join(os.path.dirname(ROOT), "reference")))

import numpy as np  # noqa: E402

from make_golden import NEAR_TIE_LIMIT, row_hashes, sha  # noqa: E402
from make_golden_groups import indices, quantize_grouped_ref  # noqa: E402
from make_golden_groups_ls import search_records  # noqa: E402

import mx_model  # noqa: E402  (the inputs, and the bit-level form of the codes: no model arithmetic enters E, Q0 or Q)

import sleekit.scaling as ref_scaling  # noqa: E402
from sleekit.codebook import Codebook  # noqa: E402

SMALL_IDX = 16384
G = 32
FACTORS = (0.125, 0.25, 0.5, 1.0)


def pow2_at_or_above(x):
    m, e = np.frexp(x)
    return np.ldexp(np.float32(1), e - (m == 0.5)).astype(np.float32)


def reference_scales(W, H, cb, mode, chosen_count):
    """(R, n / 32) float32 scales by the reference's own pieces (module docstring)."""
    hd = H.diagonal() if mode == "diag" else None
    cols = []
    for k in range(0, W.shape[1], G):
        block = W[:, k:k + G]
        base = pow2_at_or_above(ref_scaling.compute_non_saturating_scaling(block, cb, 0))
        if mode == "max":
            cols.append(base)
            continue
        best_choice = np.full(base.size, np.inf, dtype=np.float32)
        best_error = np.full(base.size, np.inf, dtype=np.float32)
        for f in FACTORS:
            scale = np.float32(f) * base
            quant = ref_scaling.quantize_with_scaling(block, scale, cb)
            error = ref_scaling._compute_mse(None if hd is None else hd[k:k + G], quant - block)
            better = error < best_error
            best_error[better] = error[better]
            best_choice[better] = f
        assert np.isfinite(best_choice).all()
        for f in FACTORS:
            chosen_count[f] += int((best_choice == f).sum())
        cols.append(base * best_choice)
    return np.stack(cols, axis=1).astype(np.float32)


def assert_no_tied_keys(W, S, H, act_order, damp):
    from groups_model import GroupGrid
    from oracle import obq_ref

    Hd = H + damp * H.diagonal().mean() * np.eye(H.shape[0])
    Z = GroupGrid(mx_model.e2m1_grid(), S, G, None)
    a = obq_ref.column_order(W, Hd, Z, act_order, "numpy")
    b = obq_ref.column_order(W, Hd, Z, act_order, "stable")
    assert np.array_equal(a, b), "tied order keys: the reference's order is not the device's"


# (R, n, act_order, scale mode, moves, seed, special)
CASES = [
    (1, 32, "none", "max", 0, 8101, None),
    (5, 64, "diag", "mse", 0, 8102, None),
    (17, 96, "err", "diag", 0, 8103, None),
    (33, 128, "sqerr", "mse", 0, 8104, None),
    (64, 256, "pivot", "diag", 0, 8105, None),
    (96, 384, "inv_diag", "max", 0, 8106, None),
    (128, 512, "combined_diag", "mse", 0, 8107, None),
    (16, 768, "diag", "mse", 10, 8108, None),           # a wave per row
    (8, 1024, "sqerr", "diag", 100, 8109, None),
    (32, 1024, "diag", "max", 0, 8110, None),
    (8, 3072, "diag", "mse", 10, 8111, None),           # a workgroup per row
    (4, 3072, "none", "diag", 100, 8112, None),
    (16, 96, "diag", "mse", 100, 8113, None),           # the general search kernel
    (8, 1056, "sqerr", "mse", 10, 8114, None),          # ... at a width whose summation tree is not regular
    (4, 4096, "diag", "diag", 0, 8115, None),
    (32, 128, "diag", "max", 0, 8116, ["zero", 1]),     # a block of zeros: its scale sits at the floor, byte 74
    (32, 128, "diag", "mse", 10, 8117, ["zero", 2]),    # ... and three candidates below it after a search, byte 71
    (16, 128, "diag", "mse", 0, 8118, ["negative", 0]),
    (64, 256, "diag", "mse", 0, 8119, ["outlier"]),     # one element of every block 8 to 64 times the rest
    (32, 256, "err", "diag", 10, 8120, ["outlier"]),
    (512, 256, "diag", "mse", 0, 8121, None),           # a taller layer: hashes only
]


def main():
    cb = Codebook(mx_model.VALUES)
    out = {}
    meta = []
    chosen = {f: 0 for f in FACTORS}
    for i, (R, n, order, mode, moves, seed, special) in enumerate(CASES):
        t0 = time.time()
        c = dict(R=R, n=n, act_order=order, mode=mode, moves=moves, seed=seed, special=special, damp=0.01, min_block_size=32,
                 num_blocks=8)
        L = mx_model.case_layer(c)
        W, H = L["W"].astype(np.float32), L["H"].astype(np.float32)
        S = reference_scales(W, H, cb, mode, chosen)
        E = mx_model.encode_model(S)
        assert E.min() >= 71 and E.max() <= 253
        if special and special[0] == "zero":
            assert (E[:, special[1]] == (74 if mode == "max" else 71)).all()
        assert_no_tied_keys(L["W"], S, L["H"], order, 0.01)
        Q0 = quantize_grouped_ref(L["W"], S, cb, L["H"], G, order, 0.01, 32, 8)
        idx0 = indices(cb, Q0, S, G)
        Q, near = (Q0, None) if moves == 0 else search_records(W, Q0, H, cb, S, G, moves)
        idx = indices(cb, Q, S, G)
        codes, _ = mx_model.pack_model(idx, S)
        assert np.array_equal(mx_model.dequantize_model(codes, E).view(np.uint32), Q.view(np.uint32)), "Q is not +-magnitude * 2^e"
        out[f"E_{i}"] = E
        out[f"row_hash_{i}"] = row_hashes(idx)
        if R * n <= SMALL_IDX:
            out[f"idx_{i}"] = idx
        if near is not None:
            for k, v in near.items():
                out[f"near_{i}/{k}"] = v
        meta.append(dict(c, sha256_idx0=sha(idx0), sha256_idx=sha(idx), sha256_codes=sha(codes), changed=int((idx != idx0).sum())))
        print(f"case {i}: {R}x{n} {order} {mode} {moves} moves {special}: {meta[-1]['changed']} indices changed, "
              f"{0 if near is None else len(near['rows'])} near-tie rows, {time.time() - t0:.1f} s", flush=True)
    print("factors chosen:", chosen)
    assert all(v > 0 for v in chosen.values()), "a factor was never chosen"
    out["meta"] = np.array(json.dumps(dict(cases=meta, near_tie_limit=NEAR_TIE_LIMIT, factors_chosen={str(k): v for k, v in chosen.items()},
                                           numpy=np.__version__)))
    np.savez_compressed(os.path.join(HERE, "mx.npz"), **out)


if __name__ == "__main__":
    main()
