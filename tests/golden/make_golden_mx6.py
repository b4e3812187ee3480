#!/usr/bin/env python3
"""Generate tests/golden/mx6.npz -- MXFP6 (E2M3) layers (sleekit_amd.mx) -- by running the REAL reference.

Run only where the reference is available (the pattern of make_golden_mx.py; SLEEKIT_REF gives its location, by default a
`reference` directory beside this repository):

    python tests/golden/make_golden_mx6.py

Inputs come from the build's own generator (tests/mx6_model.py: case_layer, keyed by the seeds and the `special` stored
here); only outputs are written.  For every case, with cb = sleekit.codebook.Codebook of the 63 E2M3 values, E, Q0 and Q are
make_golden_mx.py's, computed by its own functions with this codebook: the reference's loop body over the power-of-two
candidates for the scales, sleekit.obq.quantize_opt with the group quantizer of S = 2^(E - 127), g = 32, and the reference's
LocalSearchQuantizer driven move by move.

Checked here before writing: Q0 and Q are values[idx] / (1 / s) bit for bit (make_golden_groups.indices) AND
+-magnitude[code & 31] * 2^(E - 127) bit for bit; no two order keys tie exactly; each of the four factors is chosen somewhere
(the "small_diag" case is there for the two lowest).

Stored per case: E (uint8), the SHA-256 of the indices after the loop and after the moves, one 64-bit hash per row of the
final indices, the final indices themselves for cases of at most SMALL_IDX elements, the SHA-256 of the final codes bytes
(the stream of 6-bit codes), and the near-tie records of the search cases.

No reference source text is copied.
"""

import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden_mx import FACTORS, G, SMALL_IDX, reference_scales  # noqa: E402  (sets the paths, imports the reference)

import numpy as np  # noqa: E402

from make_golden import NEAR_TIE_LIMIT, row_hashes, sha  # noqa: E402
from make_golden_groups import indices, quantize_grouped_ref  # noqa: E402
from make_golden_groups_ls import search_records  # noqa: E402

import mx6_model  # noqa: E402  (the inputs, and the bit-level form of the codes: no model arithmetic enters E, Q0 or Q)

from sleekit.codebook import Codebook  # noqa: E402


def assert_no_tied_keys(W, S, H, act_order, damp):
    from groups_model import GroupGrid
    from oracle import obq_ref

    Hd = H + damp * H.diagonal().mean() * np.eye(H.shape[0])
    Z = GroupGrid(mx6_model.e2m3_grid(), S, G, None)
    a = obq_ref.column_order(W, Hd, Z, act_order, "numpy")
    b = obq_ref.column_order(W, Hd, Z, act_order, "stable")
    assert np.array_equal(a, b), "tied order keys: the reference's order is not the device's"


# (R, n, act_order, scale mode, moves, seed, special)
CASES = [
    (1, 32, "none", "max", 0, 9101, None),
    (16, 96, "diag", "mse", 10, 9102, None),                 # the general search kernel
    (17, 288, "err", "diag", 0, 9103, None),                 # 9 blocks a row
    (8, 1056, "sqerr", "mse", 0, 9104, None),                # a width whose summation tree is not regular
    (16, 768, "pivot", "mse", 10, 9105, None),               # a wave per row
    (32, 128, "inv_diag", "max", 0, 9106, ["zero", 1]),      # a block of zeros: its scale sits at the floor, byte 74
    (16, 128, "combined_diag", "mse", 0, 9107, ["negative", 0]),
    (64, 256, "diag", "diag", 0, 9108, ["small_diag", 5]),   # an outlier where diag(H) is 1e-4 of the rest: all four factors
    (24, 160, "diag", "mse", 0, 9109, ["outlier"]),
    (128, 256, "diag", "mse", 0, 9110, None),                # a taller layer: hashes only
]


def main():
    cb = Codebook(mx6_model.VALUES)
    assert len(cb) == 63
    out = {}
    meta = []
    chosen = {f: 0 for f in FACTORS}
    for i, (R, n, order, mode, moves, seed, special) in enumerate(CASES):
        t0 = time.time()
        c = dict(R=R, n=n, act_order=order, mode=mode, moves=moves, seed=seed, special=special, damp=0.01, min_block_size=32,
                 num_blocks=8)
        L = mx6_model.case_layer(c)
        W, H = L["W"].astype(np.float32), L["H"].astype(np.float32)
        before = dict(chosen)
        S = reference_scales(W, H, cb, mode, chosen)
        E = mx6_model.encode_model(S)
        assert E.min() >= 71 and E.max() <= 253
        if special and special[0] == "zero":
            assert (E[:, special[1]] == (74 if mode == "max" else 71)).all()
        if special and special[0] == "negative":
            assert (W[:, :G] < 0).all()
        if special and special[0] == "small_diag":
            assert all(chosen[f] > before[f] for f in FACTORS), "the small-diagonal case does not reach every factor"
            assert np.linalg.eigvalsh(H.astype(np.float64)).min() > 0
        assert_no_tied_keys(L["W"], S, L["H"], order, 0.01)
        Q0 = quantize_grouped_ref(L["W"], S, cb, L["H"], G, order, 0.01, 32, 8)
        idx0 = indices(cb, Q0, S, G)
        Q, near = (Q0, None) if moves == 0 else search_records(W, Q0, H, cb, S, G, moves)
        idx = indices(cb, Q, S, G)
        codes, _ = mx6_model.pack_model(idx, S)
        assert not (mx6_model.act6.unpack_codes(codes) == 0x20).any()
        assert np.array_equal(mx6_model.dequantize_model(codes, E).view(np.uint32), Q.view(np.uint32)), "Q is not +-magnitude * 2^e"
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
    path = os.path.join(HERE, "mx6.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(HERE, "mx.npz")), "larger than mx.npz"


if __name__ == "__main__":
    main()
