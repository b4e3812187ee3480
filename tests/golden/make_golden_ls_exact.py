#!/usr/bin/env python3
"""Generate tests/golden/ls_exact.npz -- the local search on exact ("dyadic") layers -- by running the REAL reference.

Run only where the reference is available (same pattern as make_golden_groups_ls.py; SLEEKIT_REF overrides its location):

    python tests/golden/make_golden_ls_exact.py

Inputs come from tests/ls_exact_model.py (keyed by the seeds and parameters stored here); only outputs are written.  On
these layers every float32 operation of the search is exact, so the reference's moves do not depend on its BLAS: what is
stored is its behaviour at exact ties (np.argmax: the first column; down when best_up == best_down), recorded rather than
inferred from the oracle.  For every case the reference's own LocalSearchQuantizer(W, Q0, H, codebook) is driven move by
move as quantize_local_search drives it; the move of every row is read off its Q before and after each do_move(), and
checked against what ls_exact_model.decision (which only inspects arrays) reads off the gain arrays beforehand.

Stored per case: the reference's trace (int32, R x moves: 2 * column + up, -1 = none) and the final codebook indices (uint8;
the final Q itself, float32, for the 257-level grid, whose indices do not fit a byte).

No reference source text is copied.
"""

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.environ.get("SLEEKIT_REF", "/root/reference"))

import numpy as np  # noqa: E402

import ls_exact_model as M  # noqa: E402

import sleekit.codebook as ref_codebook  # noqa: E402
import sleekit.obq as ref_obq  # noqa: E402

# random cases: (n, grid, symmetric); the plateau case: rows of (kind, columns) at n = 1024
CASES = [
    dict(n=7, grid="9", symmetric=True),
    dict(n=96, grid="9", symmetric=True),
    dict(n=300, grid="9", symmetric=True),
    dict(n=1100, grid="9", symmetric=True),
    dict(n=1100, grid="table", symmetric=True),
    dict(n=1100, grid="257", symmetric=True),
    dict(n=300, grid="9", symmetric=False),
    dict(n=1024, grid="9", symmetric=True,
         plateau=[["updown", [2, 9]], ["updown", [0, 1023, 5]], ["down", [2, 9]], ["down", [3, 259, 700]]]),
]


def reference_moves(W, Q0, H, cb, moves):
    """The reference's final Q and its moves as OBSERVED: Q before and after every do_move() gives the column that moved
    and its direction (at most one per row and move).  What ls_exact_model.decision reads off the gain arrays beforehand
    -- the tie rule as the tests state it -- must say the same, a "stay" (no entry of the row changed) included."""
    ls = ref_obq.LocalSearchQuantizer(W, Q0, H, cb)
    rows = np.arange(W.shape[0])
    trace = np.full((W.shape[0], moves), -1, dtype=np.int32)
    for m in range(moves):
        foretold = M.decision(ls.gain_up, ls.gain_down, ls.Q, ls.Q_up, ls.Q_down)[0]
        before = ls.Q.copy()
        ls.do_move()
        changed = ls.Q != before
        assert (changed.sum(axis=1) <= 1).all()
        col = changed.argmax(axis=1)
        up = ls.Q[rows, col] > before[rows, col]
        trace[:, m] = np.where(changed.any(axis=1), 2 * col + up, -1)
        assert np.array_equal(trace[:, m], foretold), (m, trace[:, m], foretold)
    return ls.Q, trace


def main():
    out, meta = {}, []
    for i, c in enumerate(CASES):
        c = dict(c, moves=M.MOVES)
        if "plateau" not in c:
            c["R"] = M.rows_of(c["n"])
            c["seed"] = M.SEEDS.get((c["n"], c["grid"], c["symmetric"]), M.SEED + c["n"])
        W, Q0, H = M.fixture_inputs(c)
        cb = M.reference_codebook(ref_codebook, c["grid"])
        Q, trace = reference_moves(W, Q0, H, cb, c["moves"])
        assert Q.dtype == np.float32
        out[f"trace_{i}"] = trace
        if len(cb) <= 256:
            out[f"idx_{i}"] = np.asarray(cb.quantize_index(Q), dtype=np.uint8)
            assert np.array_equal(cb.quantize_value(Q), Q)
        else:
            out[f"Q_{i}"] = Q
        c["changed"] = int((Q != Q0).sum())
        meta.append(c)
        print(f"case {i}: {c}: {int((trace >= 0).sum())} moves", flush=True)
    out["meta"] = np.array(json.dumps(dict(cases=meta, numpy=np.__version__)))
    np.savez_compressed(os.path.join(HERE, "ls_exact.npz"), **out)


if __name__ == "__main__":
    main()
