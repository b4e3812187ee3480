"""NumPy model of the expert-grouped MX product (sleekit_amd.mx: matmul_mx_experts; slk_mx_gemm_experts), written from the
rules alone.

Offsets rule: offsets[0] == 0, offsets[e] <= offsets[e + 1], offsets[E] == M.  Tile tables, in expert order: an expert with
1 .. 64 rows gives ceil(m / 16) tiles of 16 rows, one with more gives ceil(m / 64) tiles of 64 rows, each entry (expert,
first row, row bound = the expert's last row + 1); invalid offsets give no tile at all.  The product: per expert, the
model of the dense product (tests/mx_gemm_model.py, mx_act4_model.py, mx_act6_model.py, mx6_model.py) on that expert's
rows, layer and bias row.
"""

import numpy as np

import mx6_model
import mx_act4_model
import mx_act6_model
import mx_gemm_model

SPLIT_MAX_M = 64


def offsets_valid(offsets, M):
    o = np.asarray(offsets).astype(np.int64)
    return bool(o.ndim == 1 and o.size >= 2 and o[0] == 0 and o[-1] == M and (np.diff(o) >= 0).all())


def tile_tables(offsets, M):
    """(valid, tiles16 (n16, 3), tiles64 (n64, 3)) as int32; both tables are empty when the offsets are invalid."""
    t16, t64 = [], []
    valid = offsets_valid(offsets, M)
    if valid:
        o = np.asarray(offsets).astype(np.int64)
        for e in range(o.size - 1):
            lo, hi = int(o[e]), int(o[e + 1])
            m = hi - lo
            if 1 <= m <= SPLIT_MAX_M:
                t16 += [(e, r, hi) for r in range(lo, hi, 16)]
            elif m > SPLIT_MAX_M:
                t64 += [(e, r, hi) for r in range(lo, hi, 64)]
    return valid, np.array(t16, np.int32).reshape(-1, 3), np.array(t64, np.int32).reshape(-1, 3)


def offsets_of(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)


DEQUANTIZE_ACT = {
    "mxfp8": mx_gemm_model.dequantize_act_model,
    "mxfp4": mx_act4_model.dequantize_act4_model,
    "mxfp6_e2m3": mx_act6_model.dequantize_act6_model,
}
DENSE_W4 = {"mxfp8": mx_gemm_model.matmul_model, "mxfp4": mx_act4_model.matmul_model, "mxfp6_e2m3": mx_act6_model.matmul_model}


def matmul_model(a_codes, a_scales, codes, scales, offsets, bias=None, activations="mxfp8", weights="mxfp4"):
    """(Y float64 (M, N), sum_k |a w| (M, N)): expert by expert, the dense model of the format pair on that expert's rows,
    layer and bias row.  Rows of no expert do not exist under valid offsets."""
    M, (E, N, _) = a_codes.shape[0], codes.shape
    assert offsets_valid(offsets, M) and len(offsets) == E + 1 and (weights == "mxfp4" or activations != "mxfp4")
    Y, S = np.zeros((M, N)), np.zeros((M, N))
    for e in range(E):
        lo, hi = int(offsets[e]), int(offsets[e + 1])
        if hi == lo:
            continue
        b = None if bias is None else bias[e]
        if weights == "mxfp4":
            Y[lo:hi], S[lo:hi] = DENSE_W4[activations](a_codes[lo:hi], a_scales[lo:hi], codes[e], scales[e], b)
        else:
            A = np.asarray(DEQUANTIZE_ACT[activations](a_codes[lo:hi], a_scales[lo:hi]), np.float64)
            Y[lo:hi], S[lo:hi] = mx6_model.matmul_model(A, codes[e], scales[e], b)
    return Y, S
