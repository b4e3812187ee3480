"""NumPy model of the MoE route (sleekit_amd/routing.py, sleekit_amd/csrc/moe.hip), written from the rules alone.

Selection: expert a ranks before expert b when v[a] > v[b], or v[a] == v[b] and a < b -- a stable argsort of -v with -0
normalised to +0.  Gates: m = the row's largest logit, e = exp(v - m), g = e / s; "selected" sums the k selected e's, "all"
every expert's.  gates_f32 follows the kernel's float32 order of operations but for expf itself (NumPy's float32 exp may
differ from the device's in the last place: the test that compares bits uses rows where exp is exact); gates_f64 is the
same function in float64 on the same float32 logits.  The sort is a stable argsort plus counts, the row-mapped quantizer the
existing quantizer models on x[rows // div], the combine the ordered float32 sum."""

import numpy as np

import mx_act4_model
import mx_act6_model
import mx_gemm_model


def normalised(v):
    """float32 logits with -0 as +0 (the two tie)."""
    v = np.asarray(v, np.float32).copy()
    v[v == 0] = 0.0
    return v


def row_flagged(v, k):
    """Whether a row of logits is refused: a NaN, +inf, or fewer than k logits above -inf."""
    v = np.asarray(v, np.float32)
    return bool(np.isnan(v).any() or np.isposinf(v).any() or (v > -np.inf).sum() < k)


def topk_ids(logits, k):
    """(T, k) int32: column j the expert of the j-th largest logit, ties to the lower index."""
    L = np.atleast_2d(np.asarray(logits, np.float32))
    return np.stack([np.argsort(-normalised(row), kind="stable")[:k] for row in L]).astype(np.int32)


def _tree16(e):
    """((e0 + e1) + (e2 + e3)) + ... of 16 float32 values, the kernel's row sum."""
    e = np.asarray(e, np.float32)
    while e.size > 1:
        e = (e[0::2] + e[1::2]).astype(np.float32)
    return e[0]


def gates_f32(logits, k, gating="selected"):
    """(T, k) float32 gates in the kernel's order of float32 operations (NumPy's exp in place of expf)."""
    L = np.atleast_2d(np.asarray(logits, np.float32))
    ids = topk_ids(L, k)
    out = np.zeros((L.shape[0], k), np.float32)
    for t, row in enumerate(L):
        if row_flagged(row, k):
            continue
        v = normalised(row)
        m = v[ids[t, 0]]
        with np.errstate(invalid="ignore"):
            e_sel = np.exp((v[ids[t]] - m).astype(np.float32)).astype(np.float32)
            if gating == "selected":
                s = _tree16(np.concatenate([e_sel, np.zeros(16 - k, np.float32)]))
            else:
                e_all = np.exp((v - m).astype(np.float32)).astype(np.float32)
                lanes = np.zeros(64, np.float32)
                for l in range(min(64, v.size)):
                    acc = e_all[l]
                    for i in range(l + 64, v.size, 64):
                        acc = np.float32(acc + e_all[i])
                    lanes[l] = acc
                r = [_tree16(lanes[16 * i:16 * i + 16]) for i in range(4)]
                s = np.float32(np.float32(r[0] + r[1]) + np.float32(r[2] + r[3]))
        out[t] = (e_sel / s).astype(np.float32)
    return out


def gates_f64(logits, k, gating="selected"):
    """(T, k) float64 gates of the same float32 logits; a refused row's are 0."""
    L = np.atleast_2d(np.asarray(logits, np.float32))
    ids = topk_ids(L, k)
    out = np.zeros((L.shape[0], k), np.float64)
    for t, row in enumerate(L):
        if row_flagged(row, k):
            continue
        v = normalised(row).astype(np.float64)
        e = np.exp(v - v[ids[t, 0]])
        out[t] = e[ids[t]] / (e[ids[t]].sum() if gating == "selected" else e.sum())
    return out


def sort_model(ids, E):
    """(order, pos, offsets, bad) of flat expert ids: the stable sort of the ids clamped into 0 .. E - 1, its inverse, the
    E + 1 offsets, and whether an id was outside the range."""
    ids = np.asarray(ids).reshape(-1).astype(np.int64)
    bad = bool(((ids < 0) | (ids >= E)).any())
    key = np.clip(ids, 0, E - 1)
    order = np.argsort(key, kind="stable").astype(np.int32)
    pos = np.empty_like(order)
    pos[order] = np.arange(order.size, dtype=np.int32)
    offsets = np.concatenate([[0], np.cumsum(np.bincount(key, minlength=E))]).astype(np.int32)
    return order, pos, offsets, bad


QUANTIZERS = {"mxfp8": mx_gemm_model.quantize_act_model, "mxfp4": mx_act4_model.quantize_act4_model, "mxfp6_e2m3": mx_act6_model.quantize_act6_model}


def quantize_rows_model(X, rows, div, activations):
    """(a_codes, a_scales) of X[rows // div] by the plain quantizer's model; a source row outside X reads as zeros."""
    X, src = np.asarray(X, np.float32), np.asarray(rows, np.int64) // div
    ok = (np.asarray(rows) >= 0) & (src < X.shape[0])
    G = np.where(ok[:, None], X[np.where(ok, src, 0)], np.float32(0))
    return QUANTIZERS[activations](G)


def combine_model(Y, pos, gates, T, k):
    """(T, N) float32: sum_j gates[t][j] * Y[pos[t k + j]] in float32, product then sum, j = 0, 1, ..., k - 1; gates None: ones."""
    Y = np.asarray(Y, np.float32)[np.asarray(pos).reshape(T, k)]
    total = None
    for j in range(k):
        term = Y[:, j] if gates is None else (Y[:, j] * np.asarray(gates, np.float32)[:, j:j + 1]).astype(np.float32)
        total = term if total is None else (total + term).astype(np.float32)
    return total
