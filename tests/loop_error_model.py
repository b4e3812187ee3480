"""NumPy model of the layer error the loop carries (slk_gptq_quantize_batch_error), for the tests.

With Hd = H + lambda I the damped Hessian the factor was made from (U^T U = Hd[order][:, order]^-1) and
E[r, j] = (w'_j - q_j) / U[j, j] the scaled errors the loop stores for every column (obq.py:115), row by row

    (Ws - Q) Hd (Ws - Q)^T  =  sum_j E[r, j]^2                                      (scaled domain, any column order)
    (W - Qw) H  (W - Qw)^T  =  scale_r^2 * sum_j E[r, j]^2  -  lambda * sum_j (W - Qw)[r, j]^2

The kernel's arithmetic: float32 differences of the stored values, float64 squares and sums, lambda the float32 damping
term, the result rounded to float32.
"""

import numpy as np

from oracle import obq_ref
from oracle.grid import UniformGrid


def damping_term(H, damp):
    """float32(damp) * mean(diag H) in float32, as obq.py:198 forms it under NEP 50."""
    return np.float32(damp) * H.diagonal().mean(dtype=np.float32)


def carried_row_errors(W, Qw, E, H, damp, scale=None):
    """row_err (R,) float32 from the loop's E (any column order), W and the de-scaled Q the caller receives."""
    lam = damping_term(H.astype(np.float32), damp)
    d = (W.astype(np.float32) - Qw.astype(np.float32)).astype(np.float64)
    s_e = np.square(E.astype(np.float64)).sum(axis=1)
    s_d = np.square(d).sum(axis=1)
    s = np.ones(W.shape[0]) if scale is None else scale.astype(np.float64)
    return ((s * s) * s_e - np.float64(lam) * s_d).astype(np.float32)


def product_row_errors(W, Qw, H):
    """(W - Qw) H (W - Qw)^T per row in float64, of the float32 values as stored."""
    D = W.astype(np.float64) - Qw.astype(np.float64)
    return ((D @ H.astype(np.float64)) * D).sum(axis=1)


def quantize(W, H, grid, scale=None, order="diag", damp=0.01):
    """The oracle's loop on W / scale; returns (Qw, E): the de-scaled Q (scaling.py:80: a division by the reciprocal) and
    the scaled errors in processing order."""
    W = W.astype(np.float32)
    Ws = W if scale is None else (W / scale[:, None]).astype(np.float32)
    Q, _, _, E = obq_ref.quantize_layer_debug(Ws, H, grid, order_mode=order, damp=damp)
    Qw = Q if scale is None else (Q / (np.float32(1.0) / scale)[:, None]).astype(np.float32)
    return Qw, E


def uniform(levels):
    return UniformGrid(levels, -1.0, 1.0)


def decaying_hessian(n=1024, seed=7):
    """A Hessian with a steeply decaying spectrum: column scales k^-1.5 mixed by a random matrix; bit-wise symmetric float32."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((2 * n, n)) * (np.arange(1, n + 1, dtype=np.float64) ** -1.5)[None, :]
    X = X @ (rng.standard_normal((n, n)) / np.sqrt(n))
    H = (X.T @ X) / X.shape[0]
    return ((H + H.T) / 2).astype(np.float32)
