"""NumPy model of asymmetric group quantization (sleekit_amd.groups with `offsets`), built from oracle pieces: the
midpoint offsets, the asymmetric group quantizer, the grouped loop and the per-group scale search on the centred weights.
tests/test_groups_offsets_cpu.py pins it to the reference's own results (tests/golden/groups_offsets.npz), so the GPU
tests may use it as their oracle beyond the fixtures' shapes."""

import numpy as np

from groups_model import group_scales_model, oracle_grid
from oracle import obq_ref
from sleekit_amd import synth


class AsymGrid:
    """The asymmetric group quantizer over an oracle grid: whole matrices by column, leaf columns in processing order."""

    def __init__(self, grid, S, O, g, order):
        self.grid, self.S, self.O, self.g, self.order, self.i = grid, S, O, g, order, 0

    def __call__(self, x):
        if x.ndim == 2:
            s, o = np.repeat(self.S, self.g, axis=1), np.repeat(self.O, self.g, axis=1)
        else:
            k = self.order[self.i] // self.g
            s, o = self.S[:, k], self.O[:, k]
            self.i += 1
        return (self.grid.value((x - o) / s) / (np.float32(1) / s) + o).astype(np.float32)


def midpoints(W, g):
    """compute_group_offsets: np.float32(0.5) * (min + max) of every group, float32."""
    R, n = W.shape
    V = W.reshape(R, n // g, g)
    return (np.float32(0.5) * (V.min(axis=2) + V.max(axis=2))).astype(np.float32)


def centred(W, O, g):
    return (W - np.repeat(O, g, axis=1)).astype(np.float32)


def model_asym(W, S, O, grd, H, g, act_order, damp, mb, nb, ties="numpy", factor=None):
    """quantize_grouped_asym as NumPy: the loop on the unscaled, uncentred W.  factor = (order, U): the loop on a given
    factor, as quantize_layer_grouped(factor=..., offsets=O) runs it; H, act_order and damp are then not used."""
    n = W.shape[1]
    if factor is None:
        H_damped = H + damp * H.diagonal().mean() * np.eye(n)
        order = obq_ref.column_order(W, H_damped, AsymGrid(grd, S, O, g, None), act_order, ties)
        U = obq_ref.inverse_factor_upper(H_damped[order][:, order])
    else:
        order, U = factor
    Q = W[:, order].copy()
    E = np.zeros_like(Q)
    Z = AsymGrid(grd, S, O, g, order)
    obq_ref.run_schedule(Q, E, U, Z, obq_ref.block_schedule(n, mb, nb))
    assert Z.i == n
    return Q[:, np.argsort(order)]


def offsets_model(W, H, cbn, g, act_order, mode, damp, mb, nb, ties="numpy"):
    """(O, S, Q) of one fixture case: midpoints, the scale search on the centred weights, the asymmetric loop."""
    grd = oracle_grid(cbn)
    O = midpoints(W, g)
    S = group_scales_model(centred(W, O, g), grd, H, g, mode)
    return O, S, model_asym(W, S, O, grd, H, g, act_order, damp, mb, nb, ties)


def shaped_layer(R, n, g, seed, variant):
    """synth.make_layer shaped by a fixture variant (tests/golden/make_golden_offsets.py)."""
    L = synth.make_layer(R, n, seed)
    W = L["W"]
    if variant == "pos":
        W = np.abs(W) + np.float32(0.01)
    elif variant == "shift":
        W = W + np.float32(3) * np.abs(W).max()
    elif variant == "const":
        W[:, g:2 * g] = np.float32(0.37)
    elif variant == "huge":
        W[:, g:2 * g] = np.float32(4194304) + np.rint(W[:, g:2 * g] / np.abs(W).max() * 4).astype(np.float32)
    L["W"] = np.ascontiguousarray(W, dtype=np.float32)
    return L


def values(name, idx):
    """Codebook values of the indices, formed like quantize_value (t * step + zero in float32, or the table)."""
    if name == "nf4":
        return np.asarray(oracle_grid("nf4").values, np.float32)[idx]
    levels = int(name)
    return idx.astype(np.float32) * np.float32(2 / (levels - 1)) + np.float32(-1)


def rebuild(idx, S, O, name, g):
    """Q = value(idx) / (1 / s) + o."""
    return (values(name, idx) / (np.float32(1) / np.repeat(S, g, axis=1)) + np.repeat(O, g, axis=1)).astype(np.float32)
