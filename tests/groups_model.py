"""NumPy model of group-wise scales (sleekit_amd.groups), built from oracle pieces: the group quantizer, the grouped loop
and the per-group scale search.  tests/test_groups_cpu.py pins it to the reference's own results (tests/golden/groups.npz
and groups_edges.npz), so the GPU tests may use it as their oracle beyond the fixtures' shapes."""

import numpy as np

from oracle import grid, obq_ref, scaling_ref


class GroupGrid:
    """The group quantizer over an oracle grid: whole matrices by column, leaf columns in processing order."""

    def __init__(self, grid, S, g, order):
        self.grid, self.S, self.g, self.order, self.i = grid, S, g, order, 0

    def __call__(self, x):
        if x.ndim == 2:
            s = np.repeat(self.S, self.g, axis=1)
        else:
            s = self.S[:, self.order[self.i] // self.g]
            self.i += 1
        return (self.grid.value(x / s) / (np.float32(1) / s)).astype(np.float32)


def model_grouped(W, S, grd, H, g, act_order, damp, mb, nb, ties="numpy", factor=None):
    """quantize_grouped as NumPy, from oracle.obq_ref's pieces.

    ties: "numpy" breaks exact key ties like the reference's argsort, "stable" by column index like the device
    (obq_ref.column_order).  factor = (order, U): the loop on a given factor, as quantize_layer_grouped(factor=...) runs
    it; H, act_order and damp are then not used."""
    n = W.shape[1]
    if factor is None:
        H_damped = H + damp * H.diagonal().mean() * np.eye(n)
        order = obq_ref.column_order(W, H_damped, GroupGrid(grd, S, g, None), act_order, ties)
        U = obq_ref.inverse_factor_upper(H_damped[order][:, order])
    else:
        order, U = factor
    Q = W[:, order].copy()
    E = np.zeros_like(Q)
    Z = GroupGrid(grd, S, g, order)
    obq_ref.run_schedule(Q, E, U, Z, obq_ref.block_schedule(n, mb, nb))
    assert Z.i == n
    return Q[:, np.argsort(order)]


def group_scales_model(W, grd, H, g, mode, **search):
    """compute_group_scaling as NumPy: column k is oracle.scaling_ref.pick_scale of the k-th column block of W with the
    k-th diagonal block of H (the reference's compute_scaling per group)."""
    n = W.shape[1]
    cols = [scaling_ref.pick_scale(W[:, k:k + g], grd, None if H is None else H[k:k + g, k:k + g], mode, **search)
            for k in range(0, n, g)]
    return np.stack(cols, axis=1).astype(np.float32)


def oracle_grid(name):
    return grid.TableGrid.nf4() if name == "nf4" else grid.UniformGrid(int(name), -1, 1)


def indices(Q, S, grd, g):
    """uint8 codebook indices of Q / S (what quantize_grouped(return_indices=True) returns)."""
    return grd.index(Q / np.repeat(S, g, axis=1)).astype(np.uint8)


def rebuild(idx, S, name, g):
    """Q = value(idx) / (1 / s): the codebook value formed like quantize_value (t * step + zero in float32, or the table)."""
    if name == "nf4":
        vals = np.asarray(grid.TableGrid.nf4().values, np.float32)[idx]
    else:
        levels = int(name)
        vals = idx.astype(np.float32) * np.float32(2 / (levels - 1)) + np.float32(-1)
    return (vals / (np.float32(1) / np.repeat(S, g, axis=1))).astype(np.float32)
