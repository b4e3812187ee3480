"""NumPy model of the local search on group-scaled layers (sleekit_amd.groups.local_search_grouped), built from oracle
pieces: oracle.obq_ref's per-row search state with the group quantizer's up / down neighbours as candidates.
tests/test_groups_ls_cpu.py pins it to the reference's own moves (tests/golden/groups_ls.npz), so the GPU tests may use it
as their oracle beyond the fixtures' shapes."""

import numpy as np

from oracle import obq_ref


class GroupCandidates:
    """quantize_up / quantize_down of the group quantizer of S over an oracle grid: codebook(x / s) / (1 / s), float32.
    Whole matrices by column; the 1-D arrays of a move at the entries `at` = (rows, cols) being changed."""

    def __init__(self, grid, S, g):
        self.grid, self.S, self.g, self.at = grid, S, g, None

    def _scales(self, x):
        if x.ndim == 2:
            return np.repeat(self.S, self.g, axis=1)
        rows, cols = self.at
        return self.S[rows, cols // self.g]

    def quantize_up(self, x):
        s = self._scales(x)
        return (self.grid.quantize_up(x / s) / (np.float32(1) / s)).astype(np.float32)

    def quantize_down(self, x):
        s = self._scales(x)
        return (self.grid.quantize_down(x / s) / (np.float32(1) / s)).astype(np.float32)


class _GroupedState(obq_ref._SearchState):
    """obq_ref's search state; a move first notes the entries it changes (their scales give the new candidates)."""

    def _apply(self, sign, mask):
        self.grid.at = (np.arange(self.W.shape[0])[mask], self.gain[sign].argmax(axis=1)[mask])
        super()._apply(sign, mask)


def local_search_grouped(W, Q, S, grid, H, g, moves, records=None):
    """local_search_grouped as NumPy: W unscaled, Q de-scaled, S (R, n / g), H undamped.  Returns Q itself for 0 moves.
    records (a list, optional): one obq_ref.move_record per move, as obq_ref.local_search fills it."""
    if moves == 0:
        return Q
    state = _GroupedState(W, Q, H, GroupCandidates(grid, S, g))
    noise = obq_ref.gain_noise_scale(W, Q, H) if records is not None else None
    for _ in range(moves):
        if records is not None:
            records.append(obq_ref.move_record(state.gain[+1], state.gain[-1], state.cand[+1] - state.Q,
                                               state.cand[-1] - state.Q, noise))
        state.move()
    return state.Q


def trace_of(records):
    """(R, moves) int32: the moves taken, in the device's trace convention (2 * column + up, -1 = none)."""
    return np.stack([r["choice"] for r in records], axis=1).astype(np.int32)
