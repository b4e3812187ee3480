"""Group-wise scales: one scale per row and per group of `g` columns, from the scale search through the GPTQ loop.

    S = compute_group_scaling(W, cb, g, H, mode="diag")        # (R, n / g) float32
    Q = quantize_grouped(W, S, cb, H, g, act_order="sqerr")     # de-scaled values, like W
    Q, idx = quantize_grouped(..., return_indices=True)         # idx uint8: (idx, S) is the compact form of the layer
    Q == dequantize_grouped(idx, S, cb, g)                      # bit for bit
    Q = quantize_grouped(..., nb_ls_moves=100)                  # then the best-first local search, group quantizer's candidates
    Q = local_search_grouped(W, Q, S, cb, H, g, 100)            # the search alone
    O = compute_group_offsets(W, g)                             # (R, n / g) float32: each group's midpoint
    S = compute_group_scaling(W, cb, g, H, mode="mse", offsets=O)   # the scales of the centred weights W - O
    Q, idx = quantize_grouped_asym(W, S, O, cb, H, g, return_indices=True)
    Q == dequantize_grouped(idx, S, cb, g, offsets=O)           # bit for bit: (idx, S, O) is the compact form

Element (r, c) belongs to group c // g.  The GROUP QUANTIZER maps x in column c of row r to

    codebook.quantize_value(x / s) / (np.float32(1) / s),   s = S[r, c // g]

(float32 IEEE divides: the arithmetic of sleekit/scaling.py:73, 80).  `quantize_grouped` returns what the reference's
own `quantize_opt(W, H, Z, act_order, damp, 0, min_block_size, num_blocks)` (sleekit/obq.py:169-217) returns for a
callable Z that applies the group quantizer by column: the loop runs on the UNSCALED weights with the reference's rank-1
and block updates, only the leaves scale, and the err / sqerr keys come from Z(W) - W in original units.
`local_search_grouped` is the reference's `quantize_local_search(W, Q, H, quantizer, nb_moves)` (sleekit/obq.py:234-358)
with that quantizer's up / down neighbours as candidates: codebook.quantize_up(x / s) / (np.float32(1) / s) for x in column
c, s = S[r, c // g], with the reference's gains, decisions and incremental updates.
`compute_group_scaling` gives column k of S as the reference's `compute_scaling` of the k-th column block of W with
the k-th diagonal block of H.

ASYMMETRIC groups: an offset o = O[r, c // g] per group beside the scale, and the quantizer

    codebook.quantize_value((x - o) / s) / (np.float32(1) / s) + o

(float32 IEEE in exactly this order: subtract, divide, codebook, divide, add; O = 0 gives the group quantizer).  With
offsets O, quantize_grouped_asym (and quantize_layer_grouped(..., offsets=O)) is quantize_opt with that quantizer (the loop still runs on the unscaled, uncentred W; the
err / sqerr keys come from Z(W) - W), compute_group_scaling is the symmetric search on the centred weights W - O (O
repeated over each group, a float32 subtract), and dequantize_grouped rebuilds Q from (idx, S, O) bit for bit.
`compute_group_offsets` gives each group's midpoint, np.float32(0.5) * (min + max).  Offsets have no local search yet
(NotImplementedError with nb_ls_moves > 0).

Same conventions as the rest of the package: NumPy in gives NumPy out, device tensors in give device tensors out, and
every step runs on the GPU (no CPU fallback).
"""

import numpy as np
import torch

from . import _device as dev
from . import _lib
from . import engine
from . import scaling

_MODES = ("max", "mse", "diag", "hessian")  # and diagN / hessianN


def _groups(n, g):
    g = int(g)
    if g < 1 or n % g != 0:
        raise ValueError(f"group_size must be >= 1 and divide the {n} columns (got {g})")
    return g, n // g


def _diag_mean(Hb):
    """float32 mean of the diagonal of a square device matrix, summed in NumPy's order (slk_diag_mean)."""
    out = torch.empty(1, dtype=torch.float32, device=Hb.device)
    ws, ws_bytes = dev.workspace(0, Hb.shape[0])
    _lib.check(_lib.lib.slk_diag_mean(dev.ptr(Hb), Hb.shape[0], dev.ptr(out), dev.ptr(ws), ws_bytes, dev.stream_handle()))
    return out


def _check_offsets(O, R, n, g):
    """The device copy of the (R, n / g) float32 offsets."""
    Od = dev.to_device(O)
    if tuple(Od.shape) != (R, n // g) or Od.dtype != torch.float32:
        raise ValueError(f"group offsets must be float32 ({R}, {n // g}) for a ({R}, {n}) layer with group_size {g}; "
                         f"got {Od.dtype} {tuple(Od.shape)}")
    return Od.contiguous()


def compute_group_offsets(W, group_size, centred=False):
    """O (R, n / group_size) float32: the midpoint of each group's range, np.float32(0.5) * (min + max), in one pass over W.
    centred: (O, Wc), Wc = W - O (O repeated over each group, a float32 subtract) from the same pass -- what
    compute_group_scaling(W, ..., offsets=O) searches on, so compute_group_scaling(Wc, ...) gives the same S."""
    assert W.ndim == 2
    Wd = dev.to_device(W).contiguous()
    R, n = Wd.shape
    g, G = _groups(n, group_size)
    O = torch.empty((R, G), dtype=torch.float32, device=Wd.device)
    Wc = torch.empty_like(Wd) if centred else None
    _lib.check(_lib.lib.slk_group_midpoints(dev.ptr(Wd), g, R, n, dev.ptr(O), dev.ptr(Wc), dev.stream_handle()))
    return (dev.like_input(O, W), dev.like_input(Wc, W)) if centred else dev.like_input(O, W)


def center_groups(Wd, Od, group_size):
    """W - O by element, O repeated over each group (float32 subtract; device tensors)."""
    R, n = Wd.shape
    Wc = torch.empty_like(Wd)
    _lib.check(_lib.lib.slk_group_center(dev.ptr(Wd), dev.ptr(Od), int(group_size), R, n, dev.ptr(Wc), dev.stream_handle()))
    return Wc


def compute_group_scaling(W, codebook, group_size, H=None, mode="mse", min_factor=0.05, max_factor=1.0, grid_size=100,
                          offsets=None):
    """S (R, n / group_size) float32: column k is the reference's compute_scaling(W[:, k g : (k + 1) g], codebook,
    H[k g : (k + 1) g, k g : (k + 1) g], mode) (sleekit/scaling.py:193-238).  offsets (R, n / group_size): the same on the
    centred weights W - O.

    Modes max, mse, diag[N], hessian[N]; "obq" and "norm" raise NotImplementedError.  mse and diag search every group
    of every row in one launch; hessian runs the stacked search of sleekit_amd.scaling group by group (with that
    search's known deviation: near-tied grid points may fall the other way, see sleekit_amd.scaling).
    """
    assert W.ndim == 2
    cb_abi = engine.require_uniform(codebook)
    if mode in ("obq", "norm"):
        raise NotImplementedError(f'group scales support modes {", ".join(_MODES)} (and diagN / hessianN), not "{mode}"')
    if not (mode in ("max", "mse") or mode.startswith("diag") or mode.startswith("hessian")):
        raise RuntimeError(f"Unknown scaling mode {mode}")
    if mode not in ("max", "mse") and H is None:
        raise ValueError(f'scaling mode "{mode}" needs the Hessian H')
    Wd = dev.to_device(W)
    R, n = Wd.shape
    g, G = _groups(n, group_size)
    if offsets is not None:
        Wd = center_groups(Wd.contiguous(), _check_offsets(offsets, R, n, g), g)
    view = Wd.view(R * G, g)  # row r G + k = group k of row r: the reference's per-group problem, row for row
    if mode == "max":
        return dev.like_input(scaling._no_clip_scale(view, codebook).view(R, G), W)
    Hd = None if H is None else dev.to_device(H)
    if Hd is not None:
        assert Hd.shape == (n, n)
    kw = dict(min_factor=min_factor, max_factor=max_factor, grid_size=grid_size)
    if mode.startswith("hessian"):
        cols = []
        for k in range(G):
            Hk = Hd[k * g:(k + 1) * g, k * g:(k + 1) * g].contiguous()
            if len(mode) > 7:  # scaling.py:222-225 on the group's block
                Hk.diagonal().add_(np.float32(0.01 * float(mode[7:])) * Hk.diagonal().mean())
            cols.append(scaling.compute_min_mse_scaling(Wd[:, k * g:(k + 1) * g].contiguous(), codebook, H=Hk, **kw))
        return dev.like_input(torch.stack(cols, dim=1).contiguous(), W)
    hd = None
    if mode.startswith("diag"):
        hd = Hd.diagonal().contiguous()
        if len(mode) > 4:  # scaling.py:226-229: each group's penalty is from its own block's mean diagonal
            pen = np.float32(0.01 * float(mode[4:]))
            parts = []
            for k in range(G):
                mean = _diag_mean(Hd[k * g:(k + 1) * g, k * g:(k + 1) * g].contiguous())
                parts.append(hd[k * g:(k + 1) * g] + mean * float(pen))  # float32(pen) * mean, rounded once
            hd = torch.cat(parts).contiguous()
    base = scaling._no_clip_scale(view, codebook)
    factors = torch.from_numpy(np.linspace(min_factor, max_factor, grid_size, dtype=np.float32)).to(Wd.device)
    out = torch.empty(R * G, dtype=torch.float32, device=Wd.device)
    levels, lo, hi, table = cb_abi
    _lib.check(
        _lib.lib.slk_scale_search_grouped(
            dev.ptr(Wd), dev.ptr(base), dev.ptr(factors), grid_size, dev.ptr(hd), g, R, n, levels, lo, hi, dev.ptr(table),
            dev.ptr(out), dev.stream_handle(),
        )
    )
    return dev.like_input(out.view(R, G), W)


def column_miss_grouped(W, S, group_size, cb_abi, squared, O=None):
    """engine.column_miss with the group quantizer (O given: the asymmetric one), device tensors."""
    return engine.column_miss(W, cb_abi, squared, S, group_size, O)


def grouped_keys(W, S, group_size, cb_abi, act_order, H, damp, O=None):
    """engine.sort_keys of a grouped layer."""
    return engine.sort_keys(W, H, cb_abi, act_order, damp, gscale=S, group_size=group_size, goffset=O)


def run_loop_batch_grouped(W, S, order, U, cb_abi, group_size, min_block, num_blocks, want_idx=True, offsets=None):
    """The grouped loop over a batch of layers stacked by rows (engine.gptq_loop).

    W (B, R, n) float32, S (B, R, n / group_size) float32, order (B, n) int64, U (B, n, n) float64, all contiguous.
    Returns (Q, idx) shaped (B, R, n), Q de-scaled: what B single-layer grouped loops return, in launches that cover all B.
    offsets (B, R, n / group_size) float32, contiguous: the asymmetric loop.
    """
    assert W.dim() == 3
    g, _ = _groups(W.shape[2], group_size)
    return engine.gptq_loop(W, cb_abi, order, U, min_block, num_blocks, gscale=S, group_size=g, goffset=offsets, want_idx=want_idx)[:2]


def run_search_grouped(W, Q, S, H, cb_abi, group_size, moves, idx=None, want_trace=False, row_err=None):
    """engine.local_search with the group quantizer's candidates, in place on Q (and idx) (device tensors): W, Q (R, n),
    S (R, n / group_size), H (n, n)."""
    return engine.local_search(W, Q, H, cb_abi, moves, idx, want_trace=want_trace, row_err=row_err, gscale=S, group_size=group_size)


def _check_scales(S, R, n, g):
    g, G = _groups(n, g)
    if tuple(S.shape) != (R, G):
        raise ValueError(f"group scales must be ({R}, {G}) for a ({R}, {n}) layer with group_size {g}; got {tuple(S.shape)}")
    return g


def local_search_grouped(W, Q, S, quantizer, H, group_size, nb_moves, return_indices=False):
    """Best-first local search with the group quantizer's candidates (module docstring): the grouped counterpart of
    obq.quantize_local_search.  W unscaled, Q de-scaled (what quantize_grouped returns), S (R, n / group_size), H the
    undamped Hessian in original column order.  Returns Q itself when nb_moves == 0.  return_indices: (Q, idx) with idx the
    uint8 codebook indices of Q / S (dequantize_grouped(idx, S, quantizer, group_size) == Q bit for bit)."""
    assert W.ndim == 2 and H.ndim == 2 and Q.shape == W.shape and H.shape[0] == H.shape[1] == W.shape[1]
    cb_abi = engine.require_uniform(quantizer)
    if return_indices and cb_abi[0] > 256:
        raise ValueError("uint8 indices need a codebook of at most 256 entries")
    R, n = W.shape
    g = _check_scales(S, R, n, group_size)
    if nb_moves == 0 and not return_indices:
        return Q
    Wd, Sd, Hd = dev.to_device(W), dev.to_device(S), dev.to_device(H)
    Qd = dev.to_device(Q).clone()
    idx = torch.empty((R, n), dtype=torch.uint8, device=Wd.device) if return_indices else None
    run_search_grouped(Wd, Qd, Sd, Hd, cb_abi, g, nb_moves, idx)
    Qo = Q if nb_moves == 0 else dev.like_input(Qd, W)
    return (Qo, dev.like_input(idx, W)) if return_indices else Qo


def quantize_layer_grouped(W, S, quantizer, H, group_size, act_order="diag", damp=0.01, min_block_size=32, num_blocks=8,
                           want_idx=True, factor=None, lookahead=True, nb_ls_moves=0, want_ls_trace=False, offsets=None):
    """The grouped layer on device tensors (engine.quantize_layer with gscale): W (R, n), S (R, n / group_size), H (n, n), all
    float32.  Returns an engine.LayerResult (Q de-scaled, idx uint8 or None, order, U, info); raises LinAlgError if H + damping is not
    positive definite.  `factor` = (order, U, info) re-uses a factor made elsewhere (sleekit_amd.dist: a row shard), as
    engine.quantize_layer does; its status is then the caller's to check.  lookahead: this layer is alone on the GPU
    (engine.factorize).  nb_ls_moves > 0: the local search (local_search_grouped) runs after the loop, on Q and idx in
    place; res.ls_error holds the rows' errors after the moves (carried through the search) and, with want_ls_trace,
    res.ls_trace the moves taken.  offsets (R, n / group_size): the asymmetric group quantizer (no local search)."""
    assert W.ndim == 2 and H.ndim == 2 and H.shape[0] == H.shape[1] == W.shape[1]
    assert min_block_size >= 1
    cb_abi = engine.require_uniform(quantizer)
    R, n = W.shape
    g = _check_scales(S, R, n, group_size)
    if want_idx and cb_abi[0] > 256:
        raise ValueError("uint8 indices need a codebook of at most 256 entries")
    O = None
    if offsets is not None:
        if nb_ls_moves > 0:
            raise NotImplementedError("local search with group offsets is not supported (nb_ls_moves must be 0)")
        O = _check_offsets(offsets, R, n, g)
    return engine.quantize_layer(W, H, quantizer, None, act_order, damp, nb_ls_moves, min_block_size, num_blocks, factor,
                                 want_idx=want_idx, want_ls_trace=want_ls_trace, lookahead=lookahead, gscale=S, group_size=g, goffset=O)


def quantize_grouped(W, S, quantizer, H, group_size, act_order="diag", damp=0.01, min_block_size=32, num_blocks=8,
                     return_indices=False, nb_ls_moves=0):
    """GPTQ-style quantization of one layer with group scales S (R, n / group_size).

    Returns the de-scaled values Q (float32, shaped like W): what sleekit/obq.py:169-217 returns for the group quantizer
    (module docstring), with nb_ls_moves of its local search after the loop.  return_indices: (Q, idx) with idx the uint8
    codebook indices of Q / S.  (The asymmetric form, with offsets, is quantize_grouped_asym.)
    """
    assert W.ndim == 2 and H.ndim == 2
    res = quantize_layer_grouped(dev.to_device(W), dev.to_device(S), quantizer, dev.to_device(H), group_size, act_order, damp,
                                 min_block_size, num_blocks, want_idx=return_indices, nb_ls_moves=nb_ls_moves)
    Q = dev.like_input(res.Q, W)
    return (Q, dev.like_input(res.idx, W)) if return_indices else Q


def quantize_grouped_asym(W, S, O, quantizer, H, group_size, act_order="diag", damp=0.01, min_block_size=32, num_blocks=8,
                          return_indices=False):
    """quantize_grouped with offsets O (R, n / group_size) beside the scales: the asymmetric group quantizer (module
    docstring).  return_indices: (Q, idx), from which dequantize_grouped(idx, S, quantizer, group_size, offsets=O) rebuilds
    Q bit for bit.  No local search with offsets yet.  (quantize_grouped keeps its parameter list, return_indices and
    nb_ls_moves included, as it was; the offset form is this sibling.)"""
    assert W.ndim == 2 and H.ndim == 2
    res = quantize_layer_grouped(dev.to_device(W), dev.to_device(S), quantizer, dev.to_device(H), group_size, act_order, damp,
                                 min_block_size, num_blocks, want_idx=return_indices, offsets=O)
    Q = dev.like_input(res.Q, W)
    return (Q, dev.like_input(res.idx, W)) if return_indices else Q


def dequantize_grouped(idx, S, codebook, group_size, offsets=None):
    """Q[r, c] = value(idx[r, c]) / (1 / S[r, c // group_size]) (+ offsets[r, c // group_size]): bit for bit the Q of
    quantize_grouped."""
    assert idx.ndim == 2
    levels, lo, hi, table = engine.require_uniform(codebook)
    idx_d = dev.to_device(idx, torch.uint8)
    Sd = dev.to_device(S)
    R, n = idx_d.shape
    g = _check_scales(Sd, R, n, group_size)
    Q = torch.empty((R, n), dtype=torch.float32, device=Sd.device)
    if offsets is not None:
        Od = _check_offsets(offsets, R, n, g)
        _lib.check(
            _lib.lib.slk_dequantize_grouped_asym(dev.ptr(idx_d), dev.ptr(Sd), dev.ptr(Od), g, R, n, levels, lo, hi, dev.ptr(table),
                                                 dev.ptr(Q), dev.stream_handle())
        )
        return dev.like_input(Q, idx)
    _lib.check(
        _lib.lib.slk_dequantize_grouped(dev.ptr(idx_d), dev.ptr(Sd), g, R, n, levels, lo, hi, dev.ptr(table), dev.ptr(Q),
                                        dev.stream_handle())
    )
    return dev.like_input(Q, idx)
