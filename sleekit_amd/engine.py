"""Device-resident pipeline for one layer: the hot path end to end.

    [W / scale] -> column statistics -> damp + order + gather -> factor (float64)
               -> blocked quantize / propagate loop -> [local search] -> [un-scale]

Every stage is one call into libsleekit_amd.so on the current torch stream; tensors stay
in HBM and nothing synchronises unless the caller asks for NumPy results.  This is the
function `sleekit_amd.obq.quantize_opt` and `sleekit_amd.scaling.quantize_with_scaling`
(the reference's entry points, sleekit/obq.py:169 and sleekit/scaling.py:58) are thin
wrappers of, and what bench.py times.
"""

import ctypes

import torch

from . import _device as dev
from . import _lib
from .codebook import DeviceCodebook

_INVERSE_ORDERS = {"inv_diag": 0, "combined_diag": 1}  # need diag(Hd^-1): two factorisations
_KEY_ORDERS = ("inv_diag", "combined_diag", "pivot")     # sort keys computed by a kernel of their own


def order_mode_code(act_order):
    if act_order in _lib.ORDER_MODES:
        return _lib.ORDER_MODES[act_order]
    if act_order in _KEY_ORDERS:
        return _lib.ORDER_KEYS
    raise RuntimeError(f"Invalid act_order value {act_order}")


def inverse_diag_keys(H, n, damp, combined):
    """Sort keys of inv_diag / combined_diag (obq.py:70-75) from a first factorisation in the original order."""
    _, U0, info = factorize(H, n, damp, _lib.ORDER_NONE)
    dev.note_info(info, "compute_hessian_chol")
    ws, ws_bytes = dev.workspace(0, n)
    keys = torch.empty(n, dtype=torch.float64, device=H.device)
    _lib.check(
        _lib.lib.slk_inverse_diag_keys(
            dev.ptr(U0), dev.ptr(H), n, float(damp), int(combined), dev.ptr(keys), dev.ptr(ws), ws_bytes, dev.stream_handle()
        )
    )
    return keys


def pivot_keys(H, n, damp):
    """Sort keys of the greedy pivoted-Cholesky order (obq.py:78, 140-166): the step at which each column is picked."""
    ws, ws_bytes = dev.workspace(0, n)
    keys = torch.empty(n, dtype=torch.float64, device=H.device)
    _lib.check(_lib.lib.slk_pivot_keys(dev.ptr(H), n, float(damp), dev.ptr(keys), dev.ptr(ws), ws_bytes, dev.stream_handle()))
    return keys


def order_keys(H, n, damp, act_order):
    """Keys of the orders that are not a function of the damped diagonal and the column statistics alone."""
    if act_order == "pivot":
        return pivot_keys(H, n, damp)
    return inverse_diag_keys(H, n, damp, _INVERSE_ORDERS[act_order])


def require_uniform(quantizer):
    """(levels, lo, hi, table) of a UniformCodebook or a general Codebook; anything else has no device form."""
    if not isinstance(quantizer, DeviceCodebook):
        raise NotImplementedError(
            "sleekit_amd runs UniformCodebook / Codebook quantizers on the GPU and has no CPU fallback for arbitrary "
            f"callables (got {type(quantizer).__name__})"
        )
    abi = quantizer._abi()
    if len(quantizer) > 256 and abi[3] is not None:
        raise NotImplementedError("general (table) codebooks on the device hold at most 256 entries")
    return abi


class LayerResult:
    """Device tensors produced for one layer."""

    __slots__ = ("Q", "idx", "order", "U", "info", "E", "ls_trace", "ls_error", "loop_error", "S", "O", "codes", "scales", "rotation")

    def __init__(self):
        self.Q = self.idx = self.order = self.U = self.info = self.E = self.ls_trace = self.ls_error = self.loop_error = None
        self.S = self.O = None  # group scales and offsets (Sleekit.quantize with offsets)
        self.codes = self.scales = None  # the MXFP4 packed form (Sleekit.quantize_mxfp4)
        self.rotation = None  # the Rotation whose basis Q, idx and the scales are in (Sleekit.quantize*(..., rotation=))


def factorize(H, n, damp, mode, miss=None, keep=None, lookahead=False):
    """Damping + order + float64 factor for a float32 device Hessian. Returns (order, U, info).
    lookahead: one layer at a time (latency matters, nothing else is in flight): the factorisation forks the bulk of
    its outer updates onto a helper stream (slk_chol_inverse_upper_lookahead: an argument of THIS call, no process-wide
    switch; off for the multi-stream pipelines of sleekit_amd.dist, where the extra streams cost more than they save)."""
    ws, ws_bytes = dev.workspace(0, n)
    s = dev.stream_handle()
    ld = _lib.lib.slk_factor_ld(n)
    order = torch.empty(n, dtype=torch.int64, device=H.device)
    A = torch.empty(ld * ld, dtype=torch.float64, device=H.device)
    U = torch.empty((n, n), dtype=torch.float64, device=H.device)
    info = torch.empty(1, dtype=torch.int32, device=H.device)
    _lib.check(
        _lib.lib.slk_hessian_prepare(
            dev.ptr(H), n, float(damp), mode, dev.ptr(miss), dev.ptr(order), dev.ptr(A), dev.ptr(ws), ws_bytes, s
        )
    )
    chol = _lib.lib.slk_chol_inverse_upper_lookahead if lookahead else _lib.lib.slk_chol_inverse_upper
    _lib.check(chol(dev.ptr(A), n, dev.ptr(U), dev.ptr(info), dev.ptr(ws), ws_bytes, s))
    return order, U, info


def factorize_batch(Hs, n, damp, mode):
    """Damping + order + float64 factor of B same-sized float32 device Hessians in launches that cover them all
    (slk_hessian_prepare_batch / slk_chol_inverse_upper_batch).  Returns order (B, n), U (B, n, n), info (B,):
    the results of B calls of factorize."""
    B = len(Hs)
    device = Hs[0].device
    assert all(H.shape == (n, n) and H.is_contiguous() and H.dtype == torch.float32 for H in Hs)
    ws, ws_bytes = dev.scratch(_lib.lib.slk_factor_workspace_bytes_batch(B, n), "factor_batch")
    s = dev.stream_handle()
    ld = _lib.lib.slk_factor_ld(n)
    order = torch.empty((B, n), dtype=torch.int64, device=device)
    A = torch.empty(B * ld * ld, dtype=torch.float64, device=device)
    U = torch.empty((B, n, n), dtype=torch.float64, device=device)
    info = torch.empty(B, dtype=torch.int32, device=device)
    ptrs = (ctypes.c_void_p * B)(*[dev.ptr(H) for H in Hs])
    _lib.check(_lib.lib.slk_hessian_prepare_batch(ptrs, B, n, float(damp), mode, dev.ptr(order), dev.ptr(A), dev.ptr(ws), ws_bytes, s))
    _lib.check(_lib.lib.slk_chol_inverse_upper_batch(dev.ptr(A), B, n, dev.ptr(U), dev.ptr(info), dev.ptr(ws), ws_bytes, s))
    return order, U, info


def factorize_order_only(H, n, mode, miss=None):
    """Column order of an already damped float32 Hessian (compute_hessian_order, obq.py:58-86)."""
    ws, ws_bytes = dev.workspace(0, n)
    ld = _lib.lib.slk_factor_ld(n)
    order = torch.empty(n, dtype=torch.int64, device=H.device)
    A = torch.empty(ld * ld, dtype=torch.float64, device=H.device)
    _lib.check(
        _lib.lib.slk_hessian_prepare(
            dev.ptr(H), n, 0.0, mode, dev.ptr(miss), dev.ptr(order), dev.ptr(A), dev.ptr(ws), ws_bytes,
            dev.stream_handle(),
        )
    )
    return order, None, None


def loop_error_route():
    """Whether callers may take the layer error the loop carries (slk_gptq_quantize_batch_error) instead of the product
    (slk_row_errors_batch): yes unless slk_set_option("no_loop_error", 1).  The caller still has to vouch for the rest: H
    bit-wise symmetric, the factor made from this H with this damp, the loop itself de-scaling (or no scales)."""
    return _lib.lib.slk_get_option(b"no_loop_error") == 0


def gptq_loop(W, cb_abi, order, U, min_block, num_blocks, scale=None, gscale=None, group_size=None, goffset=None, want_idx=True,
              want_E=False, unscale=False, latency=False, Hs=None, damp=None):
    """The column-sequential loop on device tensors: the package's one binding of slk_gptq_quantize*.

    W (R, n) float32 is one layer: order (n,) int64 (None: the columns as they lie), U (n, n) float64.  W (B, R, n) is a batch
    of layers stacked by rows (R a multiple of 64): order (B, n), U (B, n, n), launches that cover all B layers.  A LIST of B
    layers' W (R, n) -- with lists of their orders, factors and (if any) row scales, every tensor contiguous, anywhere in memory
    -- is the same batch without the copies into stacks (slk_gptq_quantize_layers: at most 16 layers, no group scales); what
    comes back is stacked, as for a stacked batch.  At most one kind
    of scales, shaped like W without its columns: `scale` (one per row; `unscale`: Q comes back de-scaled), or `gscale` over
    groups of `group_size` columns (n / group_size per row; Q de-scaled), optionally with the offsets `goffset` beside it.
    latency: the layer is alone on the GPU (SLK_LOOP_LATENCY: 16-row window workgroups; same results).
    Hs (a list of the layers' (n, n) float32 Hessians) and damp: the rows' errors (W - Q) H (W - Q)^T carried by the loop
    (slk_gptq_quantize_batch_error: H symmetric, U its factor at this damp; `scale` then needs `unscale`; not with group scales).
    Returns (Q, idx, E, row_err): Q, idx (uint8) and E shaped like W, row_err like W without its columns; None when not asked for.
    """
    layers = isinstance(W, (list, tuple))
    if layers:
        (R, n), device = W[0].shape, W[0].device
        B, lead = len(W), (len(W), R)
        assert gscale is None and len(order) == B and len(U) == B and (scale is None or len(scale) == B)
        for b in range(B):
            assert W[b].shape == (R, n) and W[b].dtype == torch.float32 and W[b].is_contiguous()
            assert order[b].shape == (n,) and order[b].dtype == torch.int64 and order[b].is_contiguous()
            assert U[b].shape == (n, n) and U[b].dtype == torch.float64 and U[b].is_contiguous()
            assert scale is None or (scale[b].shape == (R,) and scale[b].dtype == torch.float32 and scale[b].is_contiguous())
    else:
        lead, n, device = tuple(W.shape[:-1]), W.shape[-1], W.device
        B, R = lead if len(lead) == 2 else (1,) + lead
        assert W.is_contiguous() and U.shape == lead[:-1] + (n, n) and U.is_contiguous()
        assert order is None or (order.shape == lead[:-1] + (n,) and order.is_contiguous())
        assert scale is None or (gscale is None and scale.shape == lead and scale.is_contiguous())
    assert (gscale is None) == (group_size is None) and (goffset is None or gscale is not None)
    g = 0
    if gscale is not None:
        g = int(group_size)
        assert g >= 1 and n % g == 0 and Hs is None
        assert all(t is None or (t.shape == lead + (n // g,) and t.dtype == torch.float32 and t.is_contiguous()) for t in (gscale, goffset))
    if Hs is not None:
        assert len(Hs) == B and damp is not None and (scale is None or unscale)
        assert all(H.shape == (n, n) and H.dtype == torch.float32 and H.is_contiguous() for H in Hs)
    # (one layer: slk_workspace_bytes, whatever its scales; a batch: slk_workspace_bytes_batch, for the grouped loop at every size)
    ws, ws_bytes = dev.workspace(R, n, batch=B, grouped=gscale is not None and len(lead) == 2)
    Q = torch.empty(lead + (n,), dtype=torch.float32, device=device)
    idx = torch.empty(lead + (n,), dtype=torch.uint8, device=device) if want_idx else None
    E = torch.empty_like(Q) if want_E else None
    row_err = torch.empty(lead, dtype=torch.float32, device=device) if Hs is not None else None
    levels, lo, hi, table = cb_abi

    def pointers(tensors):
        return None if tensors is None else (ctypes.c_void_p * B)(*[dev.ptr(t) for t in tensors])

    factor = (pointers(order), pointers(U)) if layers else (dev.ptr(order), dev.ptr(U))
    rest = (B, R, n, levels, lo, hi, dev.ptr(table), int(min_block), int(num_blocks), (1 if unscale else 0) | (2 if latency else 0),
            dev.ptr(Q), dev.ptr(idx), dev.ptr(E))
    end = (dev.ptr(ws), ws_bytes, dev.stream_handle())
    if layers:
        rc = _lib.lib.slk_gptq_quantize_layers(pointers(W), pointers(scale), *factor, pointers(Hs), float(damp or 0.0), None, 0, *rest,
                                               dev.ptr(row_err), *end)
    elif goffset is not None:
        rc = _lib.lib.slk_gptq_quantize_grouped_asym_batch(dev.ptr(W), dev.ptr(gscale), dev.ptr(goffset), g, *factor, *rest, *end)
    elif gscale is not None:
        rc = _lib.lib.slk_gptq_quantize_grouped_batch(dev.ptr(W), dev.ptr(gscale), g, *factor, *rest, *end)
    elif Hs is not None:
        rc = _lib.lib.slk_gptq_quantize_batch_error(dev.ptr(W), dev.ptr(scale), *factor, pointers(Hs), float(damp), *rest, dev.ptr(row_err), *end)
    else:
        rc = _lib.lib.slk_gptq_quantize_batch(dev.ptr(W), dev.ptr(scale), *factor, *rest, *end)
    _lib.check(rc)
    return Q, idx, E, row_err


def run_loop(W, scale, order, U, cb_abi, min_block, num_blocks, want_idx=True, want_E=False, unscale=False, latency=False,
             H=None, damp=None):
    """gptq_loop for one layer W (R, n) with row scales or none.  Returns (Q, idx, E); with H (n, n) float32 and damp,
    (Q, idx, E, row_err), row_err (R,) the rows' errors carried by the loop."""
    out = gptq_loop(W, cb_abi, order, U, min_block, num_blocks, scale=scale, want_idx=want_idx, want_E=want_E, unscale=unscale,
                    latency=latency, Hs=None if H is None else [H], damp=damp)
    return out[:3] if H is None else out


def run_loop_batch(W, scale, order, U, cb_abi, min_block, num_blocks, want_idx=True, unscale=False, Hs=None, damp=None):
    """gptq_loop over a batch W (B, R, n), scale (B, R) or None: what B calls of run_loop return.  Returns (Q, idx); with Hs
    (a list of B Hessians) and damp, (Q, idx, row_err), row_err (B, R)."""
    Q, idx, _, row_err = gptq_loop(W, cb_abi, order, U, min_block, num_blocks, scale=scale, want_idx=want_idx, unscale=unscale,
                                   Hs=Hs, damp=damp)
    return (Q, idx) if Hs is None else (Q, idx, row_err)


def row_errors_batch(W, Q, Hs, symmetric=None):
    """Row errors of a batch of layers stacked by rows: W, Q (B, R, n); Hs a list of B (n, n) float32 tensors.
    symmetric: (B,) int32 verdicts of symmetry_flag (None: checked here)."""
    B, R, n = W.shape
    assert len(Hs) == B and W.is_contiguous() and Q.is_contiguous()
    assert symmetric is None or (symmetric.dtype == torch.int32 and symmetric.numel() == B and symmetric.is_contiguous())
    ws, ws_bytes = dev.workspace(R, n, batch=B)
    out = torch.empty((B, R), dtype=torch.float32, device=W.device)
    ptrs = (ctypes.c_void_p * B)(*[dev.ptr(H) for H in Hs])
    _lib.check(
        _lib.lib.slk_row_errors_batch(dev.ptr(W), dev.ptr(Q), ptrs, B, R, n, dev.ptr(symmetric), dev.ptr(out), dev.ptr(ws), ws_bytes,
                                      dev.stream_handle())
    )
    return out


def symmetry_flag(H):
    """int32[1] on the device: 1 iff H is bit-wise symmetric (what lets the layer error skip half its products)."""
    flag = torch.empty(1, dtype=torch.int32, device=H.device)
    _lib.check(_lib.lib.slk_symmetry_flag(dev.ptr(H), H.shape[0], dev.ptr(flag), dev.stream_handle()))
    return flag


def local_search(W, Q, H, cb_abi, moves, idx=None, want_trace=False, gains=None, gains_mode=0, row_err=None, gscale=None,
                 group_size=None):
    """In place on Q (and idx).  want_trace: returns the (R, moves) int32 record of the moves taken
    (2 * column + up, -1 = none); gains / gains_mode: the carried state of a stateful search (slk_local_search);
    row_err (R,) float32: receives the rows' errors (W - Q) H (W - Q)^T after the moves.
    gscale (R, n / group_size) with group_size: the group quantizer's candidates (slk_local_search_grouped: W unscaled, Q
    de-scaled; no carried state)."""
    R, n = W.shape
    levels, lo, hi, table = cb_abi
    ws, ws_bytes = dev.workspace(R, n)
    trace = torch.empty((R, int(moves)), dtype=torch.int32, device=W.device) if want_trace else None
    assert gains is None or (gains.shape == (R, 2, n) and gains.dtype == torch.float32 and gains.is_contiguous())
    if gscale is not None:
        assert gains is None and group_size is not None
        _lib.check(
            _lib.lib.slk_local_search_grouped(
                dev.ptr(W), dev.ptr(Q), dev.ptr(H), dev.ptr(gscale), int(group_size), R, n, levels, lo, hi, dev.ptr(table), int(moves),
                dev.ptr(idx), dev.ptr(trace), dev.ptr(row_err), dev.ptr(ws), ws_bytes, dev.stream_handle(),
            )
        )
        return trace
    _lib.check(
        _lib.lib.slk_local_search(
            dev.ptr(W), dev.ptr(Q), dev.ptr(H), R, n, levels, lo, hi, dev.ptr(table), int(moves), dev.ptr(idx), dev.ptr(trace),
            dev.ptr(gains), int(gains_mode), dev.ptr(row_err), dev.ptr(ws), ws_bytes, dev.stream_handle(),
        )
    )
    return trace


def local_search_batch(W, Q, Hs, cb_abi, moves, idx=None, symmetric=None, row_err=None):
    """local_search over a batch of layers stacked by rows: W, Q (B, R, n) (idx (B, R, n) uint8 or None), Hs a list of B
    Hessians; in place on Q and idx, the results of B separate searches.  row_err (B, R) float32: receives the rows' errors
    after the moves, in the domain of W and Q (carried through the search: no product of its own)."""
    B, R, n = W.shape
    assert len(Hs) == B and W.is_contiguous() and Q.is_contiguous() and (idx is None or idx.is_contiguous())
    levels, lo, hi, table = cb_abi
    ws, ws_bytes = dev.workspace(R, n, batch=B)
    ptrs = (ctypes.c_void_p * B)(*[dev.ptr(H) for H in Hs])
    _lib.check(
        _lib.lib.slk_local_search_batch(dev.ptr(W), dev.ptr(Q), ptrs, B, R, n, levels, lo, hi, dev.ptr(table), int(moves), dev.ptr(idx),
                                        dev.ptr(symmetric), dev.ptr(row_err), dev.ptr(ws), ws_bytes, dev.stream_handle())
    )


def stack_rows(parts, rows_padded, fill=0.0):
    """torch.stack of the layers' row shards (each rows x cols, or rows,) with every layer padded to `rows_padded` rows of
    `fill`: ONE launch (slk_stack_rows) instead of a copy per layer."""
    B = len(parts)
    rows = parts[0].shape[0]
    cols = parts[0].shape[1] if parts[0].dim() == 2 else 1
    for t in parts:
        if t.dtype != torch.float32 or not t.is_contiguous() or t.shape != parts[0].shape:
            raise ValueError("stack_rows wants contiguous float32 shards of one shape")
    out = torch.empty((B, rows_padded, cols) if parts[0].dim() == 2 else (B, rows_padded), dtype=torch.float32, device=parts[0].device)
    ptrs = (ctypes.c_void_p * B)(*[dev.ptr(t) for t in parts])
    _lib.check(_lib.lib.slk_stack_rows(ptrs, B, rows, int(rows_padded), cols, float(fill), dev.ptr(out), dev.stream_handle()))
    return out


def rows_divide(x, scale, invert=False):
    R, n = x.shape
    out = torch.empty_like(x)
    _lib.check(
        _lib.lib.slk_rows_divide(dev.ptr(x), dev.ptr(scale), R, n, 1 if invert else 0, dev.ptr(out), dev.stream_handle())
    )
    return out


def column_miss(W, cb_abi, squared, gscale=None, group_size=None, goffset=None):
    """Column sums of |Z(W) - W| (or squared) in NumPy's row-after-row order (n == 1: its pairwise order over the rows, as NumPy
    reduces a single column): Z the codebook, or with gscale (R, n / group_size) the group quantizer (goffset beside it: the
    asymmetric one), in original units."""
    R, n = W.shape
    levels, lo, hi, table = cb_abi
    out = torch.empty(n, dtype=torch.float32, device=W.device)
    rest = (R, n, levels, lo, hi, dev.ptr(table), 1 if squared else 0, dev.ptr(out), dev.stream_handle())
    if goffset is not None:
        rc = _lib.lib.slk_column_miss_grouped_asym(dev.ptr(W), dev.ptr(gscale), dev.ptr(goffset), int(group_size), *rest)
    elif gscale is not None:
        rc = _lib.lib.slk_column_miss_grouped(dev.ptr(W), dev.ptr(gscale), int(group_size), *rest)
    else:
        rc = _lib.lib.slk_column_miss(dev.ptr(W), *rest)
    _lib.check(rc)
    return out


def sort_keys(W, H, cb_abi, act_order, damp, scale=None, gscale=None, group_size=None, goffset=None):
    """The `miss` argument of slk_hessian_prepare for an order, a layer and its scales: None for none / diag, the kernel-made
    keys of inv_diag / combined_diag / pivot, and for err / sqerr the statistics of ALL rows of the layer's quantizer -- the
    codebook on W / scale (`scale` (R,), or W pre-divided already), or the group quantizer of gscale (and goffset) on W."""
    mode = order_mode_code(act_order)
    if mode == _lib.ORDER_KEYS:
        return order_keys(H, H.shape[0], damp, act_order)
    if mode < _lib.ORDER_ERR:
        return None
    if scale is not None:
        W = rows_divide(W, scale)
    return column_miss(W, cb_abi, mode == _lib.ORDER_SQERR, gscale, group_size, goffset)


def row_errors(W, Q, H, want_G=False):
    R, n = W.shape
    ws, ws_bytes = dev.workspace(R, n)
    out = torch.empty(R, dtype=torch.float32, device=W.device)
    G = torch.empty((R, n), dtype=torch.float32, device=W.device) if want_G else None
    _lib.check(
        _lib.lib.slk_row_errors(
            dev.ptr(W), dev.ptr(Q), dev.ptr(H), R, n, dev.ptr(out), dev.ptr(G), dev.ptr(ws), ws_bytes, dev.stream_handle()
        )
    )
    return (out, G) if want_G else out


def quantize_layer(
    W, H, quantizer, scale=None, act_order="diag", damp=0.01, nb_ls_moves=0, min_block_size=32, num_blocks=8,
    factor=None, unscale=True, want_idx=True, want_ls_trace=False, lookahead=True, want_ls_error=False, want_loop_error=False,
    *, gscale=None, group_size=None, goffset=None,
):
    """One layer through the whole path, on device tensors.

    W (R, n) float32, H (n, n) float32, scale (R,) float32 or None.  `factor` = (order, U, info)
    re-uses a factor computed elsewhere (another GPU: see sleekit_amd.dist); its status is then the caller's to check.
    Returns a LayerResult whose Q is de-scaled when `scale` is given and `unscale` is true
    (sleekit/scaling.py:58-81), else the codebook values in the scaled domain
    (sleekit/obq.py:169-217).  want_ls_trace: res.ls_trace = the local search's moves (slk_local_search).
    lookahead: this layer is alone on the GPU (the default of this single-layer API; sleekit_amd.dist passes False): the
    factorisation looks ahead (see factorize) and the loop's window kernel takes 16-row workgroups (SLK_LOOP_LATENCY).
    want_ls_error: res.ls_error = the rows' errors after the moves, carried through the search, in the domain it ran in.
    want_loop_error: the caller vouches that H is bit-wise symmetric (and that `factor`, if given, is H's at this damp):
    res.loop_error = the rows' errors (W - Q) H (W - Q)^T carried by the loop (gptq_loop with Hs) -- when there is no local
    search and the loop itself de-scales (or there are no scales); None otherwise: the caller then computes the product.
    gscale (R, n / group_size) float32 with group_size, instead of `scale`: the group quantizer of sleekit_amd.groups (Q
    de-scaled, idx the codebook indices of Q / s); goffset beside it: the asymmetric one (no local search).

    What the kinds of scales change:
    row scales   with err / sqerr keys or a local search, everything runs on the pre-divided copy W / scale, in the scaled
                 domain, and Q is de-scaled at the end; otherwise the loop's last kernel de-scales on the way out (one pass
                 over Q less) and can carry the error.
    group scales the loop runs on the unscaled W (only its leaves scale) with the group quantizer's keys, the search on the
                 de-scaled Q with that quantizer's candidates; res.ls_error is in original units, filled whenever there are
                 moves.  The loop carries no error.
    """
    assert W.ndim == 2
    assert H.ndim == 2
    assert H.shape[0] == H.shape[1]
    assert H.shape[0] == W.shape[1]
    assert min_block_size >= 1
    assert scale is None or gscale is None
    if goffset is not None and nb_ls_moves > 0:
        raise NotImplementedError("local search with group offsets is not supported (nb_ls_moves must be 0)")
    cb_abi = require_uniform(quantizer)
    if cb_abi[0] > 256:
        want_idx = False  # (the kernels emit uint8 indices; wider ones come from quantizer.quantize_index on the values)
    mode = order_mode_code(act_order)
    R, n = W.shape
    res = LayerResult()
    group = dict(gscale=gscale, group_size=group_size)

    need_scaled_copy = scale is not None and (mode in (_lib.ORDER_ERR, _lib.ORDER_SQERR) or nb_ls_moves > 0)
    Ws, loop_scale = (rows_divide(W, scale), None) if need_scaled_copy else (W, scale)

    check_factor = factor is None
    if factor is None:
        miss = sort_keys(Ws, H, cb_abi, act_order, damp, goffset=goffset, **group)
        factor = factorize(H, n, damp, mode, miss, lookahead=lookahead)
    res.order, res.U, res.info = factor[:3]

    fused = loop_scale is not None and unscale and nb_ls_moves == 0
    carried = want_loop_error and nb_ls_moves == 0 and gscale is None and (scale is None or fused)
    res.Q, res.idx, _, res.loop_error = gptq_loop(Ws, cb_abi, res.order, res.U, min_block_size, num_blocks, scale=loop_scale,
                                                  goffset=goffset, want_idx=want_idx, unscale=fused, latency=lookahead,
                                                  Hs=[H] if carried else None, damp=damp, **group)
    if nb_ls_moves > 0:
        if want_ls_error or gscale is not None:
            res.ls_error = torch.empty(R, dtype=torch.float32, device=W.device)
        res.ls_trace = local_search(Ws, res.Q, H, cb_abi, nb_ls_moves, res.idx, want_trace=want_ls_trace, row_err=res.ls_error, **group)
    if scale is not None and unscale and not fused:
        res.Q = rows_divide(res.Q, scale, invert=True)
    # The factorisation's status word is read back only now, with the loop (and the search) already enqueued behind it: read
    # right after the factorisation, the round trip to the host kept the loop's first launch waiting 35-45 us per layer.  A
    # matrix that is not positive definite still raises here (numpy.linalg.LinAlgError, as np.linalg.cholesky does in
    # sleekit/obq.py:49-50); the loop then ran on a void factor, memory-safe, its results never returned.
    if check_factor:
        dev.note_info(res.info, "compute_hessian_chol")
    return res
