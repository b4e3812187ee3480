"""Mixture-of-experts routing on the device: top-k gates, the sort by expert, the row-mapped quantizer, the combine.

    r = route_topk(logits, k, gating="selected")          # Routing(expert_ids, gates, order, pos, offsets)
    order, pos, offsets = sort_experts(expert_ids, E)     # int32, from the counting sort
    y = experts.forward_logits(x, logits, k)              # MXExperts / MXExpertsMLP: the whole route, one wait for the stream

SELECTION.  Column j of expert_ids (T, k) int32 is the expert of the token's j-th largest logit; expert a ranks before
expert b when v[a] > v[b], or v[a] == v[b] and a < b (+0 and -0 tie; of equal logits the lower index wins -- torch.topk
promises no order among equal values).  logits (T, E) float32, bfloat16 or float16 are converted to float32 first.
GATES.  float32 (T, k).  gating="selected" is a softmax over the k selected logits: gpt-oss, and Mixtral's and Qwen3's
"softmax over all, top-k, renormalise", which is the same function.  gating="all" is a softmax over all E logits with the
selected probabilities left as they are (no renormalisation).  m = the token's largest logit, e = expf(v - m), g = e / s in
float32, s summed in a fixed order (include/sleekit_amd.h, slk_moe_topk).
MASKS.  -inf masks an expert.  A NaN or +inf in a token's row, or fewer than k logits above -inf: ValueError.
SORT.  order[p] is the flat index t k + j of the p-th row in expert order (equal ids in their original order), pos its
inverse, offsets (E + 1,) the table matmul_mx_experts takes.  mx.sort_by_expert gives the same order as int64 from torch ops.

Device tensors in give device tensors out, NumPy in gives NumPy out; everything runs on the GPU on the current stream.
"""

import collections

import numpy as np
import torch

from . import _device as dev
from . import _lib

Routing = collections.namedtuple("Routing", "expert_ids gates order pos offsets")

_GATINGS = {"selected": _lib.MOE_GATE_SELECTED, "all": _lib.MOE_GATE_ALL}
_DTYPES = {torch.float32: _lib.DTYPE_F32, torch.bfloat16: _lib.DTYPE_BF16, torch.float16: _lib.DTYPE_F16}
_NP_DTYPES = {np.dtype(np.float32): torch.float32, np.dtype(np.float16): torch.float16}
MAX_ROWS = 1 << 24

LOGITS_MESSAGE = ("router logits must be finite or -inf, with at least k of a token's logits above -inf: "
                  "logits holds a NaN or +inf, or a token with fewer than k unmasked experts")
ROWS_MESSAGE = "the row map points outside x: a source row outside 0 .. T - 1"
POS_MESSAGE = "pos must lie in 0 .. T k - 1"


def ids_message(E):
    return f"expert ids must lie in 0 .. {E - 1}"


def _check_logits(logits, k, gating, T=None, E=None):
    """(T, E, the logits' torch dtype) of router logits, everything that needs no device checked.  T, E: what the caller's x
    and experts make them."""
    if not isinstance(logits, (np.ndarray, torch.Tensor)) or logits.ndim != 2:
        raise ValueError(f"logits must be a 2-D NumPy array or torch tensor (tokens, experts); got {tuple(getattr(logits, 'shape', ()))}")
    dtype = logits.dtype if isinstance(logits, torch.Tensor) else _NP_DTYPES.get(logits.dtype)
    if dtype not in _DTYPES:
        raise ValueError(f"logits must be torch.float32, torch.bfloat16 or torch.float16 (got {logits.dtype})")
    if (T is not None and logits.shape[0] != T) or (E is not None and logits.shape[1] != E):
        raise ValueError(f"logits must be ({T if T is not None else 'T'}, {E if E is not None else 'E'}): one row a token, one column an "
                         f"expert; got {tuple(logits.shape)}")
    T, E = int(logits.shape[0]), int(logits.shape[1])
    if T < 1 or E < 1 or E > _lib.MX_MAX_EXPERTS:
        raise ValueError(f"logits must have at least one token and 1 .. {_lib.MX_MAX_EXPERTS} experts (got {tuple(logits.shape)})")
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1 or k > min(E, _lib.MOE_MAX_K):
        raise ValueError(f"k must be an int in 1 .. min(E, {_lib.MOE_MAX_K}) = {min(E, _lib.MOE_MAX_K)} (got {k!r})")
    if not isinstance(gating, str) or gating not in _GATINGS:
        raise ValueError(f'gating must be "selected" or "all" (got {gating!r})')
    if T * int(k) > MAX_ROWS:
        raise ValueError(f"T k must be at most 2^24 routed rows (got {T} x {k})")
    return T, E, dtype


def _topk(Ld, T, E, k, gating):
    """(expert_ids (T, k) int32, gates (T, k) float32, flag) of contiguous device logits; the caller reads the flag."""
    ids = torch.empty((T, k), dtype=torch.int32, device=Ld.device)
    gates = torch.empty((T, k), dtype=torch.float32, device=Ld.device)
    flag = torch.empty(1, dtype=torch.int32, device=Ld.device)
    _lib.check(_lib.lib.slk_moe_topk(dev.ptr(Ld), _DTYPES[Ld.dtype], T, E, k, _GATINGS[gating], dev.ptr(ids), dev.ptr(gates), dev.ptr(flag),
                                     dev.stream_handle()))
    return ids, gates, flag


def _sort(ids, n, E):
    """(order, pos, offsets, flag), int32 device tensors, of n contiguous int32 device ids; the caller reads the flag (an id
    outside 0 .. E - 1; such ids are clamped for the sort)."""
    order = torch.empty(n, dtype=torch.int32, device=ids.device)
    pos = torch.empty(n, dtype=torch.int32, device=ids.device)
    offsets = torch.empty(E + 1, dtype=torch.int32, device=ids.device)
    flag = torch.empty(1, dtype=torch.int32, device=ids.device)
    need = int(_lib.lib.slk_moe_sort_workspace_bytes(n, E))
    ws, ws_bytes = dev.scratch(need, "moe_sort") if need else (None, 0)
    _lib.check(_lib.lib.slk_moe_sort(dev.ptr(ids), n, E, dev.ptr(order), dev.ptr(pos), dev.ptr(offsets), dev.ptr(flag), dev.ptr(ws), ws_bytes,
                                     dev.stream_handle()))
    return order, pos, offsets, flag


def _quantize_rows(Xd, T, K, rows, div, M, c_fmt, bits):
    """(a_codes (M, K bits / 8), a_scales (M, K / 32), flags) of a contiguous device X (T, K): output row i quantizes
    X[rows[i] // div].  flags[0]: a NaN or an infinity in a mapped row; flags[1]: a source row outside X."""
    Xd = dev.aligned(Xd)
    codes = torch.empty((M, K * bits // 8), dtype=torch.uint8, device=Xd.device)
    scales = torch.empty((M, K // 32), dtype=torch.uint8, device=Xd.device)
    flags = torch.empty(2, dtype=torch.int32, device=Xd.device)
    _lib.check(_lib.lib.slk_mx_quantize_act_rows(dev.ptr(Xd), _DTYPES[Xd.dtype], T, K, dev.ptr(rows), div, M, c_fmt, dev.ptr(codes), dev.ptr(scales),
                                                 dev.ptr(flags), dev.stream_handle()))
    return codes, scales, flags


def _combine(Yd, pos, gates, T, k, N, dtype):
    """(out (T, N) of `dtype`, flag): sum_j gates[t][j] * Y[pos[t k + j]] of a contiguous device Y (T k, N); gates None: ones."""
    Yd = dev.aligned(Yd)
    out = torch.empty((T, N), dtype=dtype, device=Yd.device)
    flag = torch.empty(1, dtype=torch.int32, device=Yd.device)
    _lib.check(_lib.lib.slk_moe_combine(dev.ptr(Yd), _DTYPES[Yd.dtype], dev.ptr(pos), dev.ptr(gates), T, k, N, dev.ptr(out), _DTYPES[dtype],
                                        dev.ptr(flag), dev.stream_handle()))
    return out, flag


def _raise_flags(*checks):
    """(device flag or None, message) pairs read in ONE device -> host transfer, the first raised flag's message raised."""
    checks = [(f, m) for f, m in checks if f is not None]
    if not checks:
        return
    for v, (_, message) in zip(torch.cat([f.reshape(1).to(torch.int32) for f, _ in checks]).tolist(), checks):
        if v:
            raise ValueError(message)


def route_topk(logits, k, gating="selected"):
    """Routing(expert_ids, gates, order, pos, offsets) of router logits (T, E): the k experts of every token and their gates
    (module docstring), then the sort of the T k ids by expert -- two launches (four above 1024 routed rows), one wait for the
    stream to read the two flags.  A NaN or +inf among the logits, or a token with fewer than k logits above -inf: ValueError."""
    T, E, dtype = _check_logits(logits, k, gating)
    k = int(k)
    ids, gates, bad_logits = _topk(dev.to_device(logits, dtype), T, E, k, gating)
    order, pos, offsets, bad_ids = _sort(ids.reshape(-1), T * k, E)
    _raise_flags((bad_logits, LOGITS_MESSAGE), (bad_ids, ids_message(E)))
    return Routing(*(dev.like_input(t, logits) for t in (ids, gates, order, pos, offsets)))


def sort_experts(expert_ids, E):
    """(order, pos, offsets), int32, of int32 or int64 expert ids of any shape, flattened: the stable counting sort
    (slk_moe_sort; module docstring).  order is mx.sort_by_expert's, as int32.  An id outside 0 .. E - 1: ValueError."""
    if not isinstance(expert_ids, (np.ndarray, torch.Tensor)) or expert_ids.dtype not in (torch.int32, torch.int64, np.int32, np.int64):
        raise ValueError(f"expert_ids must be an int32 or int64 NumPy array or torch tensor (got {getattr(expert_ids, 'dtype', type(expert_ids).__name__)})")
    if isinstance(E, bool) or not isinstance(E, (int, np.integer)) or E < 1 or E > _lib.MX_MAX_EXPERTS:
        raise ValueError(f"E must be an int in 1 .. {_lib.MX_MAX_EXPERTS} (got {E!r})")
    n = int(expert_ids.size if isinstance(expert_ids, np.ndarray) else expert_ids.numel())
    if n < 1 or n > MAX_ROWS:
        raise ValueError(f"expert_ids must hold 1 .. 2^24 ids (got {n})")
    if isinstance(expert_ids, torch.Tensor) and expert_ids.dtype == torch.int64 or isinstance(expert_ids, np.ndarray) and expert_ids.dtype == np.int64:
        # (an int64 id that int32 does not hold is outside every range of experts: -1 says so to the kernel)
        wide = dev.to_device(expert_ids, torch.int64).reshape(-1)
        ids = torch.where((wide < 0) | (wide >= int(E)), torch.full_like(wide, -1), wide).to(torch.int32)
    else:
        ids = dev.to_device(expert_ids, torch.int32).reshape(-1)
    order, pos, offsets, bad = _sort(ids, n, int(E))
    _raise_flags((bad, ids_message(int(E))))
    return tuple(dev.like_input(t, expert_ids) for t in (order, pos, offsets))
