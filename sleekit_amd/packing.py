"""Bit-packed codebook indices: the stored form of (idx, S) and (idx, S, O), at `bits` bits an index instead of a byte.

    b = index_bits(cb)                                  # ceil(log2(len(cb))), at least 1; more than 256 entries: ValueError
    P = pack_indices(idx, b)                            # (R, b * ceil(n / 32)) 32-bit words
    idx == unpack_indices(P, n, b)                      # uint8 (R, n)
    Q = dequantize_packed(P, n, cb, group_scales=S, offsets=O)   # straight from the words: no uint8 idx in between

FORMAT.  Each row is cut into chunks of 32 consecutive indices, the last one padded with zero indices, so a row takes
b * ceil(n / 32) words and starts on a word boundary.  Chunk k of row r is words [b k, b k + b) of that row, read as one
little-endian integer of 32 b bits (word j holds bits [32 j, 32 j + 32)); index 32 k + i sits in its bits [i b, i b + b).
Only the low b bits of an index are stored: an index >= 2^b is a caller error and comes back masked.  b = 8 is the idx
bytes read as little-endian words, each row padded to a multiple of 32 bytes.  A stack of B layers of one width,
(B, R, n), is B R rows: reshape it to (B R, n).

`dequantize_packed` rebuilds value(k), k = min(index, len(cb) - 1), de-scaled by at most one of
    scale (R,):                         value / (1 / scale[r])          -- the per-row path (engine.quantize_layer with a
                                                                           scale, scaling.quantize_with_scaling)
    group_scales (R, n / g):            value / (1 / S[r, c // g])      -- groups.dequantize_grouped
    group_scales and offsets (R, n / g): value / (1 / S[r, c // g]) + O[r, c // g]
(float32 IEEE divides, in this order) and returns it in float32 -- bit for bit what those paths return -- or rounded to
nearest even as bfloat16 / float16, exactly `.to(dtype)` of the float32 result.

Same conventions as the rest of the package: NumPy in gives NumPy out (words as np.uint32), device tensors in give
device tensors out (words as torch.int32 holding the same bits), everything runs on the GPU on the current stream, and
there is no CPU fallback.
"""

import numpy as np
import torch

from . import _device as dev
from . import _lib
from . import engine

_OUT = {torch.float32: _lib.DTYPE_F32, torch.bfloat16: _lib.DTYPE_BF16, torch.float16: _lib.DTYPE_F16}
_NUMPY_OUT = {torch.float32: np.float32, torch.float16: np.float16}


def index_bits(codebook):
    """Bits an index of `codebook` needs: ceil(log2(len(codebook))), at least 1."""
    levels = len(codebook)
    if levels > 256:
        raise ValueError(f"packed indices hold at most 8 bits: a codebook of {levels} entries does not fit")
    return max(1, (levels - 1).bit_length())


def packed_shape(R, n, bits):
    """Shape of the words of an (R, n) index matrix at `bits` bits."""
    return (int(R), int(bits) * ((int(n) + 31) // 32))


def _check_bits(bits):
    if isinstance(bits, bool) or not isinstance(bits, (int, np.integer)) or not 1 <= int(bits) <= 8:
        raise ValueError(f"bits must be an integer in 1..8 (got {bits!r})")
    return int(bits)


def _check_extent(R, n, what):
    if R < 1 or n < 1 or R >= 1 << 31 or n >= 1 << 31:
        raise ValueError(f"{what} must have 1 <= rows, columns < 2^31 (got ({R}, {n}))")


def _words_to_device(P, n, bits):
    """The device int32 view of packed words (np.uint32 / np.int32 arrays, int32 tensors) and its row count."""
    if isinstance(P, np.ndarray):
        if P.dtype not in (np.uint32, np.int32):
            raise ValueError(f"packed words must be uint32 or int32 (got {P.dtype})")
        P = np.ascontiguousarray(P).view(np.int32)
    elif isinstance(P, torch.Tensor):
        if P.dtype != torch.int32:
            raise ValueError(f"packed words must be an int32 tensor (got {P.dtype})")
    else:
        raise ValueError(f"packed words must be a NumPy array or a torch tensor (got {type(P).__name__})")
    if P.ndim != 2:
        raise ValueError(f"packed words must be 2-D (got shape {tuple(P.shape)})")
    R = int(P.shape[0])
    _check_extent(R, int(n), "the index matrix")
    if tuple(P.shape) != packed_shape(R, n, bits):
        raise ValueError(f"{R} rows of {n} indices at {bits} bits are {packed_shape(R, n, bits)} words; got {tuple(P.shape)}")
    return dev.to_device(P, torch.int32), R


def pack_indices(idx, bits):
    """uint8 indices (R, n) -> (R, bits * ceil(n / 32)) words in the module's format: np.uint32 for a NumPy array,
    torch.int32 (the same bits) for a device tensor."""
    bits = _check_bits(bits)
    if not isinstance(idx, (np.ndarray, torch.Tensor)) or idx.ndim != 2:
        raise ValueError("indices must be a 2-D NumPy array or torch tensor")
    if idx.dtype not in (np.uint8, torch.uint8):
        raise ValueError(f"indices must be uint8 (got {idx.dtype})")
    R, n = (int(s) for s in idx.shape)
    _check_extent(R, n, "the index matrix")
    d = dev.to_device(idx, torch.uint8)
    out = torch.empty(packed_shape(R, n, bits), dtype=torch.int32, device=d.device)
    _lib.check(_lib.lib.slk_pack_indices(dev.ptr(d), R, n, bits, dev.ptr(out), dev.stream_handle()))
    out = dev.like_input(out, idx)
    return out.view(np.uint32) if isinstance(out, np.ndarray) else out


def unpack_indices(P, n, bits):
    """Packed words (R, bits * ceil(n / 32)) -> uint8 indices (R, n)."""
    bits = _check_bits(bits)
    Pd, R = _words_to_device(P, n, bits)
    idx = torch.empty((R, int(n)), dtype=torch.uint8, device=Pd.device)
    _lib.check(_lib.lib.slk_unpack_indices(dev.ptr(Pd), R, int(n), bits, dev.ptr(idx), dev.stream_handle()))
    return dev.like_input(idx, P)


def _side(x, shape, what):
    d = dev.to_device(x)
    if tuple(d.shape) != shape:
        raise ValueError(f"{what} must be {shape}; got {tuple(d.shape)}")
    return d


def dequantize_packed(P, n, codebook, bits=None, scale=None, group_scales=None, group_size=None, offsets=None,
                      dtype=torch.float32):
    """The layer rebuilt from its packed indices (module docstring): (R, n) of `dtype` (float32, bfloat16 or float16).

    bits defaults to index_bits(codebook).  scale (R,) and group_scales (R, n / group_size) are mutually exclusive;
    offsets (R, n / group_size) need group_scales; group_size defaults to n / group_scales.shape[1].  NumPy words give a
    NumPy array, which has no bfloat16 (ValueError)."""
    levels, lo, hi, table = engine.require_uniform(codebook)
    if levels > 256:
        raise ValueError(f"packed indices hold at most 8 bits: a codebook of {levels} entries does not fit")
    bits = index_bits(codebook) if bits is None else _check_bits(bits)
    if bits < index_bits(codebook):
        raise ValueError(f"{bits} bits cannot index a codebook of {levels} entries (it needs {index_bits(codebook)})")
    if dtype not in _OUT:
        raise ValueError(f"dtype must be torch.float32, torch.bfloat16 or torch.float16 (got {dtype})")
    if isinstance(P, np.ndarray) and dtype not in _NUMPY_OUT:
        raise ValueError(f"NumPy has no {dtype}: pass the words as a device tensor for a {dtype} result")
    if scale is not None and group_scales is not None:
        raise ValueError("scale and group_scales are mutually exclusive")
    if offsets is not None and group_scales is None:
        raise ValueError("offsets need group_scales")
    n = int(n)
    g = 1
    if group_scales is not None:
        G = int(group_scales.shape[1]) if getattr(group_scales, "ndim", 0) == 2 else 0
        if group_size is None:
            if G < 1 or n % G != 0:
                raise ValueError(f"group scales of shape {tuple(group_scales.shape)} do not split {n} columns into groups")
            group_size = n // G
        g = int(group_size)
        if g < 1 or n % g != 0:
            raise ValueError(f"group_size must be >= 1 and divide the {n} columns (got {g})")
    Pd, R = _words_to_device(P, n, bits)
    Sd = _side(scale, (R,), "scale") if scale is not None else None
    Gd = _side(group_scales, (R, n // g), "group scales") if group_scales is not None else None
    Od = _side(offsets, (R, n // g), "group offsets") if offsets is not None else None
    out = torch.empty((R, n), dtype=dtype, device=Pd.device)
    _lib.check(
        _lib.lib.slk_dequantize_packed(
            dev.ptr(Pd), R, n, bits, levels, lo, hi, dev.ptr(table), dev.ptr(Sd), dev.ptr(Gd), dev.ptr(Od), g, _OUT[dtype],
            dev.ptr(out), dev.stream_handle(),
        )
    )
    return dev.like_input(out, P)
