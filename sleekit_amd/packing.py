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

LINEAR.  The packed layer runs as stored, de-quantized inside a bfloat16 / float16 MFMA GEMM (slk_packed_gemm):
    y = linear_packed(x, P, cb, group_scales=S, offsets=O, bias=b)      # x (..., K) float32 / bfloat16 / float16 -> (..., N)
    layer = PackedLinear.from_result(nn_linear, st.quantize_packed(3, group_size=128, offsets="mid"), UniformCodebook(8, -1, 1))
  weights      dequantize_packed(P, K, cb, ..., dtype=c) bit for bit, c the compute type: torch.float16 when x is float16,
               otherwise torch.bfloat16 (`compute=` overrides); nothing de-quantized is written to memory
  activations  x rounded to nearest even to c (the identity when x has that type); NaN and infinity are not looked for
               and propagate; 16-bit subnormals behave as the hardware defines them
  sums         the products are exact in float32, the sums float32 over K in a fixed order (a repeated call gives the same
               bits); the float32 bias is added in float32 and the result rounded once to `dtype` (default: x's)
  shapes       K >= 8 and K % 8 == 0; with group scales g % 8 == 0 and g divides K; anything else is a ValueError before
               any launch: such layers go through dequantize_packed
The module is forward only (inference): it registers no autograd function.

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


# ---------------------------------------------------------------------------------------------------------------- linear
_ACT = (torch.float32, torch.bfloat16, torch.float16, np.float32, np.float16)
_COMPUTE = (torch.bfloat16, torch.float16)


def _torch_dtype(x):
    return x.dtype if isinstance(x, torch.Tensor) else {np.dtype(np.float32): torch.float32, np.dtype(np.float16): torch.float16}[x.dtype]


def _check_shape(x, shape, what):
    if not isinstance(x, (np.ndarray, torch.Tensor)) or tuple(x.shape) != shape:
        raise ValueError(f"{what} must be {shape}; got {tuple(getattr(x, 'shape', ()))}")


def _check_words(P):
    if isinstance(P, np.ndarray):
        if P.dtype not in (np.uint32, np.int32):
            raise ValueError(f"packed words must be uint32 or int32 (got {P.dtype})")
    elif isinstance(P, torch.Tensor):
        if P.dtype != torch.int32:
            raise ValueError(f"packed words must be an int32 tensor (got {P.dtype})")
    else:
        raise ValueError(f"packed words must be a NumPy array or a torch tensor (got {type(P).__name__})")
    if P.ndim != 2:
        raise ValueError(f"packed words must be 2-D (got shape {tuple(P.shape)})")


def _linear_shapes(K, group_size, what="the layer"):
    """The shapes slk_packed_gemm takes: a lane's 8 consecutive columns lie in one row and under one scale."""
    if K < 8 or K % 8 != 0:
        raise ValueError(f"linear_packed needs a positive multiple of 8 input features ({what} has {K}): "
                         "de-quantize such a layer with dequantize_packed")
    if group_size is not None and (group_size < 8 or group_size % 8 != 0 or K % group_size != 0):
        raise ValueError(f"linear_packed needs a group_size that is a multiple of 8 and divides the {K} input features "
                         f"(got {group_size}): de-quantize such a layer with dequantize_packed")


def linear_packed(x, P, codebook, bits=None, scale=None, group_scales=None, group_size=None, offsets=None, bias=None, dtype=None,
                  compute=None):
    """torch.nn.functional.linear with a weight kept as packed indices (module docstring, LINEAR): x (..., K) float32,
    bfloat16 or float16 against the layer P (N, bits * ceil(K / 32)) words de-scaled as in dequantize_packed (same
    arguments, same defaults), plus the float32 bias (N,); the result is (..., N) in `dtype`, or in x's dtype when `dtype`
    is None.  compute: torch.bfloat16 or torch.float16, the type of both MFMA operands (default: float16 for a float16 x,
    bfloat16 otherwise)."""
    if not isinstance(x, (np.ndarray, torch.Tensor)) or x.ndim < 1:
        raise ValueError("x must be a NumPy array or torch tensor of at least one dimension")
    if x.dtype not in _ACT:
        raise ValueError(f"x must be {_ACT[0]}, torch.bfloat16 or torch.float16 (got {x.dtype})")
    if dtype is None:
        dtype = _torch_dtype(x)
    if dtype not in _OUT:
        raise ValueError(f"dtype must be torch.float32, torch.bfloat16 or torch.float16 (got {dtype})")
    if isinstance(x, np.ndarray) and dtype not in _NUMPY_OUT:
        raise ValueError("NumPy has no bfloat16: pass the input as a device tensor for a bfloat16 result")
    if compute is None:
        compute = torch.float16 if _torch_dtype(x) == torch.float16 else torch.bfloat16
    if compute not in _COMPUTE:
        raise ValueError(f"compute must be torch.bfloat16 or torch.float16 (got {compute})")
    levels = len(codebook)
    if levels > 256:
        raise ValueError(f"packed indices hold at most 8 bits: a codebook of {levels} entries does not fit")
    bits = index_bits(codebook) if bits is None else _check_bits(bits)
    if bits < index_bits(codebook):
        raise ValueError(f"{bits} bits cannot index a codebook of {levels} entries (it needs {index_bits(codebook)})")
    if scale is not None and group_scales is not None:
        raise ValueError("scale and group_scales are mutually exclusive")
    if offsets is not None and group_scales is None:
        raise ValueError("offsets need group_scales")
    _check_words(P)
    N, K = int(P.shape[0]), int(x.shape[-1])
    _check_extent(N, max(K, 1), "the layer")
    g = None
    if group_scales is not None:
        G = int(group_scales.shape[1]) if getattr(group_scales, "ndim", 0) == 2 else 0
        if group_size is None:
            if G < 1 or K % G != 0:
                raise ValueError(f"group scales of shape {tuple(group_scales.shape)} do not split {K} columns into groups")
            group_size = K // G
        g = int(group_size)
    _linear_shapes(K, g, "x")
    if tuple(P.shape) != packed_shape(N, K, bits):
        raise ValueError(f"x has {K} columns: {N} rows of them at {bits} bits are {packed_shape(N, K, bits)} words; got {tuple(P.shape)}")
    if scale is not None:
        _check_shape(scale, (N,), "scale")
    if group_scales is not None:
        _check_shape(group_scales, (N, K // g), "group scales")
    if offsets is not None:
        _check_shape(offsets, (N, K // g), "group offsets")
    if bias is not None:
        _check_shape(bias, (N,), "bias")
    lead = tuple(x.shape[:-1])
    M = int(np.prod(lead, dtype=np.int64))
    if M < 1 or M >= 1 << 31:
        raise ValueError(f"x must have 1 <= rows < 2^31 (got {tuple(x.shape)})")
    levels, lo, hi, table = engine.require_uniform(codebook)
    Xd = dev.aligned(dev.to_device(x, _torch_dtype(x)).reshape(M, K))
    Pd = dev.to_device(P.view(np.int32) if isinstance(P, np.ndarray) else P, torch.int32)
    Sd = dev.to_device(scale) if scale is not None else None
    Gd = dev.to_device(group_scales) if group_scales is not None else None
    Od = dev.to_device(offsets) if offsets is not None else None
    Bd = dev.to_device(bias) if bias is not None else None
    out = torch.empty((M, N), dtype=dtype, device=Xd.device)
    _lib.check(
        _lib.lib.slk_packed_gemm(
            dev.ptr(Xd), _OUT[Xd.dtype], dev.ptr(Pd), bits, levels, lo, hi, dev.ptr(table), dev.ptr(Sd), dev.ptr(Gd), dev.ptr(Od),
            g or 0, dev.ptr(Bd), M, N, K, _OUT[compute], _OUT[dtype], dev.ptr(out), dev.stream_handle(),
        )
    )
    return dev.like_input(out.reshape(lead + (N,)), x)


class PackedLinear(torch.nn.Module):
    """A linear layer kept as packed codebook indices: forward(x) = linear_packed(x, words, codebook, ...).  Buffers, present
    only where used: `words` int32 (N, bits * ceil(K / 32)); `values`, the codebook -- the float32 table, or float64 (levels,
    lo, hi) of a uniform one; `scale` (N,) (row_scale) or `group_scales` (N, K / group_size); `offsets` (N, K / group_size);
    `bias` (N,) float32.  Forward only (inference): it registers no autograd function and its buffers take no gradient."""

    def __init__(self, in_features, out_features, codebook, bits=None, group_size=None, offsets=False, row_scale=False, bias=True,
                 device=None):
        super().__init__()
        from .codebook import Codebook, UniformCodebook

        if not isinstance(codebook, (Codebook, UniformCodebook)):
            raise ValueError(f"PackedLinear takes a UniformCodebook or a Codebook (got {type(codebook).__name__})")
        self.in_features, self.out_features = int(in_features), int(out_features)
        self.bits = index_bits(codebook) if bits is None else _check_bits(bits)
        if self.bits < index_bits(codebook):
            raise ValueError(f"{self.bits} bits cannot index a codebook of {len(codebook)} entries (it needs {index_bits(codebook)})")
        self.group_size = None if group_size is None else int(group_size)
        if row_scale and self.group_size is not None:
            raise ValueError("row_scale and group_size are mutually exclusive")
        if offsets and self.group_size is None:
            raise ValueError("offsets need group_size")
        _linear_shapes(self.in_features, self.group_size)
        N, K = self.out_features, self.in_features
        self.codebook = codebook
        if isinstance(codebook, UniformCodebook):
            values = torch.tensor([len(codebook), float(codebook.min_val), float(codebook.max_val)], dtype=torch.float64, device=device)
        else:
            values = torch.tensor(np.asarray(codebook.values, np.float32), device=device)
        self.register_buffer("words", torch.zeros(packed_shape(N, K, self.bits), dtype=torch.int32, device=device))
        self.register_buffer("values", values)
        self.register_buffer("scale", torch.ones(N, dtype=torch.float32, device=device) if row_scale else None)
        G = K // self.group_size if self.group_size else 0
        self.register_buffer("group_scales", torch.ones((N, G), dtype=torch.float32, device=device) if G else None)
        self.register_buffer("offsets", torch.zeros((N, G), dtype=torch.float32, device=device) if offsets else None)
        self.register_buffer("bias", torch.zeros(N, dtype=torch.float32, device=device) if bias else None)

    def _load_from_state_dict(self, *args, **kwargs):
        super()._load_from_state_dict(*args, **kwargs)
        self._codebook_from_values()

    def _codebook_from_values(self):
        """`codebook` follows the `values` buffer (after load_state_dict)."""
        from .codebook import Codebook, UniformCodebook

        v = self.values.detach().cpu().numpy()
        if v.dtype == np.float64:
            same = isinstance(self.codebook, UniformCodebook) and [len(self.codebook), self.codebook.min_val, self.codebook.max_val] == v.tolist()
            self.codebook = self.codebook if same else UniformCodebook(int(v[0]), float(v[1]), float(v[2]))
        elif not (isinstance(self.codebook, Codebook) and np.array_equal(self.codebook.values, v)):
            self.codebook = Codebook(v)

    @classmethod
    def from_result(cls, layer, result, codebook, scale=None, bits=None):
        """The module of a torch.nn.Linear and the engine.LayerResult of its quantization (taken after the quantizing call,
        so that a corrected bias comes along): result.idx is packed; the scales are result.S (and result.O) when set --
        Sleekit.quantize_packed sets them on every path -- else `scale`: (out,) per row, or None for an unscaled layer.
        Beware: the result of a plain Sleekit.quantize(nbits) on the per-row path has no S, so it needs its scale passed as
        `scale=` (or quantize_packed); without it the module is that of an unscaled layer, wrong by the row scales."""
        if not isinstance(layer, torch.nn.Linear):
            raise ValueError(f"PackedLinear.from_result takes a torch.nn.Linear (got {type(layer).__name__})")
        idx = getattr(result, "idx", None)
        if idx is None or idx.ndim != 2 or tuple(idx.shape) != (layer.out_features, layer.in_features):
            raise ValueError(f"the result is of a {tuple(getattr(idx, 'shape', ()))} layer, not of this "
                             f"({layer.out_features}, {layer.in_features}) one")
        N, K = layer.out_features, layer.in_features
        S, O = getattr(result, "S", None), getattr(result, "O", None)
        if S is None:
            S = scale
        grouped = S is not None and S.ndim == 2
        if grouped and (S.shape[0] != N or S.shape[1] < 1 or K % S.shape[1] != 0):
            raise ValueError(f"group scales of shape {tuple(S.shape)} do not split a ({N}, {K}) layer into groups")
        if S is not None and not grouped:
            _check_shape(S, (N,), "scale")
        if O is not None and not grouped:
            raise ValueError("offsets need group scales")
        self = cls(K, N, codebook, bits, K // int(S.shape[1]) if grouped else None, O is not None, S is not None and not grouped,
                   layer.bias is not None, layer.weight.device)
        self.words.copy_(torch.as_tensor(pack_indices(dev.to_device(idx, torch.uint8), self.bits)))
        if S is not None:
            (self.group_scales if grouped else self.scale).copy_(torch.as_tensor(S))
        if O is not None:
            self.offsets.copy_(torch.as_tensor(O))
        if layer.bias is not None:
            self.bias.copy_(layer.bias.detach().float())
        return self

    def forward(self, x):
        return linear_packed(x, self.words, self.codebook, self.bits, self.scale, self.group_scales, self.group_size, self.offsets,
                             self.bias)

    def extra_repr(self):
        return (f"in_features={self.in_features}, out_features={self.out_features}, bits={self.bits}, levels={len(self.codebook)}, "
                f"group_size={self.group_size}, offsets={self.offsets is not None}, bias={self.bias is not None}")
