"""Randomized block Hadamard rotation of a layer's input features, before quantization and in front of the stored layer.

    rot = Rotation(layer.in_features, seed=0)                   # R = diag(s) blockdiag(H_b) / sqrt(b), orthogonal
    res = Sleekit(layer).quantize_packed(3, rotation=rot)       # quantizes (W R, R^T H R); layer.weight = Q R^T
    fast = RotatedLinear.from_result(layer, res, UniformCodebook(8, -1, 1))     # forward(x) = inner(x R)

W x = (W R)(R^T x) for an orthogonal R, so a layer quantized in the rotated basis computes the same function of the
rotated input x R (x a ROW of features, as everywhere in this package).  The rotation spreads outlier channels of the
Hessian and outlier weights over a whole block of `block` features, and the grid no longer spends its range on a few entries.

`s` is n signs of +-1, H_b the Sylvester-Hadamard matrix of order `block` (a power of two in 2..4096 that divides n).
Every product with R is ONE call of slk_hadamard_rows (include/sleekit_amd.h holds the arithmetic, which is a contract:
the butterfly network fixes both operands of every addition, so the result's bits are the same on any kernel):

    apply(x)     x R      sign, then butterflies, then 1 / sqrt(b)        x (..., n) float32, bfloat16, float16 or float64
    apply_t(x)   x R^T    butterflies, then 1 / sqrt(b), then sign
    hessian(H)   R^T H R  in float64 (two passes and a transpose), mirrored to bit-symmetry, back in float32

Float64 in gives float64 out; the other three compute in float32 and come out in `dtype` (default: x's).  NumPy in gives
NumPy out, device tensors in give device tensors out, everything runs on the GPU on the current stream, and there is no
CPU fallback.
"""

import numpy as np
import torch

from . import _device as dev
from . import _lib
from . import synth

_DTYPES = {torch.float32: _lib.DTYPE_F32, torch.bfloat16: _lib.DTYPE_BF16, torch.float16: _lib.DTYPE_F16, torch.float64: _lib.DTYPE_F64}
_NUMPY = {np.dtype(np.float32): torch.float32, np.dtype(np.float16): torch.float16, np.dtype(np.float64): torch.float64}
MAX_BLOCK = 4096


def default_block(n):
    """The largest power of two that divides n, capped at 4096."""
    n = int(n)
    if n < 1:
        raise ValueError(f"a rotation needs at least one feature (got {n})")
    return min(n & -n, MAX_BLOCK)


def make_signs(n, seed):
    """The sign rule: +1 where bit 13 of synth.hash_grid(seed, 7, 1, n) is set, else -1; (n,) float32 on the host."""
    bit = (synth.hash_grid(int(seed), 7, 1, int(n))[0] >> np.uint64(13)) & np.uint64(1)
    return np.where(bit != 0, np.float32(1.0), np.float32(-1.0)).astype(np.float32)


def _check_block(n, block):
    if isinstance(block, bool) or not isinstance(block, (int, np.integer)):
        raise ValueError(f"block must be an integer (got {block!r})")
    block = int(block)
    if block < 2 or block > MAX_BLOCK or block & (block - 1):
        raise ValueError(f"block must be a power of two in 2..{MAX_BLOCK} (got {block})")
    if n % block != 0:
        raise ValueError(f"block {block} does not divide the {n} features")
    return block


def _torch_dtype(x):
    if isinstance(x, torch.Tensor):
        return x.dtype
    if isinstance(x, np.ndarray):
        return _NUMPY.get(x.dtype)
    return None


class Rotation:
    """R = diag(signs) blockdiag(H_block) / sqrt(block) over n features; `signs` is (n,) float32 on the device."""

    def __init__(self, n, block=None, seed=0, device=None):
        self._set(torch.from_numpy(make_signs(n, seed)).to(dev.require_gpu() if device is None else device), block)
        self.seed = int(seed)

    def _set(self, signs, block):
        # the kernel reads n float32: whatever float type the signs arrive in (a module's .half() casts its buffers), they
        # are held as contiguous float32, which loses nothing of +-1
        if not isinstance(signs, torch.Tensor) or signs.ndim != 1 or signs.numel() < 1 or not signs.dtype.is_floating_point:
            raise ValueError("signs must be a 1-D floating-point tensor")
        signs = signs.detach().to(torch.float32).contiguous()
        self.n = int(signs.numel())
        self.block = _check_block(self.n, default_block(self.n) if block is None else block)  # (an odd n has no block)
        self.signs = signs

    @classmethod
    def from_signs(cls, signs, block):
        """The rotation of stored signs ((n,) of +-1, NumPy or tensor) and a block."""
        if not isinstance(signs, (np.ndarray, torch.Tensor)) or signs.ndim != 1 or signs.shape[0] < 1:
            raise ValueError("signs must be a 1-D NumPy array or torch tensor")
        signs = dev.to_device(signs)
        if not bool((signs.abs() == 1.0).all()):
            raise ValueError("signs must be +1 or -1")
        return cls._of(signs, block)

    @classmethod
    def _of(cls, signs, block):
        """from_signs for a device tensor that is known to hold +-1 (no read-back of the values)."""
        self = cls.__new__(cls)
        self._set(signs, block)
        self.seed = None
        return self

    def _rows(self, x, dtype, transposed):
        src = _torch_dtype(x)
        if src not in _DTYPES or x.ndim < 1:
            raise ValueError("x must be a NumPy array or torch tensor of float32, bfloat16, float16 or float64 with at least one "
                             f"dimension (got {type(x).__name__} of {getattr(x, 'dtype', None)})")
        if x.shape[-1] != self.n:
            raise ValueError(f"x has {x.shape[-1]} features but the rotation has {self.n}")
        dtype = src if dtype is None else dtype
        if dtype not in _DTYPES:
            raise ValueError(f"dtype must be torch.float32, torch.bfloat16, torch.float16 or torch.float64 (got {dtype})")
        if (src == torch.float64) != (dtype == torch.float64):
            raise ValueError(f"float64 goes to float64 and nothing else does (x is {src}, dtype {dtype})")
        if isinstance(x, np.ndarray) and dtype == torch.bfloat16:
            raise ValueError("NumPy has no bfloat16: pass the input as a device tensor for a bfloat16 result")
        lead = tuple(x.shape[:-1])
        rows = int(np.prod(lead, dtype=np.int64))
        out_shape = lead + (self.n,)
        Xd = dev.to_device(x, src)
        signs = self.signs if self.signs.device == Xd.device else self.signs.to(Xd.device)
        assert signs.dtype == torch.float32 and signs.numel() == self.n and signs.is_contiguous()
        out = torch.empty(out_shape, dtype=dtype, device=Xd.device)
        if rows > 0:
            _lib.check(
                _lib.lib.slk_hadamard_rows(dev.ptr(Xd), _DTYPES[src], dev.ptr(out), _DTYPES[dtype], rows, self.n, self.block,
                                           dev.ptr(signs), 1 if transposed else 0, dev.stream_handle())
            )
        return dev.like_input(out, x)

    def apply(self, x, dtype=None):
        """x R for x (..., n): the rotated features (of activations), the rotated weight (of a weight's rows)."""
        return self._rows(x, dtype, False)

    def apply_t(self, x, dtype=None):
        """x R^T: back from the rotated basis; apply_t(apply(x)) is x up to rounding (exactly, for a block that is a power of 4,
        wherever nothing overflows)."""
        return self._rows(x, dtype, True)

    def hessian(self, H):
        """R^T H R of a symmetric float32 H (n, n), in float32 and bit-symmetric: float64 rows pass, transpose, rows pass, the
        lower triangle mirrored onto the upper one, one rounding to float32."""
        if not isinstance(H, (np.ndarray, torch.Tensor)) or H.ndim != 2 or tuple(H.shape) != (self.n, self.n):
            raise ValueError(f"H must be ({self.n}, {self.n}); got {tuple(getattr(H, 'shape', ()))}")
        Hd = dev.to_device(H).double()
        half = self._rows(Hd, None, False).t().contiguous()   # (H R)^T = R^T H, H symmetric
        full = self._rows(half, None, False)                    # R^T H R
        i = torch.arange(self.n, device=full.device)
        out = torch.where(i[:, None] >= i[None, :], full, full.t()).float().contiguous()
        return dev.like_input(out, H)


class RotatedLinear(torch.nn.Module):
    """A stored layer behind its rotation: forward(x) = inner(x R), the transform's output in x's dtype.  `inner` is the module
    of a layer quantized in the rotated basis (PackedLinear, MXLinear).  The rotation is kept as the buffer `signs` (n,)
    float32 and `block` (extra state).  `.half()` / `.bfloat16()` cast the buffer like any other; the transform then takes
    a float32 copy of it (+-1 is exact in every float type).  Forward only (inference).

    fused=True (an MXLinear inside; anything else: ValueError) hands the rotation to mx.linear_mxfp4, which runs it inside the
    activation quantizer: x is read once and only the codes are written.  That path quantizes the transform's float32 value,
    so for a 16-bit x it differs from the default forward by the one rounding of x R to x's dtype that the default makes
    between the transform and the layer -- which is why it is opt-in; for a float32 x the two give the same bits.  `fused`
    is extra state beside `block`; a state dict without it means False."""

    def __init__(self, inner, rotation, fused=False):
        super().__init__()
        if not isinstance(rotation, Rotation):
            raise ValueError(f"RotatedLinear takes a Rotation (got {type(rotation).__name__})")
        self.fused = bool(fused)
        if self.fused:
            from .mx import MXLinear

            if not isinstance(inner, MXLinear):
                raise ValueError(f"fused=True needs an MXLinear inside (got {type(inner).__name__})")
        features = getattr(inner, "in_features", None)
        if features is not None and int(features) != rotation.n:
            raise ValueError(f"the rotation has {rotation.n} features but the layer takes {features}")
        self.inner = inner
        self.block = rotation.block
        self.register_buffer("signs", rotation.signs.detach().clone())

    @property
    def rotation(self):
        return Rotation._of(self.signs, self.block)

    def get_extra_state(self):
        return {"block": self.block, "fused": True} if self.fused else {"block": self.block}

    def set_extra_state(self, state):
        self.block = _check_block(int(self.signs.numel()), state["block"])
        fused = bool(state.get("fused", False))
        if fused:
            from .mx import MXLinear

            if not isinstance(self.inner, MXLinear):
                raise ValueError(f"fused=True needs an MXLinear inside (got {type(self.inner).__name__})")
        self.fused = fused

    @classmethod
    def from_result(cls, layer, result, codebook=None, fused=False, activations="mxfp8", **kw):
        """The module of a torch.nn.Linear and the result of Sleekit(layer).quantize_packed / quantize_mxfp4 / quantize_mxfp6 (rotation=):
        MXLinear.from_result(layer, result) inside when the result carries `codes`, else PackedLinear.from_result(layer,
        result, codebook, **kw).  fused and activations ("mxfp8" | "mxfp4" | "mxfp6_e2m3" | "bfloat16" | "float16") are the MXLinear's (class docstring, mx.MXLinear)."""
        rotation = getattr(result, "rotation", None)
        if rotation is None:
            raise ValueError("the result carries no rotation: it was not quantized with rotation=")
        if getattr(result, "codes", None) is not None:
            from .mx import MXLinear

            inner = MXLinear.from_result(layer, result, activations=activations)
        else:
            from .packing import PackedLinear

            if activations != "mxfp8":
                raise ValueError("activations is the MXLinear's: this result carries no MX codes")
            inner = PackedLinear.from_result(layer, result, codebook, **kw)
        return cls(inner, rotation, fused)

    def forward(self, x):
        if self.fused or self._weight_only():
            return self.inner(x, rotation=self.rotation)
        return self.inner(self.rotation.apply(x))

    def _weight_only(self):
        """An MXLinear with 16-bit activations inside: it has no quantizer to fuse the rotation into, and rotates x itself --
        the transform writing the compute type, then the product -- so both values of `fused` are that one route."""
        from .mx import _HALVES, MXLinear

        return isinstance(self.inner, MXLinear) and self.inner.activations in _HALVES

    def extra_repr(self):
        return f"features={self.signs.numel()}, block={self.block}" + (", fused=True" if self.fused else "")
