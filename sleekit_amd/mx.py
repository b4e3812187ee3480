"""MXFP4: the block format the MI355X computes in, as an output of the quantizer.

    S, E = compute_mx_scales(W, H, mode="mse")           # power-of-two scales (R, n / 32): float32, and E8M0 bytes
    res = quantize_mxfp4(W, H, nb_ls_moves=10)            # MXResult(Q, idx, S, codes, scales)
    res.Q == dequantize_mxfp4(res.codes, res.scales)      # bit for bit; dtype=torch.bfloat16 / float16: == Q.to(dtype)
    codes, scales = pack_mxfp4(idx, S);  idx, S = unpack_mxfp4(codes, scales)

FORMAT.  A block is BLOCK = 32 consecutive original columns of one row (n % 32 != 0: ValueError).
  elements  FP4 E2M1, code = sign << 3 | m, magnitudes m = 0 .. 7: 0, 0.5, 1, 1.5, 2, 3, 4, 6.  The codebook E2M1 is the
            15-entry table -6 .. 6 whose limits are the midpoints (a tie goes upward); table index i < 7 is code
            8 | (7 - i), otherwise i - 7.  Code 0x8 (-0) is never written and reads back as index 7, value +0; an index
            above 14 is a caller error and is stored as code 7.
  codes     uint8 (R, n / 2): byte j of a row holds column 2 j in its low nibble, column 2 j + 1 in its high nibble --
            packing.pack_indices(code, 4) viewed as bytes.
  scales    uint8 (R, n / 32), E8M0: byte b means 2^(b - 127).  Scales chosen here have b in [71, 253] (2^-56 .. 2^126, so s
            and 1 / s are normal float32); byte 255 (NaN) is never written and is a ValueError on input.
Known answers: indices 0 .. 14 are codes f e d c b a 9 0 1 2 3 4 5 6 7; columns with codes [1, 2, 0xf, 0] pack to bytes
[0x21, 0x0f]; the scale 0.0078125 is byte 120.

SCALES.  For every (row, block): b0 = compute_non_saturating_scaling(block, E2M1) (sleekit/scaling.py:44-55), base the
smallest power of two >= b0; mode "max" gives base, "mse" and "diag" run the reference's loop body (scaling.py:127-134)
over the factors 0.125, 0.25, 0.5, 1 instead of its linspace -- quantize_with_scaling at f * base, the error with None or
diag(H) of the block's columns as a float32 row sum in NumPy's order, the first minimum kept -- and give base * best factor.
(Where no error is below +inf -- squares that overflow float32 -- the reference's answer is not a scale; base is kept.)

THE LOOP is groups.quantize_layer_grouped(W, S, E2M1, H, 32, ...) untouched: with a power-of-two s every step of the group
quantizer codebook(x / s) / (1 / s) is exact, so Q is +-magnitude * 2^(b - 127) bit for bit and the packed form loses nothing.

LINEAR.  The packed layer runs on the block-scaled MFMA without being de-quantized:
    y = linear_mxfp4(x, res.codes, res.scales, bias)      # x (..., K) float32 / bfloat16 / float16 -> (..., N)
    a_codes, a_scales = quantize_mxfp8(X)                  # what it does to x first: MXFP8 E4M3, (M, K) and (M, K / 32)
    Y = matmul_mx(a_codes, a_scales, res.codes, res.scales)   # sum_k deq(A)[m][k] deq(W)[n][k], float32 sums
    layer = MXLinear.from_result(nn_linear, res)           # a torch.nn.Module with buffers codes, scales, bias
  activations  blocks of 32 along K, scale byte = exponent + 127 of the smallest power of two >= max(amax / 448, 1e-16)
            (float32; compute_mx_scales' "max" with 448 for 6; a block of zeros: byte 74), elements x / s rounded to
            nearest even onto OCP E4M3 (e4m3fn: bias 7, subnormals k 2^-9, largest 448 = 0x7e), code = sign << 7 |
            exp << 3 | man; a zero magnitude is 0x00 (never -0) and 0x7f / 0xff are never written.  NaN or inf: ValueError.
Known answers: amax 1.0 gives byte 119 and 1.0, -0.3, 0.001, 0 the codes 78 ea 28 00; amax 1.75 gives byte 119 and 1.75,
-1.75, 0.01, 1e-5 the codes 7e fe 42 01.  The product does not look for scale byte 255: it yields NaN, as the hardware does.

W4A4.  `activations="mxfp4"` (matmul_mx, linear_mxfp4, MXLinear) quantizes x to MXFP4 instead: the same instruction with
E2M1 on both sides runs at twice the E4M3 rate and the activation operand is half the bytes.
    a_codes, a_scales = quantize_mxfp4_act(X)              # (M, K / 2) and (M, K / 32); dequantize_mxfp4 inverts it
  activations  the MXFP8 rule with 6 in place of 448: scale byte = exponent + 127 of the smallest power of two >=
            max(amax / 6, 1e-16), elements x / s rounded to nearest onto 0, .5, 1, 1.5, 2, 3, 4, 6, ties to the even code,
            clamped at 6, code = sign << 3 | index, a zero magnitude 0x0 (never 0x8); two codes a byte, the even k in the
            low nibble -- the layer's own layout.
Known answers: amax 6.0 gives byte 127 and 6, -0.3, 0.75, 2.5 the codes 7 9 2 4; amax 1.0 gives byte 125 and 1.0, -1.0,
0.3, 0.0625 the codes 6 e 2 0.
FP4 keeps 2 significant bits, so one outlier channel costs its whole block its small values: this format is meant to
follow a rotation (sleekit_amd.rotation), which spreads an outlier over its block.  `rotation=R` in linear_mxfp4 runs the
rotation inside the quantizer (slk_mx_rotate_quantize_act: x is read once and only the codes are written); the result is
linear_mxfp4(R.apply(x, dtype=torch.float32), ...) bit for bit.

W4A6.  `activations="mxfp6_e2m3"` quantizes x to MXFP6 (E2M3) instead: FP6 operands run at the FP4 rate on this chip, so the
product costs what W4A4's does, on three quarters of MXFP8's activation bytes, and inside a block of 32 under a power-of-two
scale E2M3 carries the three mantissa bits E4M3 carries -- behind a rotation W4A6's output error is W4A8's to three digits
(DESIGN.md section 20).  The bare "mxfp6" is refused: there are two FP6 element formats.
    a_codes, a_scales = quantize_mxfp6_act(X)              # (M, 3 K / 4) and (M, K / 32); dequantize_mxfp6_act inverts it
  activations  the MXFP8 rule with 7.5 in place of 448: scale byte = exponent + 127 of the smallest power of two >=
            max(amax / 7.5, 1e-16), elements x / s rounded to nearest onto OCP E2M3 (bias 1, subnormals m / 8, normals
            2^(e - 1) (1 + m / 8), e = 1 .. 3: 0 .. 1.875 in steps of 0.125, 2 .. 3.75 of 0.25, 4 .. 7.5 of 0.5), ties to the
            even code, clamped at 7.5, code = sign << 5 | e << 3 | m, a zero magnitude 0x00 (never 0x20).  A row of a_codes
            is a little-endian bit stream, element k at bits 6 k .. 6 k + 5: 24 bytes a block, four codes c0 .. c3 the three
            bytes of c0 | c1 << 6 | c2 << 12 | c3 << 18.
Known answers: amax 7.5 gives byte 127 and 7.5, -0.3, 0.0625, 0.1875 the codes 1f 22 00 02, bytes 9f 08 08; amax 1.0 gives
byte 125 and 1.0, -1.0, 0.3, 0.0625 the codes 18 38 0a 02, bytes 18 ae 08.
`rotation=R` works as for the other formats (slk_mx_rotate_quantize_act6).

MXFP6 LAYERS.  `weights="mxfp6_e2m3"` (compute_mx_scales, matmul_mx, MXLinear) and quantize_mxfp6, pack_mxfp6, unpack_mxfp6,
dequantize_mxfp6, linear_mxfp6 are the same pipeline with E2M3 elements: 6.25 bits a weight for about a sixteenth of MXFP4's
squared rounding error, on the same MFMA at the FP4 rate (W6A8 with "mxfp8" activations, W6A6 with "mxfp6_e2m3"; "mxfp4"
activations against such a layer are refused).  The usual recipe: MXFP6 for the few sensitive layers, MXFP4 for the rest.
  elements  OCP E2M3, code = sign << 5 | e << 3 | m, the activation format's values.  The codebook E2M3 is the 63-entry table
            -7.5 .. 7.5 whose limits are the midpoints (a tie goes upward); table index i < 31 is code 0x20 | (31 - i),
            otherwise i - 31.  Code 0x20 (-0) is never written and reads back as index 31; an index above 62 is a caller
            error and is stored as code 0x1f.
  codes     uint8 (R, 3 n / 4): a row is a little-endian stream of 6-bit codes, element k at bits 6 k .. 6 k + 5, 24 bytes a
            block -- the MXFP6 activations' form, so dequantize_mxfp6 is dequantize_mxfp6_act's kernel.
  scales    as MXFP4's; the scale rule is the one above with E2M3 and 7.5 in place of E2M1 and 6.
Known answers: indices 0, 1, 30, 31, 32, 61, 62 are codes 3f 3e 21 00 01 1e 1f; indices [0, 62, 31, 32] pack to bytes ff 07 04.
    res = quantize_mxfp6(W, H, nb_ls_moves=10);  y = linear_mxfp6(x, res.codes, res.scales, bias, activations="mxfp6_e2m3")
    layer = MXLinear.from_result(nn_linear, res)          # the format is read off the widths of res.codes and res.scales

WEIGHT-ONLY (W4A16, W6A16).  `activations="bfloat16"` or "float16" (linear_mxfp4, linear_mxfp6, linear_mx_experts, MXLinear,
MXExperts; both weight formats) quantizes nothing: the layer is de-quantized inside a bfloat16 / float16 MFMA GEMM
(slk_mx_gemm_a16) and x, rounded to that type where it is float32, meets dequantize_mxfp4 / _mxfp6(codes, scales, dtype=that
type) bit for bit.  One launch, no flag, no wait for the stream; a NaN or an infinity in x propagates as in any GEMM.  The
operand contract is promised where every non-zero weight is a normal number of the type: scale bytes 10 .. 245 for bfloat16,
116 .. 140 for float16.  `rotation=R` is the call on R.apply(x, dtype=that type).  matmul_mx* and the gated MLP take coded
activations only and refuse the two names.
    y = linear_mxfp4(x, res.codes, res.scales, bias, activations="bfloat16");  layer = MXLinear.from_result(nn_linear, res, "bfloat16")

EXPERTS.  A mixture-of-experts layer is E packed layers of one shape, stacked: codes (E, N, K bits / 8), scales (E, N, K / 32),
bias (E, N).  One call multiplies every row with the layer of its expert (slk_mx_gemm_experts): the rows are sorted by expert
and `offsets`, int32 (E + 1,) on the device, says where each expert's rows begin -- offsets[0] == 0, never decreasing,
offsets[E] == M; the host never reads it, and offsets that break the rule are a ValueError after the launches.  Each expert's
rows are bit for bit matmul_mx of that slice.  Every format pair of matmul_mx is taken.
    results = quantize_experts(Ws, Hs)                         # E MXResults, each quantize_mxfp4(W, H)'s bit for bit
    experts = MXExperts.from_results(results, biases)          # buffers codes, scales, bias
    y = experts.forward_tokens(x, expert_ids, gates)           # x (T, K), expert_ids and gates (T, k) -> (T, N)
    order, offsets = sort_by_expert(expert_ids, E);  Y = linear_mx_experts(x[order // k], codes, scales, offsets, bias)
    y = experts.forward_logits(x, logits, k)                   # from router logits (T, E): top-k gates, sort, row-mapped quantizer,
                                                               # product and combine in HIP (sleekit_amd.routing), forward_tokens' bits

GATED MLP.  down(act(gate(x)) * up(x)) in three launches: the up layer holds gate and up (2 N rows), and the fused product
(slk_mx_gemm_glu) applies the gate in float32 and writes h as the down layer's a_codes / a_scales -- the section "gated MLP"
at the end of this file has the gate, the two layouts and the calls.
    h_codes, h_scales = matmul_mx_glu(a_codes, a_scales, up_codes, up_scales, up_bias)      # (M, N bits / 8), (M, N / 32)
    y = gated_mlp_mx(x, up_codes, up_scales, down_codes, down_scales);  y = MXGatedMLP(up, down)(x)
    y = MXExpertsMLP(up_experts, down_experts).forward_tokens(x, expert_ids, gates)
A down layer quantized behind a rotation of the hidden features (down_rotation=; matmul_mx_glu(rotation=)) keeps the three
launches when the rotation's block is at most 32: the product rotates each MX block of h before it quantizes it
(slk_mx_gemm_glu_rot).  A larger block takes the elementwise route between the two products, with the same bits.

Same conventions as the rest of the package: NumPy in gives NumPy out, device tensors in give device tensors out,
everything runs on the GPU on the current stream, and there is no CPU fallback.
"""

import collections
import math

import numpy as np
import torch

from . import _device as dev
from . import _lib
from . import groups
from . import routing
from .codebook import Codebook

BLOCK = 32
E2M1 = Codebook([-6, -4, -3, -2, -1.5, -1, -0.5, 0, 0.5, 1, 1.5, 2, 3, 4, 6])
_E2M3_MAGNITUDES = [m / 8 for m in range(1, 8)] + [2.0 ** (e - 1) * (1 + m / 8) for e in (1, 2, 3) for m in range(8)]
E2M3 = Codebook([-v for v in reversed(_E2M3_MAGNITUDES)] + [0.0] + _E2M3_MAGNITUDES)

MXResult = collections.namedtuple("MXResult", "Q idx S codes scales")

_MODES = {"max": _lib.MX_MAX, "mse": _lib.MX_MSE, "diag": _lib.MX_DIAG}
_OUT = {torch.float32: _lib.DTYPE_F32, torch.bfloat16: _lib.DTYPE_BF16, torch.float16: _lib.DTYPE_F16}

# A weight format as plain data: the bits of a code (codes is (R, n bits / 8)), its C constant, the codebook of the loop, its
# largest magnitude, the activation formats its product takes, and the C entries of the scale search, the pack, the unpack
# and the de-quantizer.
_Weights = collections.namedtuple("_Weights", "name bits c_fmt codebook largest activations scale_entry pack_entry unpack_entry dequantize_entry")
_WEIGHTS = {f.name: f for f in (
    _Weights("mxfp4", 4, _lib.MX_W_FP4, E2M1, 6.0, ("mxfp8", "mxfp4", "mxfp6_e2m3"),
             "slk_mx_scale_search", "slk_mx_pack", "slk_mx_unpack", "slk_mx_dequantize"),
    _Weights("mxfp6_e2m3", 6, _lib.MX_W_FP6, E2M3, 7.5, ("mxfp8", "mxfp6_e2m3"),
             "slk_mx_scale_search6", "slk_mx_pack6", "slk_mx_unpack6", "slk_mx_dequantize_act6"),
)}
_FP4, _FP6 = _WEIGHTS["mxfp4"], _WEIGHTS["mxfp6_e2m3"]


def _weight_format(weights):
    """The _Weights of a `weights` value.  (The bare "mxfp6" names two element formats and is refused.)"""
    if not isinstance(weights, str) or weights not in _WEIGHTS:
        raise ValueError(f'weights must be "mxfp4" or "mxfp6_e2m3" (got {weights!r})')
    return _WEIGHTS[weights]


def _blocks(n):
    if n < BLOCK or n % BLOCK != 0:
        raise ValueError(f"MX blocks are {BLOCK} columns: the column count must be a positive multiple of {BLOCK} (got {n})")
    return n // BLOCK


def _matrix(x, what, dtypes):
    if not isinstance(x, (np.ndarray, torch.Tensor)) or x.ndim != 2:
        raise ValueError(f"{what} must be a 2-D NumPy array or torch tensor")
    if x.dtype not in dtypes:
        raise ValueError(f"{what} must be {dtypes[0]} (got {x.dtype})")
    if x.shape[0] < 1 or x.shape[0] >= 1 << 31 or x.shape[1] >= 1 << 31:
        raise ValueError(f"{what} must have 1 <= rows, columns < 2^31 (got {tuple(x.shape)})")
    return int(x.shape[0]), int(x.shape[1])


def _raise_flag(flag, message):
    if flag is not None and int(flag.item()):
        raise ValueError(message)


def compute_mx_scales(W, H=None, mode="mse", weights="mxfp4"):
    """(S, E): the blocks' power-of-two scales as float32 and as E8M0 bytes, (R, n / 32) each (module docstring).
    mode "max", "mse" or "diag"; "diag" weighs the errors with diag(H) and needs H.  weights: the element format the scales
    are chosen for, "mxfp4" (E2M1) or "mxfp6_e2m3"."""
    wf = _weight_format(weights)
    if mode not in _MODES:
        raise ValueError(f'MX scale modes are "max", "mse" and "diag" (got "{mode}")')
    if mode == "diag" and H is None:
        raise ValueError('scale mode "diag" needs the Hessian H')
    R, n = _matrix(W, "W", (torch.float32, np.float32))
    G = _blocks(n)
    Wd = dev.to_device(W)
    hd = None
    if mode == "diag":
        Hd = dev.to_device(H)
        if tuple(Hd.shape) != (n, n):
            raise ValueError(f"H must be ({n}, {n}); got {tuple(Hd.shape)}")
        hd = Hd.diagonal().contiguous()
    S = torch.empty((R, G), dtype=torch.float32, device=Wd.device)
    E = torch.empty((R, G), dtype=torch.uint8, device=Wd.device)
    _lib.check(getattr(_lib.lib, wf.scale_entry)(dev.ptr(Wd), dev.ptr(hd), _MODES[mode], R, n, dev.ptr(E), dev.ptr(S), dev.stream_handle()))
    return dev.like_input(S, W), dev.like_input(E, W)


def _pack(idx_d, S_d, R, n, wf=_FP4):
    """(codes, scales) of device idx (R, n) and / or S (R, n / 32); either may be None."""
    device = (idx_d if idx_d is not None else S_d).device
    codes = torch.empty((R, n * wf.bits // 8), dtype=torch.uint8, device=device) if idx_d is not None else None
    scales = torch.empty((R, n // BLOCK), dtype=torch.uint8, device=device) if S_d is not None else None
    flag = torch.empty(1, dtype=torch.int32, device=device) if S_d is not None else None
    _lib.check(getattr(_lib.lib, wf.pack_entry)(dev.ptr(idx_d), dev.ptr(S_d), R, n, dev.ptr(codes), dev.ptr(scales), dev.ptr(flag), dev.stream_handle()))
    _raise_flag(flag, "MX scales must be positive powers of two in 2^-126 .. 2^127 (E8M0)")
    return codes, scales


def _unpack(codes_d, scales_d, R, n, wf=_FP4):
    device = (codes_d if codes_d is not None else scales_d).device
    idx = torch.empty((R, n), dtype=torch.uint8, device=device) if codes_d is not None else None
    S = torch.empty((R, n // BLOCK), dtype=torch.float32, device=device) if scales_d is not None else None
    flag = torch.empty(1, dtype=torch.int32, device=device) if scales_d is not None else None
    _lib.check(getattr(_lib.lib, wf.unpack_entry)(dev.ptr(codes_d), dev.ptr(scales_d), R, n, dev.ptr(idx), dev.ptr(S), dev.ptr(flag), dev.stream_handle()))
    _raise_flag(flag, "scale byte 255 is E8M0's NaN, not a scale")
    return idx, S


def _check_scale_shape(x, R, n, what):
    if tuple(x.shape) != (R, n // BLOCK):
        raise ValueError(f"{what} must be ({R}, {n // BLOCK}) for a ({R}, {n}) layer; got {tuple(x.shape)}")


def _pack_layer(idx, S, wf):
    R, n = _matrix(idx, "indices", (torch.uint8, np.uint8))
    _blocks(n)
    _matrix(S, "scales", (torch.float32, np.float32))
    _check_scale_shape(S, R, n, "scales")
    codes, scales = _pack(dev.aligned(dev.to_device(idx, torch.uint8)), dev.to_device(S), R, n, wf)
    return dev.like_input(codes, idx), dev.like_input(scales, idx)


def _unpack_layer(codes, scales, wf):
    R, n = _weights(codes, scales, wf)
    idx, S = _unpack(dev.aligned(dev.to_device(codes, torch.uint8)), dev.to_device(scales, torch.uint8), R, n, wf)
    return dev.like_input(idx, codes), dev.like_input(S, codes)


def pack_mxfp4(idx, S):
    """uint8 table indices (R, n) and float32 power-of-two scales (R, n / 32) -> (codes uint8 (R, n / 2), scales uint8
    (R, n / 32)).  A scale that is not a power of two E8M0 holds: ValueError."""
    return _pack_layer(idx, S, _FP4)


def unpack_mxfp4(codes, scales):
    """(codes (R, n / 2), scales (R, n / 32)) -> (idx uint8 (R, n), S float32 (R, n / 32))."""
    return _unpack_layer(codes, scales, _FP4)


def pack_mxfp6(idx, S):
    """pack_mxfp4 for an MXFP6 layer: indices into the 63-entry E2M3 table -> (codes uint8 (R, 3 n / 4), scales uint8
    (R, n / 32)) (module docstring, MXFP6 LAYERS)."""
    return _pack_layer(idx, S, _FP6)


def unpack_mxfp6(codes, scales):
    """(codes (R, 3 n / 4), scales (R, n / 32)) -> (idx uint8 (R, n), S float32 (R, n / 32))."""
    return _unpack_layer(codes, scales, _FP6)


def encode_scales(S):
    """float32 power-of-two scales (R, G) -> E8M0 bytes (R, G); anything E8M0 does not hold: ValueError."""
    R, G = _matrix(S, "scales", (torch.float32, np.float32))
    return dev.like_input(_pack(None, dev.to_device(S), R, G * BLOCK)[1], S)


def decode_scales(E):
    """E8M0 bytes (R, G) -> float32 scales 2^(b - 127); byte 255: ValueError."""
    R, G = _matrix(E, "scale bytes", (torch.uint8, np.uint8))
    return dev.like_input(_unpack(None, dev.to_device(E, torch.uint8), R, G * BLOCK)[1], E)


def dequantize_mxfp4(codes, scales, dtype=torch.float32):
    """The layer rebuilt from its packed form: (R, n) of `dtype` (float32: bit for bit the Q that was packed; bfloat16 or
    float16: that value rounded to nearest even, `.to(dtype)`).  NumPy input gives a NumPy array, which has no bfloat16."""
    return _dequantize(codes, scales, dtype, _FP4, "codes")


def dequantize_mxfp6(codes, scales, dtype=torch.float32):
    """dequantize_mxfp4 for an MXFP6 layer (codes (R, 3 n / 4)): float32 is bit for bit the Q that was packed."""
    return _dequantize(codes, scales, dtype, _FP6, "codes")


def _quantize_layer(wf, W, H, act_order, damp, scale_mode, nb_ls_moves, scales, min_block_size, num_blocks, want_ls_trace):
    R, n = W.shape
    _blocks(n)
    if scales is None:
        S = compute_mx_scales(W, H, scale_mode, wf.name)[0]
    else:
        S = dev.to_device(scales)
        _check_scale_shape(S, R, n, "scales")
    res = groups.quantize_layer_grouped(W, S, wf.codebook, H, BLOCK, act_order, damp, min_block_size, num_blocks, nb_ls_moves=nb_ls_moves,
                                        want_ls_trace=want_ls_trace)
    codes, E = _pack(res.idx, S, R, n, wf)  # (scales given by the caller are checked here: not a power of two, ValueError)
    return MXResult(res.Q, res.idx, S, codes, E), res


def _quantize_checked(wf, W, H, act_order, damp, scale_mode, nb_ls_moves, scales, min_block_size, num_blocks):
    _matrix(W, "W", (torch.float32, np.float32))
    if H is None or H.ndim != 2 or tuple(H.shape) != (W.shape[1], W.shape[1]):
        raise ValueError(f"H must be ({W.shape[1]}, {W.shape[1]})")
    if scale_mode not in _MODES:
        raise ValueError(f'MX scale modes are "max", "mse" and "diag" (got "{scale_mode}")')
    _blocks(int(W.shape[1]))
    out, _ = _quantize_layer(wf, dev.to_device(W), dev.to_device(H), act_order, damp, scale_mode, nb_ls_moves, scales, min_block_size,
                             num_blocks, False)
    return MXResult(*(dev.like_input(t, W) for t in out))


def quantize_layer_mxfp4(W, H, act_order="diag", damp=0.01, scale_mode="mse", nb_ls_moves=0, scales=None, min_block_size=32,
                         num_blocks=8, want_ls_trace=False):
    """quantize_mxfp4 on device tensors (W (R, n), H (n, n), float32): (MXResult of device tensors, the grouped loop's
    engine.LayerResult; want_ls_trace: with the moves taken in its ls_trace)."""
    return _quantize_layer(_FP4, W, H, act_order, damp, scale_mode, nb_ls_moves, scales, min_block_size, num_blocks, want_ls_trace)


def quantize_layer_mxfp6(W, H, act_order="diag", damp=0.01, scale_mode="mse", nb_ls_moves=0, scales=None, min_block_size=32,
                         num_blocks=8, want_ls_trace=False):
    """quantize_layer_mxfp4 with the E2M3 codebook: the MXResult's codes are (R, 3 n / 4)."""
    return _quantize_layer(_FP6, W, H, act_order, damp, scale_mode, nb_ls_moves, scales, min_block_size, num_blocks, want_ls_trace)


def quantize_mxfp4(W, H, act_order="diag", damp=0.01, scale_mode="mse", nb_ls_moves=0, scales=None, min_block_size=32,
                   num_blocks=8):
    """GPTQ-style quantization of one layer to MXFP4: the scales of compute_mx_scales(W, H, scale_mode) (or `scales`,
    float32 powers of two (R, n / 32)), groups.quantize_layer_grouped with the E2M1 codebook and groups of 32 (nb_ls_moves of
    its local search after the loop, up to 16384 columns), then the pack.  Returns MXResult(Q, idx, S, codes, scales):
    Q float32 de-scaled like W, idx the uint8 table indices, S the float32 scales, codes and scales the packed form."""
    return _quantize_checked(_FP4, W, H, act_order, damp, scale_mode, nb_ls_moves, scales, min_block_size, num_blocks)


def quantize_mxfp6(W, H, act_order="diag", damp=0.01, scale_mode="mse", nb_ls_moves=0, scales=None, min_block_size=32,
                   num_blocks=8):
    """quantize_mxfp4 to MXFP6: the scales of compute_mx_scales(..., weights="mxfp6_e2m3"), the grouped loop and its local
    search with the 63-entry E2M3 codebook, then pack_mxfp6.  The same MXResult fields; codes are (R, 3 n / 4) and
    dequantize_mxfp6(codes, scales) is Q bit for bit."""
    return _quantize_checked(_FP6, W, H, act_order, damp, scale_mode, nb_ls_moves, scales, min_block_size, num_blocks)


# ---------------------------------------------------------------------------------------------------------------- linear
_ACT = (torch.float32, torch.bfloat16, torch.float16, np.float32, np.float16)
_NP_OUT = {torch.float32: np.float32, torch.float16: np.float16}


def _out_dtype(dtype, template, what="input"):
    if dtype not in _OUT:
        raise ValueError(f"dtype must be torch.float32, torch.bfloat16 or torch.float16 (got {dtype})")
    if isinstance(template, np.ndarray) and dtype == torch.bfloat16:
        raise ValueError(f"NumPy has no bfloat16: pass the {what} as a device tensor for a bfloat16 result")


def _torch_dtype(x):
    return x.dtype if isinstance(x, torch.Tensor) else {np.dtype(np.float32): torch.float32, np.dtype(np.float16): torch.float16}[x.dtype]


# An activation format as plain data: the bits of a code (a_codes is (M, K bits / 8)), its C constant, the C entries of its
# plain quantizer and its de-quantizer, and how the fused rotate-and-quantize entry is called: its name and whether it takes
# the constant as its `fmt` argument.  (The product's entry depends on the layer's format too: _GEMM below.)
_Format = collections.namedtuple("_Format", "name bits c_fmt quantize_entry dequantize_entry rotate_entry rotate_takes_fmt")
_FORMATS = {f.name: f for f in (
    _Format("mxfp8", 8, _lib.MX_ACT_FP8, "slk_mx_quantize_act", "slk_mx_dequantize_act", "slk_mx_rotate_quantize_act", True),
    _Format("mxfp4", 4, _lib.MX_ACT_FP4, "slk_mx_quantize_act4", "slk_mx_dequantize", "slk_mx_rotate_quantize_act", True),
    _Format("mxfp6_e2m3", 6, _lib.MX_ACT_FP6, "slk_mx_quantize_act6", "slk_mx_dequantize_act6", "slk_mx_rotate_quantize_act6", False),
)}
# The 16-bit activations of the weight-only mode (module docstring, W4A16 / W6A16) are no coded format: x itself, rounded to
# `dtype` inside the product, which de-quantizes the layer to that type (slk_mx_gemm_a16).  Both weight formats take both.
_Half = collections.namedtuple("_Half", "name dtype")
_HALVES = {h.name: h for h in (_Half("bfloat16", torch.bfloat16), _Half("float16", torch.float16))}
_ACTIVATIONS = tuple(_FORMATS) + tuple(_HALVES)
_ACTIVATIONS_ARE = "activations must be " + ", ".join(f'"{name}"' for name in _ACTIVATIONS[:-1]) + f' or "{_ACTIVATIONS[-1]}"'
# What refuses a 16-bit name where only coded activations make sense (each text names the way that does exist)
_CODES_ONLY = ('16-bit activations are not codes: matmul_mx* multiply activations that exist as MX codes; for "bfloat16" or "float16" '
               "call linear_mxfp4, linear_mxfp6 or linear_mx_experts on x itself")
_GATED_CODES_ONLY = ('a gated MLP writes its hidden activations as MX codes: 16-bit activations ("bfloat16", "float16") through the gated '
                     "epilogue are not supported; use \"mxfp8\", \"mxfp4\" or \"mxfp6_e2m3\", or run the layers as MXLinear / MXExperts")
_STATS_CODES_ONLY = ('add_codes takes rows that exist as MX codes ("mxfp8", "mxfp4" or "mxfp6_e2m3"): 16-bit rows go to add / add_tokens '
                     "as they are")


def _activations(activations, coded=None):
    """The _Format of an `activations` value, or the _Half of a 16-bit one.  (The bare "mxfp6" names two element formats and is
    refused.)  coded: the caller takes coded activations only, and this is its text for a 16-bit name."""
    if not isinstance(activations, str) or activations not in _ACTIVATIONS:
        raise ValueError(f"{_ACTIVATIONS_ARE} (got {activations!r})")
    if activations in _HALVES:
        if coded is not None:
            raise ValueError(f'{coded} (got "{activations}")')
        return _HALVES[activations]
    return _FORMATS[activations]


def _act_outputs(Xd, M, K, fmt):
    codes = torch.empty((M, K * fmt.bits // 8), dtype=torch.uint8, device=Xd.device)
    scales = torch.empty((M, K // BLOCK), dtype=torch.uint8, device=Xd.device)
    return codes, scales, torch.empty(1, dtype=torch.int32, device=Xd.device)


def _quantize_act(Xd, M, K, fmt=_FORMATS["mxfp8"]):
    """(a_codes, a_scales, flag) of a contiguous device X (M, K) of float32, bfloat16 or float16 in the _Format fmt; the
    caller reads the flag (_raise_finite) once everything that follows has been launched: reading it waits for the stream."""
    Xd = dev.aligned(Xd)
    codes, scales, flag = _act_outputs(Xd, M, K, fmt)
    _lib.check(getattr(_lib.lib, fmt.quantize_entry)(dev.ptr(Xd), _OUT[Xd.dtype], M, K, dev.ptr(codes), dev.ptr(scales), dev.ptr(flag),
                                                     dev.stream_handle()))
    return codes, scales, flag


# The names and the call tests/test_gpu_mx_act4.py and test_gpu_mx_act6.py hold the fused kernel against (their two steps):
# the plain quantizer of MXFP4 and of MXFP6 under a name of its own, and False / True for MXFP8 / MXFP4 below.
def _quantize_act4(Xd, M, K):
    return _quantize_act(Xd, M, K, _FORMATS["mxfp4"])


def _quantize_act6(Xd, M, K):
    return _quantize_act(Xd, M, K, _FORMATS["mxfp6_e2m3"])


def _rot_signs(rotation, device):
    """The rotation's signs on `device`, aligned: what the rotating entries take beside rotation.block."""
    return dev.aligned(rotation.signs if rotation.signs.device == device else rotation.signs.to(device))


def _rotate_quantize_act(Xd, M, K, rotation, fmt):
    """_quantize_act of (X R) without X R in memory: the transform's float32 value goes into the quantizer."""
    if isinstance(fmt, bool):
        fmt = _FORMATS["mxfp4" if fmt else "mxfp8"]
    Xd = dev.aligned(Xd)
    signs = _rot_signs(rotation, Xd.device)
    codes, scales, flag = _act_outputs(Xd, M, K, fmt)
    which = (fmt.c_fmt,) if fmt.rotate_takes_fmt else ()
    _lib.check(getattr(_lib.lib, fmt.rotate_entry)(dev.ptr(Xd), _OUT[Xd.dtype], M, K, rotation.block, dev.ptr(signs), *which, dev.ptr(codes),
                                                   dev.ptr(scales), dev.ptr(flag), dev.stream_handle()))
    return codes, scales, flag


# The quantizers' message, of x and of the hidden activations h of a gated MLP alike: h is the down layer's X.
_H_FINITE = "activations must be finite: X holds a NaN or an infinity"


def _raise_finite(flag):
    _raise_flag(flag, _H_FINITE)


def _quantize_x(Xd, M, K, rotation, fmt):
    """_quantize_act of a contiguous device X (M, K), behind `rotation` where there is one (inside the quantizer)."""
    return _rotate_quantize_act(Xd, M, K, rotation, fmt) if rotation is not None else _quantize_act(Xd, M, K, fmt)


_MXFP6_TAKES = 'an MXFP6 layer takes "mxfp8" or "mxfp6_e2m3" activations'  # (the one weight format that refuses any)


def _check_pair(fmt, wf):
    if fmt.name not in wf.activations and fmt.name not in _HALVES:
        raise ValueError(f'{_MXFP6_TAKES} (got "{fmt.name}")')


# The dense product of each (activations, weights) pair: its C entry and whether that entry takes the activations' constant
# as its `a_fmt` argument (the MXFP6 layer's one entry serves both of its pairs).
_GEMM = {("mxfp8", "mxfp4"): ("slk_mx_gemm", False), ("mxfp4", "mxfp4"): ("slk_mx_gemm_a4", False),
         ("mxfp6_e2m3", "mxfp4"): ("slk_mx_gemm_a6", False),
         ("mxfp8", "mxfp6_e2m3"): ("slk_mx_gemm_w6", True), ("mxfp6_e2m3", "mxfp6_e2m3"): ("slk_mx_gemm_w6", True)}


def _gemm(ac, asc, wc, wsc, bias, M, N, K, dtype, fmt=_FORMATS["mxfp8"], wf=_FP4):
    out = torch.empty((M, N), dtype=dtype, device=ac.device)
    entry, takes_fmt = _GEMM[fmt.name, wf.name]
    which = (fmt.c_fmt,) if takes_fmt else ()
    _lib.check(getattr(_lib.lib, entry)(dev.ptr(ac), dev.ptr(asc), dev.ptr(wc), dev.ptr(wsc), dev.ptr(bias), M, N, K, *which, _OUT[dtype],
                                        dev.ptr(out), dev.stream_handle()))
    return out


def _rotated_x(Xd, rotation, half):
    """What the weight-only product reads: x, or behind a rotation x R in the compute type (slk_hadamard_rows writing it)."""
    return Xd if rotation is None else rotation.apply(Xd, dtype=half.dtype)


def _gemm_a16(Xd, wc, wsc, bias, M, N, K, dtype, half, wf):
    """out (M, N) of a contiguous device x (M, K) against a packed layer, weight-only: one launch, no flag, nothing to wait for."""
    Xd = dev.aligned(Xd)
    out = torch.empty((M, N), dtype=dtype, device=Xd.device)
    _lib.check(_lib.lib.slk_mx_gemm_a16(dev.ptr(Xd), _OUT[Xd.dtype], dev.ptr(wc), dev.ptr(wsc), wf.c_fmt, dev.ptr(bias), M, N, K,
                                        _OUT[half.dtype], _OUT[dtype], dev.ptr(out), dev.stream_handle()))
    return out


def _columns(width, bits, what):
    """K of `what`, `width` bytes a row of `bits`-bit codes: a whole number of codes, and of blocks (4 bits bytes each)."""
    if 8 * width % bits != 0:
        raise ValueError(f"{what} has {width} columns of bytes, which is no whole number of {bits}-bit codes")
    return BLOCK * _blocks(8 * width // bits)


def _weights(codes, scales, wf=_FP4):
    """(N, K) of a packed layer in the _Weights wf, its shapes and dtypes checked."""
    N, width = _matrix(codes, "codes", (torch.uint8, np.uint8))
    K = _columns(width, wf.bits, "codes")
    _matrix(scales, "scale bytes", (torch.uint8, np.uint8))
    _check_scale_shape(scales, N, K, "scale bytes")
    return N, K


def _expert_weights(codes, scales, wf):
    """(E, N, K) of stacked packed layers, codes (E, N, K bits / 8) and scales (E, N, K / 32), shapes and dtypes checked."""
    for x, what in ((codes, "codes"), (scales, "scale bytes")):
        if not isinstance(x, (np.ndarray, torch.Tensor)) or x.ndim != 3:
            raise ValueError(f"{what} of stacked experts must be a 3-D NumPy array or torch tensor (experts, rows, bytes)")
        if x.dtype not in (torch.uint8, np.uint8):
            raise ValueError(f"{what} must be torch.uint8 (got {x.dtype})")
    E, N, width = (int(v) for v in codes.shape)
    if E < 1 or E > _lib.MX_MAX_EXPERTS or N < 1:
        raise ValueError(f"codes must hold 1 .. {_lib.MX_MAX_EXPERTS} experts of at least one row (got {tuple(codes.shape)})")
    K = _columns(width, wf.bits, "codes")
    if tuple(scales.shape) != (E, N, K // BLOCK):
        raise ValueError(f"scale bytes must be ({E}, {N}, {K // BLOCK}) for {E} ({N}, {K}) layers; got {tuple(scales.shape)}")
    return E, N, K


def _check_bias(bias, shape):
    """A bias of a layer (N,) or of a stack of layers (E, N), or None."""
    if bias is not None and (not isinstance(bias, (np.ndarray, torch.Tensor)) or tuple(bias.shape) != shape):
        raise ValueError(f"bias must be {shape}; got {tuple(getattr(bias, 'shape', ()))}")


def _hidden(rows, what="the up layer"):
    """N of an up layer of `rows` = 2 N rows: gate and up, and whole blocks of 32 hidden columns."""
    if rows % 2 != 0:
        raise ValueError(f"{what} holds gate and up: its row count must be even (got {rows})")
    if rows // 2 < BLOCK or rows // 2 % BLOCK != 0:
        raise ValueError(f"{what} must have 2 N rows with N a positive multiple of {BLOCK} (got {rows} rows)")
    return rows // 2


def _to_device(codes, scales, bias=None):
    """One side of a product on the device: (codes, aligned for 16-byte loads, scale bytes, float32 bias or None)."""
    return dev.aligned(dev.to_device(codes, torch.uint8)), dev.to_device(scales, torch.uint8), None if bias is None else dev.to_device(bias)


class _Layer(collections.namedtuple("_Layer", "codes scales bias wf E rows N K")):
    """A packed layer as its caller gave it, checked (_layer): dense (E None) or a stack of E, `rows` rows of K columns in the
    _Weights wf.  N is the width of what its product writes: rows, or for the up layer of a gated MLP the rows / 2 hidden columns."""

    __slots__ = ()

    def operands(self):
        return _to_device(self.codes, self.scales, self.bias)

    def has(self, role=""):
        """The subject of a width mismatch: "the layer has", "the experts' layers have", with the layer's role in an MLP ("up ")."""
        return f"the {role}layer has" if self.E is None else f"the experts' {role}layers have"


def _layer(codes, scales, bias, wf, stacked=False, gated=False):
    """The _Layer of (codes, scales, bias): shapes and dtypes of a dense layer or of a stack, of N rows or of 2 N (gate and up)."""
    E, rows, K = _expert_weights(codes, scales, wf) if stacked else (None,) + _weights(codes, scales, wf)
    N = rows if not gated else _hidden(rows, "every expert's up layer" if stacked else "the up layer")
    _check_bias(bias, (rows,) if E is None else (E, rows))
    return _Layer(codes, scales, bias, wf, E, rows, N, K)


def _check_rotation(rotation, features, what, owner="the layer has"):
    if rotation is not None:
        from .rotation import Rotation

        if not isinstance(rotation, Rotation):
            raise ValueError(f"{what} must be a Rotation (got {type(rotation).__name__})")
        if rotation.n != features:
            raise ValueError(f"the {what} has {rotation.n} features but {owner} {features}")


def _act_operands(a_codes, a_scales, fmt):
    """(M, K) of activations given as codes in the _Format fmt, shapes and dtypes checked."""
    M, width = _matrix(a_codes, "a_codes", (torch.uint8, np.uint8))
    K = _columns(width, fmt.bits, "a_codes")
    _matrix(a_scales, "activation scale bytes", (torch.uint8, np.uint8))
    _check_scale_shape(a_scales, M, K, "activation scale bytes")
    return M, K


def _check_same_k(K, layer):
    if layer.K != K:
        raise ValueError(f"a_codes has {K} columns but {layer.has()} {layer.K}")


def _float_rows(x, layer, role, dtype):
    """x given as floats, for the K columns of `layer` (`role`: _Layer.has): (Xd (M, K) on the device, x's leading dimensions,
    M, the result's dtype -- x's where `dtype` is None).  A dense layer takes x (..., K), a stack of experts x (M, K)."""
    if layer.E is None:
        if not isinstance(x, (np.ndarray, torch.Tensor)) or x.ndim < 1:
            raise ValueError("x must be a NumPy array or torch tensor of at least one dimension")
        if x.dtype not in _ACT:
            raise ValueError(f"x must be {_ACT[0]}, torch.bfloat16 or torch.float16 (got {x.dtype})")
    else:
        _matrix(x, "x", _ACT)
    x_dtype = _torch_dtype(x)
    if dtype is None:
        dtype = x_dtype
    _out_dtype(dtype, x)
    if x.shape[-1] != layer.K:
        raise ValueError(f"x has {x.shape[-1]} columns but {layer.has(role)} {layer.K}")
    lead = tuple(x.shape[:-1])
    M = math.prod(lead)
    if M < 1 or M >= 1 << 31:
        raise ValueError(f"x must have 1 <= rows < 2^31 (got {tuple(x.shape)})")
    Xd = dev.to_device(x, x_dtype)
    return Xd if layer.E is not None else Xd.reshape(M, layer.K), lead, M, dtype


def _quantize(X, fmt):
    M, K = _matrix(X, "X", _ACT)
    _blocks(K)
    codes, scales, flag = _quantize_act(dev.to_device(X, _torch_dtype(X)), M, K, fmt)
    _raise_finite(flag)
    return dev.like_input(codes, X), dev.like_input(scales, X)


def quantize_mxfp8(X):
    """X (M, K) float32, bfloat16 or float16 -> (a_codes uint8 (M, K), a_scales uint8 (M, K / 32)): MXFP8 E4M3 under
    non-saturating power-of-two block scales (module docstring).  A NaN or an infinity in X: ValueError."""
    return _quantize(X, _FORMATS["mxfp8"])


def quantize_mxfp4_act(X):
    """X (M, K) float32, bfloat16 or float16 -> (a_codes uint8 (M, K / 2), a_scales uint8 (M, K / 32)): MXFP4 activations
    (module docstring, W4A4); dequantize_mxfp4(a_codes, a_scales) is the inverse.  A NaN or an infinity in X: ValueError."""
    return _quantize(X, _FORMATS["mxfp4"])


def quantize_mxfp6_act(X):
    """X (M, K) float32, bfloat16 or float16 -> (a_codes uint8 (M, 3 K / 4), a_scales uint8 (M, K / 32)): MXFP6 E2M3
    activations (module docstring, W4A6); dequantize_mxfp6_act is the inverse.  A NaN or an infinity in X: ValueError."""
    return _quantize(X, _FORMATS["mxfp6_e2m3"])


def _dequantize(codes, scales, dtype, fmt, what):
    """value(code) * 2^(b - 127) of codes in the _Format fmt, (M, K) of `dtype`; `what` names the codes in an error."""
    _out_dtype(dtype, codes, "codes" if what == "codes" else "input")
    M, width = _matrix(codes, what, (torch.uint8, np.uint8))
    K = _columns(width, fmt.bits, "a_codes")
    _matrix(scales, "scale bytes", (torch.uint8, np.uint8))
    _check_scale_shape(scales, M, K, "scale bytes")
    cd, sd = dev.aligned(dev.to_device(codes, torch.uint8)), dev.to_device(scales, torch.uint8)
    out = torch.empty((M, K), dtype=dtype, device=cd.device)
    flag = torch.empty(1, dtype=torch.int32, device=cd.device)
    _lib.check(getattr(_lib.lib, fmt.dequantize_entry)(dev.ptr(cd), dev.ptr(sd), M, K, _OUT[dtype], dev.ptr(out), dev.ptr(flag),
                                                       dev.stream_handle()))
    _raise_flag(flag, "scale byte 255 is E8M0's NaN, not a scale")
    return dev.like_input(out, codes)


def dequantize_mxfp6_act(a_codes, a_scales, dtype=torch.float32):
    """value(code) * 2^(b - 127) of MXFP6 E2M3 activations, (M, K) of `dtype`: exact in float32; bfloat16 or float16: that
    value rounded to nearest even."""
    return _dequantize(a_codes, a_scales, dtype, _FORMATS["mxfp6_e2m3"], "a_codes")


def dequantize_mxfp8(a_codes, a_scales, dtype=torch.float32):
    """value(code) * 2^(b - 127), (M, K) of `dtype` (bfloat16 or float16: the float32 value rounded to nearest even)."""
    return _dequantize(a_codes, a_scales, dtype, _FORMATS["mxfp8"], "a_codes")


def matmul_mx(a_codes, a_scales, codes, scales, bias=None, dtype=torch.float32, activations="mxfp8", weights="mxfp4"):
    """Y (M, N) = deq(a_codes, a_scales) @ deq(codes, scales).T + bias on the block-scaled MFMA: MXFP8 activations (M, K)
    -- or, with activations="mxfp4", MXFP4 activations (M, K / 2), or, with "mxfp6_e2m3", MXFP6 ones (M, 3 K / 4) -- against
    an MXFP4 layer (N, K), float32 sums in a fixed order, the result rounded once to `dtype`.  weights="mxfp6_e2m3": against
    an MXFP6 layer, codes (N, 3 K / 4), with "mxfp8" or "mxfp6_e2m3" activations."""
    fmt, wf = _activations(activations, _CODES_ONLY), _weight_format(weights)
    _check_pair(fmt, wf)
    _out_dtype(dtype, a_codes)
    M, K = _act_operands(a_codes, a_scales, fmt)
    layer = _layer(codes, scales, bias, wf)
    _check_same_k(K, layer)
    out = _gemm(*_to_device(a_codes, a_scales)[:2], *layer.operands(), M, layer.N, K, dtype, fmt, wf)
    return dev.like_input(out, a_codes)


def linear_mxfp4(x, codes, scales, bias=None, dtype=None, activations="mxfp8", rotation=None):
    """torch.nn.functional.linear with a packed MXFP4 weight: x (..., K) float32, bfloat16 or float16 is quantized to MXFP8
    (quantize_mxfp8; activations="mxfp4": to MXFP4, quantize_mxfp4_act, the W4A4 path; "mxfp6_e2m3": to MXFP6,
    quantize_mxfp6_act, the W4A6 path), multiplied with the layer (N, K) as
    in matmul_mx and the float32 bias (N,) added; the result is (..., N) in `dtype`, or in x's dtype when `dtype` is None.
    rotation (a rotation.Rotation over K features): x R is quantized instead of x, the rotation running inside the
    quantizer -- bit for bit linear_mxfp4(rotation.apply(x, dtype=torch.float32), ...) with the same `dtype` result.
    activations="bfloat16" or "float16": weight-only (module docstring) -- nothing is quantized, the layer is de-quantized
    inside a 16-bit MFMA GEMM, one launch; a non-finite x is not refused; rotation= is then the call on
    rotation.apply(x, dtype=that type)."""
    return _linear(x, codes, scales, bias, dtype, activations, rotation, _FP4)


def linear_mxfp6(x, codes, scales, bias=None, dtype=None, activations="mxfp8", rotation=None):
    """linear_mxfp4 with a packed MXFP6 weight, codes (N, 3 K / 4): W6A8 with activations="mxfp8", W6A6 with "mxfp6_e2m3"
    ("mxfp4": ValueError), W6A16 with "bfloat16" or "float16".  The activation quantizers, the fused rotation, the
    weight-only mode and the result's dtype are linear_mxfp4's."""
    return _linear(x, codes, scales, bias, dtype, activations, rotation, _FP6)


def _linear(x, codes, scales, bias, dtype, activations, rotation, wf):
    fmt = _activations(activations)
    _check_pair(fmt, wf)
    layer = _layer(codes, scales, bias, wf)
    _check_rotation(rotation, layer.K, "rotation")
    Xd, lead, M, dtype = _float_rows(x, layer, "", dtype)
    if isinstance(fmt, _Half):
        out = _gemm_a16(_rotated_x(Xd, rotation, fmt), *layer.operands(), M, layer.N, layer.K, dtype, fmt, wf)
    else:
        ac, asc, flag = _quantize_x(Xd, M, layer.K, rotation, fmt)
        out = _gemm(ac, asc, *layer.operands(), M, layer.N, layer.K, dtype, fmt, wf)
        _raise_finite(flag)
    return dev.like_input(out.reshape(lead + (layer.N,)), x)


class _MXModule(torch.nn.Module):
    """What MXLinear and MXExperts share: `activations` and `weights` as the module's extra state."""

    # `activations` and `weights` travel as the module's extra state, each written only when it is not the default: the state
    # dict of a default module has the keys it always had, and a state dict without the key -- every one saved before --
    # means "mxfp8" activations and "mxfp4" weights
    _STATE_KEY = torch.nn.modules.module._EXTRA_STATE_KEY_SUFFIX

    def _save_to_state_dict(self, destination, prefix, keep_vars):
        super()._save_to_state_dict(destination, prefix, keep_vars)
        state = {}
        if self.activations != "mxfp8":
            state["activations"] = self.activations
        if self.weights != "mxfp4":
            state["weights"] = self.weights
        if state:
            destination[prefix + self._STATE_KEY] = state

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        key = prefix + self._STATE_KEY
        activations, weights = "mxfp8", "mxfp4"
        if key in state_dict:
            state = state_dict[key]
            activations = state.get("activations", "mxfp8") if isinstance(state, dict) else None
            weights = state.get("weights", "mxfp4") if isinstance(state, dict) else None
            if not isinstance(activations, str) or activations not in _ACTIVATIONS:
                error_msgs.append(f"{key}: {_ACTIVATIONS_ARE} (got {activations!r})")
                activations = self.activations
            state_dict = {k: v for k, v in state_dict.items() if k != key}  # (the base class knows no such key)
        if weights != self.weights:  # (the buffers have the module's shape: another format is never read into them)
            error_msgs.append(f"{key}: the state is of an {weights!r} layer, this module holds {self.weights!r} weights")
        elif activations not in _WEIGHTS[self.weights].activations and activations not in _HALVES:
            error_msgs.append(f"{key}: {_MXFP6_TAKES} (got {activations!r})")
            activations = self.activations
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)
        self.activations = activations


def _result_format(result):
    """The _Weights of an MXResult, read off its widths: bits a code = 8 * codes width / (32 * scales width), 4 or 6."""
    wide, blocks = int(result.codes.shape[-1]), int(result.scales.shape[-1])
    by_bits = {wf.bits * BLOCK * blocks: wf for wf in _WEIGHTS.values()}
    if result.codes.ndim != 2 or result.scales.ndim != 2 or blocks < 1 or 8 * wide not in by_bits:
        raise ValueError(f"codes of {wide} bytes a row under {blocks} scale bytes are neither 4 nor 6 bits a weight")
    return by_bits[8 * wide]


class MXLinear(_MXModule):
    """A linear layer kept in its packed MX form: buffers `codes` (N, K / 2), `scales` (N, K / 32) and `bias` (N,) float32
    or None; forward(x) = linear_mxfp4(x, codes, scales, bias, activations=activations).  `activations` ("mxfp8", the
    default, "mxfp4", "mxfp6_e2m3", or weight-only "bfloat16" / "float16") is plain extra state: a state_dict saved before it existed has none, loads unchanged and means "mxfp8".
    weights="mxfp6_e2m3": an MXFP6 layer, `codes` (N, 3 K / 4), forward through linear_mxfp6; it refuses "mxfp4" activations.
    `weights` is extra state too, written only when it is not "mxfp4"; a state of the other weight format is an error."""

    def __init__(self, in_features, out_features, bias=True, device=None, activations="mxfp8", weights="mxfp4"):
        super().__init__()
        _blocks(int(in_features))
        _check_pair(_activations(activations), _weight_format(weights))
        self.activations, self.weights = activations, weights
        self.in_features, self.out_features = int(in_features), int(out_features)
        width = self.in_features * _WEIGHTS[weights].bits // 8
        self.register_buffer("codes", torch.zeros((self.out_features, width), dtype=torch.uint8, device=device))
        self.register_buffer("scales", torch.full((self.out_features, self.in_features // BLOCK), 127, dtype=torch.uint8, device=device))
        self.register_buffer("bias", torch.zeros(self.out_features, dtype=torch.float32, device=device) if bias else None)

    @classmethod
    def from_result(cls, layer, result, activations="mxfp8"):
        """The module of a torch.nn.Linear and the MXResult that Sleekit(layer).quantize_mxfp4() or quantize_mxfp6() returned
        (taken after the call, so that a corrected bias comes along).  The weight format is read off the result's widths:
        bits a code = 8 * codes width / (32 * scales width), 4 or 6."""
        if not isinstance(layer, torch.nn.Linear):
            raise ValueError(f"MXLinear.from_result takes a torch.nn.Linear (got {type(layer).__name__})")
        wf = _result_format(result)
        N, K = _weights(result.codes, result.scales, wf)
        if (N, K) != (layer.out_features, layer.in_features):
            raise ValueError(f"the result is of a ({N}, {K}) layer, not of this ({layer.out_features}, {layer.in_features}) one")
        self = cls(K, N, layer.bias is not None, layer.weight.device, activations, wf.name)
        self.codes.copy_(torch.as_tensor(result.codes))
        self.scales.copy_(torch.as_tensor(result.scales))
        if layer.bias is not None:
            self.bias.copy_(layer.bias.detach().float())
        return self

    def forward(self, x, rotation=None):
        return _linear(x, self.codes, self.scales, self.bias, None, self.activations, rotation, _WEIGHTS[self.weights])

    def extra_repr(self):
        return (f"in_features={self.in_features}, out_features={self.out_features}, bias={self.bias is not None}, "
                f"activations={self.activations}" + ("" if self.weights == "mxfp4" else f", weights={self.weights}"))


# --------------------------------------------------------------------------------------------------------------- experts
# A mixture-of-experts layer: E packed layers of one shape, every row of x against the layer of its expert, in one call
# (slk_mx_gemm_experts; module docstring, EXPERTS).
_OFFSETS_RULE = ("offsets must start at 0, never decrease and end at the number of rows: "
                 "offsets[0] == 0, offsets[e] <= offsets[e + 1], offsets[E] == M")


_raise_flags = routing._raise_flags  # (device flag or None, message) pairs read in ONE device -> host transfer


def _check_offsets(offsets, E):
    if not isinstance(offsets, (np.ndarray, torch.Tensor)) or offsets.dtype not in (torch.int32, np.int32) or tuple(offsets.shape) != (E + 1,):
        raise ValueError(f"offsets must be int32 ({E + 1},): one more than the {E} experts "
                         f"(got {getattr(offsets, 'dtype', type(offsets).__name__)} {tuple(getattr(offsets, 'shape', ()))})")


def _gemm_experts(ac, asc, wc, wsc, bias, offsets, E, M, N, K, dtype, fmt, wf):
    """(out (M, N), flag) of device operands: the caller reads the flag (_OFFSETS_RULE) once everything is launched."""
    out = torch.empty((M, N), dtype=dtype, device=ac.device)
    flag = torch.empty(1, dtype=torch.int32, device=ac.device)
    ws, ws_bytes = dev.scratch(_lib.lib.slk_mx_experts_workspace_bytes(E, M), "mx_experts")
    _lib.check(_lib.lib.slk_mx_gemm_experts(dev.ptr(ac), dev.ptr(asc), dev.ptr(wc), dev.ptr(wsc), dev.ptr(bias), dev.ptr(offsets), E, M, N, K,
                                            fmt.c_fmt, wf.c_fmt, _OUT[dtype], dev.ptr(out), dev.ptr(flag), dev.ptr(ws), ws_bytes,
                                            dev.stream_handle()))
    return out, flag


def _gemm_experts_a16(Xd, wc, wsc, bias, offsets, E, M, N, K, dtype, half, wf):
    """_gemm_experts for 16-bit activations (slk_mx_gemm_experts_a16): the same workspace, the same flag."""
    Xd = dev.aligned(Xd)
    out = torch.empty((M, N), dtype=dtype, device=Xd.device)
    flag = torch.empty(1, dtype=torch.int32, device=Xd.device)
    ws, ws_bytes = dev.scratch(_lib.lib.slk_mx_experts_workspace_bytes(E, M), "mx_experts")
    _lib.check(_lib.lib.slk_mx_gemm_experts_a16(dev.ptr(Xd), _OUT[Xd.dtype], dev.ptr(wc), dev.ptr(wsc), wf.c_fmt, dev.ptr(bias), dev.ptr(offsets),
                                                E, M, N, K, _OUT[half.dtype], _OUT[dtype], dev.ptr(out), dev.ptr(flag), dev.ptr(ws), ws_bytes,
                                                dev.stream_handle()))
    return out, flag


def _expert_tile_tables(E, M):
    """The two tile tables the last grouped product of (E, M) on this stream left in its workspace, as NumPy arrays (tiles, 3)
    of (expert, first row, row bound): 16-row tiles, then 64-row tiles (tests/test_gpu_mx_experts.py holds them to a model)."""
    ws = dev.scratch(_lib.lib.slk_mx_experts_workspace_bytes(E, M), "mx_experts")[0]
    words = ws[:_lib.lib.slk_mx_experts_workspace_bytes(E, M)].view(torch.int32).cpu().numpy()
    n16, n64, cap16 = int(words[0]), int(words[1]), M // 16 + E
    return words[4:4 + 3 * n16].reshape(n16, 3).copy(), words[4 + 3 * cap16:4 + 3 * cap16 + 3 * n64].reshape(n64, 3).copy()


def matmul_mx_experts(a_codes, a_scales, codes, scales, offsets, bias=None, dtype=torch.float32, activations="mxfp8", weights="mxfp4"):
    """matmul_mx for a stack of E experts in one call: rows offsets[e] .. offsets[e + 1] - 1 of the quantized activations
    (M rows, sorted by expert) are multiplied with expert e's layer, codes (E, N, K bits / 8) and scales (E, N, K / 32), and
    bias (E, N) float32 added: Y (M, N), each expert's rows bit for bit matmul_mx of that slice against that layer.
    offsets is int32 (E + 1,) and stays on the device; it must start at 0, never decrease and end at M (an expert may have
    no rows).  The rule is checked on the device: where it does not hold nothing is computed and a ValueError is raised --
    after the launches, by one read of the call's flag (which waits for the stream)."""
    fmt, wf = _activations(activations, _CODES_ONLY), _weight_format(weights)
    _check_pair(fmt, wf)
    _out_dtype(dtype, a_codes)
    M, K = _act_operands(a_codes, a_scales, fmt)
    layer = _layer(codes, scales, bias, wf, stacked=True)
    _check_same_k(K, layer)
    _check_offsets(offsets, layer.E)
    out, flag = _gemm_experts(*_to_device(a_codes, a_scales)[:2], *layer.operands(), dev.to_device(offsets, torch.int32), layer.E, M, layer.N, K,
                              dtype, fmt, wf)
    _raise_flags((flag, _OFFSETS_RULE))
    return dev.like_input(out, a_codes)


def _gathered(Xd, routed):
    """The routed rows x[order // k] of a device x (T, K) in memory, by one torch index: what the paths without a row-mapped
    quantizer read (a rotation, 16-bit activations).  (order is slk_moe_sort's: a permutation of 0 .. T k - 1, every place of
    which was checked against n before it was written.)"""
    order, k = routed
    return Xd[torch.div(order, k, rounding_mode="floor").long()]


def _quantize_routed(Xd, T, K, routed, rotation, fmt):
    """_quantize_x of the routed rows x[order // k], routed = (order, k): (a_codes, a_scales, finite flag, row-map flag).
    Without a rotation the quantizer reads x through the row map (slk_mx_quantize_act_rows) and the routed rows are never in
    memory; with one they are gathered first and the row-map flag is None."""
    if rotation is None:
        ac, asc, flags = routing._quantize_rows(Xd, T, K, routed[0], routed[1], routed[0].numel(), fmt.c_fmt, fmt.bits)
        return ac, asc, flags[0], flags[1]
    return (*_quantize_x(_gathered(Xd, routed), routed[0].numel(), K, rotation, fmt), None)


def _settle(checks, deferred, out, x):
    """How a grouped call ends: its flags read now and the result handed back the way x came in, or (deferred, a list) its
    checks appended for the caller to read with its own, and the device result."""
    if deferred is not None:
        deferred.extend(checks)
        return out
    _raise_flags(*checks)
    return dev.like_input(out, x)


def _linear_experts(x, codes, scales, offsets, bias, dtype, activations, rotation, wf, also=(), routed=None, deferred=None):
    """routed = (order, k): x is (T, K) and the rows that are multiplied are x[order // k] (forward_logits)."""
    fmt = _activations(activations)
    _check_pair(fmt, wf)
    layer = _layer(codes, scales, bias, wf, stacked=True)
    _check_rotation(rotation, layer.K, "rotation", "the layers have")
    _check_offsets(offsets, layer.E)
    Xd, _, M, dtype = _float_rows(x, layer, "", dtype)
    od = dev.to_device(offsets, torch.int32)
    off = None
    if isinstance(fmt, _Half):
        finite = None
        if routed is not None:
            Xd, M = _gathered(Xd, routed), routed[0].numel()
        out, flag = _gemm_experts_a16(_rotated_x(Xd, rotation, fmt), *layer.operands(), od, layer.E, M, layer.N, layer.K, dtype, fmt, wf)
    else:
        if routed is None:
            ac, asc, finite = _quantize_x(Xd, M, layer.K, rotation, fmt)
        else:
            (ac, asc, finite, off), M = _quantize_routed(Xd, M, layer.K, routed, rotation, fmt), routed[0].numel()
        out, flag = _gemm_experts(ac, asc, *layer.operands(), od, layer.E, M, layer.N, layer.K, dtype, fmt, wf)
    return _settle((*also, (off, routing.ROWS_MESSAGE), (finite, _H_FINITE), (flag, _OFFSETS_RULE)), deferred, out, x)


def linear_mx_experts(x, codes, scales, offsets, bias=None, dtype=None, activations="mxfp8", weights="mxfp4", rotation=None):
    """linear_mxfp4 / linear_mxfp6 for a stack of experts: x (M, K) float32, bfloat16 or float16, its rows sorted by expert
    as `offsets` says (matmul_mx_experts), is quantized by ONE launch of the activation quantizer over all rows (with
    `rotation`, of the fused rotate-and-quantize kernel), then multiplied by one grouped product; (M, N) in `dtype`, or in
    x's dtype when `dtype` is None.  The two flags -- finite activations, the offsets rule -- are read together after the
    launches: one wait for the stream a call.  With rotation= the result is the call on rotation.apply(x,
    dtype=torch.float32) bit for bit.  activations="bfloat16" or "float16": weight-only as in linear_mxfp4 -- no quantizer, the
    offsets flag alone is read, and rotation= is the call on rotation.apply(x, dtype=that type)."""
    return _linear_experts(x, codes, scales, offsets, bias, dtype, activations, rotation, _weight_format(weights))


def _sorted_by_expert(ids, E):
    """(order, offsets, bad) of a flat device tensor of expert ids: all three stay on the device.  Ids outside 0 .. E - 1 are
    clamped for the sort, so the offsets always follow the rule, and `bad` (one int32) says whether there were any."""
    bad = ((ids < 0) | (ids >= E)).any().to(torch.int32)
    key, order = torch.sort(ids.clamp(0, E - 1), stable=True)
    offsets = torch.searchsorted(key, torch.arange(E + 1, device=ids.device, dtype=key.dtype), out_int32=True)
    return order, offsets, bad


def _expert_ids(expert_ids, E):
    if not isinstance(expert_ids, (np.ndarray, torch.Tensor)) or expert_ids.dtype not in (torch.int32, torch.int64, np.int32, np.int64):
        raise ValueError(f"expert_ids must be an int32 or int64 NumPy array or torch tensor (got {getattr(expert_ids, 'dtype', type(expert_ids).__name__)})")
    if isinstance(E, bool) or not isinstance(E, int) or E < 1 or E > _lib.MX_MAX_EXPERTS:
        raise ValueError(f"E must be an int in 1 .. {_lib.MX_MAX_EXPERTS} (got {E!r})")
    if expert_ids.size == 0 if isinstance(expert_ids, np.ndarray) else expert_ids.numel() == 0:
        raise ValueError("expert_ids is empty")
    return dev.to_device(expert_ids, torch.int64).reshape(-1)


_ids_message = routing.ids_message


def sort_by_expert(expert_ids, E):
    """(order, offsets) of expert ids of any shape, flattened: `order` (int64) is the stable sort of the ids -- rows
    x[order] are sorted by expert, equal ids in their original order -- and `offsets` the int32 (E + 1,) table
    matmul_mx_experts takes.  Built from torch ops on the device; the offsets are never read by the host.  An id outside
    0 .. E - 1 is a ValueError: that check is one reduction whose single int is read before returning, which is this
    function's only synchronisation (MXExperts.forward_tokens reads it together with its product's flags instead)."""
    ids = _expert_ids(expert_ids, E)
    order, offsets, bad = _sorted_by_expert(ids, E)
    _raise_flags((bad, _ids_message(E)))
    return dev.like_input(order, expert_ids), dev.like_input(offsets, expert_ids)


def _route_tokens(x, expert_ids, gates, num_experts, out_features, run):
    """What MXExperts.forward_tokens and MXExpertsMLP.forward_tokens share: the T k rows x[order // k] sorted by expert,
    run(rows, offsets, also) -- a grouped layer or MLP on sorted rows, which reads `also` (the id check) together with its own
    flags -- the gather back into (T, k) order, and the gate-weighted float32 sum in the order j = 0, 1, ..., k - 1."""
    T, _ = _matrix(x, "x", _ACT)
    if not isinstance(expert_ids, (np.ndarray, torch.Tensor)) or expert_ids.ndim != 2 or expert_ids.shape[0] != T or expert_ids.shape[1] < 1:
        raise ValueError(f"expert_ids must be ({T}, k) for x of {T} rows; got {tuple(getattr(expert_ids, 'shape', ()))}")
    k = int(expert_ids.shape[1])
    if gates is not None and (not isinstance(gates, (np.ndarray, torch.Tensor)) or tuple(gates.shape) != (T, k)):
        raise ValueError(f"gates must be ({T}, {k}); got {tuple(getattr(gates, 'shape', ()))}")
    ids = _expert_ids(expert_ids, num_experts)
    order, offsets, bad = _sorted_by_expert(ids, num_experts)
    Xd = dev.to_device(x, _torch_dtype(x))
    y = run(Xd[order // k], offsets, ((bad, _ids_message(num_experts)),))
    back = torch.empty_like(order)
    back[order] = torch.arange(order.numel(), device=order.device)
    y = y[back].reshape(T, k, out_features).float()
    g = None if gates is None else dev.to_device(gates, torch.float32)
    total = y[:, 0] if g is None else y[:, 0] * g[:, 0:1]
    for j in range(1, k):
        total = total + (y[:, j] if g is None else y[:, j] * g[:, j:j + 1])
    return dev.like_input(total.to(_torch_dtype(x)), x)


def _route_logits(x, logits, k, gating, num_experts, out_features, run):
    """What MXExperts.forward_logits and MXExpertsMLP.forward_logits share, every step a HIP launch (sleekit_amd.routing):
    top-k ids and gates of the logits, the counting sort of the T k ids, run(Xd, (order, k), offsets, checks) -- a grouped
    layer or MLP that reads x (T, K) through the row map, appends its own flags to `checks` and returns the device result
    (T k, N) in x's dtype --, and the combine.  Every flag of the call is read together after the last launch: one wait."""
    T, _ = _matrix(x, "x", _ACT)
    _out_dtype(_torch_dtype(x), x)
    _, E, l_dtype = routing._check_logits(logits, k, gating, T, num_experts)
    k = int(k)
    ids, gates, bad_logits = routing._topk(dev.to_device(logits, l_dtype), T, E, k, gating)
    order, pos, offsets, bad_ids = routing._sort(ids.reshape(-1), T * k, E)
    checks = [(bad_logits, routing.LOGITS_MESSAGE), (bad_ids, _ids_message(E))]
    y = run(dev.to_device(x, _torch_dtype(x)), (order, k), offsets, checks)
    out, bad_pos = routing._combine(y, pos, gates, T, k, out_features, _torch_dtype(x))
    _raise_flags(*checks, (bad_pos, routing.POS_MESSAGE))
    return dev.like_input(out, x)


class MXExperts(_MXModule):
    """The experts of a mixture-of-experts layer kept in their packed MX form: buffers `codes` (E, N, K bits / 8), `scales`
    (E, N, K / 32) and `bias` (E, N) float32 or None; `activations` and `weights` are extra state as in MXLinear.
    forward(x, offsets) = linear_mx_experts(x, codes, scales, offsets, bias, ...) for rows sorted by expert;
    forward_tokens(x, expert_ids, gates) routes, runs and combines."""

    def __init__(self, num_experts, in_features, out_features, bias=True, device=None, activations="mxfp8", weights="mxfp4"):
        super().__init__()
        _blocks(int(in_features))
        _check_pair(_activations(activations), _weight_format(weights))
        if not 1 <= int(num_experts) <= _lib.MX_MAX_EXPERTS:
            raise ValueError(f"num_experts must be 1 .. {_lib.MX_MAX_EXPERTS} (got {num_experts})")
        self.activations, self.weights = activations, weights
        self.num_experts, self.in_features, self.out_features = int(num_experts), int(in_features), int(out_features)
        shape = (self.num_experts, self.out_features)
        self.register_buffer("codes", torch.zeros(shape + (self.in_features * _WEIGHTS[weights].bits // 8,), dtype=torch.uint8, device=device))
        self.register_buffer("scales", torch.full(shape + (self.in_features // BLOCK,), 127, dtype=torch.uint8, device=device))
        self.register_buffer("bias", torch.zeros(shape, dtype=torch.float32, device=device) if bias else None)

    @classmethod
    def from_results(cls, results, biases=None, activations="mxfp8", device=None):
        """The module of a list of MXResults of one shape and format (quantize_experts) and, optionally, `biases` (E, N).
        The weight format is read off the widths, as in MXLinear.from_result."""
        results = list(results)
        if not results:
            raise ValueError("MXExperts.from_results takes at least one MXResult")
        first = results[0]
        wf = _result_format(first)
        N, K = _weights(first.codes, first.scales, wf)
        for e, r in enumerate(results):
            if tuple(r.codes.shape) != tuple(first.codes.shape) or tuple(r.scales.shape) != tuple(first.scales.shape):
                raise ValueError(f"expert {e} is not a ({N}, {K}) layer of the first expert's format")
        _check_bias(biases, (len(results), N))
        if device is None:
            device = first.codes.device if isinstance(first.codes, torch.Tensor) else dev.require_gpu()
        self = cls(len(results), K, N, biases is not None, device, activations, wf.name)
        for e, r in enumerate(results):
            self.codes[e].copy_(torch.as_tensor(r.codes))
            self.scales[e].copy_(torch.as_tensor(r.scales))
        if biases is not None:
            self.bias.copy_(torch.as_tensor(biases).float())
        return self

    def forward(self, x, offsets, rotation=None):
        return _linear_experts(x, self.codes, self.scales, offsets, self.bias, None, self.activations, rotation, _WEIGHTS[self.weights])

    def forward_tokens(self, x, expert_ids, gates=None, rotation=None):
        """x (T, K), expert_ids (T, k) -- token t goes to its k experts -- and gates (T, k), None meaning ones: (T, N) in x's
        dtype, sum_j gates[t][j] * expert expert_ids[t][j] (x[t]).  The T k rows x[order // k] are sorted by expert
        (sort_by_expert's order and offsets, on the device), run through forward, put back in (T, k) order by a gather, and
        added up in float32 in the order j = 0, 1, ..., k - 1 (product, then sum: no atomics, no index_add_), so a repeated
        call gives the same bits.  The id check and the product's two flags are read together: one wait for the stream."""
        def run(rows, offsets, also):
            return _linear_experts(rows, self.codes, self.scales, offsets, self.bias, None, self.activations, rotation, _WEIGHTS[self.weights], also=also)

        return _route_tokens(x, expert_ids, gates, self.num_experts, self.out_features, run)

    def forward_logits(self, x, logits, k, gating="selected", rotation=None):
        """x (T, K) and router logits (T, E) -> (T, N) in x's dtype: the whole route in hand-written kernels -- top-k ids and
        gates (routing.route_topk's: `gating` "selected" or "all"), the counting sort by expert, the activation quantizer
        reading x through the row map order // k (no (T k, K) float matrix is in memory), the grouped product, and the
        gate-weighted float32 sum in the order j = 0, 1, ..., k - 1 (no atomics).  The bits are those of
        forward_tokens(x, r.expert_ids, r.gates) for r = routing.route_topk(logits, k, gating).  Every flag of the call
        -- logits, ids, row map, finite activations, offsets, combine -- is read together after the last launch: one wait for
        the stream.  With rotation=, or with activations="bfloat16" / "float16", there is no row-mapped quantizer: those paths
        gather x[order // k] with one torch index, as forward_tokens does, and only the rest is new; rotation= is the call
        on rotation.apply(x) as in forward_tokens."""
        def run(Xd, routed, offsets, checks):
            return _linear_experts(Xd, self.codes, self.scales, offsets, self.bias, None, self.activations, rotation, _WEIGHTS[self.weights],
                                   routed=routed, deferred=checks)

        return _route_logits(x, logits, k, gating, self.num_experts, self.out_features, run)

    def extra_repr(self):
        return (f"num_experts={self.num_experts}, in_features={self.in_features}, out_features={self.out_features}, "
                f"bias={self.bias is not None}, activations={self.activations}" + ("" if self.weights == "mxfp4" else f", weights={self.weights}"))


def quantize_experts(Ws, Hs, weights="mxfp4", act_order="diag", damp=0.01, scale_mode="mse"):
    """quantize_mxfp4 / quantize_mxfp6 (nb_ls_moves = 0) for the E experts of a layer: Ws (E, R, n) or a list of (R, n),
    Hs one (n, n) Hessian per expert.  Returns a list of E MXResults, each bit for bit the single call's.  The loops go
    through dist.quantize_stream -- same-shaped small layers are factored and looped in launches that cover them all -- and
    the indices of all experts are packed by one call (rows are independent).  The stream has no local search."""
    from . import dist

    wf = _weight_format(weights)
    if scale_mode not in _MODES:
        raise ValueError(f'MX scale modes are "max", "mse" and "diag" (got "{scale_mode}")')
    Ws, Hs = list(Ws), list(Hs)
    if not Ws or len(Ws) != len(Hs):
        raise ValueError(f"quantize_experts takes one Hessian per expert (got {len(Ws)} layers and {len(Hs)} Hessians)")
    R, n = _matrix(Ws[0], "W", (torch.float32, np.float32))
    _blocks(n)
    for W, H in zip(Ws, Hs):
        if _matrix(W, "W", (torch.float32, np.float32)) != (R, n):
            raise ValueError(f"every expert must be ({R}, {n}); got {tuple(W.shape)}")
        if H is None or H.ndim != 2 or tuple(H.shape) != (n, n):
            raise ValueError(f"H must be ({n}, {n})")
    Wd, Hd = [dev.to_device(W) for W in Ws], [dev.to_device(H) for H in Hs]
    S = [compute_mx_scales(W, H, scale_mode, wf.name)[0] for W, H in zip(Wd, Hd)]
    layers = [dict(W=W, H=H, gscale=s, group_size=BLOCK) for W, H, s in zip(Wd, Hd, S)]
    shards = dist.quantize_stream(layers, dist.HipBackend(wf.codebook, act_order, damp, 0, with_error=False))
    E = len(layers)
    codes, scales = _pack(dev.aligned(torch.cat([sh["idx"] for sh in shards])), torch.cat(S), E * R, n, wf)
    codes, scales = codes.reshape(E, R, -1), scales.reshape(E, R, -1)
    return [MXResult(*(dev.like_input(t, Ws[e]) for t in (shards[e]["Q"], shards[e]["idx"], S[e], codes[e], scales[e]))) for e in range(E)]


# ------------------------------------------------------------------------------------------------------------ gated MLP
# down(act(gate(x)) * up(x)): the fused gate/up product writes the down layer's activations directly (slk_mx_gemm_glu).
#
# GATED MLP.  The up layer holds gate and up, 2 N rows; hidden column j takes gate = row j and up = row N + j, or, with
# interleaved=True (gpt-oss), gate = row 2 j and up = row 2 j + 1.  The gate, all float32, each operation rounded once:
#     g' = min(g, limit);  u' = clamp(u, -limit, limit);  h = (u' + shift) * (g' * (1 / (1 + exp(-(alpha * g')))))
# alpha=1, limit=None, shift=0 (the defaults) is SwiGLU, silu(g) * u; alpha=1.702, limit=7, shift=1 is gpt-oss.
#     h_codes, h_scales = matmul_mx_glu(a_codes, a_scales, up_codes, up_scales, up_bias)   # (M, N bits / 8), (M, N / 32)
#     y = gated_mlp_mx(x, up_codes, up_scales, down_codes, down_scales)                     # quantizer, fused product, product
#     mlp = MXGatedMLP.from_results(up_linear, up_result, down_linear, down_result);  y = mlp(x)
# h_codes / h_scales are in the activations' own format, exactly as that format's quantizer writes them, and bit for bit
# those of the three-step route matmul_mx(..., dtype=float32), glu(..., dtype=float32), quantize_mxfp8 / _mxfp4_act / _mxfp6_act.
# With rotation=R (matmul_mx_glu*) or down_rotation=R (the MLP calls), R a Rotation of the N hidden features, they are those of
# R.apply(glu(...), dtype=float32) and that quantizer: inside the product's epilogue for a block of at most 32, by those steps above it.
_Gate = collections.namedtuple("_Gate", "alpha limit shift interleaved")
_GATE_DEFAULT = _Gate(1.0, None, 0.0, False)


def _gate(alpha, limit, shift, interleaved):
    """The checked gate parameters as a _Gate (limit None: no clamp)."""
    for v, what in ((alpha, "alpha"), (shift, "shift")):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not np.isfinite(v):
            raise ValueError(f"{what} must be a finite number (got {v!r})")
    if limit is not None and (isinstance(limit, bool) or not isinstance(limit, (int, float)) or not limit > 0):
        raise ValueError(f"limit must be above 0, or None for no clamp (got {limit!r})")
    if not isinstance(interleaved, (bool, np.bool_)):
        raise ValueError(f"interleaved must be True or False (got {interleaved!r})")
    return _Gate(float(alpha), None if limit is None or limit == float("inf") else float(limit), float(shift), bool(interleaved))


def _gate_args(gate):
    return gate.alpha, float("inf") if gate.limit is None else gate.limit, gate.shift, int(gate.interleaved)


def _glu(Yd, M, N, gate, dtype):
    """H (M, N) of `dtype` from a contiguous device Y (M, 2 N)."""
    Yd = dev.aligned(Yd)
    out = torch.empty((M, N), dtype=dtype, device=Yd.device)
    _lib.check(_lib.lib.slk_mx_glu(dev.ptr(Yd), _OUT[Yd.dtype], M, N, *_gate_args(gate), _OUT[dtype], dev.ptr(out), dev.stream_handle()))
    return out


def glu(y, alpha=1.0, limit=None, shift=0.0, interleaved=False, dtype=None):
    """The gate, elementwise (slk_mx_glu): y (..., 2 N) float32, bfloat16 or float16 -> h (..., N) in `dtype` (None: y's),
    the float32 h rounded once.  Column j of h takes gate = y[..., j] and up = y[..., N + j]; interleaved=True: gate =
    y[..., 2 j] and up = y[..., 2 j + 1].  alpha, limit (None: no clamp) and shift as in the section's header."""
    gate = _gate(alpha, limit, shift, interleaved)
    if not isinstance(y, (np.ndarray, torch.Tensor)) or y.ndim < 1:
        raise ValueError("y must be a NumPy array or torch tensor of at least one dimension")
    if y.dtype not in _ACT:
        raise ValueError(f"y must be {_ACT[0]}, torch.bfloat16 or torch.float16 (got {y.dtype})")
    if dtype is None:
        dtype = _torch_dtype(y)
    _out_dtype(dtype, y)
    if y.shape[-1] < 2 or y.shape[-1] % 2 != 0 or y.shape[-1] >= 1 << 31:
        raise ValueError(f"y holds gate and up: its last dimension must be even and at least 2 (got {y.shape[-1]})")
    N, lead = int(y.shape[-1]) // 2, tuple(y.shape[:-1])
    M = int(np.prod(lead, dtype=np.int64))
    if M < 1 or M >= 1 << 31:
        raise ValueError(f"y must have 1 <= rows < 2^31 (got {tuple(y.shape)})")
    out = _glu(dev.to_device(y, _torch_dtype(y)).reshape(M, 2 * N), M, N, gate, dtype)
    return dev.like_input(out.reshape(lead + (N,)), y)


_GLU_ROT_MAX_BLOCK = BLOCK  # the fused product rotates h inside the MX block it stages: Hadamard blocks of 2 .. 32 hidden columns


def _gemm_glu(ac, asc, wc, wsc, bias, M, N, K, fmt, wf, gate, fused=True, rotation=None):
    """(h_codes, h_scales, flag) of device operands: the fused product -- with a `rotation` of the N hidden features whose
    block is at most 32, its rotating form (slk_mx_gemm_glu_rot) --, or (fused=False, or a rotation of a larger block, which
    spans more than the product stages of a row) the three-step route -- the product to float32, slk_mx_glu to float32, the
    plain or the rotating quantizer.  The caller reads the flag (_H_FINITE) once everything that follows has been launched."""
    if fused and (rotation is None or rotation.block <= _GLU_ROT_MAX_BLOCK):
        codes, scales, _ = _act_outputs(ac, M, N, fmt)
        flag = torch.zeros(1, dtype=torch.int32, device=ac.device)
        args = (dev.ptr(ac), dev.ptr(asc), dev.ptr(wc), dev.ptr(wsc), dev.ptr(bias), M, N, K, fmt.c_fmt, wf.c_fmt, *_gate_args(gate), dev.ptr(codes),
                dev.ptr(scales), dev.ptr(flag))
        if rotation is None:
            _lib.check(_lib.lib.slk_mx_gemm_glu(*args, dev.stream_handle()))
        else:
            signs = _rot_signs(rotation, ac.device)
            _lib.check(_lib.lib.slk_mx_gemm_glu_rot(*args, rotation.block, dev.ptr(signs), dev.stream_handle()))
        return codes, scales, flag
    h = _glu(_gemm(ac, asc, wc, wsc, bias, M, 2 * N, K, torch.float32, fmt, wf), M, N, gate, torch.float32)
    return _quantize_x(h, M, N, rotation, fmt)


def _gemm_glu_experts(ac, asc, wc, wsc, bias, offsets, E, M, N, K, fmt, wf, gate, fused=True, rotation=None):
    """(h_codes, h_scales, offsets flag, finite flag): _gemm_glu over rows sorted by expert.  (Unfused under invalid offsets,
    the product writes nothing and the next two steps run on an unwritten matrix: the offsets flag is the one to read first.)"""
    if fused and (rotation is None or rotation.block <= _GLU_ROT_MAX_BLOCK):
        codes, scales, _ = _act_outputs(ac, M, N, fmt)
        flags = torch.zeros(2, dtype=torch.int32, device=ac.device)
        ws, ws_bytes = dev.scratch(_lib.lib.slk_mx_experts_workspace_bytes(E, M), "mx_experts")
        args = (dev.ptr(ac), dev.ptr(asc), dev.ptr(wc), dev.ptr(wsc), dev.ptr(bias), dev.ptr(offsets), E, M, N, K, fmt.c_fmt, wf.c_fmt,
                *_gate_args(gate), dev.ptr(codes), dev.ptr(scales), dev.ptr(flags), dev.ptr(ws), ws_bytes)
        if rotation is None:
            _lib.check(_lib.lib.slk_mx_gemm_glu_experts(*args, dev.stream_handle()))
        else:
            signs = _rot_signs(rotation, ac.device)
            _lib.check(_lib.lib.slk_mx_gemm_glu_experts_rot(*args, rotation.block, dev.ptr(signs), dev.stream_handle()))
        return codes, scales, flags[0], flags[1]
    y, bad = _gemm_experts(ac, asc, wc, wsc, bias, offsets, E, M, 2 * N, K, torch.float32, fmt, wf)
    h = _glu(y, M, N, gate, torch.float32)
    codes, scales, flag = _quantize_x(h, M, N, rotation, fmt)
    return codes, scales, bad, flag


def _matmul_mx_glu(a_codes, a_scales, codes, scales, bias, activations, weights, alpha, limit, shift, interleaved, fused=True, rotation=None):
    """matmul_mx_glu before its flag is read: (h_codes, h_scales, flag), device tensors."""
    fmt, wf = _activations(activations, _GATED_CODES_ONLY), _weight_format(weights)
    _check_pair(fmt, wf)
    gate = _gate(alpha, limit, shift, interleaved)
    M, K = _act_operands(a_codes, a_scales, fmt)
    up = _layer(codes, scales, bias, wf, gated=True)
    _check_same_k(K, up)
    _check_rotation(rotation, up.N, "rotation", "the up layer gives")
    return _gemm_glu(*_to_device(a_codes, a_scales)[:2], *up.operands(), M, up.N, K, fmt, wf, gate, fused, rotation)


def matmul_mx_glu(a_codes, a_scales, codes, scales, bias=None, activations="mxfp8", weights="mxfp4", alpha=1.0, limit=None, shift=0.0,
                  interleaved=False, rotation=None):
    """(h_codes (M, N bits / 8), h_scales (M, N / 32)): quantized activations (M, K) against an up layer of 2 N rows (codes
    (2 N, K bits / 8), scales (2 N, K / 32), bias (2 N,) float32), the gate applied to the float32 sums, and h quantized to
    the activations' own format -- one launch, and the bits of matmul_mx(dtype=float32), glu(dtype=float32) and that format's
    quantizer.  N must be a multiple of 32.  A NaN or an infinity in h: ValueError, as from the quantizers.
    rotation (a rotation.Rotation over the N hidden features): h R is quantized instead of h, for a down layer quantized
    behind R -- the bits of rotation.apply(glu(...), dtype=float32) and that format's quantizer.  With a block of at most 32
    the product's epilogue rotates h itself (slk_mx_gemm_glu_rot), still one launch; a larger block takes the three steps."""
    hc, hs, flag = _matmul_mx_glu(a_codes, a_scales, codes, scales, bias, activations, weights, alpha, limit, shift, interleaved, rotation=rotation)
    _raise_flags((flag, _H_FINITE))
    return dev.like_input(hc, a_codes), dev.like_input(hs, a_codes)


def _matmul_mx_glu_experts(a_codes, a_scales, codes, scales, offsets, bias, activations, weights, alpha, limit, shift, interleaved, fused=True,
                           rotation=None):
    """matmul_mx_glu_experts before its flags are read: (h_codes, h_scales, offsets flag, finite flag), device tensors."""
    fmt, wf = _activations(activations, _GATED_CODES_ONLY), _weight_format(weights)
    _check_pair(fmt, wf)
    gate = _gate(alpha, limit, shift, interleaved)
    M, K = _act_operands(a_codes, a_scales, fmt)
    up = _layer(codes, scales, bias, wf, stacked=True, gated=True)
    _check_same_k(K, up)
    _check_offsets(offsets, up.E)
    _check_rotation(rotation, up.N, "rotation", "the up layers give")
    return _gemm_glu_experts(*_to_device(a_codes, a_scales)[:2], *up.operands(), dev.to_device(offsets, torch.int32), up.E, M, up.N, K, fmt, wf, gate,
                             fused, rotation)


def matmul_mx_glu_experts(a_codes, a_scales, codes, scales, offsets, bias=None, activations="mxfp8", weights="mxfp4", alpha=1.0, limit=None,
                          shift=0.0, interleaved=False, rotation=None):
    """matmul_mx_glu for a stack of E experts in one call (slk_mx_gemm_glu_experts): rows sorted by expert under `offsets`
    (matmul_mx_experts' rule and its ValueError), codes (E, 2 N, K bits / 8), scales (E, 2 N, K / 32), bias (E, 2 N).  Each
    expert's rows are bit for bit matmul_mx_glu of that slice.  Offsets that break the rule leave nothing computed.
    rotation: as in matmul_mx_glu, one Rotation of the N hidden features shared by all experts (slk_mx_gemm_glu_experts_rot)."""
    hc, hs, bad, flag = _matmul_mx_glu_experts(a_codes, a_scales, codes, scales, offsets, bias, activations, weights, alpha, limit, shift, interleaved,
                                               rotation=rotation)
    _raise_flags((bad, _OFFSETS_RULE), (flag, _H_FINITE))
    return dev.like_input(hc, a_codes), dev.like_input(hs, a_codes)


def _mlp_layers(up, down, wf_up, wf_down, stacked=False):
    """The two _Layers of a gated MLP from (codes, scales, bias) each, the down layer over the up layer's hidden columns."""
    up, down = _layer(*up, wf_up, stacked, gated=True), _layer(*down, wf_down, stacked)
    if stacked and down.E != up.E:
        raise ValueError(f"the up layers are of {up.E} experts but the down layers of {down.E}")
    if down.K != up.N:
        raise ValueError(f"the down layers have {down.K} columns but the up layers give {up.N} hidden columns" if stacked else
                         f"the down layer has {down.K} columns but the up layer gives {up.N} hidden columns")
    return up, down


def _gated_mlp(x, up, down, dtype, activations, gate, rotation, down_rotation, fused, wf_up, wf_down):
    """gated_mlp_mx on up = (codes, scales, bias) and down = the same, each layer in its own weight format."""
    fmt = _activations(activations, _GATED_CODES_ONLY)
    _check_pair(fmt, wf_up)
    _check_pair(fmt, wf_down)
    up, down = _mlp_layers(up, down, wf_up, wf_down)
    _check_rotation(rotation, up.K, "rotation")
    _check_rotation(down_rotation, up.N, "down_rotation")
    Xd, lead, M, dtype = _float_rows(x, up, "up ", dtype)
    ac, asc, finite = _quantize_x(Xd, M, up.K, rotation, fmt)
    hc, hs, h_finite = _gemm_glu(ac, asc, *up.operands(), M, up.N, up.K, fmt, wf_up, gate, fused, down_rotation)
    out = _gemm(hc, hs, *down.operands(), M, down.N, up.N, dtype, fmt, wf_down)
    _raise_flags((finite, _H_FINITE), (h_finite, _H_FINITE))
    return dev.like_input(out.reshape(lead + (down.N,)), x)


def gated_mlp_mx(x, up_codes, up_scales, down_codes, down_scales, up_bias=None, down_bias=None, dtype=None, activations="mxfp8", weights="mxfp4",
                 alpha=1.0, limit=None, shift=0.0, interleaved=False, rotation=None, fused=True, down_rotation=None):
    """down(act(gate(x)) * up(x)) with both layers packed, in three launches: x (..., K) is quantized (with `rotation` inside
    the quantizer, as in linear_mxfp4), the fused product writes the hidden activations h as codes (matmul_mx_glu: up layer
    (2 N, K), up_bias (2 N,)), and matmul_mx runs the down layer (Nd, N) on them, + down_bias (Nd,): (..., Nd) in `dtype`, or
    in x's dtype when it is None.  The flags of x and of h are read together after the launches: one wait for the stream.
    fused=False runs the three-step route between the products instead -- the up product to float32, glu to float32, the plain
    quantizer -- with the same bits.  When the down layer sits behind a rotation (down_rotation, a Rotation over the N hidden
    features) of a block of at most 32, the fused product rotates each MX block of h before it quantizes it
    (matmul_mx_glu(rotation=)): still three launches.  A larger Hadamard block spans more of a row than the product stages, so
    that case takes the three-step route, glu's float32 h feeding the fused rotate-and-quantize kernel -- the same bits."""
    wf = _weight_format(weights)
    gate = _gate(alpha, limit, shift, interleaved)
    return _gated_mlp(x, (up_codes, up_scales, up_bias), (down_codes, down_scales, down_bias), dtype, activations, gate, rotation, down_rotation,
                      fused, wf, wf)


def _gated_mlp_experts(x, up, down, offsets, dtype, activations, gate, rotation, down_rotation, fused, wf_up, wf_down, also=(), routed=None,
                       deferred=None):
    """routed, deferred: as in _linear_experts."""
    fmt = _activations(activations, _GATED_CODES_ONLY)
    _check_pair(fmt, wf_up)
    _check_pair(fmt, wf_down)
    up, down = _mlp_layers(up, down, wf_up, wf_down, stacked=True)
    _check_rotation(rotation, up.K, "rotation")
    _check_rotation(down_rotation, up.N, "down_rotation")
    _check_offsets(offsets, up.E)
    Xd, _, M, dtype = _float_rows(x, up, "up ", dtype)
    od = dev.to_device(offsets, torch.int32)
    off = None
    if routed is None:
        ac, asc, finite = _quantize_x(Xd, M, up.K, rotation, fmt)
    else:
        (ac, asc, finite, off), M = _quantize_routed(Xd, M, up.K, routed, rotation, fmt), routed[0].numel()
    hc, hs, bad, h_finite = _gemm_glu_experts(ac, asc, *up.operands(), od, up.E, M, up.N, up.K, fmt, wf_up, gate, fused, down_rotation)
    out, _ = _gemm_experts(hc, hs, *down.operands(), od, up.E, M, down.N, up.N, dtype, fmt, wf_down)
    return _settle((*also, (off, routing.ROWS_MESSAGE), (finite, _H_FINITE), (bad, _OFFSETS_RULE), (h_finite, _H_FINITE)), deferred, out, x)


class _GatedModule(torch.nn.Module):
    """What MXGatedMLP and MXExpertsMLP share: the sub-modules `up` and `down` and the four gate parameters, which travel as
    the module's extra state -- written only when they are not the defaults (SwiGLU, not interleaved), as in _MXModule."""

    _STATE_KEY = torch.nn.modules.module._EXTRA_STATE_KEY_SUFFIX

    def _init_gate(self, up, down, kind, alpha, limit, shift, interleaved):
        if not isinstance(up, kind) or not isinstance(down, kind):
            raise ValueError(f"up and down must be {kind.__name__} modules (got {type(up).__name__} and {type(down).__name__})")
        self.gate = _gate(alpha, limit, shift, interleaved)
        N = _hidden(up.out_features)
        if down.in_features != N:
            raise ValueError(f"the down layer has {down.in_features} columns but the up layer gives {N} hidden columns")
        _activations(up.activations, _GATED_CODES_ONLY), _activations(down.activations, _GATED_CODES_ONLY)
        if up.activations != down.activations:
            raise ValueError(f"up and down must take the same activations: h is written in x's format (got {up.activations!r} and {down.activations!r})")
        self.up, self.down = up, down
        self.in_features, self.hidden_features, self.out_features = up.in_features, N, down.out_features

    alpha, limit, shift, interleaved = (property(lambda self, i=i: self.gate[i]) for i in range(4))

    @property
    def activations(self):
        return self.up.activations

    def _save_to_state_dict(self, destination, prefix, keep_vars):
        super()._save_to_state_dict(destination, prefix, keep_vars)
        state = {k: v for k, v, d in zip(_Gate._fields, self.gate, _GATE_DEFAULT) if v != d}
        if state:
            destination[prefix + self._STATE_KEY] = state

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        key = prefix + self._STATE_KEY
        gate = _GATE_DEFAULT
        if key in state_dict:
            state = state_dict[key]
            try:
                gate = _gate(**{**_GATE_DEFAULT._asdict(), **state})
            except (TypeError, ValueError) as e:
                error_msgs.append(f"{key}: {e}")
                gate = self.gate
            state_dict = {k: v for k, v in state_dict.items() if k != key}  # (the base class knows no such key)
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)
        self.gate = gate

    def extra_repr(self):
        return (f"in_features={self.in_features}, hidden_features={self.hidden_features}, out_features={self.out_features}, "
                + ", ".join(f"{k}={v}" for k, v in self.gate._asdict().items()))


class MXGatedMLP(_GatedModule):
    """A gated MLP kept in its packed MX form: `up` an MXLinear of 2 N rows (gate and up), `down` an MXLinear over the N
    hidden features, and the gate parameters alpha, limit, shift, interleaved (gated_mlp_mx).  forward(x) = gated_mlp_mx(x,
    up.codes, up.scales, down.codes, down.scales, up.bias, down.bias, ...): three launches.  The two layers may differ in
    their weight format and must take the same activations.  The state dict is the two sub-modules' (`up.codes`, ...,
    `down.bias`) plus the gate parameters as extra state, written only when they are not the defaults."""

    def __init__(self, up, down, alpha=1.0, limit=None, shift=0.0, interleaved=False):
        super().__init__()
        self._init_gate(up, down, MXLinear, alpha, limit, shift, interleaved)

    @classmethod
    def from_results(cls, up_layer, up_result, down_layer, down_result, activations="mxfp8", alpha=1.0, limit=None, shift=0.0, interleaved=False):
        """The module of two torch.nn.Linear layers and their MXResults (MXLinear.from_result of each)."""
        return cls(MXLinear.from_result(up_layer, up_result, activations), MXLinear.from_result(down_layer, down_result, activations),
                   alpha, limit, shift, interleaved)

    def forward(self, x, rotation=None, fused=True, down_rotation=None):
        return _gated_mlp(x, (self.up.codes, self.up.scales, self.up.bias), (self.down.codes, self.down.scales, self.down.bias), None,
                          self.activations, self.gate, rotation, down_rotation, fused, _WEIGHTS[self.up.weights], _WEIGHTS[self.down.weights])


class MXExpertsMLP(_GatedModule):
    """The gated MLPs of a mixture-of-experts layer: `up` an MXExperts of E layers of 2 N rows, `down` an MXExperts of E layers
    over the N hidden features, and the gate parameters.  forward(x, offsets) runs rows sorted by expert -- the quantizer, the
    fused grouped product (slk_mx_gemm_glu_experts), the grouped down product: three launches and the prologues --;
    forward_tokens(x, expert_ids, gates) routes, runs and combines as MXExperts.forward_tokens does.  The id check and every
    device flag of a call are read together: one wait for the stream.  State dict as MXGatedMLP's."""

    def __init__(self, up, down, alpha=1.0, limit=None, shift=0.0, interleaved=False):
        super().__init__()
        self._init_gate(up, down, MXExperts, alpha, limit, shift, interleaved)
        if up.num_experts != down.num_experts:
            raise ValueError(f"the up layers are of {up.num_experts} experts but the down layers of {down.num_experts}")
        self.num_experts = up.num_experts

    @classmethod
    def from_results(cls, up_results, down_results, up_biases=None, down_biases=None, activations="mxfp8", device=None, alpha=1.0, limit=None,
                     shift=0.0, interleaved=False):
        """The module of two lists of E MXResults and, optionally, biases (E, 2 N) and (E, Nd) (MXExperts.from_results of each)."""
        return cls(MXExperts.from_results(up_results, up_biases, activations, device), MXExperts.from_results(down_results, down_biases, activations, device),
                   alpha, limit, shift, interleaved)

    def _run(self, x, offsets, rotation, fused, down_rotation, also=(), routed=None, deferred=None):
        return _gated_mlp_experts(x, (self.up.codes, self.up.scales, self.up.bias), (self.down.codes, self.down.scales, self.down.bias), offsets, None,
                                  self.activations, self.gate, rotation, down_rotation, fused, _WEIGHTS[self.up.weights], _WEIGHTS[self.down.weights],
                                  also, routed, deferred)

    def forward(self, x, offsets, rotation=None, fused=True, down_rotation=None):
        return self._run(x, offsets, rotation, fused, down_rotation)

    def forward_tokens(self, x, expert_ids, gates=None, rotation=None, fused=True, down_rotation=None):
        """x (T, K), expert_ids (T, k) and gates (T, k) or None -> (T, Nd) in x's dtype: sum_j gates[t][j] * MLP of expert
        expert_ids[t][j] (x[t]), the routing, the gather back and the ordered float32 sum of MXExperts.forward_tokens."""
        return _route_tokens(x, expert_ids, gates, self.num_experts, self.out_features,
                             lambda rows, offsets, also: self._run(rows, offsets, rotation, fused, down_rotation, also))

    def forward_logits(self, x, logits, k, gating="selected", rotation=None, fused=True, down_rotation=None):
        """x (T, K) and router logits (T, E) -> (T, Nd) in x's dtype: MXExperts.forward_logits with the gated MLP of every
        expert in place of its layer -- top-k, sort, the quantizer reading x through the row map, the fused grouped product,
        the grouped down product, the combine --, the bits of forward_tokens(x, r.expert_ids, r.gates, ...) for r =
        routing.route_topk(logits, k, gating), one wait for the stream.  `fused` and `down_rotation` as in forward; with
        rotation= there is no row-mapped quantizer and x[order // k] is gathered with one torch index, as forward_tokens does."""
        return _route_logits(x, logits, k, gating, self.num_experts, self.out_features,
                             lambda Xd, routed, offsets, checks: self._run(Xd, offsets, rotation, fused, down_rotation, (), routed, checks))
