"""NumPy model of the weight-only MX linear layer (sleekit_amd.mx.linear_mxfp4 / linear_mxfp6 / linear_mx_experts with
activations="bfloat16" or "float16"), written from its contract alone.

    Y[m][n] = sum_k Xc[m][k] Wc[n][k] + bias[n]

Wc is the layer's de-quantized form -- mx_model.dequantize_model (E2M1) or mx6_model.dequantize_model (E2M3): value(code)
2^(b - 127) in float32 -- rounded to nearest even to the compute type, Xc is x rounded the same way; both roundings are
torch's on the CPU.  The products and sums here are float64: the product of two 8- or 11-bit significands is exact in it,
and the sums are the reference the kernels' float32 sums are held to.  Nothing here follows the kernels.
"""

import numpy as np
import torch

import mx6_model
import mx_model

DEQUANTIZE = {"mxfp4": mx_model.dequantize_model, "mxfp6_e2m3": mx6_model.dequantize_model}
LEVELS = {"mxfp4": 16, "mxfp6_e2m3": 64}  # codes a format has
# the scale bytes under which every non-zero weight is a normal number of the compute type (include/sleekit_amd.h)
NORMAL_BYTES = {torch.bfloat16: (10, 245), torch.float16: (116, 140)}


def round_to(x, compute):
    """x (NumPy float32 / float16, or a torch tensor of any float type) rounded to `compute`, as float64."""
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
    return t.cpu().to(torch.float32).to(compute).to(torch.float64).numpy()


def pack_codes(c, weights):
    """Codes (R, n) of 4 or 6 bits -> the stored bytes: two a byte, the even k low, or the 6-bit little-endian stream."""
    c = np.asarray(c, np.uint8)
    if weights == "mxfp4":
        return (c[:, 0::2] | (c[:, 1::2] << 4)).astype(np.uint8)
    return mx6_model.act6.pack_codes(c)


def weights_model(codes, scales, weights, compute):
    """(Wc float64 (N, K), the float32 de-quantized layer it was rounded from)."""
    W32 = DEQUANTIZE[weights](np.asarray(codes), np.asarray(scales)).astype(np.float32)
    return round_to(W32, compute), W32


def linear_model(x, codes, scales, weights, compute, bias=None):
    """(Y float64 (M, N), sum_k |x w| (+ |bias|) float64 (M, N)) for x (M, K)."""
    Wc, _ = weights_model(codes, scales, weights, compute)
    Xc = round_to(x, compute)
    Y, A = Xc @ Wc.T, np.abs(Xc) @ np.abs(Wc).T
    if bias is not None:
        b = np.asarray(bias, np.float32).astype(np.float64)
        Y, A = Y + b[None, :], A + np.abs(b)[None, :]
    return Y, A


def experts_model(x, codes, scales, offsets, weights, compute, bias=None):
    """linear_model per expert: rows offsets[e] .. offsets[e + 1] - 1 of x against layer e (codes (E, N, .), bias (E, N))."""
    x = x if isinstance(x, np.ndarray) else x.cpu().float().numpy()
    N = codes.shape[1]
    Y, A = np.zeros((x.shape[0], N)), np.zeros((x.shape[0], N))
    for e in range(codes.shape[0]):
        lo, hi = int(offsets[e]), int(offsets[e + 1])
        if hi > lo:
            Y[lo:hi], A[lo:hi] = linear_model(x[lo:hi], codes[e], scales[e], weights, compute, None if bias is None else bias[e])
    return Y, A
