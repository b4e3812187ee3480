"""NumPy model of the packed-index linear layer (sleekit_amd.packing.linear_packed), written from its contract alone.

    Y[m][n] = sum_k Xc[m][k] Wc[n][k] + bias[n]

Wc is packing_model.dequantize_model (value(min(k, levels - 1)) / (1 / s) [+ o] in float32) rounded to nearest even to the
compute type, Xc is x rounded the same way; both roundings are torch's on the CPU.  The products and sums here are float64:
the products of two 8- or 11-bit significands are exact in it, and the sums are the reference the kernels' float32 sums
are held to.  `fragment_indices` is the one piece that follows the kernels: the rule by which a lane finds the eight
indices of its quarter of a chunk.
"""

import numpy as np
import torch

from packing_model import dequantize_model


def round_to(x, compute):
    """x (NumPy float32 / float16, or a torch tensor of any float type) rounded to `compute`, as float64."""
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
    return t.cpu().to(compute).to(torch.float64).numpy()


def weights_model(P, K, bits, values, compute, scale=None, group_scales=None, offsets=None):
    """(Wc float64 (N, K), the float32 de-quantized layer it was rounded from)."""
    W32 = dequantize_model(P, K, bits, values, scale=scale, group_scales=group_scales, offsets=offsets).astype(np.float32)
    return round_to(W32, compute), W32


def linear_model(x, P, K, bits, values, compute, scale=None, group_scales=None, offsets=None, bias=None):
    """(Y float64 (M, N), sum_k |x w| (+ |bias|) float64 (M, N)) for x (M, K)."""
    Wc, _ = weights_model(P, K, bits, values, compute, scale, group_scales, offsets)
    Xc = round_to(x, compute)
    Y, A = Xc @ Wc.T, np.abs(Xc) @ np.abs(Wc).T
    if bias is not None:
        b = np.asarray(bias, np.float32).astype(np.float64)
        Y, A = Y + b[None, :], A + np.abs(b)[None, :]
    return Y, A


def fragment_indices(words, q, bits):
    """The kernels' rule: the 8 indices of quarter q of a chunk from its `bits` words.  They are bits [8 q b, 8 q b + 8 b)
    of the chunk, found in at most three words: word w0 = (8 q b) >> 5 shifted down by sh = (8 q b) & 31, joined by word
    w0 + 1 when sh + 8 b > 32 and by word w0 + 2 when sh + 8 b > 64; index j is bits [j b, j b + b) of that."""
    b = int(bits)
    bit = 8 * q * b
    w0, sh, end = bit >> 5, bit & 31, (bit & 31) + 8 * b
    x = int(words[w0])
    if end > 32:
        x |= int(words[w0 + 1]) << 32
    x >>= sh
    if end > 64:
        x |= (int(words[w0 + 2]) << (64 - sh)) & ((1 << 64) - 1)
    x &= (1 << 64) - 1
    return [(x >> (j * b)) & ((1 << b) - 1) for j in range(8)]
