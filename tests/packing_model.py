"""NumPy model of bit-packed codebook indices (sleekit_amd.packing), written from the format alone.

Each row is cut into chunks of 32 indices (the last padded with zeros); chunk k is words [b k, b k + b) of the row, read
as one little-endian integer of 32 b bits, and index 32 k + i sits in its bits [i b, i b + b).  Only the low b bits of an
index are kept.  The model works bit by bit, so that it shares nothing with the kernels' word arithmetic.
"""

import numpy as np


def pack_model(idx, bits):
    """uint8 (R, n) -> uint32 (R, bits * ceil(n / 32))."""
    idx = np.asarray(idx, dtype=np.uint8)
    R, n = idx.shape
    C = (n + 31) // 32
    padded = np.zeros((R, 32 * C), np.uint8)
    padded[:, :n] = idx
    # bit t of index i of a chunk is bit i b + t of the chunk's 32 b bits, which are its b words lowest bit first
    bitplanes = (padded[:, :, None] >> np.arange(bits, dtype=np.uint8)) & 1   # (R, 32 C, b)
    stream = bitplanes.reshape(R, C * bits * 32)                              # chunk after chunk, bit i b + t in place
    return np.packbits(stream, axis=1, bitorder="little").view("<u4").astype(np.uint32)


def unpack_model(P, n, bits):
    """uint32 (R, bits * ceil(n / 32)) -> uint8 (R, n)."""
    P = np.ascontiguousarray(P)
    P = P.view(np.uint32) if P.dtype == np.int32 else P.astype(np.uint32)
    R = P.shape[0]
    C = (n + 31) // 32
    assert P.shape == (R, bits * C)
    stream = np.unpackbits(P.astype("<u4").view(np.uint8), axis=1, bitorder="little")   # (R, 32 b C) bits, lowest first
    per_index = stream.reshape(R, 32 * C, bits)                                            # index i: bits [i b, i b + b)
    idx = np.zeros((R, 32 * C), np.uint8)
    for t in range(bits):
        idx |= per_index[:, :, t] << np.uint8(t)
    return idx[:, :n]


def codebook_values(levels, lo=-1.0, hi=1.0, table=None):
    """The float32 value of each index: the table, or t * step + zero as the library forms a uniform codebook's values."""
    if table is not None:
        return np.asarray(table, np.float32)[:levels]
    zero = np.float32(lo)
    step = np.float32((hi - lo) / (levels - 1))
    return np.arange(levels, dtype=np.float32) * step + zero


def dequantize_model(P, n, bits, values, scale=None, group_scales=None, offsets=None):
    """float32 (R, n): value(min(k, levels - 1)), then / (1 / s) per row or per group, then + o per group."""
    idx = unpack_model(P, n, bits).astype(np.int64)
    values = np.asarray(values, np.float32)
    v = values[np.minimum(idx, len(values) - 1)]
    one = np.float32(1)
    if scale is not None:
        return v / (one / np.asarray(scale, np.float32)[:, None])
    if group_scales is not None:
        S = np.asarray(group_scales, np.float32)
        g = n // S.shape[1]
        out = v / np.repeat(one / S, g, axis=1)
        if offsets is not None:
            out = out + np.repeat(np.asarray(offsets, np.float32), g, axis=1)
        return out
    return v
