"""Bit-packed indices without a GPU: the format's known answers on the NumPy model (tests/packing_model.py), the C entry
points' argument checks and the Python layer's refusals.  The device kernels are held to the model in
tests/test_gpu_packing.py."""

import ctypes

import numpy as np
import pytest

from packing_model import dequantize_model, pack_model, unpack_model


def test_known_answers():
    from sleekit_amd import packing

    i = (np.arange(32) % 8).astype(np.uint8)[None]
    assert pack_model(i, 3).tolist() == [[0x88FAC688, 0xC688FAC6, 0xFAC688FA]]
    assert pack_model(i, 4).tolist() == [[0x76543210] * 4]
    assert pack_model(np.array([[1, 2, 3, 4, 5]], np.uint8), 3).tolist() == [[0x58D1, 0, 0]]
    assert packing.packed_shape(7, 5, 3) == (7, 3) and packing.packed_shape(2, 33, 5) == (2, 10)


@pytest.mark.parametrize("bits", range(1, 9))
def test_model_round_trips(bits):
    from sleekit_amd import packing

    rng = np.random.default_rng(bits)
    for n in (1, 5, 31, 32, 33, 100, 16512):
        idx = rng.integers(0, 1 << bits, (3, n)).astype(np.uint8)
        P = pack_model(idx, bits)
        assert P.dtype == np.uint32 and P.shape == packing.packed_shape(3, n, bits)
        assert np.array_equal(unpack_model(P, n, bits), idx)
        assert np.array_equal(unpack_model(P.view(np.int32), n, bits), idx)


def test_eight_bits_are_the_padded_bytes():
    rng = np.random.default_rng(8)
    for n in (1, 5, 32, 33, 100):
        idx = rng.integers(0, 256, (4, n)).astype(np.uint8)
        padded = np.zeros((4, 32 * ((n + 31) // 32)), np.uint8)
        padded[:, :n] = idx
        assert np.array_equal(pack_model(idx, 8), padded.view("<u4"))


def test_wide_indices_come_back_masked():
    rng = np.random.default_rng(3)
    for bits in range(1, 8):
        idx = rng.integers(0, 256, (2, 70)).astype(np.uint8)
        P = pack_model(idx, bits)
        assert np.array_equal(unpack_model(P, 70, bits), idx & ((1 << bits) - 1))
        assert np.array_equal(P, pack_model(idx & ((1 << bits) - 1), bits))


def test_dequantize_model_clamps_and_descales():
    vals = np.array([-1, -0.5, 0, 0.5, 1], np.float32)
    P = pack_model(np.array([[7, 4, 0, 2]], np.uint8), 3)
    assert dequantize_model(P, 4, 3, vals).tolist() == [[1, 1, -1, 0]]
    S = np.array([[2.0, 0.5]], np.float32)
    O = np.array([[0.25, -1.0]], np.float32)
    assert dequantize_model(P, 4, 3, vals, group_scales=S, offsets=O).tolist() == [[2.25, 2.25, -1.5, -1.0]]


def test_index_bits():
    from sleekit_amd import packing
    from sleekit_amd.codebook import UniformCodebook

    assert [packing.index_bits(UniformCodebook(k, -1, 1)) for k in (2, 3, 4, 5, 8, 9, 16, 17, 256)] == [1, 2, 2, 3, 3, 4, 4, 5, 8]
    with pytest.raises(ValueError):
        packing.index_bits(UniformCodebook(257, -1, 1))


def test_argument_errors_do_not_touch_the_gpu():
    """Bad arguments are rejected on the host before any launch (safe without a GPU)."""
    from sleekit_amd import _lib

    L, A = _lib.lib, 8  # (a non-null address that is never dereferenced: each call below fails its checks first)
    for bits in (0, 9, -1):
        assert L.slk_pack_indices(A, 4, 32, bits, A, None) == _lib.E_ARG
        assert b"bits" in L.slk_last_error()
        assert L.slk_unpack_indices(A, 4, 32, bits, A, None) == _lib.E_ARG
        assert L.slk_dequantize_packed(A, 4, 32, bits, 8, -1.0, 1.0, None, None, None, None, 1, 0, A, None) == _lib.E_ARG
    for R, n in ((0, 32), (4, 0), (-1, 32)):
        assert L.slk_pack_indices(A, R, n, 3, A, None) == _lib.E_ARG
        assert L.slk_unpack_indices(A, R, n, 3, A, None) == _lib.E_ARG
        assert L.slk_dequantize_packed(A, R, n, 3, 8, -1.0, 1.0, None, None, None, None, 1, 0, A, None) == _lib.E_ARG
    assert L.slk_pack_indices(None, 4, 32, 3, A, None) == _lib.E_ARG
    assert L.slk_pack_indices(A, 4, 32, 3, None, None) == _lib.E_ARG
    assert L.slk_unpack_indices(None, 4, 32, 3, A, None) == _lib.E_ARG
    assert L.slk_unpack_indices(A, 4, 32, 3, None, None) == _lib.E_ARG
    dq = L.slk_dequantize_packed
    assert dq(None, 4, 32, 3, 8, -1.0, 1.0, None, None, None, None, 1, 0, A, None) == _lib.E_ARG
    assert dq(A, 4, 32, 3, 8, -1.0, 1.0, None, None, None, None, 1, 0, None, None) == _lib.E_ARG
    for levels in (1, 257):
        assert dq(A, 4, 32, 3, levels, -1.0, 1.0, None, None, None, None, 1, 0, A, None) == _lib.E_ARG
        assert b"levels" in L.slk_last_error()
    assert dq(A, 4, 32, 3, 8, 1.0, 1.0, None, None, None, None, 1, 0, A, None) == _lib.E_ARG  # lo == hi, no table
    assert dq(A, 4, 32, 3, 8, -1.0, 1.0, None, None, A, None, 5, 0, A, None) == _lib.E_ARG  # 5 does not divide 32
    assert b"group_size" in L.slk_last_error()
    assert dq(A, 4, 32, 3, 8, -1.0, 1.0, None, None, A, None, 0, 0, A, None) == _lib.E_ARG
    assert dq(A, 4, 32, 3, 8, -1.0, 1.0, None, A, A, None, 8, 0, A, None) == _lib.E_ARG  # scale and gscale
    assert dq(A, 4, 32, 3, 8, -1.0, 1.0, None, None, None, A, 8, 0, A, None) == _lib.E_ARG  # goffset without gscale
    assert dq(A, 4, 32, 3, 8, -1.0, 1.0, None, None, None, None, 1, 3, A, None) == _lib.E_ARG  # no such out_dtype
    assert b"out_dtype" in L.slk_last_error()
    assert L.slk_dequantize_packed.argtypes[-2] is ctypes.c_void_p


def test_python_shape_errors():
    import torch

    from sleekit_amd import packing
    from sleekit_amd.codebook import UniformCodebook

    cb = UniformCodebook(8, -1, 1)
    idx = np.zeros((4, 40), np.uint8)
    P = np.zeros((4, 6), np.uint32)
    for call in (
        lambda: packing.pack_indices(idx, 0),
        lambda: packing.pack_indices(idx, 9),
        lambda: packing.pack_indices(idx.astype(np.int32), 3),
        lambda: packing.pack_indices(idx[0], 3),
        lambda: packing.pack_indices(np.zeros((0, 4), np.uint8), 3),
        lambda: packing.unpack_indices(P, 40, 2),                          # 2 bits: (4, 4) words, not (4, 6)
        lambda: packing.unpack_indices(P.astype(np.int64), 40, 3),
        lambda: packing.dequantize_packed(P, 40, cb, bits=2),               # 2 bits cannot index 8 levels
        lambda: packing.dequantize_packed(P, 40, cb, dtype=torch.bfloat16),  # NumPy has no bfloat16
        lambda: packing.dequantize_packed(P, 40, cb, dtype=torch.float64),
        lambda: packing.dequantize_packed(P, 40, cb, scale=np.ones(4, np.float32), group_scales=np.ones((4, 5), np.float32)),
        lambda: packing.dequantize_packed(P, 40, cb, offsets=np.ones((4, 5), np.float32)),
        lambda: packing.dequantize_packed(P, 40, cb, group_scales=np.ones((4, 3), np.float32)),  # 3 groups do not split 40
        lambda: packing.dequantize_packed(P, 40, cb, group_scales=np.ones((4, 5), np.float32), group_size=7),
    ):
        with pytest.raises(ValueError):
            call()


def test_numpy_calls_have_no_cpu_path(monkeypatch):
    """With no GPU visible, NumPy input raises rather than falling back to a CPU computation."""
    import torch

    from sleekit_amd import _device, packing
    from sleekit_amd.codebook import UniformCodebook

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setattr(_device, "_gpu_seen", False)
    cb = UniformCodebook(8, -1, 1)
    idx = np.zeros((4, 40), np.uint8)
    P = np.zeros((4, 6), np.uint32)
    for call in (
        lambda: packing.pack_indices(idx, 3),
        lambda: packing.unpack_indices(P, 40, 3),
        lambda: packing.dequantize_packed(P, 40, cb),
        lambda: packing.dequantize_packed(P, 40, cb, group_scales=np.ones((4, 5), np.float32), offsets=np.zeros((4, 5), np.float32)),
    ):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
