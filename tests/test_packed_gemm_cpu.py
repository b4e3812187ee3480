"""CPU checks of the packed-index linear layer: the entry is named in every layer, its argument errors are raised on the
host before any launch (C and Python), the NumPy model agrees with a plain integer product, and the rule by which a lane
finds its eight indices in a chunk's words agrees with the format's bit-by-bit model."""

import os
import re
import types

import numpy as np
import pytest
import torch

import packed_gemm_model as model
from conftest import ROOT
from packing_model import pack_model, unpack_model


def test_the_entry_is_named_in_every_layer():
    import sleekit_amd
    from sleekit_amd import _lib, packing

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sleekit_amd.h")).read(), flags=re.S)
    assert re.search(r"\bslk_packed_gemm\s*\(", header)
    assert "slk_packed_gemm" in _lib.PROTOTYPES and hasattr(_lib.lib, "slk_packed_gemm")
    assert len(_lib.PROTOTYPES["slk_packed_gemm"][1]) == 20
    assert hasattr(packing, "linear_packed") and issubclass(packing.PackedLinear, torch.nn.Module)
    assert sleekit_amd.PackedLinear is packing.PackedLinear
    assert callable(sleekit_amd.Sleekit.quantize_packed)
    assert _lib.lib.slk_abi_version() == 8


def test_argument_errors_do_not_touch_the_gpu():
    from sleekit_amd import _lib

    lib, p = _lib.lib, 4096  # (an aligned address that is never followed)
    F32, BF16, F16 = _lib.DTYPE_F32, _lib.DTYPE_BF16, _lib.DTYPE_F16

    def call(X=p, xd=BF16, words=p, bits=3, levels=8, lo=-1.0, hi=1.0, table=None, scale=None, gscale=None, goffset=None, g=0, bias=None,
             M=4, N=4, K=64, cd=BF16, od=F32, out=p):
        return lib.slk_packed_gemm(X, xd, words, bits, levels, lo, hi, table, scale, gscale, goffset, g, bias, M, N, K, cd, od, out, None)

    bad = [dict(K=36), dict(K=0), dict(K=4), dict(K=-8), dict(M=0), dict(N=0), dict(M=-1), dict(bits=0), dict(bits=9),
           dict(levels=1), dict(levels=9), dict(bits=8, levels=257), dict(scale=p, gscale=p, g=8), dict(goffset=p),
           dict(gscale=p, g=12), dict(gscale=p, g=4), dict(gscale=p, g=0), dict(gscale=p, g=24), dict(gscale=p, goffset=p, g=48),
           dict(X=None), dict(words=None), dict(out=None), dict(xd=3), dict(od=7), dict(od=-1), dict(cd=F32), dict(cd=5),
           dict(X=p + 8), dict(out=p + 4), dict(words=p + 2), dict(lo=1.0, hi=1.0)]
    for kw in bad:
        assert call(**kw) == _lib.E_ARG, kw
    assert call(K=36) == _lib.E_ARG and b"8" in lib.slk_last_error() and b"dequantize_packed" in lib.slk_last_error()
    assert call(gscale=p, g=12) == _lib.E_ARG and b"8" in lib.slk_last_error() and b"dequantize_packed" in lib.slk_last_error()
    assert call(X=p + 8) == _lib.E_ARG and b"aligned" in lib.slk_last_error()
    assert call(words=p + 2) == _lib.E_ARG and b"aligned" in lib.slk_last_error()
    assert call(xd=3) == _lib.E_ARG and b"dtype" in lib.slk_last_error()
    assert call(cd=F32) == _lib.E_ARG and b"compute_dtype" in lib.slk_last_error()
    assert call(levels=9) == _lib.E_ARG and b"levels" in lib.slk_last_error()
    assert call(scale=p, gscale=p, g=8) == _lib.E_ARG and b"exclusive" in lib.slk_last_error()
    assert call(goffset=p) == _lib.E_ARG and b"goffset" in lib.slk_last_error()
    assert F16 == 2


def test_python_refusals_come_before_the_device():
    """Shape and dtype errors are ValueError and need no GPU."""
    from sleekit_amd import packing
    from sleekit_amd.codebook import Codebook, UniformCodebook

    cb = UniformCodebook(8, -1, 1)
    x = np.zeros((4, 64), np.float32)
    P = np.zeros((8, 6), np.uint32)
    S, O = np.ones((8, 2), np.float32), np.zeros((8, 2), np.float32)
    with pytest.raises(ValueError, match="dequantize_packed"):
        packing.linear_packed(np.zeros((4, 36), np.float32), np.zeros((8, 6), np.uint32), cb)
    with pytest.raises(ValueError, match="dequantize_packed"):  # g = 12
        packing.linear_packed(np.zeros((4, 96), np.float32), np.zeros((8, 9), np.uint32), cb, group_scales=np.ones((8, 8), np.float32))
    with pytest.raises(ValueError):  # g = 40 does not divide 64
        packing.linear_packed(x, P, cb, group_scales=S, group_size=40)
    with pytest.raises(ValueError, match="exclusive"):
        packing.linear_packed(x, P, cb, scale=np.ones(8, np.float32), group_scales=S)
    with pytest.raises(ValueError, match="offsets"):
        packing.linear_packed(x, P, cb, offsets=O)
    with pytest.raises(ValueError, match="bias"):
        packing.linear_packed(x, P, cb, bias=np.zeros(7, np.float32))
    with pytest.raises(ValueError):
        packing.linear_packed(x.astype(np.float64), P, cb)
    with pytest.raises(ValueError, match="dtype"):
        packing.linear_packed(x, P, cb, dtype=torch.float64)
    with pytest.raises(ValueError, match="bfloat16"):
        packing.linear_packed(x, P, cb, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="compute"):
        packing.linear_packed(x, P, cb, compute=torch.float32)
    with pytest.raises(ValueError, match="bits"):
        packing.linear_packed(x, np.zeros((8, 4), np.uint32), cb, bits=2)
    with pytest.raises(ValueError, match="words"):
        packing.linear_packed(x, np.zeros((8, 5), np.uint32), cb)
    with pytest.raises(ValueError, match="scale"):
        packing.linear_packed(x, P, cb, scale=np.ones(7, np.float32))
    with pytest.raises(ValueError):
        packing.linear_packed(x, P, cb, group_scales=S, offsets=O[:, :1])
    with pytest.raises(ValueError):
        packing.linear_packed(x, P.astype(np.float32), cb)
    result = types.SimpleNamespace(idx=np.zeros((8, 64), np.uint8), S=None, O=None)
    with pytest.raises(ValueError, match="Linear"):
        packing.PackedLinear.from_result(torch.nn.Conv1d(64, 8, 1), result, cb)
    with pytest.raises(ValueError, match="layer"):
        packing.PackedLinear.from_result(torch.nn.Linear(32, 8), result, cb)
    with pytest.raises(ValueError, match="dequantize_packed"):
        packing.PackedLinear(36, 8, cb)
    with pytest.raises(ValueError, match="dequantize_packed"):
        packing.PackedLinear(96, 8, cb, group_size=12)
    with pytest.raises(ValueError, match="bits"):
        packing.PackedLinear(64, 8, Codebook(np.arange(16.0)), bits=3)
    mod = packing.PackedLinear(64, 8, cb, group_size=32, offsets=True)  # (built on the host: no device is touched)
    assert sorted(mod.state_dict()) == ["bias", "group_scales", "offsets", "values", "words"]
    assert tuple(mod.words.shape) == (8, 6) and mod.words.dtype == torch.int32 and mod.values.tolist() == [8.0, -1.0, 1.0]
    assert sorted(packing.PackedLinear(64, 8, Codebook([-1.0, 0.0, 2.0]), row_scale=True, bias=False).state_dict()) == ["scale", "values", "words"]


def test_the_model_against_itself():
    """With integer data the model's product is a plain integer matmul."""
    rng = np.random.default_rng(3)
    N, K, bits = 9, 40, 3
    values = np.arange(-4, 4, dtype=np.float32)
    idx = rng.integers(0, 8, (N, K)).astype(np.uint8)
    P = pack_model(idx, bits)
    S = 2.0 ** rng.integers(-1, 2, (N, K // 8)).astype(np.float32)
    O = rng.integers(-2, 3, (N, K // 8)).astype(np.float32)
    x = rng.integers(-4, 5, (5, K)).astype(np.float32)
    bias = (rng.integers(-64, 65, N) / 8.0).astype(np.float32)
    W2 = (2 * (values[idx] * np.repeat(S, 8, axis=1) + np.repeat(O, 8, axis=1))).astype(np.int64)  # twice the weights: integers
    for compute in (torch.bfloat16, torch.float16):
        Y, A = model.linear_model(x, P, K, bits, values, compute, group_scales=S, offsets=O, bias=bias)
        assert np.array_equal(Y, (x.astype(np.int64) @ W2.T) / 2.0 + bias.astype(np.float64)[None, :])
        assert np.array_equal(A, (np.abs(x).astype(np.int64) @ np.abs(W2).T) / 2.0 + np.abs(bias).astype(np.float64)[None, :])
    # the clamp: a stored index above levels - 1 reads the last value
    Wc, W32 = model.weights_model(pack_model(np.full((1, 8), 7, np.uint8), 3), 8, 3, values[:5], torch.bfloat16)
    assert (Wc == 0.0).all() and W32.dtype == np.float32
    # rounding is to the compute type: 1 + 2^-9 is a float16 but rounds to 1 in bfloat16
    x = np.full((1, 8), 1 + 2.0 ** -9, np.float32)
    P1 = pack_model(np.full((1, 8), 5, np.uint8), 3)  # value 1
    assert model.linear_model(x, P1, 8, 3, values, torch.bfloat16)[0][0, 0] == 8.0
    assert model.linear_model(x, P1, 8, 3, values, torch.float16)[0][0, 0] == 8.0 * (1 + 2.0 ** -9)


@pytest.mark.parametrize("bits", range(1, 9))
def test_fragment_bits_rule(bits):
    """The 8 indices of quarter q of a chunk, taken from its words by the kernels' rule, are the format's."""
    rng = np.random.default_rng(bits)
    words = rng.integers(0, 1 << 32, (50, 3 * bits), dtype=np.uint64).astype(np.uint32)  # 50 rows of 3 chunks
    words[0], words[1] = 0xFFFFFFFF, 0
    want = unpack_model(words, 96, bits)
    for r in range(words.shape[0]):
        for c in range(3):
            for q in range(4):
                got = model.fragment_indices(words[r, bits * c:bits * (c + 1)], q, bits)
                assert got == want[r, 32 * c + 8 * q:32 * c + 8 * q + 8].tolist(), (r, c, q)
