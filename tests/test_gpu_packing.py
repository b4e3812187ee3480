"""Bit-packed indices on the MI355X (sleekit_amd.packing) against the NumPy model of tests/packing_model.py and against
the layers the quantizers return: dequantize_packed in float32 is bit for bit the Q of each path it stands for.

Run on the GPU box:  python -m pytest tests/test_gpu_packing.py -m gpu -q
"""

import numpy as np
import pytest
import torch

from packing_model import codebook_values, dequantize_model, pack_model

pytestmark = pytest.mark.gpu

WIDTHS = (1, 31, 33, 100, 4096, 11008, 16512, 28672)


@pytest.fixture(scope="module", autouse=True)
def gpu():
    assert torch.cuda.is_available(), "these tests need the GPU"
    torch.cuda.set_device(0)


def host_words(P):
    return P.cpu().numpy().view(np.uint32)


def make_codebook(name):
    from sleekit_amd.codebook import Codebook, UniformCodebook

    return Codebook.nf4() if name == "nf4" else UniformCodebook(int(name), -1, 1)


def values_of(cb):
    from sleekit_amd.codebook import Codebook

    if isinstance(cb, Codebook):
        return np.asarray(cb.values, np.float32)
    return codebook_values(len(cb))


@pytest.mark.parametrize("bits", range(1, 9))
def test_device_words_equal_the_model(bits):
    from sleekit_amd import packing

    rng = np.random.default_rng(100 + bits)
    for R in (1, 3, 4096):
        for n in WIDTHS:
            idx = rng.integers(0, 256, (R, n)).astype(np.uint8)  # every byte value: the high bits must be masked away
            d = torch.from_numpy(idx).cuda()
            P = packing.pack_indices(d, bits)
            assert P.dtype == torch.int32 and P.is_cuda and tuple(P.shape) == packing.packed_shape(R, n, bits)
            assert np.array_equal(host_words(P), pack_model(idx, bits)), (R, n)
            back = packing.unpack_indices(P, n, bits)
            assert back.dtype == torch.uint8 and back.is_cuda
            assert np.array_equal(back.cpu().numpy(), idx & ((1 << bits) - 1)), (R, n)


@pytest.mark.parametrize("bits", (1, 3, 4, 8))
def test_unpack_of_pack_is_the_identity(bits):
    from sleekit_amd import packing

    g = torch.Generator(device="cuda").manual_seed(bits)
    for R, n in ((7, 5), (96, 4096), (4096, 11008), (33, 28672)):
        idx = torch.randint(0, 1 << bits, (R, n), dtype=torch.uint8, device="cuda", generator=g)
        assert torch.equal(packing.unpack_indices(packing.pack_indices(idx, bits), n, bits), idx), (R, n)


def test_numpy_and_device_forms_agree():
    from sleekit_amd import packing

    rng = np.random.default_rng(7)
    cb = make_codebook("8")
    for n in (33, 100, 256):
        idx = rng.integers(0, 8, (5, n)).astype(np.uint8)
        P = packing.pack_indices(idx, 3)
        assert isinstance(P, np.ndarray) and P.dtype == np.uint32
        Pd = packing.pack_indices(torch.from_numpy(idx).cuda(), 3)
        assert np.array_equal(P, host_words(Pd))
        back = packing.unpack_indices(P, n, 3)
        assert isinstance(back, np.ndarray) and np.array_equal(back, idx)
        assert np.array_equal(packing.unpack_indices(P.view(np.int32), n, 3), idx)
        Q = packing.dequantize_packed(P, n, cb)
        assert isinstance(Q, np.ndarray) and Q.dtype == np.float32
        assert np.array_equal(Q, packing.dequantize_packed(Pd, n, cb).cpu().numpy())
        assert np.array_equal(Q, dequantize_model(P, n, 3, values_of(cb)))
        Qh = packing.dequantize_packed(P, n, cb, dtype=torch.float16)
        assert Qh.dtype == np.float16 and np.array_equal(Qh, Q.astype(np.float16))


def check_all_dtypes(P, n, cb, Q, **kw):
    """dequantize_packed is Q bit for bit in float32, and exactly Q.to(dtype) in bfloat16 and float16."""
    from sleekit_amd import packing

    got = packing.dequantize_packed(P, n, cb, **kw)
    assert got.dtype == torch.float32 and torch.equal(got.view(torch.int32), Q.view(torch.int32))
    for dtype in (torch.bfloat16, torch.float16):
        low = packing.dequantize_packed(P, n, cb, dtype=dtype, **kw)
        assert low.dtype == dtype and torch.equal(low.view(torch.int16), Q.to(dtype).view(torch.int16)), dtype


CODEBOOKS = ("2", "5", "8", "256", "nf4")


def layer(R, n, seed):
    from sleekit_amd import synth

    L = synth.make_layer(R, n, seed)
    return torch.from_numpy(L["W"]).cuda(), torch.from_numpy(L["H"]).cuda(), torch.from_numpy(L["scale"]).cuda()


@pytest.mark.parametrize("name", CODEBOOKS)
def test_dequantize_equals_the_per_row_paths(name):
    from sleekit_amd import engine, packing, scaling

    cb = make_codebook(name)
    bits = packing.index_bits(cb)
    for R, n in ((48, 100), (64, 256)):
        W, H, s = layer(R, n, 4100 + n)
        res = engine.quantize_layer(W, H, cb)  # unscaled: Q holds the codebook's values
        P = packing.pack_indices(res.idx, bits)
        check_all_dtypes(P, n, cb, res.Q)
        assert np.array_equal(packing.dequantize_packed(P, n, cb).cpu().numpy(),
                              dequantize_model(host_words(P), n, bits, values_of(cb)))
        for moves in (0, 10):
            res = engine.quantize_layer(W, H, cb, s, nb_ls_moves=moves)
            P = packing.pack_indices(res.idx, bits)
            check_all_dtypes(P, n, cb, res.Q, scale=s)
            assert torch.equal(res.Q, scaling.quantize_with_scaling(W, s, cb, H, nb_ls_moves=moves))
            assert np.array_equal(res.Q.cpu().numpy(), dequantize_model(host_words(P), n, bits, values_of(cb), scale=s.cpu().numpy()))


@pytest.mark.parametrize("name", CODEBOOKS)
def test_dequantize_equals_the_grouped_paths(name):
    from sleekit_amd import groups, packing

    cb = make_codebook(name)
    bits = packing.index_bits(cb)
    R, n = 64, 256
    W, H, _ = layer(R, n, 4200)
    for g in (1, 32, 128, n):
        S = groups.compute_group_scaling(W, cb, g, H, mode="max" if g == 1 else "mse")
        for moves in ((0,) if g == 1 else (0, 10)):
            Q, idx = groups.quantize_grouped(W, S, cb, H, g, return_indices=True, nb_ls_moves=moves)
            P = packing.pack_indices(idx, bits)
            check_all_dtypes(P, n, cb, Q, group_scales=S, group_size=g)
            assert torch.equal(packing.dequantize_packed(P, n, cb, group_scales=S), groups.dequantize_grouped(idx, S, cb, g))
        if g == 1:
            continue  # (a group of one column is its own midpoint: nothing left to scale)
        O = groups.compute_group_offsets(W, g)
        S = groups.compute_group_scaling(W, cb, g, H, mode="mse", offsets=O)
        Q, idx = groups.quantize_grouped_asym(W, S, O, cb, H, g, return_indices=True)
        P = packing.pack_indices(idx, bits)
        check_all_dtypes(P, n, cb, Q, group_scales=S, offsets=O)
        assert torch.equal(Q, groups.dequantize_grouped(idx, S, cb, g, offsets=O))
        assert np.array_equal(Q.cpu().numpy(), dequantize_model(host_words(P), n, bits, values_of(cb),
                                                                group_scales=S.cpu().numpy(), offsets=O.cpu().numpy()))


def test_indices_past_the_codebook_rebuild_as_its_last_level():
    from sleekit_amd import packing

    cb = make_codebook("5")
    P = torch.tensor([[7 | (5 << 3) | (4 << 6), 0, 0]], dtype=torch.int32, device="cuda")  # indices 7, 5, 4, then zeros
    assert packing.unpack_indices(P, 4, 3).tolist() == [[7, 5, 4, 0]]
    assert packing.dequantize_packed(P, 4, cb).tolist() == [[1.0, 1.0, 1.0, -1.0]]
    S = torch.full((1, 2), 0.5, device="cuda")
    O = torch.full((1, 2), 0.25, device="cuda")
    assert packing.dequantize_packed(P, 4, cb, group_scales=S, offsets=O).tolist() == [[0.75, 0.75, 0.75, -0.25]]


def test_sleekit_layer_rebuilds_from_its_packed_indices():
    import torch.nn as nn

    from sleekit_amd import Sleekit, packing, synth
    from sleekit_amd.codebook import UniformCodebook

    torch.manual_seed(0)
    lay = nn.Linear(512, 96).cuda()
    with torch.no_grad():
        lay.weight.copy_(torch.from_numpy(synth.make_layer(96, 512, 9801)["W"]) + 0.05)
    st = Sleekit(lay)
    for _ in range(3):
        st.add_batch(torch.randn(64, 512, device="cuda"))
    result = st.quantize(3, group_size=128, offsets="mid")
    P = packing.pack_indices(result.idx, 3)
    assert tuple(P.shape) == (96, 3 * 512 // 32)
    Q = packing.dequantize_packed(P, 512, UniformCodebook(8, -1, 1), group_scales=result.S, offsets=result.O,
                                  dtype=lay.weight.dtype)
    assert torch.equal(Q, lay.weight.data)


def test_past_two_to_the_31_indices():
    """A stack of layers as one (R, n) matrix with R n > 2^31: the kernels' element offsets are 64-bit."""
    from sleekit_amd import packing

    R, n, bits = 16400, 131072 + 32, 3  # 2.15e9 indices
    assert R * n > 1 << 31
    g = torch.Generator(device="cuda").manual_seed(31)
    idx = torch.randint(0, 8, (R, n), dtype=torch.uint8, device="cuda", generator=g)
    P = packing.pack_indices(idx, bits)
    tail = [0, 1, R // 2, R - 2, R - 1]
    assert np.array_equal(host_words(P[tail]), pack_model(idx[tail].cpu().numpy(), bits))
    back = packing.unpack_indices(P, n, bits)
    assert torch.equal(back, idx)
    del back
    vals = torch.from_numpy(codebook_values(8)).cuda()
    Q = packing.dequantize_packed(P[R - 4:], n, make_codebook("8"))
    assert torch.equal(Q, vals[idx[R - 4:].long()])
