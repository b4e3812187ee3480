"""A layer's pack, unpack and de-quantizer past one round of their grid, and MXFP6's through a round's tail, on the MI355X.

A launch is capped at 4096 workgroups of 256 lanes; a lane takes 4 units a step, a whole grid apart, and strides over the
rest.  The smallest shapes whose last lanes take a second round:
  16385 x 4096  pack_mxfp4, pack_mxfp6, unpack_mxfp4, unpack_mxfp6 (two units a block: 2 097 280 blocks, a round holds 2 097 152)
   4097 x 4096  dequantize_mxfp4 to float32 (eight units a block: 524 416 blocks, a round holds 524 288)
   8193 x 4096  dequantize_mxfp4 to bfloat16 (four units a block: 1 048 704 blocks, a round holds 1 048 576)
Blocks are independent, so there is no host model at this size: the whole matrix must give, byte for byte, what its first
`r` rows and its other rows give in two calls, each of them a single round of the kind tests/test_gpu_mx.py and
tests/test_gpu_mx6.py hold to the NumPy models.  A flag must be raised by the last row alone, which only the second round sees.

Within a round, tests/test_gpu_mx6.py stops at 9 x 288 -- one workgroup, only the first of a lane's four units live -- so the
MXFP6 forms are held to tests/mx6_model.py at the shapes tests/test_gpu_mx.py uses for MXFP4: (33, 96), (257, 1056), where
the last of the four units is partly dead, and (600, 4096).
"""

import numpy as np
import pytest
import torch

import mx6_model as model

pytestmark = pytest.mark.gpu

N = 4096
# weights -> (table entries, pack, unpack, de-quantizer)
WEIGHTS = {
    "mxfp4": (15, "pack_mxfp4", "unpack_mxfp4", "dequantize_mxfp4"),
    "mxfp6_e2m3": (63, "pack_mxfp6", "unpack_mxfp6", "dequantize_mxfp6"),
}


@pytest.fixture(scope="module")
def layers():
    """(idx, S, E) of `rows` x N in a weight format, made once on the device: indices over the whole table, scales
    2^-9 .. 2^9 as float32 and as bytes.  Nobody writes to them."""
    made = {}

    def get(weights, rows):
        if (weights, rows) not in made:
            gen = torch.Generator(device="cuda").manual_seed(rows + WEIGHTS[weights][0])
            idx = torch.randint(0, WEIGHTS[weights][0], (rows, N), device="cuda", generator=gen, dtype=torch.uint8)
            E = torch.randint(118, 137, (rows, N // 32), device="cuda", generator=gen, dtype=torch.uint8)
            made[weights, rows] = idx, (E.float() - 127).exp2(), E
        return made[weights, rows]

    return get


def same_bytes(a, b):
    ints = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[a.element_size()]
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(ints), b.view(ints))


@pytest.mark.parametrize("weights", list(WEIGHTS))
def test_pack_and_unpack_rounds_equal_their_parts(layers, weights):
    from sleekit_amd import mx

    rows, r = 16385, 16384
    entries, pack, unpack, _ = WEIGHTS[weights]
    pack, unpack = getattr(mx, pack), getattr(mx, unpack)
    idx, S, E = layers(weights, rows)
    assert int(idx.min()) == 0 and int(idx.max()) == entries - 1 and idx[r:].data_ptr() % 16 == 0
    codes, scales = pack(idx, S)
    parts = pack(idx[:r], S[:r]), pack(idx[r:], S[r:])
    assert tuple(codes.shape) == (rows, N * (4 if entries == 15 else 6) // 8) and torch.equal(scales, E)
    assert same_bytes(codes, torch.cat([p[0] for p in parts])) and same_bytes(scales, torch.cat([p[1] for p in parts]))
    assert codes[r:].data_ptr() % 16 == 0
    back, back_S = unpack(codes, E)
    halves = unpack(codes[:r], E[:r]), unpack(codes[r:], E[r:])
    assert same_bytes(back, torch.cat([h[0] for h in halves])) and same_bytes(back_S, torch.cat([h[1] for h in halves]))
    assert torch.equal(back, idx) and same_bytes(back_S, S)
    # the flags, raised by the last row alone
    bad_S = S.clone()
    bad_S[rows - 1, 77] = 3.0
    with pytest.raises(ValueError, match="powers of two"):
        pack(idx, bad_S)
    bad_E = E.clone()
    bad_E[rows - 1, 77] = 255
    with pytest.raises(ValueError, match="255"):
        unpack(codes, bad_E)


@pytest.mark.parametrize("dtype,rows,r", [(torch.float32, 4097, 4096), (torch.bfloat16, 8193, 8192)])
def test_dequantize_rounds_equal_their_parts(layers, dtype, rows, r):
    from sleekit_amd import mx

    idx, S, E = layers("mxfp4", rows)
    codes, _ = mx.pack_mxfp4(idx, S)
    assert codes[r:].data_ptr() % 16 == 0
    whole = mx.dequantize_mxfp4(codes, E, dtype=dtype)
    stacked = torch.cat([mx.dequantize_mxfp4(codes[:r], E[:r], dtype=dtype), mx.dequantize_mxfp4(codes[r:], E[r:], dtype=dtype)])
    assert whole.dtype == dtype and tuple(whole.shape) == (rows, N) and same_bytes(whole, stacked)
    assert torch.isfinite(whole).all() and (whole[rows - 1] != 0).any()
    bad_E = E.clone()
    bad_E[rows - 1, 77] = 255
    with pytest.raises(ValueError, match="255"):
        mx.dequantize_mxfp4(codes, bad_E, dtype=dtype)


@pytest.mark.parametrize("R,n", [(33, 96), (257, 1056), (600, 4096)])
def test_mxfp6_follows_the_model_through_a_tail(R, n):
    from sleekit_amd import mx

    rng = np.random.default_rng(7300 + R + n)
    idx = rng.integers(0, 63, (R, n)).astype(np.uint8)
    idx.reshape(-1)[:3] = [0, 62, 31]
    idx.reshape(-1)[-3:] = [62, 31, 0]
    E = rng.integers(71, 254, (R, n // 32)).astype(np.uint8)
    S = model.decode_model(E)
    idx_d, E_d = torch.from_numpy(idx).cuda(), torch.from_numpy(E).cuda()
    want_codes = model.pack_model(idx, S)[0]
    codes, scales = mx.pack_mxfp6(idx_d, torch.from_numpy(S).cuda())
    assert tuple(codes.shape) == (R, 3 * n // 4)
    assert np.array_equal(codes.cpu().numpy(), want_codes) and np.array_equal(scales.cpu().numpy(), E)
    back, back_S = mx.unpack_mxfp6(codes, E_d)
    want_idx, want_S = model.unpack_model(want_codes, E)
    assert np.array_equal(back.cpu().numpy(), want_idx) and np.array_equal(want_idx, idx)
    assert np.array_equal(back_S.cpu().numpy().view(np.uint32), want_S.view(np.uint32))
    want = torch.from_numpy(model.dequantize_model(want_codes, E)).cuda()
    got = mx.dequantize_mxfp6(codes, E_d)
    assert same_bytes(got, want)
    for dtype in (torch.bfloat16, torch.float16):
        assert same_bytes(mx.dequantize_mxfp6(codes, E_d, dtype=dtype), want.to(dtype)), dtype
