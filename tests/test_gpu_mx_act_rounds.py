"""The MX activation quantizers and de-quantizers past one round of their grid on the MI355X.

A launch is capped at 4096 workgroups of 256 lanes and strides over the rest, so the smallest shapes whose last lanes take
a second round are 2049 x 4096 for MXFP8 and MXFP4 (four lanes a block: 262 272 blocks, a round holds 262 144) and
4097 x 4096 for MXFP6 (two lanes a block: 524 416 blocks, a round holds 524 288).  Blocks are independent, so there is no
host model at this size: the whole matrix must give, byte for byte, what its first `r` rows and its other rows give in two
calls, each of them a single round of the kind tests/test_gpu_mx_gemm.py, test_gpu_mx_act4.py and test_gpu_mx_act6.py hold
to the NumPy models.  The flag must survive a later round and be raised by one, and the rotation fused into the quantizer
-- which has no round loop but stores a lane's codes through the same code -- must equal the two steps at this size.
"""

import numpy as np
import pytest
import torch

from test_gpu_mx_gemm import random_weights

pytestmark = pytest.mark.gpu

K = 4096
# activations -> (rows, rows of the first part: one full round, quantizer, its inverse)
FORMATS = {
    "mxfp8": (2049, 2048, "quantize_mxfp8", "dequantize_mxfp8"),
    "mxfp4": (2049, 2048, "quantize_mxfp4_act", "dequantize_mxfp4"),
    "mxfp6_e2m3": (4097, 4096, "quantize_mxfp6_act", "dequantize_mxfp6_act"),
}
DTYPES = [torch.bfloat16, torch.float32]


@pytest.fixture(scope="module")
def activations():
    """(rows, K) of `dtype`, made once: Gaussian data whose blocks of 32 have magnitudes 2^-3 .. 2^3.  Nobody writes to it."""
    made = {}

    def get(rows, dtype):
        if (rows, dtype) not in made:
            gen = torch.Generator(device="cuda").manual_seed(rows)
            mag = torch.randint(-3, 4, (rows, K // 32), device="cuda", generator=gen).float().exp2()
            x = torch.randn((rows, K), device="cuda", generator=gen) * mag.repeat_interleave(32, dim=1)
            made[rows, dtype] = x.to(dtype)
        return made[rows, dtype]

    return get


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("activations_are", list(FORMATS))
def test_rounds_equal_their_parts(activations, activations_are, dtype):
    from sleekit_amd import mx

    rows, r, quantize, dequantize = FORMATS[activations_are]
    quantize, dequantize = getattr(mx, quantize), getattr(mx, dequantize)
    X = activations(rows, dtype)
    assert X[:r].data_ptr() % 16 == 0 and X[r:].data_ptr() % 16 == 0 and X[r:].is_contiguous()
    codes, E = quantize(X)
    parts = quantize(X[:r]), quantize(X[r:])
    assert tuple(E.shape) == (rows, K // 32) and codes.shape[0] == rows
    assert torch.equal(E, torch.cat([p[1] for p in parts]))
    wrong = (codes != torch.cat([p[0] for p in parts])).nonzero()
    assert wrong.numel() == 0, (len(wrong), wrong[:4].tolist())
    assert codes.any() and int(E.min()) > 74  # (nothing here is a block of zeros)
    for out in (torch.float32, torch.bfloat16):
        whole = dequantize(codes, E, dtype=out)
        stacked = torch.cat([dequantize(c, e, dtype=out) for c, e in parts])
        assert whole.dtype == out and tuple(whole.shape) == (rows, K)
        ints = {2: torch.int16, 4: torch.int32}[whole.element_size()]
        assert torch.equal(whole.view(ints), stacked.view(ints)), out
    # the de-quantizer's own flag across its rounds: scale byte 255 in the first row only, in the last row only
    for row in (0, rows - 1):
        bad = E.clone()
        bad[row, 77] = 255
        with pytest.raises(ValueError, match="255"):
            dequantize(codes, bad)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("activations_are", list(FORMATS))
def test_flag_across_rounds(activations, activations_are, dtype):
    """An infinity in the last row only (the second round raises the flag), a NaN in row 0 only (the flag of the first
    round survives the second)."""
    from sleekit_amd import mx

    rows, _, quantize, _ = FORMATS[activations_are]
    quantize = getattr(mx, quantize)
    for row, col, bad in ((rows - 1, K - 3, float("inf")), (rows - 1, 5, float("-inf")), (0, 37, float("nan"))):
        X = activations(rows, dtype).clone()
        X[row, col] = bad
        with pytest.raises(ValueError, match="finite"):
            quantize(X)
    quantize(activations(rows, dtype))  # ... and the data without them raises nothing


@pytest.mark.parametrize("activations_are", list(FORMATS))
def test_fused_rotation_equals_the_two_steps(activations, activations_are):
    from sleekit_amd import mx, rotation

    M, N = 2049, 16
    rot = rotation.Rotation(K, block=4096, seed=9)
    w_codes, w_scales = (torch.from_numpy(t).cuda() for t in random_weights(np.random.default_rng(3), N, K, 118, 123))
    for dtype in DTYPES:
        x = activations(M, dtype)
        got = mx.linear_mxfp4(x, w_codes, w_scales, dtype=torch.float32, activations=activations_are, rotation=rot)
        want = mx.linear_mxfp4(rot.apply(x, dtype=torch.float32), w_codes, w_scales, dtype=torch.float32, activations=activations_are)
        assert tuple(got.shape) == (M, N) and torch.isfinite(got).all()
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), dtype
