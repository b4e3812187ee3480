"""MXFP6 (E2M3) activations on the MI355X: the E2M3 A operand map of the block-scaled MFMA with one-hot data, exact integer
products bit for bit, random data within the derived bound, the quantizer and the de-quantizer against the NumPy model bit
for bit, the rotation fused into the quantizer against the two steps bit for bit in every regime of the butterfly, and the
Python surface.

Shapes, `bound` and the helpers are those of tests/test_gpu_mx_gemm.py (its docstring has the tile sizes they come from):
|y - y64| <= adds * 2^-23 * sum_k |a_k w_k|, the products being exact (4 + 2 significant bits).  Largest |err| / sum |a w|
seen on the MI355X: DESIGN.md section 20.
"""

import collections

import numpy as np
import pytest
import torch

import mx_act6_model as model
import mx_model
from test_gpu_mx_act4 import K_IN, N_OUT, REGIMES
from test_gpu_mx_gemm import EXACT_SHAPES, bits, block_gaussian, bound, one_hot_positions, pack_nibbles, random_weights

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
A6 = "mxfp6_e2m3"


def a_value(code, scale_byte):
    return float(model.e2m3_decode(code)) * 2.0 ** (int(scale_byte) - 127)


def w_value(code, scale_byte):
    return float(mx_model.MAGNITUDES[code & 7]) * (-1.0 if code & 8 else 1.0) * 2.0 ** (int(scale_byte) - 127)


# ---------------------------------------------------------------------------------------------------------------- 1. map
STRADDLERS = (4, 5, 6, 10, 11, 15, 16, 17, 21, 26)  # the elements of a block whose 6 bits straddle or start a dword


def one_hot_positions6(M, N, K):
    """Those of the other formats' tests, then the straddling elements in the first and in the last block of a row."""
    out = one_hot_positions(M, N, K)
    rows, cols = sorted({0, 5 % M, 15, M - 1}), sorted({0, 9 % N, 15, 16 % N, N - 1})
    extra = [k for k in STRADDLERS] + [K - 32 + k for k in STRADDLERS]
    return out + [(rows[i % len(rows)], cols[(i // 2) % len(cols)], k) for i, k in enumerate(extra)]


@pytest.mark.parametrize("M,N,K", [(16, 16, 128), (17, 33, 160)])
def test_operand_map_one_hot(M, N, K):
    """One non-zero E2M3 code in A and one non-zero E2M1 code in W: y[m][n] = a w s_a s_w exactly when the two k agree, and
    zero everywhere else.  Every (row, block) has its own scale byte on both sides.  The partners: k ^ 1 catches swapped
    neighbours, k ^ 16 the other 12-byte half of the block, k + 32 swapped blocks; the A codes 0x15 and 0x2a differ in every
    bit, so a reversed or shifted bit order inside an element changes the value."""
    from sleekit_amd import mx

    rng = np.random.default_rng(11)
    a_scales = rng.permutation(np.arange(M * (K // 32)) % 23 + 116).reshape(M, K // 32).astype(np.uint8)
    w_scales = rng.permutation(np.arange(N * (K // 32)) % 19 + 118).reshape(N, K // 32).astype(np.uint8)
    for m, n, k in one_hot_positions6(M, N, K):
        if k // 32 + 1 < K // 32:  # the block's right-hand neighbours differ from it on both sides
            a_scales[m, k // 32 + 1] = a_scales[m, k // 32] + 3
            w_scales[n, k // 32 + 1] = w_scales[n, k // 32] - 2
        for a_code, w_code, k2 in ((0x15, 0xd, k), (0x2a, 0x3, k), (0x15, 0x5, (k + 32) % K), (0x2a, 0x7, k ^ 1), (0x3f, 0x7, k ^ 16)):
            a = np.zeros((M, K), np.uint8)
            w_nib = np.zeros((N, K), np.uint8)
            a[m, k] = a_code
            w_nib[n, k2] = w_code
            got = mx.matmul_mx(model.pack_codes(a), a_scales, pack_nibbles(w_nib), w_scales, activations=A6)
            want = np.zeros((M, N), np.float64)
            if k2 == k:
                want[m, n] = a_value(a_code, a_scales[m, k // 32]) * w_value(w_code, w_scales[n, k // 32])
            hot = np.argwhere(got != 0)
            assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64), want), (
                f"A[{m}][{k}] = {a_code:#x}, W[{n}][{k2}] = {w_code:#x}: want y[{m}][{n}] = {want[m, n]!r}, got non-zeros at "
                f"{hot.tolist()[:8]} = {got[got != 0].tolist()[:8]}")


# ---------------------------------------------------------------------------------------------------------------- 2. exact
A_INT_CODES = np.array([c | s for s in (0, 0x20) for c in (0x00, 0x08, 0x10, 0x14, 0x18, 0x1a, 0x1c, 0x1e) if c | s != 0x20], np.uint8)


@pytest.mark.parametrize("M,N,K", EXACT_SHAPES)
def test_exact_integers_bit_for_bit(M, N, K):
    from sleekit_amd import mx

    assert sorted(model.e2m3_decode(A_INT_CODES).tolist()) == list(range(-7, 8))  # 0, +-1 .. +-7
    rng = np.random.default_rng(M * 1000 + N * 7 + K)
    a_codes = model.pack_codes(A_INT_CODES[rng.integers(0, len(A_INT_CODES), (M, K))])
    a_scales = (127 + rng.integers(-1, 2, (M, K // 32))).astype(np.uint8)
    w_codes, w_scales = random_weights(rng, N, K, 126, 128)
    bias = (rng.integers(-64, 65, N) / 8.0).astype(np.float32) if (M + N) % 2 else None
    # the test's own inputs make every order of float32 additions exact: all terms (and the bias) are multiples of
    # q = 2^-3 of magnitude at most 14 * 12 = 168, so every partial sum is a multiple of q below 2^24 q = 2^21
    A, W = model.dequantize_act6_model(a_codes, a_scales), mx_model.dequantize_model(w_codes, w_scales).astype(np.float64)
    assert np.abs(A).max() <= 14 and np.abs(W).max() <= 12 and (A * 2 == np.rint(A * 2)).all() and (W * 4 == np.rint(W * 4)).all()
    assert K * 168 + 8 < 2 ** 21
    want, _ = model.matmul_model(a_codes, a_scales, w_codes, w_scales, bias)
    got = mx.matmul_mx(a_codes, a_scales, w_codes, w_scales, bias, activations=A6)
    assert got.shape == (M, N) and got.dtype == np.float32
    wrong = np.argwhere(got.astype(np.float64) != want)
    assert wrong.size == 0, f"{len(wrong)} of {M * N} differ, first at {wrong[:4].tolist()}: got {got[tuple(wrong[0])]}, want {want[tuple(wrong[0])]}"
    assert np.array_equal(bits(got), bits(want.astype(np.float32)))


# ---------------------------------------------------------------------------------------------------------------- 3. bound
@pytest.mark.parametrize("M,N,K", [(17, 33, 160), (64, 80, 1024), (8, 8, 11008)])
def test_random_data_within_the_bound(M, N, K):
    from sleekit_amd import mx

    rng = np.random.default_rng(K + M)
    a_codes, a_scales = model.quantize_act6_model(block_gaussian(rng, M, K))
    w_codes, w_scales = random_weights(rng, N, K, 118, 123)
    bias = rng.standard_normal(N).astype(np.float32)
    want, sum_abs = model.matmul_model(a_codes, a_scales, w_codes, w_scales)
    got = mx.matmul_mx(a_codes, a_scales, w_codes, w_scales, activations=A6).astype(np.float64)
    err = np.abs(got - want)
    print(f"mx_gemm_a6 {M}x{N}x{K}: max |err| / sum|aw| = {(err / sum_abs).max():.3e} (bound {K * 2.0 ** -23:.3e})")
    assert (err <= bound(K, sum_abs)).all(), (err / sum_abs).max()
    got = mx.matmul_mx(a_codes, a_scales, w_codes, w_scales, bias, activations=A6).astype(np.float64)
    assert (np.abs(got - (want + bias)) <= bound(K + 1, sum_abs + np.abs(bias)[None, :])).all()


# ---------------------------------------------------------------------------------------------------------------- 4. quantizer
def fuzz_activations(rng, M, K):
    X = block_gaussian(rng, M, K)
    blocks = X.reshape(M * (K // 32), 32)  # a view: edits land in X
    for b in range(len(blocks)):
        kind = b % 7
        if kind == 1:
            blocks[b] = 0
        elif kind == 2:
            blocks[b] = -np.abs(blocks[b]) - 1e-3
        elif kind == 3:  # tiny values (they survive in float32 and bfloat16; float16 reads them as zeros)
            blocks[b, rng.integers(0, 32, 6)] = 1e-20
            if b % 2:
                blocks[b] = 1e-20 * rng.integers(-3, 4, 32)
        elif kind == 4:  # amax exactly 7.5 * 2^e, every other element on one of the grid's 31 midpoints (5 bits: exact in 16 bits)
            e = 2.0 ** rng.integers(-3, 4)
            blocks[b] = np.resize(rng.permutation(model.MIDPOINTS), 32) * rng.choice([-1.0, 1.0], 32) * e
            blocks[b, rng.integers(0, 32)] = 7.5 * e * (1 if b % 2 else -1)
        elif kind == 5:
            blocks[b] = np.abs(blocks[b])
    return X


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,K", [(1, 32), (3, 96), (17, 160), (64, 4096)])
def test_activation_quantizer_follows_the_model(M, K, dtype):
    from sleekit_amd import mx

    rng = np.random.default_rng(M + K)
    X = torch.from_numpy(fuzz_activations(rng, M, K)).to(dtype)  # exactly M K elements
    want_codes, want_E = model.quantize_act6_model(X.float().numpy())
    codes, E = mx.quantize_mxfp6_act(X.cuda())
    assert codes.is_cuda and codes.dtype == torch.uint8 and tuple(codes.shape) == (M, 3 * K // 4) and tuple(E.shape) == (M, K // 32)
    assert np.array_equal(E.cpu().numpy(), want_E)
    wrong = np.argwhere(model.unpack_codes(codes.cpu().numpy()) != model.unpack_codes(want_codes))
    assert wrong.size == 0, (len(wrong), wrong[:4].tolist())
    assert np.array_equal(codes.cpu().numpy(), want_codes)
    assert not (model.unpack_codes(want_codes) == 0x20).any()
    # a view that starts off a 16-byte boundary
    buf = torch.zeros(M * K + 3, dtype=dtype, device="cuda")
    view = buf[3:].view(M, K)
    view.copy_(X)
    assert view.data_ptr() % 16 != 0
    c2, E2 = mx.quantize_mxfp6_act(view)
    assert torch.equal(c2, codes) and torch.equal(E2, E)
    # and back: what the product sees of X
    want_back = model.dequantize_act6_model(want_codes, want_E, np.float32)
    back = mx.dequantize_mxfp6_act(codes, E)
    assert back.is_cuda and back.dtype == torch.float32 and tuple(back.shape) == (M, K) and np.array_equal(bits(back), bits(want_back))
    for out in (torch.bfloat16, torch.float16):
        low = mx.dequantize_mxfp6_act(codes, E, dtype=out)
        assert low.dtype == out and np.array_equal(bits(low), bits(back.to(out)))
    if dtype != torch.bfloat16:  # NumPy in, NumPy out
        c3, E3 = mx.quantize_mxfp6_act(X.numpy())
        assert isinstance(c3, np.ndarray) and np.array_equal(c3, want_codes) and np.array_equal(E3, want_E)
        b3 = mx.dequantize_mxfp6_act(c3, E3)
        assert isinstance(b3, np.ndarray) and np.array_equal(bits(b3), bits(want_back))


def test_quantizer_known_answers_and_non_finite_input():
    from sleekit_amd import mx

    x = np.zeros((5, 64), np.float32)
    x[0, :4], x[0, 31] = [7.5, -0.3, 0.0625, 0.1875], 7.5
    x[1, 32:36], x[1, 63] = [1.0, -1.0, 0.3, 0.0625], 1.0
    x[2, :4], x[2, 31] = [1.0625, 3.9, -3.875, 5.25], 7.5
    x[3, 32:34] = [1.75, -1.75]
    x[4, :32] = 1e-20
    codes, E = mx.quantize_mxfp6_act(x)
    assert codes.shape == (5, 48) and E.tolist() == [[127, 74], [74, 125], [127, 74], [74, 125], [74, 74]]
    assert codes[0, :3].tolist() == [0x9f, 0x08, 0x08] and codes[1, 24:27].tolist() == [0x18, 0xae, 0x08]
    assert codes[2, :3].tolist() == [0x08, 0x86, 0x6b]
    c = model.unpack_codes(codes)
    assert c[0, :4].tolist() == [0x1f, 0x22, 0x00, 0x02] and c[0, 31] == 0x1f and c[1, 32:36].tolist() == [0x18, 0x38, 0x0a, 0x02]
    assert c[2, :4].tolist() == [0x08, 0x18, 0x38, 0x1a] and c[3, 32:34].tolist() == [0x1e, 0x3e] and not c[4].any()
    assert not codes[0, 24:].any() and not codes[1, :24].any()
    w_codes, w_scales = np.zeros((4, 32), np.uint8), np.full((4, 2), 127, np.uint8)
    for bad in (np.nan, np.inf, -np.inf):
        y = x.copy()
        y[1, 40] = bad
        with pytest.raises(ValueError, match="finite"):
            mx.quantize_mxfp6_act(y)
        with pytest.raises(ValueError, match="finite"):
            mx.linear_mxfp4(torch.from_numpy(y).cuda().half(), w_codes, w_scales, activations=A6)


# ---------------------------------------------------------------------------------------------------------------- 5. fused
def two_steps(x, rot):
    """(codes, scales, flag): the transform to float32, then the plain quantizer."""
    from sleekit_amd import mx

    y = rot.apply(x, dtype=torch.float32)
    return mx._quantize_act6(y, y.shape[0], y.shape[1])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K,block", REGIMES)
def test_fused_rotation_equals_the_two_steps(K, block, dtype):
    from sleekit_amd import mx, rotation

    rot = rotation.Rotation(K, block=block, seed=K + block)
    fmt = mx._activations(A6)
    for rows in (1, 3, 17):  # 17 rows: a workgroup's 256 chunks straddle rows (K / 16 chunks a row)
        rng = np.random.default_rng(K + block + rows)
        x = torch.from_numpy(block_gaussian(rng, rows, K)).to(dtype).cuda()
        want = two_steps(x, rot)
        got = mx._rotate_quantize_act(x, rows, K, rot, fmt)
        what = (K, block, rows, dtype)
        assert got[0].shape == want[0].shape and got[0].shape == (rows, 3 * K // 4), what
        assert torch.equal(got[1], want[1]), what
        wrong = (got[0] != want[0]).nonzero()
        assert wrong.numel() == 0, (what, len(wrong), wrong[:4].tolist())
        assert int(got[2].item()) == 0 and int(want[2].item()) == 0, what


def test_fused_rotation_flags_what_the_two_steps_flag():
    from sleekit_amd import mx, rotation

    rot = rotation.Rotation(256, block=64, seed=5)
    x = torch.from_numpy(block_gaussian(np.random.default_rng(9), 3, 256)).half().cuda()
    x[1, 70] = float("inf")  # reaches columns 64 .. 127 of row 1 and nothing else
    want, got = two_steps(x, rot), mx._rotate_quantize_act(x, 3, 256, rot, mx._activations(A6))
    assert int(want[2].item()) == 1 and int(got[2].item()) == 1
    clean = torch.ones(3, 192, dtype=torch.bool, device="cuda")
    clean[1, 48:96] = False
    assert torch.equal(got[0][clean], want[0][clean])
    keep = torch.ones(3, 8, dtype=torch.bool, device="cuda")
    keep[1, 2:4] = False
    assert torch.equal(got[1][keep], want[1][keep])
    y = torch.zeros(4, 256 // 2, dtype=torch.uint8, device="cuda"), torch.full((4, 8), 127, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="finite"):
        mx.linear_mxfp4(x, *y, activations=A6, rotation=rot)


# ---------------------------------------------------------------------------------------------------------------- 6. surface
@pytest.fixture(scope="module")
def layer():
    rng = np.random.default_rng(77)
    codes, scales = (torch.from_numpy(t).cuda() for t in random_weights(rng, N_OUT, K_IN, 118, 123))
    return codes, scales, torch.from_numpy(rng.standard_normal(N_OUT).astype(np.float32)).cuda()


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


@pytest.mark.parametrize("dtype", DTYPES)
def test_linear_with_mxfp6_activations(layer, dtype):
    from sleekit_amd import mx

    codes, scales, bias = layer
    x = torch.from_numpy(block_gaussian(np.random.default_rng(3), 6, K_IN)).reshape(2, 3, K_IN).to(dtype).cuda()
    a_codes, a_scales = mx.quantize_mxfp6_act(x.reshape(6, K_IN))
    want_codes, want_scales = model.quantize_act6_model(x.float().cpu().numpy().reshape(6, K_IN))
    assert np.array_equal(a_codes.cpu().numpy(), want_codes) and np.array_equal(a_scales.cpu().numpy(), want_scales)
    for out in DTYPES:
        y = mx.linear_mxfp4(x, codes, scales, bias, dtype=out, activations=A6)
        assert y.is_cuda and y.dtype == out and tuple(y.shape) == (2, 3, N_OUT)
        assert same_bits(y.reshape(6, N_OUT), mx.matmul_mx(a_codes, a_scales, codes, scales, bias, dtype=out, activations=A6))
    y = mx.linear_mxfp4(x, codes, scales, bias, activations=A6)  # the output dtype follows x
    assert same_bits(y, mx.linear_mxfp4(x, codes, scales, bias, dtype=dtype, activations=A6))
    # the product is the model's within the bound, and it is neither the MXFP8 nor the MXFP4 one
    y32 = mx.linear_mxfp4(x, codes, scales, bias, dtype=torch.float32, activations=A6)
    got = y32.cpu().numpy().reshape(6, N_OUT).astype(np.float64)
    want, sum_abs = model.matmul_model(want_codes, want_scales, codes.cpu().numpy(), scales.cpu().numpy(), bias.cpu().numpy())
    assert (np.abs(got - want) <= bound(K_IN + 1, sum_abs + np.abs(bias.cpu().numpy())[None, :])).all()
    assert not torch.equal(mx.linear_mxfp4(x, codes, scales, bias, dtype=torch.float32), y32)
    assert not torch.equal(mx.linear_mxfp4(x, codes, scales, bias, dtype=torch.float32, activations="mxfp4"), y32)
    assert tuple(mx.linear_mxfp4(x[0, 0], codes, scales, activations=A6).shape) == (N_OUT,)
    if dtype != torch.bfloat16:  # NumPy in, NumPy out
        z = mx.linear_mxfp4(x.cpu().numpy(), codes.cpu().numpy(), scales.cpu().numpy(), bias.cpu().numpy(), activations=A6)
        assert isinstance(z, np.ndarray) and np.array_equal(bits(z), bits(y))


@pytest.mark.parametrize("dtype", DTYPES)
def test_linear_with_a_rotation(layer, dtype):
    from sleekit_amd import mx, rotation

    codes, scales, bias = layer
    rot = rotation.Rotation(K_IN, seed=3)
    assert rot.block == 32
    x = torch.from_numpy(block_gaussian(np.random.default_rng(4), 6, K_IN)).reshape(2, 3, K_IN).to(dtype).cuda()
    for out in DTYPES:
        got = mx.linear_mxfp4(x, codes, scales, bias, dtype=out, activations=A6, rotation=rot)
        want = mx.linear_mxfp4(rot.apply(x, dtype=torch.float32), codes, scales, bias, dtype=out, activations=A6)
        assert tuple(got.shape) == (2, 3, N_OUT) and same_bits(got, want), out
    got = mx.linear_mxfp4(x, codes, scales, bias, activations=A6, rotation=rot)
    assert got.dtype == dtype  # the output dtype follows x, not the float32 transform


Result = collections.namedtuple("Result", "codes scales rotation")


def test_modules(layer):
    import torch.nn as nn

    from sleekit_amd import MXLinear, mx, rotation
    from sleekit_amd.rotation import RotatedLinear

    codes, scales, bias = layer
    rot = rotation.Rotation(K_IN, seed=6)
    lin = nn.Linear(K_IN, N_OUT).cuda()
    lin.bias.data.copy_(bias)
    res = Result(codes, scales, rot)
    x = torch.from_numpy(block_gaussian(np.random.default_rng(5), 10, K_IN)).reshape(2, 5, K_IN).cuda()
    # MXLinear(activations="mxfp6_e2m3") and its state dict, on the device
    a6 = MXLinear.from_result(lin, res, activations=A6)
    assert a6.activations == A6
    for t in (x, x.bfloat16(), x.half()):
        assert same_bits(a6(t), mx.linear_mxfp4(t, codes, scales, bias, activations=A6))
    copy = MXLinear(K_IN, N_OUT).cuda()
    assert copy.activations == "mxfp8"
    copy.load_state_dict(a6.state_dict())
    assert copy.activations == A6 and same_bits(copy(x), a6(x))
    a8 = MXLinear.from_result(lin, res)
    assert sorted(a8.state_dict()) == ["bias", "codes", "scales"] and not torch.equal(a8(x), a6(x))
    copy.load_state_dict(a8.state_dict())
    assert copy.activations == "mxfp8" and same_bits(copy(x), a8(x))
    # RotatedLinear: plain and fused
    plain = RotatedLinear.from_result(lin, res, activations=A6)
    assert not plain.fused and plain.inner.activations == A6
    fused = RotatedLinear.from_result(lin, res, fused=True, activations=A6)
    assert fused.fused and fused.inner.activations == A6
    for t in (x, x.bfloat16(), x.half()):
        assert same_bits(plain(t), a6(rot.apply(t)))
        assert same_bits(fused(t), mx.linear_mxfp4(t, codes, scales, bias, activations=A6, rotation=rot))
        assert same_bits(fused(t), mx.linear_mxfp4(rot.apply(t, dtype=torch.float32), codes, scales, bias, dtype=t.dtype, activations=A6))
    assert same_bits(fused(x), plain(x))  # a float32 x: the default forward makes no rounding in between
    other = RotatedLinear(MXLinear(K_IN, N_OUT).cuda(), rotation.Rotation(K_IN, block=16, seed=1))
    other.load_state_dict(fused.state_dict())
    assert other.fused and other.block == rot.block and other.inner.activations == A6
    assert same_bits(other(x.bfloat16()), fused(x.bfloat16()))
    other.load_state_dict(plain.state_dict())
    assert not other.fused and same_bits(other(x.bfloat16()), plain(x.bfloat16()))
    # against the model: the rotated input quantized by the model, the product within the bound
    xr = rot.apply(x, dtype=torch.float32).reshape(10, K_IN).cpu().numpy()
    want, sum_abs = model.matmul_model(*model.quantize_act6_model(xr), codes.cpu().numpy(), scales.cpu().numpy(), bias.cpu().numpy())
    got = fused(x).reshape(10, N_OUT).cpu().numpy().astype(np.float64)
    assert (np.abs(got - want) <= bound(K_IN + 1, sum_abs + np.abs(bias.cpu().numpy())[None, :])).all()


@pytest.mark.parametrize("M", [1, 64, 65])
def test_repeated_calls_are_bit_equal(M):
    """M = 1 and 64 run the split-K kernel, 65 the tiled one."""
    from sleekit_amd import mx, rotation

    rng = np.random.default_rng(M)
    N, K = 200, 4128
    x = torch.from_numpy(block_gaussian(rng, M, K)).cuda()
    w_codes, w_scales = (torch.from_numpy(t).cuda() for t in random_weights(rng, N, K, 118, 123))
    rot = rotation.Rotation(K, seed=M)
    for kw in (dict(activations=A6), dict(activations=A6, rotation=rot)):
        first = mx.linear_mxfp4(x, w_codes, w_scales, **kw)
        for _ in range(3):
            assert torch.equal(mx.linear_mxfp4(x, w_codes, w_scales, **kw).view(torch.int32), first.view(torch.int32))


def test_refusals():
    from sleekit_amd import mx

    codes = torch.zeros((8, 32), dtype=torch.uint8, device="cuda")
    scales = torch.full((8, 2), 127, dtype=torch.uint8, device="cuda")
    x = torch.zeros((4, 64), device="cuda")
    a_codes, a_scales = mx.quantize_mxfp6_act(x)
    assert tuple(a_codes.shape) == (4, 48) and a_scales.eq(74).all() and not a_codes.any()
    a4 = mx.quantize_mxfp4_act(x)[0]
    a8 = mx.quantize_mxfp8(x)[0]
    for call in (lambda: mx.quantize_mxfp6_act(torch.zeros((4, 48), device="cuda")),
                 lambda: mx.quantize_mxfp6_act(x.double()), lambda: mx.quantize_mxfp6_act(x.long()), lambda: mx.quantize_mxfp6_act(x[0]),
                 lambda: mx.matmul_mx(a4, a_scales, codes, scales, activations=A6),  # a_codes of MXFP4 shape
                 lambda: mx.matmul_mx(a8, a_scales, codes, scales, activations=A6),  # ... of MXFP8 shape
                 lambda: mx.matmul_mx(a_codes, a_scales, codes, scales),  # (4, 48) bytes are 48 columns of MXFP8
                 lambda: mx.matmul_mx(a_codes, a_scales[:, :1], codes, scales, activations=A6),
                 lambda: mx.matmul_mx(a_codes, torch.cat([a_scales, a_scales], 1), codes, scales, activations=A6),
                 lambda: mx.matmul_mx(a_codes.float(), a_scales, codes, scales, activations=A6),
                 lambda: mx.matmul_mx(a_codes, a_scales, codes, scales, activations="mxfp6"),
                 lambda: mx.matmul_mx(a_codes, a_scales, codes, scales, activations="mxfp6_e3m2"),
                 lambda: mx.dequantize_mxfp6_act(a4, a_scales),
                 lambda: mx.dequantize_mxfp6_act(a_codes, a_scales, dtype=torch.float64),
                 lambda: mx.linear_mxfp4(x, codes, scales, activations=A6, dtype=torch.float64),
                 lambda: mx.linear_mxfp4(x.double(), codes, scales, activations=A6),
                 lambda: mx.linear_mxfp4(x, codes, scales, activations=A6, bias=torch.zeros(7, device="cuda"))):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(ValueError, match="bfloat16"):
        mx.matmul_mx(a_codes.cpu().numpy(), a_scales, codes, scales, dtype=torch.bfloat16, activations=A6)
