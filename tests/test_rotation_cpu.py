"""The rotation without a GPU: the NumPy model of slk_hadamard_rows (tests/rotation_model.py) against dense products, the
mistakes the GPU comparisons have to catch, the argument checks of the entry point, and Rotation's defaults.

The one tolerance of this file is the bound of test_random_float32_within_the_derived_bound.  In every stage the nodes that
feed one output partition the block, so the absolute values of a stage's nodes under one output sum to at most A =
sum_block |x| (1 + u)^stage, u = 2^-24; each of the log2(block) additions on the path and the final product with c rounds
once, relative u, and c itself is within u / 2 of 1 / sqrt(block).  To first order |model - exact| <= (log2(block) + 1) u A c;
the factor (1 + 2^-20) covers the higher orders ((1 + u)^13 - 1 - 13 u < 2^-40) and c's own rounding.
"""

import numpy as np
import pytest

import rotation_model as model

ALL_BLOCKS = [1 << k for k in range(1, 13)]


@pytest.fixture(scope="module")
def H4096():
    return model.hadamard(4096)


# ---------------------------------------------------------------------------------------------------------------- exact
@pytest.mark.parametrize("block", ALL_BLOCKS)
def test_integers_equal_the_dense_product(block, H4096):
    n = 2 * block
    x, s = model.integers(3, n, block), model.signs_for(n, block)
    for kind in ("f32", "f64"):
        ctype = model.COMPUTE[kind]
        for signs in (None, s):
            for transposed in (False, True):
                dense = model.dense_product(x, block, signs, transposed, H4096)
                assert np.abs(dense).max() <= 4 * block  # integers: exact in every order and in float32
                want = dense.astype(ctype) * model.scale_factor(block, ctype)
                got = model.transform(x.astype(ctype), block, signs, transposed)
                assert got.dtype == want.dtype and np.array_equal(model.bits_of(got + 0), model.bits_of(want + 0)), (kind, transposed)


def test_hadamard_matrix_is_what_the_butterflies_build():
    for block in (2, 4, 8, 64):
        H = model.hadamard(block).astype(np.float64)
        assert np.array_equal(H, H.T) and np.array_equal(H @ H, block * np.eye(block))
        got = model.transform(np.eye(block), block) * np.sqrt(block)
        assert np.array_equal(np.rint(got), H) and np.abs(got - H).max() < 1e-12
    assert np.array_equal(model.hadamard(2), [[1, 1], [1, -1]])


@pytest.mark.parametrize("block", [4, 16, 64, 256, 1024, 4096])
def test_power_of_four_round_trip_is_exact(block):
    """c is a power of two, so apply_t(apply(x)) == x exactly on integers (and wherever nothing is rounded); as values: a
    zero may come back with the other sign."""
    assert model.scale_factor(block, np.float32) == 2.0 ** -(block.bit_length() // 2)
    n = 2 * block
    x, s = model.integers(3, n, block + 1), model.signs_for(n, block + 1)
    for kind in ("f32", "bf16", "f16", "f64"):
        xin = model.to_kind(x, kind)
        there = model.rows_model(xin, kind, "f64" if kind == "f64" else "f32", block, s, False)
        back = model.rows_model(there, "f64" if kind == "f64" else "f32", kind, block, s, True)
        assert np.array_equal(model.to_compute(back, kind), model.to_compute(xin, kind)), kind


def test_bfloat16_rounding():
    x = np.array([1.0, 1.00390625, 1.01171875, -1.00390625, 3.4028235e38, np.inf, -np.inf, np.nan, 0.0, -0.0], np.float32)
    # 1 + 2^-8 is a tie and goes to even (1.0); 1 + 3 * 2^-8 is a tie and goes up to 1 + 2^-6; the largest float32 rounds to infinity
    assert model.bf16_bits(x).tolist() == [0x3F80, 0x3F80, 0x3F82, 0xBF80, 0x7F80, 0x7F80, 0xFF80, 0x7FC0, 0x0000, 0x8000]
    assert np.array_equal(model.bf16_value(np.array([0x3F80, 0xC000], np.uint16)), np.array([1.0, -2.0], np.float32))
    import torch

    r = model.block_gaussian(7, 64, 5).astype(np.float32)
    want = torch.from_numpy(r).bfloat16().view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(model.bf16_bits(r), want)


# ---------------------------------------------------------------------------------------------------------------- bound
@pytest.mark.parametrize("block", ALL_BLOCKS)
def test_random_float32_within_the_derived_bound(block, H4096):
    n = 2 * block
    x, s = model.make_input("f32", "random", 5, n, block), model.signs_for(n, block)
    u = 2.0 ** -24
    for transposed in (False, True):
        exact = model.dense_product(x, block, s, transposed, H4096) / np.sqrt(np.float64(block))
        got = model.transform(x, block, s, transposed).astype(np.float64)
        A = np.abs(x.astype(np.float64)).reshape(5, 2, block).sum(axis=2)
        limit = np.repeat((block.bit_length()) * u * A / np.sqrt(np.float64(block)) * (1 + 2.0 ** -20), block, axis=1)
        err = np.abs(got - exact)
        print(f"block {block} transposed {transposed}: max err / bound = {(err / limit).max():.3f}")
        assert (err <= limit).all()


# ---------------------------------------------------------------------------------------------------------------- mistakes
# where each mistake has to show: "descending" changes roundings only, so it needs data that rounds (random, in the
# compute type's own precision: float32 in and out, float64 in and out) and more than one stage; "signs-side" needs signs
def mistake_applies(mistake, block, x_kind, y_kind, data, signed):
    if mistake == "descending":
        return data == "random" and block >= 4 and (x_kind, y_kind) in (("f32", "f32"), ("f64", "f64"))
    if mistake == "upper-lower":
        return data == "int"
    if mistake == "signs-side":
        return signed
    return True


@pytest.mark.parametrize("block", model.BLOCKS)
def test_every_mistake_differs_at_every_shape_of_the_gpu_matrix(block):
    """At the smallest case of each shape, its first row (the 5- and 67-row cases contain it), so at all of them."""
    checked = {m: 0 for m in model.MISTAKES}
    for width in model.WIDTHS:
        n = width * block
        for x_kind, y_kind in model.KINDS:
            for data in model.DATA:
                x67, s = model.case_input(x_kind, data, block, n)
                x = x67[:1]
                for signs in (None, s):
                    for transposed in (False, True):
                        want = model.rows_model(x, x_kind, y_kind, block, signs, transposed)
                        for mistake in model.MISTAKES:
                            if mistake_applies(mistake, block, x_kind, y_kind, data, signs is not None):
                                wrong = model.rows_model(x, x_kind, y_kind, block, signs, transposed, mistake)
                                assert not model.same(wrong, want, y_kind), (mistake, n, x_kind, y_kind, data, signs is not None, transposed)
                                checked[mistake] += 1
    assert all(count > 0 for mistake, count in checked.items() if not (mistake == "descending" and block < 4)), checked


# ---------------------------------------------------------------------------------------------------------------- the entry point
def test_argument_errors_do_not_touch_the_gpu():
    """Bad arguments are rejected on the host before any launch (safe without a GPU): the pointers below are not memory."""
    from sleekit_amd import _lib

    f = _lib.lib.slk_hadamard_rows
    F32, BF16, F64 = _lib.DTYPE_F32, _lib.DTYPE_BF16, _lib.DTYPE_F64
    assert F64 == 3
    for block, n in ((3, 12), (1, 12), (8192, 8192), (0, 12), (-2, 12), (6, 12)):
        assert f(64, F32, 64, F32, 4, n, block, None, 0, None) == _lib.E_ARG, block
        assert b"power of two" in _lib.lib.slk_last_error()
    assert f(64, F32, 64, F32, 4, 24, 16, None, 0, None) == _lib.E_ARG  # n % block != 0
    assert b"does not divide" in _lib.lib.slk_last_error()
    assert f(None, F32, 64, F32, 4, 16, 16, None, 0, None) == _lib.E_ARG
    assert b"null" in _lib.lib.slk_last_error()
    assert f(64, F32, None, F32, 4, 16, 16, None, 0, None) == _lib.E_ARG
    assert f(64, F64, 64, F32, 4, 16, 16, None, 0, None) == _lib.E_ARG  # float64 in, float32 out
    assert b"float64" in _lib.lib.slk_last_error()
    assert f(64, BF16, 64, F64, 4, 16, 16, None, 0, None) == _lib.E_ARG
    assert f(64, 4, 64, F32, 4, 16, 16, None, 0, None) == _lib.E_ARG and f(64, F32, 64, -1, 4, 16, 16, None, 0, None) == _lib.E_ARG
    for rows in (0, -1):
        assert f(64, F32, 64, F32, rows, 16, 16, None, 0, None) == _lib.E_ARG
    assert f(64, F32, 64, F32, 4, 0, 2, None, 0, None) == _lib.E_ARG
    assert f(64, F32, 64, F32, 1 << 40, 4096, 4096, None, 0, None) == _lib.E_ARG  # more chunks than one grid covers
    assert b"workgroups" in _lib.lib.slk_last_error()
    assert _lib.lib.slk_abi_version() == 8


# ---------------------------------------------------------------------------------------------------------------- Rotation
def test_rotation_defaults_and_sign_rule():
    import sleekit_amd
    from sleekit_amd import rotation, synth

    assert sleekit_amd.Rotation is rotation.Rotation and sleekit_amd.RotatedLinear is rotation.RotatedLinear
    for n, block in ((4096, 4096), (11008, 256), (384, 128), (8192, 4096), (6, 2)):
        assert rotation.default_block(n) == block and rotation.Rotation(n, device="cpu").block == block
    for seed in (0, 3):
        rot = rotation.Rotation(384, seed=seed, device="cpu")
        bit = (synth.hash_grid(seed, 7, 1, 384)[0] >> np.uint64(13)) & np.uint64(1)
        want = np.where(bit == 1, 1.0, -1.0).astype(np.float32)
        assert rot.n == 384 and rot.signs.dtype.is_floating_point and np.array_equal(rot.signs.numpy(), want)
        assert 100 < (want > 0).sum() < 284
    assert rotation.Rotation(384, block=32, device="cpu").block == 32
    for n, block in ((384, 256), (384, 3), (384, 1), (8192, 8192), (7, None)):
        with pytest.raises(ValueError):
            rotation.Rotation(n, block=block, device="cpu")
    with pytest.raises(ValueError):
        rotation.RotatedLinear.from_result(None, object())  # no rotation on the result


def test_sleekit_takes_the_keyword():
    import inspect

    from sleekit_amd import Sleekit, engine

    for name in ("quantize", "quantize_packed", "__init__"):  # (quantize_mxfp4 keeps its parameter list: the object's rotation)
        p = inspect.signature(getattr(Sleekit, name)).parameters
        assert "rotation" in p and p["rotation"].default is None, name
    assert engine.LayerResult().rotation is None
