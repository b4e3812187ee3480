"""NumPy model of slk_hadamard_rows (the contract in include/sleekit_amd.h), one compute-type operation at a time, and the
input builders of the rotation tests.

    v = x, converted;  not transposed: v = s * v
    for h = 1, 2, 4, ..., block / 2:  pairs (i, i + h) with (i & h) == 0:  (v_i, v_{i+h}) <- (v_i + v_{i+h}, v_i - v_{i+h})
    y = v * c, c = compute-type rounding of 1 / sqrt(block);  transposed: y = s * y
    y converted to the output type, round to nearest even

Element kinds: "f32", "f16", "f64" are NumPy arrays of that type; "bf16" travels as uint16 bit patterns (NumPy has no
bfloat16).  NumPy rounds every float32 / float64 operation once and fuses nothing, which is what the contract asks for.

`mistake=` builds the transform with one deliberate error, for the tests that show the comparisons can fail:
    "descending"   the stages in the order block / 2, ..., 2, 1 (the same matrix, other roundings)
    "upper-lower"  the upper element of a pair takes upper - lower
    "signs-side"   the signs applied at the other end of the transform
    "no-c"         the factor c left out
    "boundary"     the blocks start one column late (and wrap at the end of the row)
"""

import numpy as np

COMPUTE = {"f32": np.float32, "bf16": np.float32, "f16": np.float32, "f64": np.float64}
MISTAKES = ("descending", "upper-lower", "signs-side", "no-c", "boundary")


# ---------------------------------------------------------------------------------------------------------------- element types
def bf16_bits(x):
    """float32 -> bfloat16 bit patterns (uint16), round to nearest even; every NaN becomes the quiet NaN 0x7fc0."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    out = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    return np.where((u & 0x7FFFFFFF) > 0x7F800000, np.uint16(0x7FC0), out)


def bf16_value(bits):
    """bfloat16 bit patterns (uint16) -> the float32 values they stand for (exact)."""
    return (np.ascontiguousarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32)


def to_kind(x, kind):
    """A float array as the element kind `kind` (round to nearest even)."""
    with np.errstate(over="ignore"):
        return bf16_bits(x) if kind == "bf16" else np.asarray(x).astype({"f32": np.float32, "f16": np.float16, "f64": np.float64}[kind])


def to_compute(x, kind):
    """Elements of kind `kind` in the compute type of that kind (exact)."""
    return bf16_value(x) if kind == "bf16" else np.asarray(x).astype(COMPUTE[kind])


def is_nan(y, kind):
    return (np.asarray(y) & 0x7FFF) > 0x7F80 if kind == "bf16" else np.isnan(y)


def bits_of(y):
    y = np.ascontiguousarray(y)
    return y.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[y.dtype.itemsize])


def same(got, want, kind):
    """Bit for bit, NaNs compared as NaN."""
    nan_g, nan_w = is_nan(got, kind), is_nan(want, kind)
    return got.shape == want.shape and np.array_equal(nan_g, nan_w) and np.array_equal(bits_of(got)[~nan_w], bits_of(want)[~nan_w])


# ---------------------------------------------------------------------------------------------------------------- the transform
def scale_factor(block, ctype):
    return ctype(1.0 / np.sqrt(np.float64(block)))


def transform(v, block, signs=None, transposed=False, mistake=None):
    """Steps 1-3 on v (rows, n) already in its compute type (float32 or float64); returns that type."""
    ctype = v.dtype.type
    assert ctype in (np.float32, np.float64) and v.ndim == 2 and v.shape[1] % block == 0 and block & (block - 1) == 0 and block >= 2
    rows, n = v.shape
    s = None if signs is None else np.asarray(signs).astype(ctype)[None, :]
    first = (not transposed) != (mistake == "signs-side")
    with np.errstate(invalid="ignore", over="ignore"):
        if s is not None and first:
            v = s * v
        if mistake == "boundary":
            v = np.roll(v, -1, axis=1)
        v = np.ascontiguousarray(v).reshape(rows, n // block, block)
        stages = [1 << k for k in range(block.bit_length() - 1)]
        for h in (stages[::-1] if mistake == "descending" else stages):
            pairs = v.reshape(rows, n // block, block // (2 * h), 2, h)
            lower, upper = pairs[:, :, :, 0, :], pairs[:, :, :, 1, :]
            diff = upper - lower if mistake == "upper-lower" else lower - upper
            v = np.stack((lower + upper, diff), axis=3).reshape(rows, n // block, block)
        v = v.reshape(rows, n)
        if mistake == "boundary":
            v = np.roll(v, 1, axis=1)
        if mistake != "no-c":
            v = v * scale_factor(block, ctype)
        if s is not None and not first:
            v = s * v
    assert v.dtype.type is ctype
    return v


def rows_model(x, x_kind, y_kind, block, signs=None, transposed=False, mistake=None):
    """slk_hadamard_rows: x (rows, n) of kind x_kind -> (rows, n) of kind y_kind."""
    assert (x_kind == "f64") == (y_kind == "f64")
    return to_kind(transform(to_compute(x, x_kind), block, signs, transposed, mistake), y_kind)


def hessian_model(H, block, signs):
    """Rotation.hessian: float64 rows pass, transpose, rows pass, the lower triangle mirrored, one rounding to float32."""
    H64 = np.asarray(H, np.float32).astype(np.float64)
    half = np.ascontiguousarray(transform(H64, block, signs).T)
    full = transform(half, block, signs)
    i = np.arange(H64.shape[0])
    return np.where(i[:, None] >= i[None, :], full, full.T).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- references
def hadamard(block):
    """The Sylvester-Hadamard matrix of order `block` as int8: entry (i, j) is (-1)^popcount(i & j)."""
    i = np.arange(block, dtype=np.uint16)
    x = i[:, None] & i[None, :]
    for shift in (8, 4, 2, 1):
        x = x ^ (x >> shift)
    return (1 - 2 * (x & 1).astype(np.int8)).astype(np.int8)


def dense_product(x, block, signs=None, transposed=False, H=None):
    """(x . s) blockdiag(H_block) (or (x blockdiag(H_block)) . s) in float64, WITHOUT the factor c: a dense product."""
    x = np.asarray(x, np.float64)
    rows, n = x.shape
    H = (hadamard(block) if H is None else H[:block, :block]).astype(np.float64)
    s = np.ones(n) if signs is None else np.asarray(signs, np.float64)
    if not transposed:
        x = x * s
    y = (x.reshape(rows * (n // block), block) @ H).reshape(rows, n)
    return y * s if transposed else y


# ---------------------------------------------------------------------------------------------------------------- inputs
def signs_for(n, seed):
    """n signs of +-1 (float32), about half of each, from a seeded generator."""
    return np.where(np.random.default_rng(1000 + seed).integers(0, 2, n) == 1, np.float32(1), np.float32(-1))


def integers(rows, n, seed):
    """Integers in -4 .. 4 as float32: every kind holds them, and every sum of up to 4096 of them, exactly."""
    return np.random.default_rng(seed).integers(-4, 5, (rows, n)).astype(np.float32)


def block_gaussian(rows, n, seed):
    """Gaussian float64 data whose stretches of 8 columns (2 at the end of a short row) have magnitudes 2^-3 .. 2^3."""
    rng = np.random.default_rng(seed)
    mag = 2.0 ** rng.integers(-3, 4, (rows, (n + 7) // 8))
    return (rng.standard_normal((rows, n)) * np.repeat(mag, 8, axis=1)[:, :n])


def make_input(kind, data, rows, n, seed):
    """(rows, n) of element kind `kind`: data "int" or "random", rounded once to the kind."""
    x = integers(rows, n, seed) if data == "int" else block_gaussian(rows, n, seed)
    return to_kind(x, kind)


# ---------------------------------------------------------------------------------------------------------------- the GPU matrix
# What tests/test_gpu_rotation.py runs against the model, and tests/test_rotation_cpu.py shows every mistake to differ at:
# blocks 2, 8, 16 stay in a lane's registers, 32 .. 1024 cross lanes, 2048 and 4096 cross waves; one block a row and three;
# the first 1, 5 and 67 rows of ONE 67-row input (so a shorter case is a prefix of the longer one).
BLOCKS = (2, 8, 16, 32, 64, 512, 1024, 2048, 4096)
WIDTHS = (1, 3)  # n / block
ROWS = (1, 5, 67)
KINDS = (("f32", "f32"), ("f32", "bf16"), ("bf16", "bf16"), ("f16", "f16"), ("bf16", "f32"), ("f64", "f64"))
DATA = ("int", "random")


def case_input(x_kind, data, block, n):
    """The 67-row input of the matrix at (block, n) and its signs."""
    seed = 31 * block + n + (7 if data == "random" else 0)
    return make_input(x_kind, data, ROWS[-1], n, seed), signs_for(n, seed)
