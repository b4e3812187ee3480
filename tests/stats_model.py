"""NumPy model of the running statistics (slk_hessian_accumulate, Sleekit.add_batch), written from the documented
arithmetic alone, and of the six-term bfloat16 product of mfma_bf16x3.h that its wide path and the layer error share.

    f = float32(c / c'),  cnt = float32(c'),  c' = c + T
    per chunk of tokens:  H = fl(fl(H * f_chunk) + fl(v_chunk / cnt)),   f_chunk = f on the first chunk, 1 after it
    mean = fl(fl(mean * f) + fl(s / cnt))

Every fl() is one float32 rounding (the library is built with -ffp-contract=off and IEEE division).  v_chunk = X^T X over
the chunk's tokens and s = the column sums are formed in float64 and rounded to float32 once: the exact tests use inputs
(the builders below) for which they are exact in float32 in ANY order of summation, so that one rounding changes nothing
and the model holds for every kernel bit for bit.  With `pieces` v_chunk is the six-term product: each operand split into
three bfloat16 pieces (split3) and only the pairs (3,1), (2,2), (1,3), (2,1), (1,2), (1,1) multiplied.

The keyword arguments after `pieces` are MUTATIONS: each makes the model compute what a kernel with one particular
mistake would compute.  tests/test_stats_model_cpu.py runs every comparison of tests/test_gpu_stats.py against them, so
that each comparison is known to fail for each mistake.  The shapes of the GPU tests live here for that reason.
"""

import functools

import numpy as np
import torch

SIX = ((3, 1), (2, 2), (1, 3), (2, 1), (1, 2), (1, 1))  # the order of the MFMAs in mfma_bf16x3.h: smallest terms first
WRONG_PAIRING = ((3, 1), (2, 2), (3, 1), (2, 1), (1, 2), (1, 1))  # a3 b1 twice, a1 b3 never

# ---- the shapes of tests/test_gpu_stats.py
F32_N = (1, 5, 127, 129, 130, 260)
F32_T = (1, 15, 16, 17, 32, 48, 75)
F32_FORCED_N = (128, 256)
F32_BATCHES = ((17, 15, 33), (48, 27))  # tokens per batch: c' = 17, 32 (a power of two), 65; and 48, 75
F32_BATCH_N = (130, 260)
BIG_COUNT = 2 ** 31 + 5
BF16_SHAPES = ((128, 32), (128, 40), (256, 64), (384, 96))  # (n, T)
BF16_ROOMS = (None, 32, 64)  # tokens the workspace has room for (None: all of them)
SHARP_SHAPES = ((128, 32), (128, 64), (256, 32), (256, 64))  # (n, T)
MEAN_T = (1, 7, 8, 9, 24, 25, 31, 32, 33, 57, 64, 65)
MEAN_N = (1, 31, 32, 33, 128)
G_SHAPES = ((130, 128, 32), (130, 256, 64))  # (R, n, modulus of the zero pattern)
STRIP_N = (1, 255, 257, 300)


def bf16_round(x):
    """float32 -> nearest bfloat16 (ties to even), as float32."""
    t = torch.from_numpy(np.array(x, dtype=np.float32))  # (a copy: torch wants a writable array)
    return t.to(torch.bfloat16).to(torch.float32).numpy()


def split3(x):
    """The three bfloat16 pieces of float32 x as split3_pair forms them, each as float32: round, subtract in float32, twice."""
    x = np.asarray(x, np.float32)
    p1 = bf16_round(x)
    r = (x - p1).astype(np.float32)
    p2 = bf16_round(r)
    s = (r - p2).astype(np.float32)
    return p1, p2, bf16_round(s)


def six_term_parts(A, B, terms=SIX):
    """[A_p^T B_q for (p, q) in terms] in float64: piece p of A (K, m) with piece q of B (K, n)."""
    a = [p.astype(np.float64) for p in split3(A)]
    b = [p.astype(np.float64) for p in split3(B)]
    return [a[p - 1].T @ b[q - 1] for p, q in terms]


def six_term(A, B, terms=SIX):
    """A^T B for A (K, m), B (K, n) over the piece pairs `terms` of mfma_bf16x3.h, in float64."""
    return sum(six_term_parts(A, B, terms))


def six_term_abs(A, B, terms=SIX):
    """sum |piece products| per entry: below 2^24 units of the entries' common quantum every order of float32 sums is exact."""
    a = [np.abs(p.astype(np.float64)) for p in split3(A)]
    b = [np.abs(p.astype(np.float64)) for p in split3(B)]
    return sum(a[p - 1].T @ b[q - 1] for p, q in terms)


def chunk_tokens(T, room):
    """Tokens per chunk of the bfloat16 path whose workspace has room for `room` tokens (a multiple of 32; None: all)."""
    whole = (T + 31) // 32 * 32
    return whole if room is None else min(room, whole)


def ws_bytes_for(n, room):
    """The workspace size that gives the bfloat16 path room for exactly `room` tokens: 4096 + 6 n room."""
    return 4096 + 6 * n * room


def mean_main_loop_tokens(T):
    """The tokens k_mean_update's four-sum loop takes (thread group g walks g, g + 8, ... in fours while t + 24 < T); the
    others are its tail loop's."""
    taken = []
    for g in range(8):
        t = g
        while t + 24 < T:
            taken += [t, t + 8, t + 16, t + 24]
            t += 32
    return sorted(taken)


def accumulate_model(H, mean, X, count_before, chunk=None, pieces=False, *, exact=False, terms=SIX, drop_token=None, pad_to=None,
                     factor_every_chunk=False, skip_mirror=False, swap_features=None, mean_tail_dropped=False, cnt_is_T=False):
    """(H', mean') float32 after one batch X (T, n) on top of `count_before` tokens.

    Mutations: `terms` other pairs than SIX; `drop_token` t: the product misses token t; `pad_to` p: every chunk is padded
    to a multiple of p tokens with copies of its last token instead of zeros; `factor_every_chunk`; `skip_mirror`: the
    strict upper triangle keeps its old values; `swap_features` (a, b): the product reads features a and b in each other's
    place; `mean_tail_dropped`: the mean misses the tokens of its kernel's tail loop; `cnt_is_T`: divides by T, not c'."""
    H = np.array(H, np.float32)
    mean = np.array(mean, np.float32)
    X = np.ascontiguousarray(X, dtype=np.float32)
    T, n = X.shape
    after = int(count_before) + T
    f = np.float32(int(count_before) / after)
    cnt = np.float32(T if cnt_is_T else after)
    Xp = X
    if swap_features is not None:
        a, b = swap_features
        Xp = X.copy()
        Xp[:, [a, b]] = X[:, [b, a]]
    step = T if chunk is None else int(chunk)
    old = H.copy()
    for t0 in range(0, T, step):
        rows = [t for t in range(t0, min(t0 + step, T)) if t != drop_token]
        Xc = Xp[rows]
        if pad_to and len(rows) % pad_to:
            Xc = np.concatenate([Xc, np.repeat(Xc[-1:], pad_to - len(rows) % pad_to, axis=0)])
        v64 = six_term(Xc, Xc, terms) if pieces else Xc.astype(np.float64).T @ Xc.astype(np.float64)
        v = v64.astype(np.float32)
        assert not exact or np.array_equal(v.astype(np.float64), v64), "this input's products are not exact in float32"
        fc = f if (t0 == 0 or factor_every_chunk) else np.float32(1.0)
        H = ((H * fc).astype(np.float32) + (v / cnt).astype(np.float32)).astype(np.float32)
    if skip_mirror:
        iu = np.triu_indices(n, 1)
        H[iu] = old[iu]
    rows = mean_main_loop_tokens(T) if mean_tail_dropped else list(range(T))
    s64 = X[rows].astype(np.float64).sum(axis=0)
    s = s64.astype(np.float32)
    assert not exact or np.array_equal(s.astype(np.float64), s64), "this input's column sums are not exact in float32"
    mean = ((mean * f).astype(np.float32) + (s / cnt).astype(np.float32)).astype(np.float32)
    return H, mean


def accumulate_batches(Xs, pieces=False, room=None, **mutation):
    """(H, mean) after the batches Xs on top of zero statistics; with `pieces` in the bfloat16 path's chunks for `room`."""
    n = Xs[0].shape[1]
    H, mean, count = np.zeros((n, n), np.float32), np.zeros(n, np.float32), 0
    for X in Xs:
        chunk = chunk_tokens(X.shape[0], room) if pieces else None
        H, mean = accumulate_model(H, mean, X, count, chunk=chunk, pieces=pieces, **mutation)
        count += X.shape[0]
    return H, mean


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.uint32), b.view(np.uint32)))


def exact_in_float32(v64, sum_abs, quantum):
    """True when every entry of v64 is a multiple of `quantum` (a power of two) and its terms' magnitudes add up to less
    than 2^24 quanta: every partial sum, in any order, is then a float32."""
    q = v64 / quantum
    return bool(np.array_equal(q, np.round(q)) and (sum_abs < 2.0 ** 24 * quantum).all())


# --------------------------------------------------------------------------------------------------------------- builders
# (each input is built, and its conditions asserted, once per session; the arrays are read-only)
def frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def integers(T, n, seed):
    """X in -4 .. 4: products and sums of integers far below 2^24, exact in every order on every kernel; as bfloat16
    pieces only the first is non-zero."""
    X = np.random.default_rng(seed).integers(-4, 5, size=(T, n)).astype(np.float32)
    p1, p2, p3 = split3(X)
    assert np.array_equal(p1, X) and not p2.any() and not p3.any()
    assert exact_in_float32(X.astype(np.float64).T @ X, np.abs(X).astype(np.float64).T @ np.abs(X), 1.0)
    return frozen(X)


def three_piece_values(shape, rng):
    """s (1.5 + e2 2^-9 + e3 2^-19) with random signs s, e2, e3, and the three pieces it must split into."""
    s, e2, e3 = (rng.integers(0, 2, size=shape).astype(np.float64) * 2 - 1 for _ in range(3))
    x = (s * (1.5 + e2 * 2.0 ** -9 + e3 * 2.0 ** -19)).astype(np.float32)
    assert np.array_equal(x.astype(np.float64), s * (1.5 + e2 * 2.0 ** -9 + e3 * 2.0 ** -19))
    return x, (1.5 * s, s * e2 * 2.0 ** -9, s * e3 * 2.0 ** -19)


def assert_three_pieces(x, want, mask):
    for got, w in zip(split3(x), want):
        assert np.array_equal(got.astype(np.float64), np.where(mask, w, 0.0))


@functools.lru_cache(maxsize=None)
def three_piece(T, n, seed, modulus=16):
    """X (T, n) with x[t][j] = s (1.5 + e2 2^-9 + e3 2^-19) where (t + j) % modulus == 0, else 0.  All three pieces of an
    element are non-zero (1.5 s, s e2 2^-9, s e3 2^-19); every six-term entry of X^T X is a multiple of 2^-20 whose terms'
    magnitudes add up to less than 16, so the bfloat16 MFMA's float32 sums are exact in any order; the two pairs the six
    terms leave out, (2,3) and (3,3), do not vanish, so the six-term value is not the float64 product.  All asserted."""
    rng = np.random.default_rng(seed)
    t, j = np.meshgrid(np.arange(T), np.arange(n), indexing="ij")
    mask = (t + j) % modulus == 0
    vals, want = three_piece_values((T, n), rng)
    X = np.where(mask, vals, np.float32(0)).astype(np.float32)
    assert_three_pieces(X, want, mask)
    v, a = six_term(X, X), six_term_abs(X, X)
    assert exact_in_float32(v, a, 2.0 ** -20) and a.max() < 16.0, (T, n, a.max())
    full = X.astype(np.float64).T @ X.astype(np.float64)
    assert (full != v).sum() * 2 > (v != 0).sum(), "the six-term value should differ from the float64 product in most entries"
    # the column sums of the mean: multiples of 2^-19 below 2^5
    assert (np.abs(X).astype(np.float64).sum(axis=0) < 32.0).all()
    return frozen(X)


@functools.lru_cache(maxsize=None)
def three_piece_layer(R, n, seed, modulus, symmetric=True):
    """(W (R, n), H (n, n)) three-piece built on the pattern (row + column) % modulus == 0, H symmetric -- or with the sign
    of one entry above the diagonal flipped.  Asserts that the six-term product W H is exact in float32 in any order."""
    rng = np.random.default_rng(seed)
    r, k = np.meshgrid(np.arange(R), np.arange(n), indexing="ij")
    wmask = (r + k) % modulus == 0
    wv, wwant = three_piece_values((R, n), rng)
    W = np.where(wmask, wv, np.float32(0)).astype(np.float32)
    assert_three_pieces(W, wwant, wmask)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    hmask = (i + j) % modulus == 0
    hv, _ = three_piece_values((n, n), rng)
    hv = np.triu(hv) + np.triu(hv, 1).T
    H = np.where(hmask, hv, np.float32(0)).astype(np.float32)
    assert np.array_equal(H, H.T)
    for piece, size in zip(split3(H), (1.5, 2.0 ** -9, 2.0 ** -19)):
        assert np.array_equal(np.abs(piece).astype(np.float64), np.where(hmask, size, 0.0))
    if not symmetric:
        ii, jj = np.nonzero(np.triu(hmask, 1))
        pick = len(ii) // 2
        H[ii[pick], jj[pick]] = -H[ii[pick], jj[pick]]
        assert not np.array_equal(H, H.T) and np.array_equal(np.abs(H), np.abs(H.T))
    v, a = six_term(W.T, H), six_term_abs(W.T, H)
    assert exact_in_float32(v, a, 2.0 ** -20) and a.max() < 16.0, (R, n, a.max())
    return frozen(W), frozen(H)


@functools.lru_cache(maxsize=None)
def block_gaussian(T, n, seed):
    """Random float32 data with a scale per feature in 0.5 .. 1.5."""
    rng = np.random.default_rng(seed)
    return frozen((rng.standard_normal((T, n)) * (0.5 + rng.random(n))).astype(np.float32))


# ------------------------------------------------------------------------------------------------ the sharp random figure
def unit(X, count_after):
    """u = 2^-24 (|X|^T |X|) / c': one rounding of the magnitude of an entry's terms."""
    A = np.abs(X.astype(np.float64))
    return 2.0 ** -24 * (A.T @ A) / count_after


def figure(H, X, count_after):
    """max |H - H64| / u for a first batch (H64 = X^T X / c' in float64)."""
    X64 = X.astype(np.float64)
    u = unit(X, count_after)
    d = np.abs(np.asarray(H, np.float64) - X64.T @ X64 / count_after)
    return float((d[u > 0] / u[u > 0]).max())


def float32_chain(X):
    """X^T X as a float32 MFMA forms it: one fused multiply-add per token, in token order, rounded to float32 each time
    (the product is exact in float64; the second rounding of the sum is below 2^-29 of a step and does not show)."""
    X64 = X.astype(np.float64)
    acc = np.zeros((X.shape[1], X.shape[1]), np.float32)
    for t in range(X.shape[0]):
        acc = (acc.astype(np.float64) + np.outer(X64[t], X64[t])).astype(np.float32)
    return acc


def six_term_chain(X, terms=SIX, pad_to=None, drop_token=None, swap_features=None):
    """X^T X as the bfloat16 MFMA forms it, simulated: per 16 tokens and per piece pair (in the order of `terms`) one exact
    16-term dot product added to the float32 accumulator with one rounding.  Mutations as in accumulate_model."""
    Xp = X
    if swap_features is not None:
        a, b = swap_features
        Xp = X.copy()
        Xp[:, [a, b]] = X[:, [b, a]]
    if drop_token is not None:
        Xp = np.delete(Xp, drop_token, axis=0)
    if pad_to and Xp.shape[0] % pad_to:
        Xp = np.concatenate([Xp, np.repeat(Xp[-1:], pad_to - Xp.shape[0] % pad_to, axis=0)])
    p = [q.astype(np.float64) for q in split3(Xp)]
    acc = np.zeros((X.shape[1], X.shape[1]), np.float32)
    for t0 in range(0, Xp.shape[0], 16):
        for a, b in terms:
            acc = (acc.astype(np.float64) + p[a - 1][t0:t0 + 16].T @ p[b - 1][t0:t0 + 16]).astype(np.float32)
    return acc


def finish(v, count_after):
    """A first batch's H from its product: fl(0 + fl(v / cnt))."""
    return (np.asarray(v, np.float32) / np.float32(count_after)).astype(np.float32)


# --------------------------------------------------------------------------------------------------------- mismatch report
def first_difference(got, want):
    """(i, j) of the first entry whose bits differ, or None."""
    g, w = np.ascontiguousarray(got, np.float32).view(np.uint32), np.ascontiguousarray(want, np.float32).view(np.uint32)
    bad = np.argwhere(g != w)
    return None if len(bad) == 0 else tuple(int(x) for x in bad[0])


def explain_mismatch(got, want, without_term):
    """'' when got == want bit for bit; otherwise the first differing entry, how many differ, and the single missing piece
    pair that would explain the value found there, if one does.  without_term(pair) -> the model with that pair dropped."""
    at = first_difference(got, want)
    if at is None:
        return ""
    n_bad = int((np.ascontiguousarray(got, np.float32).view(np.uint32) != np.ascontiguousarray(want, np.float32).view(np.uint32)).sum())
    text = f"first difference at {at}: got {float(np.asarray(got)[at])!r}, model {float(np.asarray(want)[at])!r}; {n_bad} entries differ"
    fits = []
    for pair in SIX:
        alt = np.asarray(without_term(pair), np.float32)
        if alt[at].view(np.uint32) == np.asarray(got, np.float32)[at].view(np.uint32):
            fits.append((pair, bool(first_difference(got, alt) is None)))
    if fits:
        text += "; " + ", ".join(f"a missing term a{p} b{q} gives this value" + (" and the whole matrix" if whole else "")
                                 for (p, q), whole in fits)
    else:
        text += "; no single missing term gives this value"
    return text
