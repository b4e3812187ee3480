"""NumPy model of the expert-grouped running statistics (slk_hessian_accumulate_experts, slk_hessian_accumulate_experts_mx,
sleekit_amd.ExpertStatistics), written from the documented rules alone.

Offsets rule (tests/mx_experts_model.py): offsets[0] == 0, never decreasing, offsets[E] == M.  Where it holds, every expert e
with T_e = offsets[e + 1] - offsets[e] > 0 rows gets stats_model.accumulate_model on its slice X[offsets[e] : offsets[e + 1]]
with count_before = counts[e] (`pieces=True, chunk=None` for the bfloat16 x 3 path: the grouped entry never chunks), and
counts[e] += T_e; an expert without rows keeps its H, mean and count as the very same bits.  Where it does not hold nothing
changes and the flag is 1.  For MX-coded rows the slice is first decoded by the NumPy models of the three formats
(mx_gemm_model, mx_act4_model, mx_act6_model) and the product is the plain one.

As in stats_model.py, the keyword arguments after `pieces` are MUTATIONS -- each gives what a kernel with one particular mistake
would compute -- and tests/test_expert_stats_cpu.py runs every comparison of tests/test_gpu_expert_stats.py against them.  The
shapes of the GPU tests live here for that reason.
"""

import functools

import numpy as np

import mx_act4_model
import mx_act6_model
import mx_experts_model
import mx_gemm_model
import stats_model
from mx_experts_model import offsets_of, offsets_valid  # noqa: F401  (the offsets rule has one model)

# ---- the shapes of tests/test_gpu_expert_stats.py
EXACT_COUNTS = ((0, 1, 17, 33, 0, 64), (5, 0, 17, 0, 3, 40))  # two batches: experts 1 and 3 are empty in the second, 0 and 4 in the first
EXACT_F32_N = (130, 260)
EXACT_BF16_N = (128, 256)
BIG_COUNT = 2 ** 31 + 5
BIG_COUNT_EXPERT = 2
RANDOM_COUNTS, RANDOM_N = (15, 0, 47, 130), 256
CODED_COUNTS, CODED_N = (0, 1, 15, 33, 64), (32, 160)
CODED_SCALE_BYTES = (125, 129)
RANDOM_CODED_COUNTS, RANDOM_CODED_N, RANDOM_CODED_SCALE_BYTES = (130, 0, 7, 65), 160, (100, 150)
FORMATS = ("mxfp8", "mxfp4", "mxfp6_e2m3")
BROKEN_OFFSETS = {"first is not 0": lambda o: o + np.array([1] + [0] * (len(o) - 1), np.int32),
                  "a decrease": lambda o: np.concatenate([o[:2], [o[1] - 1], o[3:]]).astype(np.int32),
                  "last is not M": lambda o: o - np.array([0] * (len(o) - 1) + [1], np.int32)}
SENTINEL = np.uint32(0x7fc12345).view(np.float32)  # a NaN with a payload: any arithmetic on it changes its bits or spreads it


def accumulate_experts_model(H, mean, counts, X, offsets, pieces=False, *, exact=False, slice_from_next=False, factor_from=None,
                             scale_empty=False, counts_not_advanced=False, token_past_bound=False):
    """(H' (E, n, n), mean' (E, n), counts' (E,), flag) after one batch X (M, n) sorted by expert under `offsets`.

    Mutations: `slice_from_next`: expert e's slice begins at expert e + 1's first row (the last expert's at its own);
    `factor_from` "next": f and cnt are those of expert (e + 1) % E, "M": c' = c + M; `scale_empty`: an expert without rows is
    scaled by its f = c / (c + 0), which is 0 / 0 for an expert never seen; `counts_not_advanced`; `token_past_bound`: the row
    at offsets[e + 1], when there is one, is taken as one of expert e's."""
    H, mean = np.array(H, np.float32), np.array(mean, np.float32)
    counts = np.array(counts, np.int64)
    X = np.ascontiguousarray(X, dtype=np.float32)
    M, E = X.shape[0], len(counts)
    if len(offsets) != E + 1 or not offsets_valid(offsets, M):
        return H, mean, counts, 1
    before = counts.copy()
    for e in range(E):
        lo, hi = int(offsets[e]), int(offsets[e + 1])
        T = hi - lo
        if T == 0:
            if scale_empty:
                with np.errstate(invalid="ignore", divide="ignore"):
                    f = np.float32(np.float64(before[e]) / np.float64(before[e]))
                    H[e], mean[e] = (H[e] * f).astype(np.float32), (mean[e] * f).astype(np.float32)
            continue
        if slice_from_next and e + 1 < E:
            lo = min(int(offsets[e + 1]), M - T)
            hi = lo + T
        if token_past_bound and hi < M:
            hi += 1
        Xs = X[lo:hi]
        if factor_from is None:
            He, me = stats_model.accumulate_model(H[e], mean[e], Xs, int(before[e]), chunk=None, pieces=pieces, exact=exact)
        else:
            o = (e + 1) % E
            c, after = (int(before[o]), int(before[o]) + int(offsets[o + 1]) - int(offsets[o])) if factor_from == "next" else \
                (int(before[e]), int(before[e]) + M)
            with np.errstate(invalid="ignore", divide="ignore"):
                f, cnt = np.float32(np.float64(c) / np.float64(after)), np.float32(after)
                v = stats_model.six_term(Xs, Xs) if pieces else Xs.astype(np.float64).T @ Xs.astype(np.float64)
                He = ((H[e] * f).astype(np.float32) + (v.astype(np.float32) / cnt).astype(np.float32)).astype(np.float32)
                s = Xs.astype(np.float64).sum(axis=0).astype(np.float32)
                me = ((mean[e] * f).astype(np.float32) + (s / cnt).astype(np.float32)).astype(np.float32)
        H[e], mean[e] = He, me
        if not counts_not_advanced:
            counts[e] = before[e] + T
    return H, mean, counts, 0


def decode(a_codes, a_scales, activations, scale_from_neighbour=False):
    """The de-quantized rows (M, n) as float64: value(code) 2^(b - 127).  Mutation `scale_from_neighbour`: block k of a row takes
    the scale byte of block (k + 1) % blocks."""
    a_scales = np.asarray(a_scales)
    if scale_from_neighbour:
        a_scales = np.roll(a_scales, -1, axis=1)
    return np.asarray(mx_experts_model.DEQUANTIZE_ACT[activations](np.asarray(a_codes), a_scales), np.float64)


def accumulate_codes_model(H, mean, counts, a_codes, a_scales, offsets, activations, *, scale_from_neighbour=False, **mutation):
    """accumulate_experts_model on the decoded rows (they are float32 -- bfloat16 -- values exactly); flag 2 stands for a scale
    byte 255 among the rows."""
    X64 = decode(a_codes, a_scales, activations, scale_from_neighbour)
    X = X64.astype(np.float32)
    nan = bool((np.asarray(a_scales) == 255).any())
    assert nan or np.array_equal(X.astype(np.float64), X64)
    with np.errstate(all="ignore" if nan else "warn"):  # (a byte 255 stands for NaN; this model only reports it)
        Hn, mn, cn, flag = accumulate_experts_model(H, mean, counts, X, offsets, **mutation)
    return Hn, mn, cn, (2 if nan and not flag else flag)


def zero_state(E, n):
    return np.zeros((E, n, n), np.float32), np.zeros((E, n), np.float32), np.zeros(E, np.int64)


def run_batches(batches, E, n, start_counts=None, pieces=False, **mutation):
    """State after the (X, offsets) batches on top of zero statistics (and `start_counts`)."""
    H, mean, counts = zero_state(E, n)
    if start_counts is not None:
        counts = np.array(start_counts, np.int64)
    for X, offsets in batches:
        H, mean, counts, flag = accumulate_experts_model(H, mean, counts, X, offsets, pieces=pieces, **mutation)
        assert flag == 0
    return H, mean, counts


def same_state(a, b):
    """Bit for bit: H, mean (float32 bits) and counts."""
    return stats_model.same_bits(a[0], b[0]) and stats_model.same_bits(a[1], b[1]) and np.array_equal(np.asarray(a[2], np.int64), np.asarray(b[2], np.int64))


def bitwise_symmetric(H):
    H = np.ascontiguousarray(H, np.float32).view(np.uint32)
    return bool(np.array_equal(H, np.swapaxes(H, -1, -2)))


# --------------------------------------------------------------------------------------------------------------- builders
@functools.lru_cache(maxsize=None)
def exact_batches(n, pieces):
    """The two batches of the exact float test: (X, offsets) each, X `integers` (float32 chain) or `three_piece` (bfloat16 x 3,
    so that the six terms are told apart), whose products stats_model asserts exact in float32."""
    out = []
    for b, counts in enumerate(EXACT_COUNTS):
        M = sum(counts)
        X = stats_model.three_piece(M, n, 40 + b, modulus=32) if pieces else stats_model.integers(M, n, 40 + b)
        out.append((X, stats_model.frozen(offsets_of(counts))))
    return tuple(out)


# columns of a format fall into classes of two neighbouring exponents, so that the terms of one entry of X^T X have one size:
# (codes of the class without sign, quantum of its values, a strict bound of their magnitudes)
def _classes(activations):
    if activations == "mxfp8":  # exponent fields 2 c and 2 c + 1; 0x7f is E4M3's NaN and no value
        out = []
        for c in range(8):
            codes = [k for k in range(16 * c, 16 * c + 16) if k != 0x7f]
            e = max(2 * c, 1) - 7
            out.append((codes, 2.0 ** (e - 3), 2.0 ** (e + 2)))
        return out
    if activations == "mxfp6_e2m3":
        return [(list(range(0, 16)), 2.0 ** -3, 2.0), (list(range(16, 32)), 2.0 ** -2, 8.0)]
    return [(list(range(8)), 0.5, 8.0)]


SIGN = {"mxfp8": 0x80, "mxfp4": 0x8, "mxfp6_e2m3": 0x20}
PACK = {"mxfp8": lambda c: c.astype(np.uint8), "mxfp4": mx_act4_model.pack_nibbles, "mxfp6_e2m3": mx_act6_model.pack_codes}
ELEMENT_CODES = {"mxfp8": sorted(set(range(256)) - {0x7f, 0xff}), "mxfp4": list(range(16)), "mxfp6_e2m3": list(range(64))}


@functools.lru_cache(maxsize=None)
def exact_codes(activations, n, seed=7):
    """(a_codes, a_scales, X float64 (M, n)) for CODED_COUNTS: scale bytes drawn from CODED_SCALE_BYTES, every element code of the
    format that is a value present (E4M3's two NaN codes are none), column j's codes of class j % classes.  Asserted: the
    float64 product of every expert's rows, and their column sums, are exact in float32 in any order of summation."""
    rng = np.random.default_rng(seed)
    M = sum(CODED_COUNTS)
    classes = _classes(activations)
    cls = np.arange(n) % len(classes)
    codes = np.zeros((M, n), np.uint8)
    for k, (members, _, _) in enumerate(classes):
        cols = np.nonzero(cls == k)[0]
        pick = rng.integers(0, len(members), size=(M, len(cols)))
        sign = rng.integers(0, 2, size=(M, len(cols))) * SIGN[activations]
        codes[:, cols] = np.array(members, np.uint8)[pick] | sign.astype(np.uint8)
    assert set(np.unique(codes).tolist()) == set(ELEMENT_CODES[activations]), "every element code must be present"
    scales = rng.integers(CODED_SCALE_BYTES[0], CODED_SCALE_BYTES[1] + 1, size=(M, n // 32)).astype(np.uint8)
    assert set(np.unique(scales).tolist()) == set(range(CODED_SCALE_BYTES[0], CODED_SCALE_BYTES[1] + 1))
    a_codes = PACK[activations](codes)
    X = decode(a_codes, scales, activations)
    q = np.array([classes[k][1] for k in cls]) * 2.0 ** (CODED_SCALE_BYTES[0] - 127)
    offsets = offsets_of(CODED_COUNTS)
    for e in range(len(CODED_COUNTS)):
        Xe = X[offsets[e]:offsets[e + 1]]
        assert stats_model.exact_in_float32(Xe.T @ Xe, np.abs(Xe).T @ np.abs(Xe), np.outer(q, q)), (activations, n, e)
        assert stats_model.exact_in_float32(Xe.sum(axis=0), np.abs(Xe).sum(axis=0), q), (activations, n, e)
    assert stats_model.exact_in_float32(X.T @ X, np.abs(X).T @ np.abs(X), np.outer(q, q)), "the dense case (E = 1) takes all rows"
    return stats_model.frozen(a_codes), stats_model.frozen(scales), stats_model.frozen(X)


@functools.lru_cache(maxsize=None)
def random_codes(activations, n=RANDOM_CODED_N, seed=11):
    """(a_codes, a_scales, X float64) for RANDOM_CODED_COUNTS: any value code, scale bytes drawn from RANDOM_CODED_SCALE_BYTES."""
    rng = np.random.default_rng(seed)
    M = sum(RANDOM_CODED_COUNTS)
    members = np.array(ELEMENT_CODES[activations], np.uint8)
    codes = members[rng.integers(0, len(members), size=(M, n))]
    scales = rng.integers(RANDOM_CODED_SCALE_BYTES[0], RANDOM_CODED_SCALE_BYTES[1] + 1, size=(M, n // 32)).astype(np.uint8)
    a_codes = PACK[activations](codes)
    return stats_model.frozen(a_codes), stats_model.frozen(scales), stats_model.frozen(decode(a_codes, scales, activations))


def coded_bound(Xe, count_after):
    """Per entry, T 2^-23 (|X|^T |X|) / c': T exact products summed in float32 in any order, each partial sum rounded once
    (T 2^-24 of the terms' magnitudes, to first order), with the factor 2 of slack the MX product tests use (K 2^-23)."""
    A = np.abs(Xe)
    return Xe.shape[0] * 2.0 ** -23 * (A.T @ A) / count_after


def coded_ratio(H, Xe, count_after):
    """max |H - H64| / bound over the entries whose bound is not 0, H64 the float64 product of the decoded rows over c'."""
    b = coded_bound(Xe, count_after)
    d = np.abs(np.asarray(H, np.float64) - Xe.T @ Xe / count_after)
    assert (d[b == 0] == 0).all()
    return float((d[b > 0] / b[b > 0]).max()) if (b > 0).any() else 0.0


def exact_products(X):
    """True when X^T X (and the column sums) of float32 rows X are exact in float32 in any order of summation: a non-zero x is
    a multiple of its lowest set bit's value, an entry's terms are multiples of the smallest product of two such units among
    them, and their magnitudes add up to less than 2^24 of it.  (Sufficient, not necessary.)"""
    X = np.asarray(X, np.float64)
    if X.shape[0] == 0:
        return True
    assert np.array_equal(X.astype(np.float32).astype(np.float64), X)
    m, e = np.frexp(np.abs(X))
    k = np.rint(m * 2.0 ** 24).astype(np.int64)
    unit = np.where(X != 0, (k & -k).astype(np.float64) * 2.0 ** (e - 24.0), np.inf)
    q = np.full((X.shape[1], X.shape[1]), np.inf)
    for t in range(X.shape[0]):
        q = np.minimum(q, np.outer(unit[t], unit[t]))
    A = np.abs(X)
    live = np.isfinite(q)
    ok = (A.T @ A)[live] < 2.0 ** 24 * q[live]
    qs = unit.min(axis=0)
    return bool(ok.all() and (A.sum(axis=0)[np.isfinite(qs)] < 2.0 ** 24 * qs[np.isfinite(qs)]).all())
