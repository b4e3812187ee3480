"""NumPy builders and comparators for the tests of the factorisation ("What the factor tests hold").

TEST INFRASTRUCTURE ONLY.  Everything here is plain NumPy (the comparators also take torch tensors, so that the GPU tests
can evaluate them with float64 products on the device); nothing reads the library.

  exact_case        matrices whose factor U (upper, U^T U = M^-1) is known in closed form, every number the factorisation
                    can form being a small integer or a power of two times one
  tiled_factor      a tiled right-looking model of the factorisation (64-wide panels, tree inverse, flip) with a switch that
                    corrupts it: what proves that the exact comparison names a wrong tile
  first_bad_pivot   the status word's definition, by bisection with LAPACK; first_bad_pivot_loop: the plain loop
  hard_hessian, reference, residual, forward_error, tile_diff ...
"""

import numpy as np

from oracle import obq_ref
from sleekit_amd import synth

TILE = 64


# --------------------------------------------------------------------------- matrices with a closed-form factor
def _off_grid(x, n):
    """x moved off every multiple of 64 (hence of 256 and 512) where the width leaves room."""
    if n > 8 and x % TILE == 0:
        x += 7
    return min(x, n)


def exact_case(n, seed, scaled=False, dense=True):
    """M = V V^T with V = Bd (I + N) [diag(d)] upper triangular, and its factor U = V^-1 in closed form.

    Bd = I + diag(s, 1), s in {-1, +1}: its inverse is triu(outer(1 / c, c)), c = [1, cumprod(-s)] -- dense, every entry +-1.
    N  = zero except N[:h0, h1:] (h0 <= h1) from {-1, 0, 1}: N N = 0, so (I + N)^-1 = I - N.
    d  = 2^e, e in {-2 .. 2} (scaled) or ones: V <- V diag(d), U <- diag(1 / d) U.
    dense=False leaves N out: the diagonal of the unscaled M is then 2, ..., 2, 1.
    The Cholesky factor of the index-reversed M is flip(V) exactly; its pivots are d^2 (1 unscaled).
    Returns dict(M, U, V, d, h0, h1), float64; M is exactly representable in float32 (test_factor_model_cpu holds that).
    """
    rng = np.random.default_rng(seed)
    s = rng.choice([-1.0, 1.0], size=max(n - 1, 0))
    h0, h1 = _off_grid((3 * n) // 8, n), _off_grid((5 * n) // 8, n)
    N = np.zeros((n, n))
    fill = rng.integers(-1, 2, size=(h0, n - h1)).astype(np.float64)
    if dense:
        N[:h0, h1:] = fill
    e = rng.integers(-2, 3, size=n)
    d = np.exp2(e.astype(np.float64)) if scaled else np.ones(n)
    Bd = np.eye(n) + np.diag(s, 1)
    c = np.concatenate([[1.0], np.cumprod(-s)])
    Binv = np.triu(np.outer(1.0 / c, c))
    BdN = N.copy()  # Bd N and N Bd^-1 without the n^3 products: a bidiagonal factor, and a running sum along the rows
    BdN[:-1] += s[:, None] * N[1:]
    NBinv = np.cumsum(N / c[None, :], axis=1) * c[None, :]
    V = (Bd + BdN) * d[None, :]
    U = (Binv - NBinv) / d[:, None]
    M = (V / d[None, :]) @ (V * d[None, :]).T  # (V d^-1) (V d)^T = V0 diag(d^2) V0^T without squaring d twice over
    return dict(M=M, U=U, V=V, d=d, h0=h0, h1=h1, n=n)


def with_pivot(case, k, value):
    """Copy of the case's M whose pivot at index k of the factorisation's order (row k of the index-reversed matrix, column
    n - 1 - k of M) is exactly `value` instead of d^2: one diagonal entry lowered by a number that M's grid holds exactly."""
    M = case["M"].copy()
    c = case["n"] - 1 - k
    M[c, c] -= case["d"][c] ** 2 - value
    return M


# --------------------------------------------------------------------------- plain non-pivoting pieces
@np.errstate(all="ignore")  # (past a pivot that is not > 0 the numbers are void and may overflow)
def potf2(T):
    """Unblocked right-looking Cholesky of the lower triangle of T, in place, the way the diagonal-tile kernels treat a pivot
    that is not > 0: note the first one, go on with 1.  Returns its index or None."""
    m = T.shape[0]
    bad = None
    for j in range(m):
        piv = T[j, j]
        if not piv > 0.0:
            bad = j if bad is None else bad
            piv = 1.0
        T[j:, j] = T[j:, j] / np.sqrt(piv)
        T[j + 1:, j + 1:] -= np.outer(T[j + 1:, j], T[j + 1:, j])
    T[...] = np.tril(T)
    return bad


@np.errstate(all="ignore")  # (past a pivot that is not > 0 the numbers are void and may overflow)
def inverse_lower(L):
    """Inverse of a lower triangular matrix without pivoting: recursive halves, forward substitution at the leaves."""
    m = L.shape[0]
    if m <= 32:
        X = np.zeros_like(L)
        for i in range(m):
            X[i, i] = 1.0 / L[i, i]
            X[i, :i] = -(L[i, :i] @ X[:i, :i]) / L[i, i]
        return X
    h = m // 2
    X = np.zeros_like(L)
    X[:h, :h] = inverse_lower(L[:h, :h])
    X[h:, h:] = inverse_lower(L[h:, h:])
    X[h:, :h] = -X[h:, h:] @ (L[h:, :h] @ X[:h, :h])
    return X


def inverse_factor_plain(M):
    """obq_ref.inverse_factor_upper with the plain inverse above in place of np.linalg.inv (which pivots)."""
    L = np.linalg.cholesky(np.flip(M))
    return np.ascontiguousarray(np.flip(inverse_lower(L)))


def first_bad_pivot_loop(P):
    """Index k, in the order of the factorisation (row k of flip(P)), of the first pivot that is not > 0; None if there is
    none.  The plain unblocked loop."""
    return potf2(np.tril(np.flip(P)).astype(np.float64))


def first_bad_pivot(P):
    """The same by bisection: the leading k x k minor of flip(P) has a Cholesky factor iff its pivots 0 .. k-1 are all > 0
    (LAPACK's potrf stops at a pivot that is <= 0 or NaN; a build of it that lets a NaN through leaves it on the factor's
    diagonal, which counts as stopping).  info - 1 of the library's status word."""
    A = np.flip(P)
    n = A.shape[0]

    def fails(m):
        try:
            return not np.isfinite(np.diag(np.linalg.cholesky(A[:m, :m]))).all()
        except np.linalg.LinAlgError:
            return True

    if not fails(n):
        return None
    lo, hi = 0, n  # minor lo passes (the empty one does), minor hi fails
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if fails(mid) else (mid, hi)
    return hi - 1


# --------------------------------------------------------------------------- a tiled model that can be corrupted
@np.errstate(all="ignore")  # (past a pivot that is not > 0 the numbers are void and may overflow)
def tiled_factor(M, corrupt=None):
    """(U, info) by the factorisation's own scheme in NumPy: A = lower triangle of flip(M) padded with an identity block to
    whole 64 x 64 tiles; per panel the diagonal tile's unblocked Cholesky, L21 = A21 inv(L11)^T, the trailing update one
    64-wide slice of K at a time; X = inv(L) without pivoting; U[i][j] = X[n-1-i][n-1-j].  info as the library's status word.

    corrupt (None: a correct model) is one of
      ("drop_k", p, ti, tj)          panel p's slice of K is left out of the trailing update of tile (ti, tj) of A
      ("swap", (ti, tj), (ui, uj))   two (whole) tiles of U change places
      ("transpose", (ti, tj))        one (whole) tile of U is transposed
    """
    n = M.shape[0]
    ld = (n + TILE - 1) // TILE * TILE
    nt = ld // TILE
    A = np.eye(ld)
    A[:n, :n] = np.tril(np.flip(M))
    info = 0
    for p in range(nt):
        k0, k1 = p * TILE, (p + 1) * TILE
        bad = potf2(A[k0:k1, k0:k1])
        if bad is not None and info == 0:
            info = k0 + bad + 1
        if k1 == ld:
            break
        A[k1:, k0:k1] = A[k1:, k0:k1] @ inverse_lower(A[k0:k1, k0:k1]).T
        L21 = A[k1:, k0:k1]
        update = L21 @ L21.T
        if corrupt is not None and corrupt[0] == "drop_k" and corrupt[1] == p:
            ti, tj = corrupt[2], corrupt[3]
            assert ti >= tj > p
            update[(ti - p - 1) * TILE:(ti - p) * TILE, (tj - p - 1) * TILE:(tj - p) * TILE] = 0.0
        A[k1:, k1:] -= np.tril(update)
    U = np.ascontiguousarray(np.flip(inverse_lower(A)[:n, :n]))

    def tile(t):
        return slice(t[0] * TILE, (t[0] + 1) * TILE), slice(t[1] * TILE, (t[1] + 1) * TILE)

    if corrupt is not None and corrupt[0] == "swap":
        a, b = tile(corrupt[1]), tile(corrupt[2])
        U[a], U[b] = U[b].copy(), U[a].copy()
    if corrupt is not None and corrupt[0] == "transpose":
        a = tile(corrupt[1])
        U[a] = U[a].T.copy()
    return U, info


# --------------------------------------------------------------------------- comparators
def tile_diff(got, want):
    """(number of 64 x 64 tiles in which got != want somewhere, coordinates of the first such tile in row-major order or
    None).  A NaN differs from everything."""
    n = want.shape[0]
    nt = (n + TILE - 1) // TILE
    ne = np.zeros((nt * TILE, nt * TILE), dtype=bool)
    ne[:n, :n] = np.asarray(got) != np.asarray(want)
    per_tile = ne.reshape(nt, TILE, nt, TILE).any(axis=(1, 3))
    where = np.argwhere(per_tile)
    return int(per_tile.sum()), (tuple(int(v) for v in where[0]) if len(where) else None)


def assert_lower_is_plus_zero(U, what="U"):
    low = np.tril(np.asarray(U), -1)
    assert not low.any() and not np.signbit(low).any(), f"{what}: the part below the diagonal is not +0.0 throughout"


def assert_exact(got, want, what="U"):
    """got == want element for element and +0.0 below the diagonal; names the first wrong tile otherwise."""
    got = np.asarray(got)
    count, first = tile_diff(got, want)
    if count:
        ti, tj = first
        a = got[ti * TILE:(ti + 1) * TILE, tj * TILE:(tj + 1) * TILE]
        b = want[ti * TILE:(ti + 1) * TILE, tj * TILE:(tj + 1) * TILE]
        with np.errstate(invalid="ignore"):
            worst = np.nanmax(np.abs(a - b)) if not np.isnan(a - b).all() else float("nan")
        raise AssertionError(f"{what}: {count} tile(s) of 64 x 64 differ from the closed form, the first is tile {first} "
                             f"(max |difference| there {worst:.6g})")
    assert_lower_is_plus_zero(got, what)


def _index(Z, n):
    if isinstance(Z, np.ndarray):
        return np.arange(n)
    import torch

    return torch.arange(n, device=Z.device)


def residual(U, P):
    """max |U^T U P - I| in float64 (NumPy arrays, or torch tensors on one device): the factor's defining property."""
    n = P.shape[0]
    Z = U.T @ (U @ P)
    i = _index(Z, n)
    Z[i, i] -= 1.0
    return float(abs(Z).max())


def forward_error(U, U_ref):
    """max |U - triu(U_ref)| / max |U_ref| (NumPy arrays or torch tensors)."""
    upper = np.triu(U_ref) if isinstance(U_ref, np.ndarray) else U_ref.triu()
    return float(abs(U - upper).max()) / float(abs(U_ref).max())


FORWARD_BOUND = 1e-9   # the bound of test_order_and_factor
RESIDUAL_BOUND = 1e-8  # likewise
HARD_RATIO = 4.0       # resid(U) <= 4 resid(U_ref) on the hard matrices (DESIGN.md gives the reasons for 4)


def check_forward(U, U_ref):
    err = forward_error(U, U_ref)
    assert err <= FORWARD_BOUND, f"max |U - U_ref| = {err:.3g} max |U_ref|, bound {FORWARD_BOUND:g}"
    return err


def check_residual(U, P):
    err = residual(U, P)
    assert err < RESIDUAL_BOUND, f"max |U^T U P - I| = {err:.3g}, bound {RESIDUAL_BOUND:g}"
    return err


def check_hard(U, U_ref, P):
    """resid(U) <= 4 resid(U_ref), both by the same float64 expression on the same P.  Returns (ratio, resid, resid_ref)."""
    got, ref = residual(U, P), residual(U_ref, P)
    assert got <= HARD_RATIO * ref, f"residual {got:.3g} is {got / ref:.2f} times the reference's {ref:.3g} (bound {HARD_RATIO:g})"
    return got / ref, got, ref


# --------------------------------------------------------------------------- float64 references of damped Hessians
def reference(H, damp):
    """(order, P, U_ref) of a float32 Hessian as the reference forms them (obq_ref.quantize_layer): the float32 damping term,
    the order by the damped diagonal with exact ties broken by index (what the device does), P = Hd[order][:, order] in
    float64 and its factor by LAPACK."""
    n = H.shape[0]
    Hd = H + damp * H.diagonal().mean() * np.eye(n)
    order = obq_ref.column_order(None, Hd, None, "diag", ties="stable")
    P = np.ascontiguousarray(Hd[order][:, order])
    return order, P, np.array(obq_ref.inverse_factor_upper(P))  # (a copy: a flipped 1 x 1 matrix keeps its negative strides)


def hard_hessian(n, seed, graded=False):
    """float32 Hessian of T = n / 4 tokens (rank-deficient before damping); graded: H <- D H D with D = exp(uniform(-3, 3))
    in float32, the products in float64 so that H stays bit-wise symmetric."""
    H = synth.make_hessian(n, seed, T=n // 4)[0]
    if graded:
        D = np.exp(np.random.default_rng(seed).uniform(-3.0, 3.0, n)).astype(np.float32).astype(np.float64)
        H = (H.astype(np.float64) * D[:, None] * D[None, :]).astype(np.float32)
    return H


def perturbed(U_ref, rel=1e-6):
    """Copy of U_ref with its largest element moved by `rel` of itself."""
    U = np.triu(U_ref)
    i, j = np.unravel_index(np.abs(U).argmax(), U.shape)
    U[i, j] *= 1.0 + rel
    return U


# --------------------------------------------------------------------------- the multi-GPU payload
def payload_words(n):
    return n * (n + 1) // 2 + n + 1


def payload_of(U, order, info):
    """int64 words [info, order, rows of the upper triangle of U] (include/sleekit_amd.h, slk_factor_pack)."""
    n = U.shape[0]
    bits = np.ascontiguousarray(U).view(np.int64)
    tri = np.concatenate([bits[i, i:] for i in range(n)])
    return np.concatenate([np.array([info], dtype=np.int64), np.asarray(order, dtype=np.int64), tri])


def payload_case(n, seed):
    """A random upper triangular U that also holds -0.0 and a NaN bit pattern (compare as int64), and a random permutation."""
    rng = np.random.default_rng(seed)
    U = np.triu(rng.standard_normal((n, n)))
    U[0, n - 1] = -0.0
    U[n // 2, n // 2] = np.array([0x7FF8DEADBEEF0001], dtype=np.uint64).view(np.float64)[0]
    return U, rng.permutation(n).astype(np.int64)
