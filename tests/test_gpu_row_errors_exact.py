"""The row errors of the layer error, bit for bit on exact inputs, over every route between its two kernels.

W, Q and H are small integers, so that every product and every partial sum of rowsum(((W - Q) H) * (W - Q)), in any
order and with the rows under the diagonal band counted twice, is an integer below 2^24: float32 holds it exactly, each
operand fits the first bfloat16 piece (the other two are zero), and the reference is int64 NumPy.  The other tests hold
the row errors to rtol 1e-5 / 2e-6; this one leaves no room for a term counted once too often or a guard off by one.

H = S is the symmetric case; H = S + A with A antisymmetric the one that is not, with (H + H^T) / 2 = S exactly -- what
the averaged planes hold -- and a nonzero of A in every 128 x 128 tile on or above the diagonal.
"""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# (rows, columns) of the single-layer calls:
#   130 x 256  two row tiles, the second with two live rows; two column tiles, so tile 1 has rows under its band
#   130 x 200  the float32 kernel's guarded loads with the symmetric split (ksplit 128, kend 208)
#   256 x 256  the float32 kernel's interior branch with the split (under no_bf16_error)
SHAPES = [(130, 256), (130, 200), (256, 256)]
BATCH, BATCH_ROWS, BATCH_N = 2, 128, 256  # two layers stacked by rows: the first Hessian symmetric, the second not

ROUTES = {
    "default": {},
    "no_bf16_dma": {"SLK_NO_BF16_DMA": 1},
    "no_bf16_error": {"SLK_NO_BF16_ERROR": 1},
    "no_sym_error": {"SLK_NO_SYM_ERROR": 1},
    "error_cb2": {"SLK_ERROR_CB": 2},
    "error_cb8": {"SLK_ERROR_CB": 8},
    "no_error_splitk": {"SLK_NO_ERROR_SPLITK": 1},
    "no_sym_average": {"SLK_NO_SYM_AVERAGE": 1},
    "no_sym_average_no_bf16_asym": {"SLK_NO_SYM_AVERAGE": 1, "SLK_NO_BF16_ASYM": 1},
}
G_ROUTES = {"default": {}, "no_bf16_asym": {"SLK_NO_BF16_ASYM": 1}}


def _hessians(rng, n):
    low = np.tril(rng.integers(-4, 5, size=(n, n)))
    S = low + np.tril(low, -1).T
    up = np.triu(rng.integers(-2, 3, size=(n, n)), 1)
    A = up - up.T
    return S.astype(np.int64), A.astype(np.int64)


def _layer(rng, R, n):
    W = rng.integers(-5, 6, size=(R, n))
    D = rng.integers(-3, 4, size=(R, n))
    return W.astype(np.int64), (W - D).astype(np.int64)


def _check_inputs(W, Q, S, A):
    """The bound the exactness rests on, asserted on the inputs themselves."""
    D, n = W - Q, S.shape[0]
    assert np.abs(D).max() <= 3 and np.abs(S).max() <= 4 and np.abs(A).max() <= 2
    assert np.array_equal(S, S.T) and np.array_equal(A, -A.T)
    for bi in range(0, n, 128):
        for bj in range(bi, n, 128):
            assert np.triu(A, 1)[bi:bi + 128, bj:bj + 128].any(), "a tile above the diagonal without a nonzero of A"
    for H in (S, S + A):
        assert np.array_equal((H + H.T) // 2, S) and np.array_equal((H + H.T) % 2, np.zeros_like(H))
        # every partial sum of the product, doubled, and of the row sum over it, in any order
        assert 2 * (((np.abs(D) @ np.abs(H)) * np.abs(D)).sum(axis=1).max()) < 2 ** 24
    for x in (W, Q, S, S + A):  # eight significant bits: the first bfloat16 piece
        assert np.abs(x).max() < 256


def _reference(W, Q, H):
    D = W - Q
    G = D @ H
    return (G * D).sum(axis=1), G


@pytest.fixture(scope="module")
def engine():
    assert torch.cuda.is_available(), "these tests need the GPU"
    from sleekit_amd import engine

    return engine


@pytest.fixture(scope="module")
def cases():
    rng = np.random.default_rng(2901)
    dev = lambda x: torch.from_numpy(x.astype(np.float32)).cuda()  # noqa: E731
    single = []
    for R, n in SHAPES:
        (W, Q), (S, A) = _layer(rng, R, n), _hessians(rng, n)
        _check_inputs(W, Q, S, A)
        for name, H in (("symmetric", S), ("not symmetric", S + A)):
            err, G = _reference(W, Q, H)
            single.append((f"{R} x {n}, H {name}", dev(W), dev(Q), dev(H), err.astype(np.float32), G.astype(np.float32)))
    W, Q = _layer(rng, BATCH * BATCH_ROWS, BATCH_N)
    S, A = _hessians(rng, BATCH_N)
    _check_inputs(W, Q, S, A)
    Hs = [S, S + A]
    err = np.stack([_reference(W[b * BATCH_ROWS:(b + 1) * BATCH_ROWS], Q[b * BATCH_ROWS:(b + 1) * BATCH_ROWS], Hs[b])[0] for b in range(BATCH)])
    shape = (BATCH, BATCH_ROWS, BATCH_N)
    batch = (dev(W).reshape(shape).contiguous(), dev(Q).reshape(shape).contiguous(), [dev(H) for H in Hs], err.astype(np.float32))
    return single, batch


def _set(slkopt, options):
    for name, value in options.items():
        slkopt.setenv(name, str(value))


@pytest.mark.parametrize("route", list(ROUTES))
def test_row_errors_exact(engine, slkopt, cases, route):
    """slk_row_errors on every shape and both Hessians under one route: the int64 row errors, bit for bit."""
    _set(slkopt, ROUTES[route])
    for what, W, Q, H, err, _ in cases[0]:
        got = engine.row_errors(W, Q, H).cpu().numpy()
        assert np.array_equal(got, err), f"{what}, {route}: {np.flatnonzero(got != err)[:8]}"


@pytest.mark.parametrize("route", list(G_ROUTES))
def test_row_errors_and_product_exact(engine, slkopt, cases, route):
    """... and with the product G = (W - Q) H wanted: both exact."""
    _set(slkopt, G_ROUTES[route])
    for what, W, Q, H, err, G in cases[0]:
        got, got_G = engine.row_errors(W, Q, H, want_G=True)
        assert np.array_equal(got_G.cpu().numpy(), G), f"G: {what}, {route}"
        assert np.array_equal(got.cpu().numpy(), err), f"{what}, {route}"


@pytest.mark.parametrize("route", list(ROUTES))
def test_row_errors_batch_exact(engine, slkopt, cases, route):
    """slk_row_errors_batch, the layers' flags and planes their own: the first Hessian symmetric, the second not; with
    the verdicts formed inside the call and handed in."""
    _set(slkopt, ROUTES[route])
    W, Q, Hs, err = cases[1]
    got = engine.row_errors_batch(W, Q, Hs).cpu().numpy()
    assert np.array_equal(got, err), f"{route}: {np.argwhere(got != err)[:8]}"
    flags = torch.cat([engine.symmetry_flag(H) for H in Hs])
    assert flags.tolist() == [1, 0]
    got = engine.row_errors_batch(W, Q, Hs, symmetric=flags).cpu().numpy()
    assert np.array_equal(got, err), f"{route}, verdicts handed in: {np.argwhere(got != err)[:8]}"
