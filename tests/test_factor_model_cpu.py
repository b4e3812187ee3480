"""The builders and comparators of tests/factor_model.py, held to one another on the CPU: the closed-form factors are what
a plain factorisation gives bit for bit, the status word's two definitions agree, and every comparison that
tests/test_gpu_factor.py makes FAILS on a factor that is subtly wrong -- a slice of K left out of one trailing update, two
tiles swapped, one transposed, one element off by 1e-6 -- so that no wrong kernel has to run on a GPU to prove it."""

import numpy as np
import pytest

import factor_model as fm
from oracle import obq_ref


@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("n", [1, 2, 3, 65, 130, 1100])
def test_closed_form_is_the_plain_factor_bit_for_bit(n, scaled):
    c = fm.exact_case(n, 100 + n, scaled)
    M, U = c["M"], c["U"]
    assert np.array_equal(M, M.T) and np.array_equal(M.astype(np.float32).astype(np.float64), M)
    assert np.array_equal(U, np.triu(U)) and np.array_equal(c["V"], np.triu(c["V"]))
    grid = 16.0 if scaled else 1.0  # everything is an integer, or one over 16 (M: d^2 >= 1/16; U: products of two 1/d <= 4)
    assert np.array_equal(np.rint(M * grid), M * grid) and np.abs(M).max() * grid < 2.0**24
    assert np.array_equal(np.rint(U * grid), U * grid) and np.abs(U).max() < 2.0**14
    L = np.linalg.cholesky(np.flip(M))
    assert np.array_equal(L, np.flip(c["V"]))  # the Cholesky factor of the reversed matrix is flip(V) exactly
    assert np.array_equal(np.diag(L) ** 2, np.flip(c["d"]) ** 2)
    assert np.array_equal(fm.inverse_factor_plain(M), U)
    assert np.array_equal(U.T @ U @ M, np.eye(n))
    if n > 8:
        assert c["h0"] % 64 and c["h1"] % 64 and c["h0"] <= c["h1"]


def test_closed_form_without_the_dense_block_has_a_flat_diagonal():
    c = fm.exact_case(130, 7, dense=False)
    assert np.array_equal(np.diag(c["M"]), np.r_[np.full(129, 2.0), 1.0])
    assert np.array_equal(fm.inverse_factor_plain(c["M"]), c["U"])


@pytest.mark.parametrize("scaled", [False, True])
def test_closed_form_against_lapack(scaled):
    """np.linalg.inv pivots, so LAPACK is close to the closed form and not equal to it: the closed form is the oracle."""
    c = fm.exact_case(1100, 1200, scaled)
    want = obq_ref.inverse_factor_upper(c["M"])
    assert fm.forward_error(c["U"], want) <= 1e-9


@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("n", [130, 1100])
def test_tiled_model_is_exact_and_its_corruptions_are_named(n, scaled):
    c = fm.exact_case(n, 300 + n, scaled)
    U, info = fm.tiled_factor(c["M"])
    assert info == 0
    fm.assert_exact(U, c["U"])
    last = (n + 63) // 64 - 1
    # one 64-wide slice of K missing from one trailing update, that of the last diagonal tile of A by the panel before it (a
    # positive semidefinite term too many: still a factor, info 0, a wrong one): the last tile row of X, tile row 0 of U
    Ub, info = fm.tiled_factor(c["M"], ("drop_k", last - 1, last, last))
    assert info == 0 and np.isfinite(Ub).all()
    with pytest.raises(AssertionError, match=r"differ from the closed form, the first is tile \(0, "):
        fm.assert_exact(Ub, c["U"])
    assert fm.tile_diff(Ub, c["U"])[0] >= 1
    if n < 192:
        return
    Ub, _ = fm.tiled_factor(c["M"], ("swap", (2, 5), (3, 9)))
    with pytest.raises(AssertionError, match=r"2 tile\(s\) of 64 x 64 differ from the closed form, the first is tile \(2, 5\)"):
        fm.assert_exact(Ub, c["U"])
    Ub, _ = fm.tiled_factor(c["M"], ("transpose", (4, 11)))
    with pytest.raises(AssertionError, match=r"1 tile\(s\) of 64 x 64 differ from the closed form, the first is tile \(4, 11\)"):
        fm.assert_exact(Ub, c["U"])
    Ub, _ = fm.tiled_factor(c["M"], ("transpose", (6, 6)))  # a diagonal tile: wrong values AND a lower triangle that is not zero
    with pytest.raises(AssertionError, match=r"the first is tile \(6, 6\)"):
        fm.assert_exact(Ub, c["U"])


def test_exact_comparison_sees_a_sign_below_the_diagonal_and_a_nan():
    c = fm.exact_case(130, 5)
    U = c["U"].copy()
    U[100, 3] = -0.0
    assert np.array_equal(U, c["U"])
    with pytest.raises(AssertionError, match="below the diagonal"):
        fm.assert_exact(U, c["U"])
    U = c["U"].copy()
    U[70, 90] = np.nan
    with pytest.raises(AssertionError, match=r"1 tile\(s\).*tile \(1, 1\)"):
        fm.assert_exact(U, c["U"])


@pytest.mark.parametrize("scaled", [False, True])
def test_first_bad_pivot_against_the_plain_loop(scaled):
    n = 150
    c = fm.exact_case(n, 41, scaled)
    assert fm.first_bad_pivot(c["M"]) is None and fm.first_bad_pivot_loop(c["M"]) is None
    for k in (0, 15, 16, 63, 64, 100, n - 1):
        for value in (-1.0, 0.0, np.nan):
            M = fm.with_pivot(c, k, value)
            assert fm.first_bad_pivot(M) == k and fm.first_bad_pivot_loop(M) == k, (k, value)
            assert fm.tiled_factor(M)[1] == k + 1
    M = fm.with_pivot(c, 70, -1.0)
    M[n - 1 - 20, n - 1 - 20] -= c["d"][n - 1 - 20] ** 2 + 1.0  # a second bad pivot, at 20: the smaller index is the answer
    assert fm.first_bad_pivot(M) == 20 and fm.first_bad_pivot_loop(M) == 20 and fm.tiled_factor(M)[1] == 21
    # on a matrix that is not built for it: the loop and the bisection agree
    rng = np.random.default_rng(3)
    B = rng.standard_normal((40, 60))
    P = B @ B.T  # rank 40 < 60 ... of size 40: positive definite
    assert fm.first_bad_pivot(P) is None
    P[17, 17] = -P[17, 17]
    assert fm.first_bad_pivot(P) == fm.first_bad_pivot_loop(P) is not None


@pytest.fixture(scope="module")
def hard():
    H = fm.hard_hessian(256, 9001, graded=True)
    return (H,) + fm.reference(H, 1e-6)


def test_forward_and_residual_comparisons_fail_on_one_element_off_by_1e_6(hard):
    H, order, P, U_ref = hard
    good = np.triu(U_ref)
    assert fm.forward_error(good, U_ref) == 0.0
    ratio, got, ref = fm.check_hard(U_ref, U_ref, P)
    assert ratio == 1.0 and ref < 1e-6
    assert fm.check_hard(good, U_ref, P)[0] < 2.0  # (LAPACK's inverse leaves rounding residue below the diagonal)
    bad = fm.perturbed(U_ref, 1e-6)
    assert (bad != good).sum() == 1
    with pytest.raises(AssertionError, match="max .U - U_ref"):
        fm.check_forward(bad, U_ref)
    with pytest.raises(AssertionError, match="times the reference's"):
        fm.check_hard(bad, U_ref, P)
    # ... and on an easy matrix (T = 2 n, 1 % damping) the absolute residual bound of part 2 fails too
    from sleekit_amd import synth

    H2 = synth.make_hessian(192, 9002)[0]
    order2, P2, U2 = fm.reference(H2, 0.01)
    fm.check_forward(np.triu(U2), U2)
    assert fm.check_residual(np.triu(U2), P2) < 1e-10
    bad2 = fm.perturbed(U2, 1e-6)
    with pytest.raises(AssertionError, match="max .U - U_ref"):
        fm.check_forward(bad2, U2)
    with pytest.raises(AssertionError, match="bound 1e-08"):
        fm.check_residual(bad2, P2)


def test_comparators_take_torch_tensors(hard):
    import torch

    H, order, P, U_ref = hard
    want = fm.residual(np.triu(U_ref), P)
    got = fm.residual(torch.from_numpy(np.triu(U_ref)), torch.from_numpy(P))
    assert abs(got - want) <= 1e-3 * want
    assert fm.forward_error(torch.from_numpy(fm.perturbed(U_ref)), torch.from_numpy(U_ref)) == fm.forward_error(fm.perturbed(U_ref), U_ref)


def test_payload_model():
    U, order = fm.payload_case(5, 1)
    words = fm.payload_of(U, order, 7)
    assert len(words) == fm.payload_words(5) == 21 and words[0] == 7 and np.array_equal(words[1:6], order)
    assert words[6:11].view(np.float64).tobytes() == U[0].tobytes() and words[-1] == U.view(np.int64)[4, 4]
    assert np.signbit(U[0, 4]) and np.isnan(U[2, 2])
