"""The numpy truth of the projection and PCA tests (tests/project_truth.py) against a triple loop and
against definitions, at tiny shapes (no GPU)."""
from fractions import Fraction

import numpy as np
import pytest

import project_truth as PT


@pytest.mark.parametrize("n,d,k", [(1, 1, 1), (3, 2, 2), (4, 5, 3), (7, 3, 1)])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_product_against_a_triple_loop(n, d, k, dtype):
    rng = np.random.default_rng(n * 100 + d * 10 + k)
    X = rng.standard_normal((n, d)).astype(dtype)
    B = rng.standard_normal((d, k))
    T, A = PT.project_truth(X, B)
    assert T.dtype == np.longdouble and T.shape == (n, k) and A.shape == (n, k)
    for r in range(n):
        for j in range(k):
            exact = sum(Fraction(float(X[r, i])) * Fraction(float(B[i, j])) for i in range(d))
            mags = sum(abs(Fraction(float(X[r, i])) * Fraction(float(B[i, j]))) for i in range(d))
            assert abs(Fraction(float(T[r, j])) - exact) <= Fraction(1, 10**15) * mags + Fraction(1, 10**300)
            assert abs(Fraction(float(A[r, j])) - mags) <= Fraction(1, 10**15) * mags
            assert A[r, j] >= abs(T[r, j]) * (1 - 1e-15)


def test_int_form_is_the_triple_loop():
    rng = np.random.default_rng(4)
    X = rng.integers(-3, 4, size=(5, 7)).astype(np.float32)
    B = rng.integers(-3, 4, size=(7, 3)).astype(np.float64)
    T = PT.project_truth_int(X, B)
    assert T.dtype == np.int64
    for r in range(5):
        for j in range(3):
            assert T[r, j] == sum(int(X[r, i]) * int(B[i, j]) for i in range(7))
    with pytest.raises(AssertionError):
        PT.project_truth_int(X + 0.5, B)


def test_check_projection_holds_the_bars():
    X = np.array([[1.0, 2.0], [3.0, -4.0]])
    B = np.array([[0.5], [0.25]])
    T, A = PT.project_truth(X, B)
    Y = np.array(T, dtype=np.float64)
    PT.check_projection(Y, T, A, "f64")
    PT.check_projection(Y.astype(np.float32), T, A, "f32")
    off = Y.copy()
    off[1, 0] += 3e-9 * float(A[1, 0])
    with pytest.raises(AssertionError, match="miss the bar"):
        PT.check_projection(off, T, A, "f64")
    nan = Y.copy()
    nan[0, 0] = np.nan
    with pytest.raises(AssertionError):
        PT.check_projection(nan, T, A, "f64")
    # one f32 rounding is allowed for f32 output only
    third = np.array([[1.0 / 3.0]])
    T3, A3 = PT.project_truth(third, np.array([[1.0]]))
    PT.check_projection(third.astype(np.float32), T3, A3, "f32")
    with pytest.raises(AssertionError):
        PT.check_projection(third.astype(np.float32).astype(np.float64), T3, A3, "f64")


def test_pca_truth_diagonalises_the_covariance():
    X = PT.scaled_rows(200, 5, 3)
    ev, V = PT.pca_truth(X)
    assert (np.diff(ev) <= 0).all() and V.shape == (5, 5)
    cov = np.cov(X, rowvar=False)
    np.testing.assert_allclose(V.T @ cov @ V, np.diag(ev), atol=1e-13 * ev[0])
    np.testing.assert_allclose(V.T @ V, np.eye(5), atol=1e-14)
    np.testing.assert_allclose(ev.sum(), np.trace(cov), rtol=1e-13)


def test_scaled_rows_survive_f32():
    X = PT.scaled_rows(50, 4, 1)
    assert (X.astype(np.float32).astype(np.float64) == X).all()


def test_the_pruned_grid_covers_every_pair():
    seen = set()
    for d, k in PT.DENSE_DK:
        assert k <= d
        seen.update(PT.combo_of(d, k))
    assert seen == set(PT.COMBOS)
    assert (16, 16) in PT.DENSE_DK and (256, 256) in PT.DENSE_DK
