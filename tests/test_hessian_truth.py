"""The numpy truth of the second-order tests (tests/hessian_truth.py) checked against independent
constructions: the weighted Gramian against a triple loop, the Hessian against central differences of
the gradient, the Newton iteration against the normal equations and its own stopping conditions (no
GPU)."""
import numpy as np
import pytest

import gram_truth as GT
import hessian_truth as HT


def test_weighted_gram_against_a_triple_loop():
    rng = np.random.default_rng(3)
    n, d = 17, 3
    X = rng.standard_normal((n, d))
    y = rng.standard_normal(n)
    om = rng.uniform(-1.0, 2.0, size=n)
    om[::5] = 0.0
    M, A = HT.weighted_gram(X, y, om)
    Z = GT.augment(X, y)
    want = np.zeros((d + 2, d + 2))
    mags = np.zeros((d + 2, d + 2))
    for i in range(n):
        for j in range(d + 2):
            for k in range(d + 2):
                want[j, k] += om[i] * Z[i, j] * Z[i, k]
                mags[j, k] += abs(om[i]) * abs(Z[i, j]) * abs(Z[i, k])
    assert (np.abs(M - want) <= 1e-13 * mags).all()
    assert (np.abs(A - mags) <= 1e-13 * mags).all()
    assert M[d + 1, d + 1] == pytest.approx(om.sum(), rel=1e-14)
    # unit weights: the plain Gramian
    assert np.allclose(HT.weighted_gram(X, y, np.ones(n))[0], GT.gram_truth(X, y)[0], rtol=1e-14, atol=0)


def test_weighted_gram_int2_is_twice_the_float_truth():
    rng = np.random.default_rng(4)
    X = rng.integers(-3, 4, size=(40, 5)).astype(np.float64)
    y = rng.integers(-3, 4, size=40).astype(np.float64)
    om = rng.choice([0.0, 0.5, 1.0, 2.0, 4.0], size=40)
    assert (2.0 * HT.weighted_gram(X, y, om)[0] == HT.weighted_gram_int2(X, y, om)).all()


def test_curvature_edges():
    X = np.array([[0.0, 0.0], [800.0, 0.0], [-800.0, 0.0], [1.0, 2.0]])
    h = HT.curvature(X, np.array([1.0, 1.0]), "logistic")
    assert h[0] == 0.25 and h[1] == 0.0 and h[2] == 0.0
    s = 1.0 / (1.0 + np.exp(-3.0))
    assert h[3] == pytest.approx(s * (1.0 - s), rel=1e-14)
    assert (HT.curvature(X, np.array([1.0, 1.0]), "least_squares") == 1.0).all()


@pytest.mark.parametrize("kind", ["logistic", "least_squares"])
def test_hessian_against_central_differences(kind):
    """H = sum h x x^T against (grad(w + s e_k) - grad(w - s e_k)) / 2 s at s = 1e-5: the truncation is
    s^2 / 6 times the third derivative (about 1e-10 of H for margins of order 1), the rounding
    2^-52 |grad| / s (about 1e-11), so 1e-6 ||H||_inf is a safe bar."""
    rng = np.random.default_rng(8)
    n, d = 200, 5
    X = rng.standard_normal((n, d))
    y = (rng.random(n) < 0.5).astype(np.float64)
    w = rng.standard_normal(d) / np.sqrt(d)
    H = HT.hessian_sum(X, w, kind)
    assert np.allclose(H, HT.weighted_gram(X, y, HT.curvature(X, w, kind))[0][:d, :d], rtol=1e-13, atol=0)
    s = 1e-5
    fd = np.empty((d, d))
    for k in range(d):
        e = np.zeros(d)
        e[k] = s
        fd[:, k] = (HT.gradient_sum(X, y, w + e, kind) - HT.gradient_sum(X, y, w - e, kind)) / (2.0 * s)
    assert np.abs(fd - H).max() <= 1e-6 * np.abs(H).sum(axis=1).max()


def test_gradient_is_the_slope_of_the_loss():
    rng = np.random.default_rng(9)
    X = rng.standard_normal((100, 4))
    y = (rng.random(100) < 0.5).astype(np.float64)
    w = rng.standard_normal(4)
    for kind in ("logistic", "least_squares"):
        g = HT.gradient_sum(X, y, w, kind)
        for k in range(4):
            e = np.zeros(4)
            e[k] = 1e-6
            fd = (HT.loss_sum(X, y, w + e, kind) - HT.loss_sum(X, y, w - e, kind)) / 2e-6
            assert abs(fd - g[k]) <= 1e-6 * max(np.abs(g).max(), 1.0)


def test_newton_least_squares_is_one_full_step_to_the_normal_equations():
    rng = np.random.default_rng(10)
    n, d, lam = 150, 6, 0.05
    X = rng.standard_normal((n, d))
    y = rng.standard_normal(n)
    r = HT.newton(X, y, rng.standard_normal(d) * 3.0, lam, kind="least_squares")
    want = np.linalg.solve(X.T @ X / n + lam * np.eye(d), X.T @ y / n)
    assert r["halvings"][0] == 0
    assert np.abs(r["weights"] - want).max() <= 1e-9 * np.abs(want).max()


def test_newton_logistic_reaches_a_stationary_point():
    X, y = HT.planted_logistic(400, 7, 21, stretch=2.0)
    lam = 0.1
    r = HT.newton(X, y, np.full(7, 3.0), lam)
    g = HT.gradient_sum(X, y, r["weights"], "logistic") / 400 + lam * r["weights"]
    assert np.linalg.norm(g) <= 1e-10
    assert len(r["history"]) == len(r["gnorm"]) == len(r["halvings"]) == len(r["margins"])
    assert all(a >= b for a, b in zip(r["history"][:-1], r["history"][1:]))    # every accepted step descends
