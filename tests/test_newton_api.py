"""newton.py and the weighted stat.Gramian on the CPU: the refusals fire before any engine is touched,
and the Newton loop driven by a numpy engine (the same methods HipEngine offers) follows its
specification -- LeastSquares in one full step to the normal equations, the history convention, empty
data, the message for a Hessian that is not positive definite (no GPU)."""
import numpy as np
import pytest

import gram_truth as GT
import hessian_truth as HT


class HostTensor:
    """What the loop asks of a device tensor."""

    def __init__(self, a):
        self.a = np.array(a, dtype=np.float64)

    def cpu(self):
        return self

    def numpy(self):
        return self.a


class Score:
    def __init__(self, lossSum, count):
        self.lossSum, self.count = lossSum, count


class NumpyEngine:
    """HipEngine's batch passes over host rows, one rank."""

    def __init__(self, X, y, P=1):
        self.X, self.y = np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64)
        self.lo, self.hi = 0, P
        self.calls = []

    @staticmethod
    def kind(gradient):
        return {0: "logistic", 1: "least_squares"}[gradient.kind]

    def to_host(self, t):
        return t.a if isinstance(t, HostTensor) else np.asarray(t, dtype=np.float64)

    def device_rows(self, values):
        return HostTensor(values)

    def gradient_sum(self, gradient, w, miniBatchFraction=1.0, iteration=0):
        self.calls.append("gradient_sum")
        w = self.to_host(w)
        k = self.kind(gradient)
        return HostTensor(np.concatenate([HT.gradient_sum(self.X, self.y, w, k),
                                          [HT.loss_sum(self.X, self.y, w, k), len(self.y)]]))

    def row_curvature(self, gradient, w):
        self.calls.append("row_curvature")
        return HostTensor(HT.curvature(self.X, self.to_host(w), self.kind(gradient)))

    def gramian(self, weights=None):
        self.calls.append("gramian")
        om = np.ones(len(self.y)) if weights is None else self.to_host(weights)
        return HostTensor(HT.weighted_gram(self.X, self.y, om)[0].ravel())

    def evaluate(self, gradient, w):
        self.calls.append("evaluate")
        return Score(HT.loss_sum(self.X, self.y, self.to_host(w), self.kind(gradient)), len(self.y))


class Untouchable:
    """An engine no call may reach."""

    def __getattr__(self, name):
        raise AssertionError(f"the engine was touched ({name}) before the refusal")


def host_data(pkg, X, y, P=3):
    return pkg.PartitionedData.parallelize(np.asarray(y, dtype=np.float64), np.asarray(X, dtype=np.float64), P)


def ls_case(n=120, d=5, seed=2):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, d)) * rng.uniform(0.5, 2.0, size=d), rng.standard_normal(n)


def test_exports(pkg):
    for name in ("Newton", "runNewton", "hessian_sum", "HessianSum"):
        assert hasattr(pkg, name) and name in pkg.__all__


def test_refusals_fire_before_the_engine_is_touched(pkg):
    X, y = ls_case()
    data = host_data(pkg, X, y)
    w0 = np.zeros(5)
    U = pkg.UnsupportedOperationException
    run = lambda g, u: pkg.runNewton(data, g, u, 5, 0.1, w0, engine=Untouchable())
    for upd in (pkg.L1SGDUpdater(), pkg.AdaGradSGDUpdater(), pkg.AdamSGDUpdater()):
        with pytest.raises(U):
            run(pkg.LogisticGradient(), upd)
    with pytest.raises(U):
        run(pkg.HingeGradient(), pkg.SimpleSGDUpdater())
    with pytest.raises(U):
        run(pkg.LogisticGradient(3), pkg.SquaredL2SGDUpdater())
    with pytest.raises(U):
        pkg.hessian_sum(data, pkg.HingeGradient(), w0, engine=Untouchable())
    with pytest.raises(U):
        pkg.hessian_sum(data, pkg.LogisticGradient(4), w0, engine=Untouchable())
    with pytest.raises(pkg.IllegalArgumentException):
        run(object(), pkg.SimpleSGDUpdater())
    with pytest.raises(pkg.IllegalArgumentException):          # the weights' size, BLAS.dot's message
        pkg.runNewton(data, pkg.LogisticGradient(), pkg.SimpleSGDUpdater(), 5, 0.0, np.zeros(4), engine=Untouchable())
    with pytest.raises(pkg.IllegalArgumentException):
        pkg.runNewton(data, pkg.LogisticGradient(), pkg.SquaredL2SGDUpdater(), 5, -1.0, w0, engine=Untouchable())
    with pytest.raises(pkg.IllegalArgumentException):
        pkg.hessian_sum(data, pkg.LogisticGradient(), np.zeros(6), engine=Untouchable())


def test_setters_and_defaults(pkg):
    nt = pkg.Newton(pkg.LogisticGradient(), pkg.SquaredL2SGDUpdater())
    assert (nt.numIterations, nt.regParam, nt.convergenceTol) == (100, 0.0, 1e-6)
    assert nt.setNumIterations(7).setRegParam(0.5).setConvergenceTol(0.25) is nt
    assert (nt.numIterations, nt.regParam, nt.convergenceTol) == (7, 0.5, 0.25)
    for bad in (lambda: nt.setNumIterations(-1), lambda: nt.setRegParam(-0.1), lambda: nt.setConvergenceTol(1.5)):
        with pytest.raises(pkg.IllegalArgumentException):
            bad()
    with pytest.raises(pkg.UnsupportedOperationException):
        nt.setComputeDtype("f32")


@pytest.mark.parametrize("lam,updater", [(0.0, "SimpleSGDUpdater"), (0.3, "SquaredL2SGDUpdater")])
@pytest.mark.parametrize("start", [0.0, 50.0])
def test_least_squares_is_one_full_step_to_the_normal_equations(pkg, lam, updater, start):
    X, y = ls_case()
    n, d = X.shape
    data, eng = host_data(pkg, X, y), NumpyEngine(X, y, 3)
    w, hist = pkg.runNewton(data, pkg.LeastSquaresGradient(), getattr(pkg, updater)(), 10, lam,
                            np.full(d, start), engine=eng)
    want = pkg.normal_equations(data, lam, engine=eng)
    assert np.abs(w - want).max() <= 1e-9 * np.abs(want).max()
    # iteration 1 takes the full step; iteration 2 finds no decrease left or a step below the tolerance
    assert 1 <= len(hist) <= 2
    assert eng.calls[:4] == ["evaluate", "gradient_sum", "row_curvature", "gramian"]
    # history[0] is f at the initial weights
    f0 = HT.loss_sum(X, y, np.full(d, start), "least_squares") / n + 0.5 * lam * d * start * start
    assert hist[0] == pytest.approx(f0, rel=1e-13)


def test_simple_updater_means_no_penalty(pkg):
    X, y = ls_case()
    data, eng = host_data(pkg, X, y), NumpyEngine(X, y, 3)
    w, _ = pkg.runNewton(data, pkg.LeastSquaresGradient(), pkg.SimpleSGDUpdater(), 10, 5.0, np.zeros(5), engine=eng)
    want = pkg.normal_equations(data, 0.0, engine=eng)
    assert np.abs(w - want).max() <= 1e-9 * np.abs(want).max()


def test_logistic_follows_the_truth_and_the_history_convention(pkg):
    X, y = HT.planted_logistic(300, 6, 77, stretch=2.0)
    lam, w0 = 0.05, np.full(6, 3.0)
    truth = HT.newton(X, y, w0, lam, num_iterations=25)
    assert sum(truth["halvings"]) >= 1           # the line search is exercised
    data, eng = host_data(pkg, X, y), NumpyEngine(X, y, 3)
    w, hist = pkg.runNewton(data, pkg.LogisticGradient(), pkg.SquaredL2SGDUpdater(), 25, lam, w0, engine=eng)
    assert np.abs(w - truth["weights"]).max() <= 1e-12 * max(np.abs(w).max(), 1.0)
    assert len(hist) == len(truth["history"])
    np.testing.assert_allclose(hist, truth["history"], rtol=1e-13, atol=0)
    # history[k] is f at the weights iteration k started from: [0] at w0, and non-increasing
    assert hist[0] == pytest.approx(HT.loss_sum(X, y, w0, "logistic") / 300 + 0.5 * lam * float(w0 @ w0), rel=1e-13)
    assert (np.diff(hist) <= 0.0).all()
    g = HT.gradient_sum(X, y, w, "logistic") / 300 + lam * w
    assert np.linalg.norm(g) <= 1e-10
    # numIterations caps the passes; the class front end gives the same weights
    w2, h2 = pkg.runNewton(data, pkg.LogisticGradient(), pkg.SquaredL2SGDUpdater(), 2, lam, w0, engine=eng)
    assert len(h2) == 2 and (h2 == hist[:2]).all()


def test_empty_data_returns_the_initial_weights(pkg):
    empty = pkg.PartitionedData([pkg.DensePartition(np.zeros(0), np.zeros((0, 4)))])
    w0 = np.array([1.0, -2.0, 3.0, 0.5])
    w, hist = pkg.runNewton(empty, pkg.LogisticGradient(), pkg.SimpleSGDUpdater(), 10, 0.0, w0, engine=Untouchable())
    assert (w == w0).all() and len(hist) == 0
    hs = pkg.hessian_sum(empty, pkg.LogisticGradient(), w0, engine=Untouchable())
    assert hs.count == 0 and hs.curvatureSum == 0.0 and (hs.hessian == 0.0).all() and hs.hessian.shape == (4, 4)


def test_hessian_that_is_not_positive_definite_raises(pkg):
    X, y = ls_case()
    X[:, 3] = X[:, 1]                                  # collinear columns, no penalty
    data, eng = host_data(pkg, X, y), NumpyEngine(X, y, 3)
    with pytest.raises(pkg.IllegalArgumentException, match="not positive definite"):
        pkg.runNewton(data, pkg.LeastSquaresGradient(), pkg.SimpleSGDUpdater(), 5, 0.0, np.zeros(5), engine=eng)
    # ... and the penalty cures it
    w, _ = pkg.runNewton(data, pkg.LeastSquaresGradient(), pkg.SquaredL2SGDUpdater(), 5, 0.1, np.zeros(5), engine=eng)
    assert np.isfinite(w).all()


def test_hessian_sum_through_an_engine(pkg):
    X, y = HT.planted_logistic(90, 4, 5)
    data, eng = host_data(pkg, X, y), NumpyEngine(X, y, 3)
    w = np.array([0.3, -0.2, 0.1, 0.4])
    hs = pkg.hessian_sum(data, pkg.LogisticGradient(), w, engine=eng)
    assert hs.count == 90 and hs.hessian.shape == (4, 4)
    assert np.allclose(hs.hessian, HT.hessian_sum(X, w, "logistic"), rtol=1e-13, atol=0)
    assert hs.curvatureSum == pytest.approx(HT.curvature(X, w, "logistic").sum(), rel=1e-13)


# ---- the weighted Gramian's host members --------------------------------------------------------------
def test_weighted_gramian_members(pkg):
    rng = np.random.default_rng(12)
    X, y = ls_case(n=80, d=4, seed=6)
    om = rng.uniform(0.0, 2.0, size=80)
    M, _ = HT.weighted_gram(X, y, om)
    g = pkg.Gramian(M, weighted=True)
    assert g.weighted and g.weightSum == M[5, 5] and g.weightSum == pytest.approx(om.sum(), rel=1e-14)
    np.testing.assert_allclose(g.mean, (om[:, None] * X).sum(axis=0) / om.sum(), rtol=1e-12)
    lam = 0.2
    w = g.normal_equations(lam)
    # the minimiser of (1 / W) sum om_i (w . x_i - y_i)^2 / 2 + (lam / 2) ||w||^2
    grad = X.T @ (om * (X @ w - y)) / om.sum() + lam * w
    assert np.abs(grad).max() <= 1e-12 * max(np.abs(w).max(), 1.0)
    for member in (g.covariance, g.corr, lambda: g.principal_components(2), lambda: g.svd(2)):
        with pytest.raises(pkg.IllegalArgumentException, match="weighted"):
            member()
    with pytest.raises(pkg.IllegalArgumentException):
        pkg.Gramian(np.zeros((6, 6)), weighted=True).normal_equations(0.1)     # no weight at all
    assert "weightSum" in repr(g)


def test_unweighted_gramian_is_unchanged(pkg):
    X, y = ls_case(n=80, d=4, seed=6)
    M, _ = GT.gram_truth(X, y)
    g = pkg.Gramian(M)
    assert not g.weighted and g.weightSum == 80.0 and g.count == 80
    np.testing.assert_allclose(g.covariance(), np.cov(X, rowvar=False), rtol=1e-10, atol=1e-12)
    unit = pkg.Gramian(HT.weighted_gram(X, y, np.ones(80))[0], weighted=True)      # unit weights: the same optimum
    np.testing.assert_allclose(unit.normal_equations(0.1), g.normal_equations(0.1), rtol=1e-12, atol=0)
    assert repr(g) == "Gramian(d=4, count=80)"


def test_stat_gramian_checks_and_slices_the_weights(pkg):
    X, y = ls_case(n=30, d=3, seed=1)
    data, eng = host_data(pkg, X, y, 4), NumpyEngine(X, y, 4)
    om = np.linspace(0.0, 2.0, 30)
    g = pkg.gramian(data, weights=om, engine=eng)
    assert g.weighted and np.allclose(g.matrix, HT.weighted_gram(X, y, om)[0], rtol=1e-14, atol=0)
    assert not pkg.gramian(data, engine=eng).weighted
    for bad in (om[:-1], -om, np.where(np.arange(30) == 3, np.nan, om), om.reshape(5, 6)):
        with pytest.raises(pkg.IllegalArgumentException):
            pkg.gramian(data, weights=bad, engine=Untouchable())
    # a rank's slice: the rows of its partitions [lo, hi) in partition order
    from spark_parallelized_sgd_amd.stat import local_row_slice
    eng.lo, eng.hi = 1, 3
    sizes = [p.n_rows for p in data.partitions]
    assert local_row_slice(data, eng) == slice(sizes[0], sizes[0] + sizes[1] + sizes[2])
