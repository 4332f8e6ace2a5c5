"""clustering.py's mixture on the CPU: GaussianMixture.run driven by a numpy engine (the methods HipEngine
offers) follows its specification -- the stopping rule, the initialisation from the seed, the argument
checks --, MultivariateGaussian meets the closed forms, and psgd_gmm_plan's paths and errors need no
device (no GPU)."""
import numpy as np
import pytest

import gmm_truth as GT
from test_kmeans_api import blobs, data_of, host


class NumpyEngine:
    """HipEngine's mixture passes over host rows, one rank."""

    def __init__(self, X):
        self.X, self.lo, self.hi, self.steps = np.asarray(X, dtype=np.float64), 0, 1, 0

    def registered_rows(self, positions):
        return self.X[np.asarray(positions)]

    def gmm_step(self, weights, gaussians):
        self.steps += 1
        _, r, lnp = GT.estep(self.X, *GT.operands(weights, [g.mu for g in gaussians], [g.sigma for g in gaussians]))
        return host(np.concatenate([GT.moments(self.X, r).ravel(), [lnp.sum(), len(self.X)]]))


def model_of(pkg, means, d=2):
    return pkg.GaussianMixtureModel(np.full(len(means), 1.0 / len(means)),
                                    [pkg.MultivariateGaussian(m, np.eye(d)) for m in means])


@pytest.mark.parametrize("maxIterations,tol", [(100, 0.01), (1, 0.01), (0, 0.01), (100, 1e300)])
def test_run_follows_the_stopping_rule(pkg, maxIterations, tol):
    X, means = blobs()
    eng = NumpyEngine(X)
    model = pkg.GaussianMixture(3, tol, maxIterations).setInitialModel(model_of(pkg, means + 0.5)).run(data_of(pkg, X), engine=eng)
    w, mus, sigmas, llh, it = GT.em(X, np.full(3, 1.0 / 3), means + 0.5, np.stack([np.eye(2)] * 3), tol, maxIterations)
    assert model.numIterations == it == eng.steps and model.k == 3
    # no step; one step; llhPrev starts at the most negative double, so the first two differences are
    # ~1.8e308 > 1e300 and two steps run before a huge tolerance ends the loop (MLlib's own count); else it converges
    want = {(0, 0.01): 0, (1, 0.01): 1, (100, 1e300): 2}.get((maxIterations, tol))
    assert it == want if want is not None else 2 <= it < 100
    if it == 0:
        assert model.logLikelihood is None and np.allclose(model.gaussians[0].mu, means[0] + 0.5)
    else:
        assert abs(model.logLikelihood - llh) <= 1e-12 * abs(llh)
        assert np.allclose(model.weights, w, rtol=1e-12) and np.allclose(np.stack([g.sigma for g in model.gaussians]), sigmas, rtol=1e-9, atol=1e-12)


def test_initialisation_from_the_seed(pkg):
    X, _ = blobs()
    model = pkg.GaussianMixture(3, maxIterations=0, seed=5).run(data_of(pkg, X), engine=NumpyEngine(X))
    pos = np.random.default_rng(5).choice(len(X), size=15, replace=False)
    for j, g in enumerate(model.gaussians):
        rows = X[pos[5 * j: 5 * j + 5]]
        assert np.allclose(g.mu, rows.mean(axis=0), rtol=1e-14)
        assert np.allclose(g.sigma, np.diag(rows.var(axis=0, ddof=1)), rtol=1e-10, atol=1e-14)
    assert (model.weights == 1.0 / 3).all() and model.numIterations == 0
    with pytest.raises(pkg.IllegalArgumentException, match="at least 5 k"):
        pkg.GaussianMixture(3, seed=5).run(data_of(pkg, X[:14]), engine=NumpyEngine(X[:14]))


def test_argument_checks(pkg):
    X, means = blobs()
    E = pkg.IllegalArgumentException
    for bad in (0, -1, 2.0, True, 257):
        with pytest.raises(E):
            pkg.GaussianMixture(bad)
    with pytest.raises(E):
        pkg.GaussianMixture(3, convergenceTol=-1.0)
    with pytest.raises(E):
        pkg.GaussianMixture(3, maxIterations=-1)
    with pytest.raises(E, match="Mismatched cluster count"):
        pkg.GaussianMixture(2).setInitialModel(model_of(pkg, means))
    with pytest.raises(E):   # wrong shapes
        pkg.MultivariateGaussian(np.zeros(2), np.eye(3))
    with pytest.raises(E):
        pkg.GaussianMixtureModel([0.5, 0.5], [pkg.MultivariateGaussian(np.zeros(2), np.eye(2))])
    with pytest.raises(E, match="positive"):
        pkg.GaussianMixtureModel([1.0, 0.0], [pkg.MultivariateGaussian(np.zeros(2), np.eye(2))] * 2)
    with pytest.raises(E, match="vector sizes do not match"):
        pkg.GaussianMixture(3).setInitialModel(model_of(pkg, np.zeros((3, 4)), 4)).run(data_of(pkg, X), engine=NumpyEngine(X))
    csr = pkg.PartitionedData([pkg.CsrPartition(np.zeros(1), np.array([0, 1], dtype=np.int64), np.zeros(1, dtype=np.int32),
                                                np.ones(1), 2)])
    with pytest.raises(E, match="dense rows"):
        pkg.GaussianMixture(3).run(csr, engine=NumpyEngine(X))
    with pytest.raises(E, match="dense rows"):
        pkg.gmm_step(csr, [1.0], [pkg.MultivariateGaussian(np.zeros(2), np.eye(2))], engine=NumpyEngine(X))


def test_multivariate_gaussian_closed_forms(pkg):
    s = np.array([0.5, 2.0, 3.0])
    mu, x = np.array([1.0, -1.0, 0.5]), np.array([[0.0, 0.0, 0.0], [1.0, 2.0, 3.0]])
    g = pkg.MultivariateGaussian(mu, np.diag(s))
    want = -0.5 * (3 * np.log(2 * np.pi) + np.log(s).sum() + (((x - mu) ** 2) / s).sum(axis=1))
    assert np.allclose(g.logpdf(x), want, rtol=1e-14) and np.allclose(g.pdf(x[0]), np.exp(want[0]), rtol=1e-13)
    # rank-deficient: the pseudo-determinant leaves the zero direction out, and R has a zero row for it
    u = np.array([1.0, 1.0]) / np.sqrt(2.0)
    h = pkg.MultivariateGaussian(np.zeros(2), 4.0 * np.outer(u, u))
    assert sorted(np.abs(h.rootSigmaInv).sum(axis=1) > 0) == [False, True]
    assert np.isclose(h.u, -0.5 * (2 * np.log(2 * np.pi) + np.log(4.0)), rtol=1e-14)
    assert np.isclose(h.logpdf(3.0 * u), h.u - 0.5 * 9.0 / 4.0, rtol=1e-13)
    assert np.isclose(h.logpdf(np.array([1.0, -1.0])), h.u, rtol=1e-13)   # off the support: no distance counted
    with pytest.raises(pkg.IllegalArgumentException, match="no non-zero singular values"):
        pkg.MultivariateGaussian(np.zeros(2), np.zeros((2, 2)))


def test_plan_paths_and_errors(pkg):
    N = pkg._native
    # f32, d = 32 (two blocks a component): 32 x 32 k operands + 8 (16 k + 16) staging doubles against 160 KiB
    for k in (1, 8, 17, 18, 19, 24):
        plan = N.gmm_plan("dense", "f32", 32, k, 100)
        fits = 8 * (32 * 32 * k + 8 * (16 * k + 16)) <= 160 * 1024
        assert plan["path"] == ("dense_lds" if fits else "dense_l2") == GT.expected_path(32, k, "f32")
        assert plan["lds_bytes"] == 8 * ((32 * 32 * k if fits else 0) + plan["waves"] * (16 * k + 16)) <= 160 * 1024
        assert plan["component_blocks"] == 2 and plan["tile_rows"] == 16
        assert plan["scratch_bytes_with_resp"] == plan["scratch_bytes"] + 100 * 16 * k * 8
    assert [N.gmm_plan("dense", "f32", 32, k, 100)["path"] for k in (17, 18)] == ["dense_lds", "dense_l2"]
    assert N.gmm_plan("dense", "f64", 8, 256, 10)["waves"] == 4 and N.gmm_plan("dense", "f64", 1, 1, 0)["items"] == 0
    big = N.gmm_plan("dense", "f32", 3, 2, 10 ** 6)
    assert big["items"] <= 8192 + 2 and big["spans"] * big["span_tiles"] >= 10 ** 6   # the item cap bounds the scratch
    L = N.lib()
    out = (np.zeros(13, dtype=np.int64)).ctypes.data
    assert L.psgd_gmm_plan(0, 1, 32, 8, 10, None) == N.PSGD_EINVAL
    for args in ((2, 1, 32, 8, 10), (0, 2, 32, 8, 10), (0, 1, 0, 8, 10), (0, 1, 32, 0, 10), (0, 1, 32, 8, -1)):
        assert L.psgd_gmm_plan(*args, out) == N.PSGD_EINVAL
    for args in ((0, 1, 32, 257, 10), (0, 1, 257, 8, 10), (1, 1, 32, 8, 10)):
        assert L.psgd_gmm_plan(*args, out) == N.PSGD_EUNSUPPORTED
