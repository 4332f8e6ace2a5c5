"""The host side of the tall-skinny QR: QRFactor over a numpy-made R, and the host-only plan."""
import numpy as np
import pytest

from tsqr_truth import lapack_r


@pytest.fixture(scope="module")
def case():
    rng = np.random.default_rng(5)
    X = rng.standard_normal((80, 6)) * rng.uniform(0.5, 2.0, size=6)
    y = X @ rng.standard_normal(6) + 0.1 * rng.standard_normal(80)
    return X, y


def test_qr_factor_members_and_least_squares(pkg, case):
    X, y = case
    f = pkg.QRFactor(lapack_r(np.c_[X, y]), 80)
    assert (f.d, f.count, f.R.shape, f.qty.shape) == (6, 80, (6, 6), (6,))
    w = np.linalg.lstsq(X, y, rcond=None)[0]
    assert np.abs(f.least_squares() - w).max() <= 1e-13 * np.abs(w).max()
    assert abs(f.residualNorm - np.linalg.norm(X @ w - y)) <= 1e-13 * np.linalg.norm(y)
    lam = 0.3
    ridge = np.linalg.solve(X.T @ X / 80 + lam * np.eye(6), X.T @ y / 80)
    assert np.abs(f.least_squares(lam) - ridge).max() <= 1e-13 * np.abs(ridge).max()
    with pytest.raises(pkg.IllegalArgumentException):
        f.least_squares(-1.0)


def test_qr_factor_svd_and_singular_r(pkg, case):
    X, y = case
    f = pkg.QRFactor(lapack_r(np.c_[X, y]), 80)
    s, V = f.svd(4)
    _, s_ref, Vt = np.linalg.svd(X)
    assert np.abs(s - s_ref[:4]).max() <= 1e-13 * s_ref[0]
    assert (V[np.argmax(np.abs(V), axis=0), np.arange(4)] > 0).all()
    assert np.abs(np.abs(V.T @ Vt[:4].T) - np.eye(4)).max() <= 1e-12
    Xd = np.c_[X[:, :3], X[:, 0]]                       # a duplicated column
    g = pkg.QRFactor(lapack_r(np.c_[Xd, y]), 80)
    with pytest.raises(pkg.IllegalArgumentException, match="not positive definite"):
        g.least_squares()
    assert len(g.svd(4)[0]) == 3


@pytest.mark.parametrize("storage", ["f32", "f64"])
def test_plan(pkg, storage):
    N = pkg._native
    for d in range(1, N.TSQR_MAX_D + 1):
        for tiles in (0, 1, 9, 293, 100000):
            p = N.tsqr_plan(storage, d, tiles)
            assert p["a"] == d + 1 and p["a_pad"] == 16 * -(-(d + 1) // 16)
            assert p["lds_bytes"] <= 160 * 1024
            assert p["items"] * p["span_tiles"] >= tiles and p["items"] <= max(tiles, 0)
            levels, m = 0, p["items"]
            while m > 1:
                m, levels = -(-m // p["fan_in"]), levels + 1
            assert p["levels"] == levels
            assert p["scratch_bytes"] == p["items"] * p["a_pad"] ** 2 * 8
    with pytest.raises(N.UnsupportedOperationException):
        N.tsqr_plan(storage, N.TSQR_MAX_D + 1, 10)
