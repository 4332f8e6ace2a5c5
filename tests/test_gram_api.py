"""stat.Gramian's host arithmetic on truth matrices, the argument checks of the entry functions and the
host-only plan of psgd_gramian (no GPU)."""
import numpy as np
import pytest

import gram_truth as GT


def case(n=200, d=6, seed=11):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d)) * rng.uniform(0.5, 3.0, size=d) + rng.uniform(-2.0, 2.0, size=d)
    y = rng.standard_normal(n)
    return X, y


def test_members(pkg):
    X, y = case()
    M, _ = GT.gram_truth(X, y)
    g = pkg.Gramian(M)
    assert g.d == 6 and g.count == 200
    assert (g.gram == M[:6, :6]).all() and (g.xty == M[:6, 6]).all()
    assert g.yty == M[6, 6] and g.labelSum == M[6, 7] and (g.columnSums == M[:6, 7]).all()
    np.testing.assert_allclose(g.mean, X.mean(axis=0), rtol=1e-12, atol=1e-14)
    assert pkg.Gramian(M.ravel()).count == 200     # a flat row-major array too


def test_covariance_and_corr_against_numpy(pkg):
    X, y = case()
    g = pkg.Gramian(GT.gram_truth(X, y)[0])
    np.testing.assert_allclose(g.covariance(), np.cov(X, rowvar=False), rtol=1e-10, atol=1e-12)
    c = g.corr()
    np.testing.assert_allclose(c, np.corrcoef(X, rowvar=False), rtol=1e-10, atol=1e-12)
    assert (np.diag(c) == 1.0).all()


def test_corr_with_a_constant_column(pkg):
    X, y = case()
    X[:, 2] = 4.0
    c = pkg.Gramian(GT.gram_truth(X, y)[0]).corr()
    assert (np.diag(c) == 1.0).all()
    off = np.ones(6, dtype=bool)
    off[2] = False
    assert np.isnan(c[2, off]).all() and np.isnan(c[off, 2]).all()
    assert not np.isnan(c[np.ix_(off, off)]).any()


@pytest.mark.parametrize("lam", [0.0, 0.1, 10.0])
def test_normal_equations_residual(pkg, lam):
    X, y = case()
    n, d = X.shape
    g = pkg.Gramian(GT.gram_truth(X, y)[0])
    w = g.normal_equations(lam)
    A = g.gram / n + lam * np.eye(d)
    b = g.xty / n
    terms = np.abs(A) @ np.abs(w) + np.abs(b)
    assert (np.abs(A @ w - b) <= 1e-12 * terms).all()
    # ... and it is the minimiser of (1 / n) sum (w . x - y)^2 / 2 + (lam / 2) ||w||^2
    grad = X.T @ (X @ w - y) / n + lam * w
    assert (np.abs(grad) <= 1e-11 * terms).all()


def test_normal_equations_recover_noiseless_weights(pkg):
    X, _ = case()
    w0 = np.linspace(-1.0, 2.0, X.shape[1])
    w = pkg.Gramian(GT.gram_truth(X, X @ w0)[0]).normal_equations(0.0)
    assert np.abs(w - w0).max() <= 1e-9


def test_argument_checks(pkg):
    E = pkg.IllegalArgumentException
    X, y = case()
    M, _ = GT.gram_truth(X, y)
    one, _ = GT.gram_truth(X[:1], y[:1])
    with pytest.raises(E, match="<= 1 row"):
        pkg.Gramian(one).covariance()
    with pytest.raises(E, match="<= 1 row"):
        pkg.Gramian(one).corr()
    with pytest.raises(E, match="nonnegative"):
        pkg.Gramian(M).normal_equations(-0.5)
    with pytest.raises(E, match="nonnegative"):
        pkg.Gramian(M).normal_equations(float("nan"))
    Xs = X.copy()
    Xs[:, 3] = Xs[:, 1] * 2.0     # collinear: singular
    Xs[:, 4] = 0.0
    with pytest.raises(E, match="positive definite"):
        pkg.Gramian(GT.gram_truth(Xs, y)[0]).normal_equations(0.0)
    assert np.isfinite(pkg.Gramian(GT.gram_truth(Xs, y)[0]).normal_equations(0.5)).all()
    with pytest.raises(E):
        pkg.Gramian(np.zeros((3, 4)))
    with pytest.raises(E):
        pkg.Gramian(np.zeros(7))


def test_entry_functions_refuse_without_a_device(pkg):
    E = pkg.IllegalArgumentException
    wide = pkg.PartitionedData([pkg.DensePartition(np.zeros(1), np.zeros((1, 4097), dtype=np.float32))])
    for call in (pkg.gramian, pkg.covariance, pkg.corr, pkg.normal_equations):
        with pytest.raises(E, match="4096"):
            call(wide)
    empty = pkg.PartitionedData([pkg.DensePartition(np.zeros(0), np.zeros((0, 5), dtype=np.float32))])
    for call in (pkg.gramian, pkg.covariance, pkg.corr, pkg.normal_equations):
        with pytest.raises(E, match="without rows"):
            call(empty)
    with pytest.raises(E, match="nonnegative"):
        pkg.normal_equations(empty, -1.0)


# ---- the plan ------------------------------------------------------------------------------------
PLAN_D = (1, 13, 14, 15, 30, 126, 127, 510, 512, 1024, 4096)
PLAN_TILES = (0, 1, 2, 255, 256, 10**4, 10**6)


@pytest.mark.parametrize("storage", ["f32", "f64"])
@pytest.mark.parametrize("d", PLAN_D)
def test_dense_plan(pkg, d, storage):
    N = pkg._native
    for tiles in PLAN_TILES:
        p = N.gramian_plan("dense", storage, d, tiles)
        assert p["path"] == "dense_mfma" and p["a"] == d + 2 and p["blocks"] == -(-(d + 2) // 16)
        assert p["tile_rows"] == (1024 if storage == "f32" else 512)
        assert 0 <= p["scratch_bytes"] <= 256 << 20
        nb, gr, gc = p["blocks"], p["gr"], p["gc"]
        assert 1 <= gr * gc <= 32     # 4 doubles a lane a block: at most 256 accumulator registers
        # the kept groups, from the rule the header states; every upper-triangle block lies in exactly
        # one group rectangle, which must be kept, and every kept group holds such a block
        nrg, ncg = -(-nb // gr), -(-nb // gc)
        kept = {(R, C) for R in range(nrg) for C in range((R * gr) // gc, ncg)}
        assert len(kept) == p["groups"]
        used = set()
        for jb in range(nb):
            for kb in range(jb, nb):
                used.add((jb // gr, kb // gc))
        assert used == kept
        # the spans cover the tiles; one record an item
        if tiles == 0:
            assert p["spans"] == 0 and p["scratch_bytes"] == 0
            continue
        assert p["span_tiles"] >= 1
        assert (p["spans"] - 1) * p["span_tiles"] < tiles <= p["spans"] * p["span_tiles"]
        items = p["spans"] * p["groups"]
        assert p["scratch_bytes"] == items * gr * gc * 256 * 8
        assert items >= min(256, tiles * p["groups"])


def test_plan_does_not_depend_on_anything_but_its_arguments(pkg):
    N = pkg._native
    assert N.gramian_plan("dense", "f32", 512, 9766) == N.gramian_plan("dense", "f32", 512, 9766)


@pytest.mark.parametrize("tiles", PLAN_TILES)
def test_csr_plan(pkg, tiles):
    p = pkg._native.gramian_plan("csr", "f32", 4096, tiles)
    assert p["path"] == "csr" and p["a"] == 4098 and p["tile_rows"] == 512
    assert p["scratch_bytes"] <= 256 << 20
    if tiles:
        assert p["spans"] * p["span_tiles"] >= tiles
        assert p["scratch_bytes"] >= (tiles + p["spans"] + 1) * 24


def test_plan_errors(pkg):
    N = pkg._native
    with pytest.raises(pkg.UnsupportedOperationException, match="4096"):
        N.gramian_plan("dense", "f32", 4097, 10)
    with pytest.raises(pkg.IllegalArgumentException):
        N.gramian_plan("dense", "f32", 0, 10)
    with pytest.raises(pkg.IllegalArgumentException):
        N.gramian_plan("dense", "f32", 5, -1)
    L = N.lib()
    assert L.psgd_gramian_plan(0, 1, 5, 1, None) == N.PSGD_EINVAL
    assert L.psgd_gramian(None, None) == N.PSGD_EINVAL
    assert L.psgd_gramian_device(None, None, None) == N.PSGD_EINVAL
