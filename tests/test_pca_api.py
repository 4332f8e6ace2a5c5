"""stat.Gramian.principal_components / svd on truth matrices, the argument checks of multiply, PCA and
the entry functions, the host-only plan of psgd_project, and PCAModel.transform over a fake engine (no GPU).

The bar is the project's fp64 one: eigenvalues within 1e-9 of the largest one, |<pc_j, truth_j>| >= 1 -
1e-9. numpy alone lands at 3e-15 and 1 - 2e-15 on exactly these inputs, so the bar tests the code, not
the data."""
import numpy as np
import pytest

import project_truth as PT

SHAPES = [(2000, 12), (300, 40), (5000, 130)]


def gramian_of(pkg, X):
    Z = np.concatenate([X, np.zeros((X.shape[0], 1)), np.ones((X.shape[0], 1))], axis=1)
    return pkg.Gramian(Z.T @ Z)


@pytest.mark.parametrize("n,d", SHAPES)
def test_principal_components_against_the_svd(pkg, n, d):
    X = PT.scaled_rows(n, d, 41 + d)
    ev, V = PT.pca_truth(X)
    m = min(d, 8)
    pc, explained = gramian_of(pkg, X).principal_components(m)
    assert pc.shape == (d, m) and explained.shape == (m,)
    cov = np.cov(X, rowvar=False)
    got = np.array([pc[:, j] @ cov @ pc[:, j] for j in range(m)])
    print(f"n={n} d={d}: eigenvalues off by {np.abs(got - ev[:m]).max() / ev[0]:.3g} of the largest, "
          f"1 - |<pc, truth>| <= {(1.0 - np.abs(np.sum(pc * V[:, :m], axis=0))).max():.3g}")
    assert (np.abs(got - ev[:m]) <= 1e-9 * ev[0]).all()
    assert (np.abs(explained * ev.sum() - ev[:m]) <= 1e-9 * ev[0]).all()
    assert (np.abs(np.sum(pc * V[:, :m], axis=0)) >= 1.0 - 1e-9).all()


@pytest.mark.parametrize("n,d", SHAPES)
def test_conventions(pkg, n, d):
    X = PT.scaled_rows(n, d, 41 + d)
    pc, explained = gramian_of(pkg, X).principal_components(d)
    # each component's largest-magnitude entry is positive (the project's convention, not LAPACK's)
    top = np.argmax(np.abs(pc), axis=0)
    assert (pc[top, np.arange(d)] > 0.0).all()
    assert (np.diff(explained) <= 0.0).all()                      # descending
    assert abs(explained.sum() - 1.0) <= 1e-12
    assert np.abs(pc.T @ pc - np.eye(d)).max() <= 1e-12
    # a leading block of a larger k is the smaller k
    assert gramian_of(pkg, X).principal_components(3)[0].tobytes() == np.ascontiguousarray(pc[:, :3]).tobytes()


@pytest.mark.parametrize("n,d", SHAPES)
def test_svd_rebuilds_the_gram_matrix(pkg, n, d):
    X = PT.scaled_rows(n, d, 41 + d)
    g = gramian_of(pkg, X)
    s, V = g.svd(d)
    m = len(s)
    # what is left out lies below rCond or the eigen-solver's noise floor, far below the bar
    assert min(d, 8) <= m <= d and (np.diff(s) <= 0.0).all() and V.shape == (d, m)
    G = X.T @ X
    assert np.abs((V * s**2) @ V.T - G).max() <= 1e-9 * s[0] ** 2
    np.testing.assert_allclose(s[: min(d, 8)], np.linalg.svd(X, compute_uv=False)[: min(d, 8)], rtol=1e-9)
    top = np.argmax(np.abs(V), axis=0)
    assert (V[top, np.arange(m)] > 0.0).all()


def test_svd_of_a_rank_deficient_matrix_returns_fewer(pkg):
    X = PT.scaled_rows(300, 6, 2)
    X[:, 4] = X[:, 1]              # a duplicated column: rank 5
    s, V = gramian_of(pkg, X).svd(6)
    assert len(s) == 5 and V.shape == (6, 5)
    assert len(gramian_of(pkg, X).svd(3)[0]) == 3


def test_argument_checks(pkg):
    E = pkg.IllegalArgumentException
    X = PT.scaled_rows(50, 6, 9)
    g = gramian_of(pkg, X)
    for bad in (0, 7, 257, True, 2.0, -1, None):
        with pytest.raises(E):
            g.principal_components(bad)
        with pytest.raises(E):
            g.svd(bad)
    with pytest.raises(E, match="rCond"):
        g.svd(2, rCond=-1.0)
    one = gramian_of(pkg, X[:1])
    with pytest.raises(E, match="<= 1 row"):
        one.principal_components(1)
    for bad in (0, 257, True, 2.0, -3):
        with pytest.raises(E):
            pkg.PCA(bad)
    assert pkg.PCA(256).k == 256
    data = pkg.PartitionedData([pkg.DensePartition(np.zeros(50), X.astype(np.float32))])
    with pytest.raises(E, match="k=7"):
        pkg.PCA(7).fit(data)                       # k > d
    for call in (pkg.computePrincipalComponents, pkg.computeSVD):
        for bad in (0, 7, True, 2.0):
            with pytest.raises(E):
                call(data, bad)
    single = pkg.PartitionedData([pkg.DensePartition(np.zeros(1), X[:1].astype(np.float32))])

    class OneRow:
        def gramian(self):
            import torch
            return torch.from_numpy(gramian_of(pkg, X[:1]).matrix.ravel())

    with pytest.raises(E, match="<= 1 row"):
        pkg.computePrincipalComponents(single, 2, engine=OneRow())
    # multiply: B's shape, k and the storage name, all before any device is touched
    for B in (np.zeros((5, 2)), np.zeros((6,)), np.zeros((6, 0)), np.zeros((6, 257)), np.zeros((6, 2, 1))):
        with pytest.raises(E):
            pkg.multiply(data, B)
    with pytest.raises(E, match="storage"):
        pkg.multiply(data, np.zeros((6, 2)), "f16")
    with pytest.raises(E):
        pkg.PCAModel(2, np.zeros((6, 3)))
    with pytest.raises(E, match="Expected 5"):
        pkg.PCAModel(2, np.zeros((5, 2))).transform(data)


class FakeEngine:
    """Records what HipEngine.project is asked for and returns a result of its own."""

    def __init__(self, pkg, k):
        self.calls = []
        self.result = pkg.PartitionedData([pkg.DensePartition(np.zeros(3), np.zeros((3, k)))])

    def project(self, B, storage=None):
        self.calls.append((np.array(B), storage))
        return self.result


def test_transform_passes_pc_through(pkg):
    X = PT.scaled_rows(50, 6, 9)
    pc, explained = gramian_of(pkg, X).principal_components(2)
    model = pkg.PCAModel(2, pc, explained)
    data = pkg.PartitionedData([pkg.DensePartition(np.zeros(50), X.astype(np.float32))])
    data.column_transform = (None, np.full(6, 2.0))
    fake = FakeEngine(pkg, 2)
    res = model.transform(data, "f64", engine=fake)
    assert res is fake.result and res.column_transform is None      # the source's transform is not copied
    assert data.column_transform is not None
    (B, storage), = fake.calls
    assert B.tobytes() == pc.tobytes() and storage == "f64"
    assert pkg.multiply(data, pc, engine=fake) is fake.result and fake.calls[-1][1] is None


# ---- the plan ------------------------------------------------------------------------------------
LDS = 163840


def gpu_shapes():
    for d, k in PT.DENSE_DK + (PT.DENSE_OFF_LDS,):
        for storage in ("f32", "f64"):
            yield "dense", storage, d, k
    for d in PT.CSR_D:
        for k in PT.CSR_K:
            for storage in ("f32", "f64"):
                yield "csr", storage, d, k


def test_plan_over_the_gpu_tests_shapes(pkg):
    N = pkg._native
    seen = set()
    for layout, storage, d, k in gpu_shapes():
        p = N.project_plan(layout, storage, d, k, 70)
        seen.add(p["path"])
        assert p["path"].startswith(layout)
        assert p["kpad"] % 16 == 0 and k <= p["kpad"] < k + 16
        assert 0 <= p["lds_bytes"] <= LDS
        assert (p["lds_bytes"] > 0) == p["path"].endswith("_lds")
        if layout == "dense":
            step = 16 if storage == "f32" else 8
            dpad = -(-d // step) * step
            assert p["rows_wave"] == 16 and p["feature_chunk"] == step and p["row_lanes"] == 0
            assert p["comp_blocks"] == {1: 1, 2: 2}.get(p["kpad"] // 16, 4)
            assert p["scratch_bytes"] == dpad * p["kpad"] * 8
            assert (p["path"] == "dense_lds") == (dpad * p["kpad"] * 8 <= LDS)
            assert p["lds_bytes"] in (0, dpad * p["kpad"] * 8)
        else:
            assert p["row_lanes"] in (1, 2, 4, 8, 16, 32, 64) and p["row_lanes"] >= min(k, 64)
            assert p["rows_wave"] * p["row_lanes"] == 64
            assert p["comp_blocks"] * p["row_lanes"] >= k and p["comp_blocks"] <= 4
            assert p["scratch_bytes"] == 0 and p["feature_chunk"] == 0
            assert (p["path"] == "csr_lds") == (d * p["kpad"] * 8 <= LDS)
    assert seen == set(N.PROJECT_PATHS)              # every path is reachable from the GPU test's shapes
    assert N.project_plan("dense", "f32", *PT.DENSE_OFF_LDS)["path"] == "dense_l2"
    assert N.project_plan("dense", "f32", 256, 256)["path"] == "dense_l2"
    # the flagship shape: c2's rows against 16 components keep B in LDS, two workgroups a CU
    assert N.project_plan("dense", "f32", 512, 16) == {
        "path": "dense_lds", "kpad": 16, "rows_wave": 16, "comp_blocks": 1, "feature_chunk": 16,
        "lds_bytes": 65536, "scratch_bytes": 65536, "row_lanes": 0}


def test_plan_at_the_largest_k(pkg):
    N = pkg._native
    for layout in ("dense", "csr"):
        for storage in ("f32", "f64"):
            for d in (1, 80, 81, 4096, 10**6):
                p = N.project_plan(layout, storage, d, N.PROJECT_MAX_K)
                assert p["kpad"] == 256 and p["lds_bytes"] <= LDS
                assert p["comp_blocks"] == 4


def test_plan_errors(pkg):
    N = pkg._native
    with pytest.raises(pkg.UnsupportedOperationException, match="256"):
        N.project_plan("dense", "f32", 512, 257)
    for d, k, nnz in ((0, 1, 0), (5, 0, 0), (5, -1, 0), (5, 1, -1)):
        with pytest.raises(pkg.IllegalArgumentException):
            N.project_plan("dense", "f32", d, k, nnz)
    L = N.lib()
    out = np.zeros(8, dtype=np.int64)
    assert L.psgd_project_plan(0, 1, 5, 1, 0, None) == N.PSGD_EINVAL
    assert L.psgd_project_plan(2, 1, 5, 1, 0, out.ctypes.data) == N.PSGD_EINVAL
    assert L.psgd_project_plan(0, 5, 5, 1, 0, out.ctypes.data) == N.PSGD_EINVAL
    assert L.psgd_project_plan(0, 1, 5, 257, 0, out.ctypes.data) == N.PSGD_EUNSUPPORTED
    assert L.psgd_project(None, 0, 1, None, None) == N.PSGD_EINVAL
    assert L.psgd_project_device(None, 1, None, 0, 2, None, None, None) == N.PSGD_EINVAL
