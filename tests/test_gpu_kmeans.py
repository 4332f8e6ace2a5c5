"""The k-means passes on the GPU against numpy's long-double restatement (tests/kmeans_truth.py, which
has the shapes and the bars). Whole numbers in -3 .. 3 make everything exact, ties included: bit for bit.
Real data: the gaps are asserted first, then assign is exact and dist2, sums and cost meet their bars.
A second call and the host forms return the same bytes (CSR: all but the sums)."""
import ctypes
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, has_gpu

import kmeans_truth as KT
from test_gpu_project import _free_port, csr_data, csr_case, dense_data, np_dtype, offsets

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not has_gpu():
        pytest.skip("no GPU")


@functools.lru_cache(maxsize=None)
def dense_case(n, d, k, storage, whole):
    rng = np.random.default_rng(7300 + 11 * d + k + (3 if storage == "f32" else 0) + (100000 if whole else 0))
    if whole:
        X = rng.integers(-3, 4, size=(n, d)).astype(np_dtype(storage))
        C = rng.integers(-3, 4, size=(k, d)).astype(np.float64)
        if k > 1:
            C[k - 1] = C[0]   # two bitwise-equal centres: the higher index gets nothing
    else:
        X = (rng.standard_normal((n, d)) * rng.uniform(0.5, 2.0, size=d) + rng.uniform(-1.0, 1.0, size=d)).astype(np_dtype(storage))
        C = rng.standard_normal((k, d)) * 1.5
    return {"X": X, "C": C, "y": np.zeros(n)}


def check_all(pkg, engine, X, C, whole, what, sums_repeat=True):
    """Everything the passes promise, on one engine: (assign, dist2, step) against the truth."""
    k, d = C.shape
    a, d2 = engine.kmeans_assign(C, distances=True)
    a, d2 = a.cpu().numpy(), d2.cpu().numpy()
    step = engine.kmeans_step(C).cpu().numpy()
    sums, counts, cost, n = step[: k * d].reshape(k, d), step[k * d: k * d + k], step[k * d + k], step[k * d + k + 1]
    t_sums, t_counts, t_cost, t_n, t_a, t_d2 = KT.step(X, C)
    assert n == t_n == len(X) and np.isfinite(step).all() and np.isfinite(d2).all()
    if whole:
        assert (a == t_a).all(), f"{what}: {int((a != t_a).sum())} assignments differ, first at row {np.argwhere(a != t_a)[0, 0]}"
        assert (d2 == t_d2.astype(np.float64)).all() and cost == float(t_cost)
        assert (sums == t_sums.astype(np.float64)).all() and (counts == t_counts).all()
        if k > 1:
            assert counts[k - 1] == 0
    else:
        g_a, _, bar = KT.check_gaps(X, C)
        assert (a == g_a).all() and (counts == t_counts).all()
        err = np.abs(d2 - t_d2.astype(np.float64))
        sbar = np.zeros((k, d))
        np.add.at(sbar, t_a, 1e-9 * np.abs(X.astype(np.float64)))
        serr = np.abs(sums - t_sums.astype(np.float64))
        print(f"{what}: worst dist2 error / bar = {np.max(err / bar):.3g}, sums = {np.max(serr / np.maximum(sbar, 1e-300)):.3g}, "
              f"cost = {abs(cost - float(t_cost)) / bar.sum():.3g}")
        assert (err <= bar).all() and (serr <= sbar).all() and abs(cost - float(t_cost)) <= bar.sum()
    # the same bytes from call to call, and from the host forms
    a2, d22 = engine.kmeans_assign(C, distances=True)
    step2 = engine.kmeans_step(C).cpu().numpy()
    h_a, h_d2 = engine.ctx.kmeans_assign(C, distances=True)
    h_step = engine.ctx.kmeans_step(C)
    for got in ((a2.cpu().numpy(), d22.cpu().numpy(), step2), (h_a, h_d2, h_step)):
        assert got[0].tobytes() == a.tobytes() and got[1].tobytes() == d2.tobytes()
        assert got[2][k * d:].tobytes() == step[k * d:].tobytes()
        if sums_repeat:
            assert got[2].tobytes() == step.tobytes()
    assert engine.kmeans_assign(C)[1] is None
    return step


@pytest.mark.parametrize("whole", [True, False], ids=["whole", "real"])
@pytest.mark.parametrize("d,k,storage", KT.DENSE_DKS, ids=[f"d{d}-k{k}-{s}" for d, k, s in KT.DENSE_DKS])
def test_dense(pkg, d, k, storage, whole):
    c = dense_case(sum(KT.SIZES), d, k, storage, whole)
    assert pkg._native.kmeans_plan("dense", storage, d, k, 15)["path"] == "dense_lds"
    check_all(pkg, pkg.HipEngine(dense_data(pkg, c, KT.SIZES)), c["X"], c["C"], whole, f"dense d={d} k={k} {storage}")


@pytest.mark.parametrize("storage", ["f32", "f64"])
def test_dense_off_lds(pkg, storage):
    """C^T too large for LDS (asserted from the plan): the MFMA operands come through L2."""
    d, k = KT.DENSE_OFF_LDS
    assert pkg._native.kmeans_plan("dense", storage, d, k, 7)["path"] == "dense_l2"
    sizes = (37, 0, 63)
    for whole in (True, False):
        c = dense_case(sum(sizes), d, k, storage, whole)
        check_all(pkg, pkg.HipEngine(dense_data(pkg, c, sizes)), c["X"], c["C"], whole, f"off-LDS {storage} whole={whole}")


def test_dense_spans_of_many_tiles(pkg):
    """More tiles than the sums' plan has items: a span is a run of tiles that crosses partitions."""
    d, k, sizes = 3, 2, (50001, 0, 7, 89990, 13)
    n_tiles = sum(-(-s // 16) for s in sizes)
    plan = pkg._native.kmeans_plan("dense", "f32", d, k, n_tiles)
    assert plan["span_tiles"] > 1 and plan["spans"] * plan["span_tiles"] >= n_tiles
    c = dense_case(sum(sizes), d, k, "f32", True)
    check_all(pkg, pkg.HipEngine(dense_data(pkg, c, sizes)), c["X"], c["C"], True, "many tiles")


@pytest.mark.parametrize("d,storage,ld", [(13, "f32", 16), (30, "f64", 32), (101, "f32", 104)])
def test_dense_zero_copy_pitch(pkg, d, storage, ld):
    """Rows with ld > d and NaN in the pad: nothing non-finite comes out of either pass."""
    import torch
    k = 17
    c = dense_case(sum(KT.SIZES), d, k, storage, False)
    dev = torch.device("cuda", 0)
    o = offsets(KT.SIZES)
    parts = []
    for a, b in zip(o[:-1], o[1:]):
        X = torch.full((b - a, ld), float("nan"), dtype=torch.float32 if storage == "f32" else torch.float64, device=dev)
        X[:, :d] = torch.from_numpy(np.array(c["X"][a:b])).to(dev)
        parts.append(pkg.DevicePartition(torch.zeros(b - a, dtype=torch.float64, device=dev), X, d))
    check_all(pkg, pkg.HipEngine(pkg.PartitionedData(parts)), c["X"], c["C"], False, f"zero-copy d={d} ld={ld}")


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("d,k,storage,path", [(70, 16, "f64", "csr_lds_sums"), (70, 3, "f32", "csr_lds_sums"),
                                              (70, 200, "f32", "csr_global_sums"), (1300, 17, "f64", "csr_global_sums")])
def test_csr(pkg, d, k, storage, path, device):
    """Ragged rows of 0, 1, 2, 17, d and 70 entries with one stored 0.0; both sums paths, asserted from the plan."""
    assert pkg._native.kmeans_plan("csr", storage, d, k, 3)["path"] == path
    sizes = (1, 3, 0, 15, 16, 17, 65, 300)
    for whole in (True, False):
        c = csr_case(sum(sizes), d, k, storage, whole)
        rng = np.random.default_rng(d + k)
        C = rng.integers(-3, 4, size=(k, d)).astype(np.float64) if whole else rng.standard_normal((k, d)) * 0.3
        if whole:
            C[k - 1] = C[0]
        # (whole numbers add exactly in any order: there the atomics' sums repeat too)
        check_all(pkg, pkg.HipEngine(csr_data(pkg, c, sizes, device)), c["X"], C, whole,
                  f"csr d={d} k={k} {storage} whole={whole}", sums_repeat=whole)


@pytest.mark.parametrize("layout", ["dense", "csr"])
def test_registry_of_empty_partitions_and_errors(pkg, layout):
    import torch
    N = pkg._native
    if layout == "dense":
        part = pkg.DensePartition(np.zeros(0), np.zeros((0, 5), dtype=np.float32))
    else:
        part = pkg.CsrPartition(np.zeros(0), np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0), 5)
    engine = pkg.HipEngine(pkg.PartitionedData([part, part]))
    C = np.ones((3, 5))
    assert (engine.kmeans_step(C).cpu().numpy() == 0.0).all() and engine.kmeans_assign(C)[0].numel() == 0
    assert (engine.ctx.kmeans_step(C) == 0.0).all()
    L, h = N.lib(), engine.ctx.handle
    Cd = torch.from_numpy(C).to(engine.dev)
    out = torch.zeros(3 * 6 + 2, dtype=torch.float64, device=engine.dev)
    assert L.psgd_kmeans_step_device(h, 3, Cd.data_ptr(), out.data_ptr(), None) == 0
    assert L.psgd_kmeans_step_device(h, 3, None, out.data_ptr(), None) == N.PSGD_EINVAL
    assert L.psgd_kmeans_step_device(h, 3, Cd.data_ptr(), None, None) == N.PSGD_EINVAL
    assert L.psgd_kmeans_step_device(h, 0, Cd.data_ptr(), out.data_ptr(), None) == N.PSGD_EINVAL
    assert L.psgd_kmeans_step_device(h, 257, Cd.data_ptr(), out.data_ptr(), None) == N.PSGD_EUNSUPPORTED
    assert L.psgd_kmeans_assign(h, 3, C.ctypes.data, None, None) == N.PSGD_EINVAL
    assert L.psgd_kmeans_assign_device(h, 3, Cd.data_ptr(), None, None, None) == N.PSGD_EINVAL
    assert (engine.kmeans_step(C.tolist()).cpu().numpy() == 0.0).all()      # a list of lists is converted first
    with pytest.raises(pkg.IllegalArgumentException):
        engine.kmeans_step([[1.0, 2.0]])
    assert L.psgd_kmeans_update_device(h, 3, 5, Cd.data_ptr(), out.data_ptr(), Cd.data_ptr(), out.data_ptr(), None) == N.PSGD_EINVAL
    fresh = ctypes.c_void_p()
    assert L.psgd_ctx_create(0, ctypes.byref(fresh)) == 0
    try:
        assert L.psgd_kmeans_step_device(fresh, 3, Cd.data_ptr(), out.data_ptr(), None) == N.PSGD_ESTATE
        assert L.psgd_kmeans_assign_device(fresh, 3, Cd.data_ptr(), out.data_ptr(), None, None) == N.PSGD_ESTATE
    finally:
        L.psgd_ctx_destroy(fresh)


# ---- end to end -------------------------------------------------------------------------------------
def blobs(n=400, d=6, seed=8):
    rng = np.random.default_rng(seed)
    means = rng.uniform(-10.0, 10.0, size=(3, d))
    X = np.concatenate([m + rng.standard_normal((n, d)) for m in means]).astype(np.float32)
    return X[rng.permutation(len(X))], means


@pytest.mark.parametrize("storage", ["f32", "f64"])
def test_kmeans_run_matches_the_restatement(pkg, storage):
    X, means = blobs()
    start = means + np.random.default_rng(1).standard_normal(means.shape)
    data = pkg.PartitionedData.parallelize(np.zeros(len(X)), X, 4, dtype=np_dtype(storage))
    model = pkg.KMeans(3, 20, 1e-4).setInitialModel(pkg.KMeansModel(start)).run(data)
    C, cost, it = KT.lloyd(X, start, 20, 1e-4)
    assert model.numIterations == it and 1 < it < 20
    np.testing.assert_allclose(model.clusterCenters, C.astype(np.float64), rtol=1e-9, atol=0)
    assert abs(model.trainingCost - float(cost)) <= 1e-9 * float(cost)
    assert abs(model.computeCost(data) - float(KT.step(X, C)[2])) <= 1e-9 * float(cost)
    pred = np.concatenate([t.cpu().numpy() for t in model.predict(data)])
    assert (pred == KT.assign(X, model.clusterCenters)[0]).all()


def test_kmeans_after_pca_and_random_initialisation(pkg):
    """KMeans runs on PCA's projected device partitions as they are; "random" reads the registered rows."""
    X, _ = blobs()
    data = pkg.PartitionedData.parallelize(np.zeros(len(X)), X, 3, dtype=np.float32)
    proj = pkg.PCA(2).fit(data).transform(data, "f64")
    rows = np.concatenate([p.x.cpu().numpy()[:, :2] for p in proj.partitions])
    model = pkg.KMeans(3, 20, seed=4).run(proj)
    pos = np.sort(np.random.default_rng(4).choice(len(X), size=3, replace=False))
    C, cost, it = KT.lloyd(rows, rows[pos], 20, 1e-4)
    assert model.numIterations == it
    np.testing.assert_allclose(model.clusterCenters, C.astype(np.float64), rtol=1e-9, atol=1e-12)
    # a scaled data set: the centres are drawn from the scaled rows, not the host rows
    scaler = pkg.StandardScaler(withMean=True, withStd=True).fit(data)
    init = pkg.KMeans(3, 0, seed=4).run(scaler.transform(data)).clusterCenters
    want = ((X[pos].astype(np.float64) - scaler.shift) * scaler.factor).astype(np.float32)
    assert (init == want).all()


@pytest.mark.parametrize("P", [5, 1])
def test_two_ranks(tmp_path, pkg, P):
    """Two ranks sharing cuda:0 over gloo, each a fresh child process (tests/two_rank_kmeans.py): both hold
    the same step, initial centres and model bytes, within the one-rank bars of the restatement, and each
    predicts its own block of partitions."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import two_rank_kmeans as T
    out = str(tmp_path / "res.json")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), PSGD_TEST_P=str(P))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "two_rank_kmeans.py"), out], env=env,
                       capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    with open(out) as f:
        res = json.load(f)
    X, means = T.make_data()
    n, k, d = len(X), T.K, X.shape[1]
    for key in ("step", "start", "centres", "cost", "iterations"):   # floats survive JSON exactly: identical bits
        assert res["0"][key] == res["1"][key], key
    got = res["0"]
    t_sums, t_counts, t_cost, _, t_a, _ = KT.step(X, means)
    _, _, bar = KT.check_gaps(X, means)
    step = np.array(got["step"])
    sbar = np.zeros((k, d))
    np.add.at(sbar, t_a, 1e-9 * np.abs(X.astype(np.float64)))
    assert (np.abs(step[: k * d].reshape(k, d) - t_sums.astype(np.float64)) <= sbar).all()
    assert (step[k * d: k * d + k] == t_counts).all() and abs(step[k * d + k] - float(t_cost)) <= bar.sum() and step[-1] == n
    pos = np.sort(np.random.default_rng(T.SEED).choice(n, size=k, replace=False))
    assert (np.array(got["start"]).reshape(k, d) == X[pos]).all()     # every row has one owner: exact
    C, cost, it = KT.lloyd(X, X[pos], 20, 1e-4)
    assert got["iterations"] == it
    np.testing.assert_allclose(np.array(got["centres"]).reshape(k, d), C.astype(np.float64), rtol=1e-9, atol=0)
    assert abs(got["cost"] - float(cost)) <= 1e-9 * float(cost)
    truth = KT.assign(X, np.array(got["centres"]).reshape(k, d))[0]
    bounds = [((i * n) // P, ((i + 1) * n) // P) for i in range(P)]
    seen = 0
    for rank in ("0", "1"):
        lo, hi = res[rank]["block"]
        assert res[rank]["rows"] == [bounds[p][1] - bounds[p][0] if lo <= p < hi else 0 for p in range(P)]
        a, b = (bounds[lo][0], bounds[hi - 1][1]) if hi > lo else (0, 0)
        assert res[rank]["pred"] == truth[a:b].tolist()
        seen += hi - lo
    assert seen == P
