"""clustering.py on the CPU: KMeans.run driven by a numpy engine (the methods HipEngine offers) follows
its specification -- the stopping rule, an empty cluster keeping its centre, the argument checks and
the k-means|| refusal -- and psgd_kmeans_plan's paths and errors, which need no device (no GPU)."""
import numpy as np
import pytest

import kmeans_truth as KT


class HostTensor(np.ndarray):
    """What the loop asks of a device tensor."""

    def cpu(self):
        return self

    def numpy(self):
        return np.asarray(self)


def host(a):
    return np.array(a, dtype=np.float64).view(HostTensor)


class NumpyEngine:
    """HipEngine's k-means passes over host rows, one rank."""

    def __init__(self, X):
        self.X, self.lo, self.hi, self.steps = np.asarray(X, dtype=np.float64), 0, 1, 0

    def device_rows(self, values):
        return host(values)

    def registered_rows(self, positions):
        return self.X[np.asarray(positions)]

    def kmeans_step(self, centres):
        self.steps += 1
        sums, counts, cost, n, _, _ = KT.step(self.X, np.asarray(centres))
        return host(np.concatenate([sums.ravel(), counts, [cost, n]]))

    def kmeans_update(self, centres, step):
        k, d = centres.shape
        new, moved = KT.update(np.asarray(centres), np.asarray(step[: k * d]).reshape(k, d), np.asarray(step[k * d: k * d + k]))
        return host(new), host(moved)


def blobs(seed=3, n=60):
    rng = np.random.default_rng(seed)
    means = np.array([[0.0, 0.0], [8.0, 0.0], [0.0, 8.0]])
    return np.concatenate([m + 0.3 * rng.standard_normal((n, 2)) for m in means]), means


def data_of(pkg, X, P=3):
    return pkg.PartitionedData.parallelize(np.zeros(len(X)), X, P)


@pytest.mark.parametrize("maxIterations,epsilon", [(20, 1e-4), (1, 1e-4), (0, 1e-4), (20, 100.0)])
def test_run_follows_the_stopping_rule(pkg, maxIterations, epsilon):
    X, means = blobs()
    eng = NumpyEngine(X)
    start = pkg.KMeansModel(means + 0.5)
    model = pkg.KMeans(3, maxIterations, epsilon).setInitialModel(start).run(data_of(pkg, X), engine=eng)
    C, cost, it = KT.lloyd(X, means + 0.5, maxIterations, epsilon)
    assert model.numIterations == it == eng.steps and model.k == 3
    # no step; one step; a step that moves no centre by more than epsilon ends the loop; else it converges
    want = {(0, 1e-4): 0, (1, 1e-4): 1, (20, 100.0): 1}.get((maxIterations, epsilon))
    assert it == want if want is not None else 2 <= it < 20
    assert np.allclose(model.clusterCenters, C.astype(np.float64), rtol=1e-12, atol=0)
    if it == 0:
        assert model.trainingCost is None
    else:   # the cost at the centres the last step started from
        assert model.trainingCost == pytest.approx(float(cost), rel=1e-12)


def test_an_empty_cluster_keeps_its_centre(pkg):
    X, means = blobs()
    far = np.array([[1e3, 1e3]])
    model = pkg.KMeans(4).setInitialModel(pkg.KMeansModel(np.concatenate([means, far]))).run(
        data_of(pkg, X), engine=NumpyEngine(X))
    assert (model.clusterCenters[3] == far[0]).all()
    step = pkg.kmeans_step(data_of(pkg, X), model.clusterCenters, engine=NumpyEngine(X))
    assert step.counts[3] == 0 and step.count == len(X) and step.sums.shape == (4, 2)


def test_argument_checks(pkg):
    I, U = pkg.IllegalArgumentException, pkg.UnsupportedOperationException
    for bad in (dict(k=0), dict(k=257), dict(k=2.5), dict(k=True), dict(maxIterations=-1), dict(epsilon=-1.0),
                dict(epsilon=float("nan")), dict(initializationMode="farthest")):
        with pytest.raises(I):
            pkg.KMeans(**bad)
    with pytest.raises(U, match="setInitialModel"):
        pkg.KMeans(3, initializationMode="k-means||")
    with pytest.raises(U):
        pkg.KMeans.train(None, 3, initializationMode="k-means||")
    with pytest.raises(I):
        pkg.KMeans(3).setInitialModel(pkg.KMeansModel(np.zeros((2, 2))))
    X, means = blobs()
    with pytest.raises(I):   # the centres' width, before any engine is touched
        pkg.KMeans(3).setInitialModel(pkg.KMeansModel(np.zeros((3, 5)))).run(data_of(pkg, X), engine=None)
    with pytest.raises(I):
        pkg.KMeansModel(np.zeros((3, 5))).computeCost(data_of(pkg, X), engine=NumpyEngine(X))
    with pytest.raises(I):
        pkg.KMeansModel(np.zeros(4))


def test_plan_paths_and_errors(pkg):
    N = pkg._native
    plan = N.kmeans_plan
    for d, k, storage in KT.DENSE_DKS:
        p = plan("dense", storage, d, k, 15)
        nb, nbf = (k + 15) // 16, (d + 1 + 15) // 16
        assert p["path"] == "dense_lds" and p["tile_rows"] == 16 and p["kpad"] == 16 * nb
        assert p["centre_blocks"] == min(nb, 4) if nb != 3 else p["centre_blocks"] == 4
        assert p["gr"] == (1 if nb == 1 else 2 if nb == 2 else 4) and p["gc"] == (2 if nbf <= 2 else 8)
        assert p["spans"] == 15 and p["items"] == 15 * -(-nb // p["gr"]) * -(-nbf // p["gc"])
    d, k = KT.DENSE_OFF_LDS
    assert plan("dense", "f32", d, k, 4)["path"] == "dense_l2" and plan("dense", "f32", d, k, 4)["lds_bytes"] == 0
    # the scratch is bounded: the items are capped however many tiles there are
    big = plan("dense", "f32", 512, 256, 625000)
    assert big["items"] <= 2048 + 4 * 5 and big["span_tiles"] * big["spans"] >= 625000
    assert plan("csr", "f64", 70, 16, 3)["path"] == "csr_lds_sums" and plan("csr", "f64", 70, 16, 3)["tile_rows"] == 256
    assert plan("csr", "f64", 1300, 16, 3)["path"] == "csr_global_sums"
    assert plan("csr", "f32", 70, 200, 3)["row_lanes"] == 64 and plan("csr", "f32", 70, 3, 3)["row_lanes"] == 4
    L = N.lib()
    out = np.zeros(12, dtype=np.int64)
    assert L.psgd_kmeans_plan(0, 1, 5, 1, 0, None) == N.PSGD_EINVAL
    for bad in ((2, 1, 5, 1, 0), (0, 5, 5, 1, 0), (0, 1, 0, 1, 0), (0, 1, 5, 0, 0), (0, 1, 5, 1, -1)):
        assert L.psgd_kmeans_plan(*bad, out.ctypes.data) == N.PSGD_EINVAL
    assert L.psgd_kmeans_plan(0, 1, 5, 257, 0, out.ctypes.data) == N.PSGD_EUNSUPPORTED
