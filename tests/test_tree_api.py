"""tree.py on the CPU: trainClassifier driven by a numpy engine (HipEngine's methods) builds the truth's tree; the
argument refusals; find_splits on few and on many distinct values; psgd_tree_plan's paths and errors (no GPU)."""
import numpy as np
import pytest

import tree_truth as TT
from test_kmeans_api import HostTensor


class NumpyEngine:
    """HipEngine's tree passes over host rows, one rank."""

    def __init__(self, X, y):
        self.X, self.y, self.lo, self.hi = np.asarray(X, dtype=np.float64), np.asarray(y), 0, 1 << 30

    def registered_rows(self, positions):
        return self.X[np.asarray(positions)]

    def tree_bin(self, thr, nbins):
        return (TT.bin_rows(self.X, thr, nbins), thr, nbins)

    def tree_slots(self):
        return np.zeros(len(self.X), dtype=np.int32)

    def tree_histogram(self, bins, slots, K, group=None):
        s0, ns = group or (0, 1)
        return TT.histogram(bins[0], self.y, slots, self.X.shape[1], bins[1].shape[1] + 1, K, s0, ns)

    def tree_best_split(self, hist, bins, impurity, min_inst, min_gain):
        K = hist.shape[3]
        rec = np.zeros((len(hist), 6 + 2 * K))
        for s, H in enumerate(hist):
            r = TT.best_split(H, bins[1], bins[2], impurity, min_inst, min_gain)
            rec[s] = [r["feature"], r["bin"], r["threshold"], r["gain"], r["impurity"], r["n"], *r["tot"], *r["L"]]
        return rec.view(HostTensor)

    def tree_route(self, bins, slots, table):
        slots[:] = TT.route(bins[0], slots, table)


def blobs(sizes=(70, 90, 113), seed=5):
    """Three blobs of unequal sizes (equal ones would make splitting off either outer blob an exact tie)."""
    rng = np.random.default_rng(seed)
    means = np.array([[0.0, 0.0, 1.0], [6.0, 0.0, -1.0], [0.0, 6.0, 0.0]])
    X = np.concatenate([m + rng.standard_normal((n, 3)) for m, n in zip(means, sizes)]).astype(np.float32)
    y = np.repeat(np.arange(3.0), sizes)
    p = rng.permutation(len(X))
    return X[p], y[p]


def same_tree(model, truth, K):
    assert sorted(truth) == model.id.tolist()
    for i, nid in enumerate(model.id.tolist()):
        t = truth[nid]
        assert (model.feature[i], model.bin[i], model.threshold[i]) == (t["feature"], t["bin"], t["threshold"]), nid
        assert (model.counts[i] == t["counts"]).all() and model.prediction[i] == int(np.argmax(t["counts"]))
        assert abs(model.gain[i] - float(t["gain"])) <= TT.bar(K)
        if t["feature"] >= 0:
            assert model.id[model.left[i]] == 2 * nid and model.id[model.right[i]] == 2 * nid + 1


@pytest.mark.parametrize("impurity", ["gini", "entropy"])
@pytest.mark.parametrize("maxDepth", [0, 4])
def test_train_builds_the_truths_tree(pkg, impurity, maxDepth):
    X, y = blobs()
    data = pkg.PartitionedData.parallelize(y, X, 3)
    model = pkg.DecisionTree.trainClassifier(data, 3, {}, impurity, maxDepth, 8, engine=NumpyEngine(X, y))
    thr, nbins = pkg.find_splits(data, 8, engine=NumpyEngine(X, y))
    same_tree(model, TT.train(X, y, 3, thr, nbins, impurity, maxDepth), 3)
    assert model.depth <= maxDepth and (model.numNodes == 1) == (maxDepth == 0)
    assert model.toDebugString().count("Predict:") == int((model.feature < 0).sum())
    # a frontier in groups of one slot (a budget of one slot's table) is the same tree
    grouped = pkg.DecisionTree.trainClassifier(data, 3, {}, impurity, maxDepth, 8, engine=NumpyEngine(X, y),
                                               scratchBudget=3 * 8 * 3 * 8)
    assert all((grouped.nodes[k] == model.nodes[k]).all() for k in model.nodes)


def test_argument_refusals(pkg):
    I, U = pkg.IllegalArgumentException, pkg.UnsupportedOperationException
    X, y = blobs()
    data = pkg.PartitionedData.parallelize(y, X, 2)
    train = pkg.DecisionTree.trainClassifier
    for bad in (dict(categoricalFeaturesInfo={0: 3}), dict(impurity="variance"), dict(maxDepth=31), dict(numClasses=33),
                dict(maxBins=257)):
        with pytest.raises(U):
            train(data, **{"numClasses": 3, **bad}, engine=NumpyEngine(X, y))
    for bad in (dict(numClasses=1), dict(numClasses=2.5), dict(impurity="mse"), dict(maxDepth=-1), dict(maxBins=1),
                dict(minInstancesPerNode=0), dict(minInfoGain=-1.0)):
        with pytest.raises(I):
            train(data, **{"numClasses": 3, **bad}, engine=NumpyEngine(X, y))
    csr = pkg.PartitionedData([pkg.CsrPartition(np.zeros(1), np.array([0, 1], dtype=np.int64), np.zeros(1, dtype=np.int32), np.ones(1), 3)])
    with pytest.raises(U, match="dense"):
        train(csr, 2, engine=NumpyEngine(X, y))


def test_find_splits_on_few_and_on_many_distinct_values(pkg):
    rng = np.random.default_rng(2)
    X = np.stack([rng.integers(0, 5, 400).astype(np.float64), rng.standard_normal(400)], axis=1)
    data = pkg.PartitionedData.parallelize(np.zeros(400), X, 2, dtype=np.float64)
    thr, nbins = pkg.find_splits(data, 8, engine=NumpyEngine(X, np.zeros(400)))
    assert nbins[0] == 6 and (thr[0, :5] == np.arange(5.0)).all() and np.isinf(thr[0, 5:]).all()   # all five values, then +Inf
    # 400 distinct values: the stride walk takes maxBins - 1 of them, ascending, near the 1/8 quantiles
    assert nbins[1] == 8 and (np.diff(thr[1]) > 0).all() and np.isin(thr[1], X[:, 1]).all()
    counts = np.bincount(TT.bin_rows(X, thr, nbins)[:, 1], minlength=8)
    assert counts.min() >= 45 and counts.max() <= 55


def test_plan_paths_and_errors(pkg):
    N = pkg._native
    plan = N.tree_plan
    p = plan("f32", 512, 32, 2, 1, 39063)            # the root of the flagship: 16 vectors a chunk, one copy
    assert (p["feature_chunk"], p["slot_subgroup"], p["replication"], p["lds_bytes"], p["groups"]) == (256, 1, 1, 65536, 1)
    assert p["pitch"] == 512 and p["items"] <= 1024 and p["span_rows"] % 256 == 0
    p = plan("f32", 17, 32, 2, 64, 10)               # a small table: all 32 feature bytes, 8 slots, no second copy
    assert (p["feature_chunk"], p["slot_subgroup"], p["replication"], p["pitch"]) == (32, 8, 1, 32)
    assert plan("f64", 16, 32, 2, 1, 10)["replication"] == 2          # everything fits twice
    p = plan("f32", 40, 256, 32, 3, 10)              # 16 features' cells exceed LDS: two features of a vector
    assert (p["feature_chunk"], p["slot_subgroup"], p["replication"], p["lds_bytes"]) == (2, 1, 1, 65536)
    per_slot = 40 * 32 * 3 * 8
    p = plan("f32", 40, 32, 3, 5, 10, budget=2 * per_slot)
    assert (p["groups"], p["group_slots"], p["scratch_bytes"]) == (3, 2, 2 * per_slot)
    assert plan("f32", 40, 32, 3, 5, 10, budget=1)["groups"] == 5 and plan("f32", 40, 32, 3, 5, 10)["groups"] == 1
    L = N.lib()
    out = np.zeros(10, dtype=np.int64)
    assert L.psgd_tree_plan(1, 5, 32, 2, 1, 0, 0, None) == N.PSGD_EINVAL
    for bad in ((5, 5, 32, 2, 1, 0, 0), (1, 0, 32, 2, 1, 0, 0), (1, 5, 1, 2, 1, 0, 0), (1, 5, 32, 1, 1, 0, 0),
                (1, 5, 32, 2, 0, 0, 0), (1, 5, 32, 2, 1, -1, 0)):
        assert L.psgd_tree_plan(*bad, out.ctypes.data) == N.PSGD_EINVAL
    assert L.psgd_tree_plan(1, 5, 257, 2, 1, 0, 0, out.ctypes.data) == N.PSGD_EUNSUPPORTED
    assert L.psgd_tree_plan(1, 5, 32, 33, 1, 0, 0, out.ctypes.data) == N.PSGD_EUNSUPPORTED
