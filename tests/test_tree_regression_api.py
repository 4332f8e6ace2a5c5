"""tree.py's regression loop on the CPU: trainRegressor driven by a numpy engine (HipEngine's methods) builds the
truth's tree, bit for bit; the argument refusals; the planner's regression mode; the new symbols (no GPU)."""
import numpy as np
import pytest

import tree_reg_truth as RT
import tree_truth as TT
from test_kmeans_api import HostTensor
from test_tree_api import NumpyEngine


class RegEngine(NumpyEngine):
    """HipEngine's regression passes over host rows, one rank."""

    def tree_targets(self):
        q, ymin, s = RT.targets(self.y)
        self.err = RT.bar(q, s)
        return self.pkg.TreeTargets(q, ymin, s)

    def tree_moments(self, targets, slots, n_slots=1):
        return np.array(RT.moments(targets.q, slots, n_slots), dtype=np.int64).view(HostTensor)

    def tree_histogram_reg(self, bins, targets, slots, group=None):
        s0, ns = group or (0, 1)
        return RT.histogram(bins[0], targets.q, slots, self.X.shape[1], bins[1].shape[1] + 1, s0, ns)

    def tree_best_split_reg(self, hist, moments, bins, targets, min_inst, min_gain):
        rec = np.zeros((len(hist), 4))
        for i, H in enumerate(hist):
            r = RT.best_split(H, int(moments[i][0]), int(moments[i][1]), bins[1], bins[2], targets.s, self.err, min_inst, min_gain)
            rec[i] = [r["feature"], r["bin"], r["threshold"], float(r["gain"])]
        return rec.view(HostTensor)


def waves(n=1500, d=17, seed=3):
    """Seeded rows whose labels take negative values over a range that is no power of two; column d - 1 is constant."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d)).astype(np.float32)
    X[:, d - 1] = 0.5
    y = 2.5 * X[:, 0] - 1.75 * X[:, 1] ** 2 + np.where(X[:, 2] > 0.3, 3.0, -1.0) + 0.25 * rng.standard_normal(n)
    return X, y.astype(np.float64)


def same_tree(model, truth, err):
    assert sorted(truth) == model.id.tolist()
    for i, nid in enumerate(model.id.tolist()):
        t = truth[nid]
        assert (model.feature[i], model.bin[i], model.threshold[i], model.n[i]) == (t["feature"], t["bin"], t["threshold"], t["n"]), nid
        assert (model.prediction[i], model.impurity[i]) == (t["prediction"], t["impurity"]), nid     # bit for bit
        assert abs(model.gain[i] - float(t["gain"])) <= err
        if t["feature"] >= 0:
            assert model.id[model.left[i]] == 2 * nid and model.id[model.right[i]] == 2 * nid + 1


@pytest.mark.parametrize("maxDepth,minInst", [(0, 1), (4, 1), (4, 40)])
def test_train_builds_the_truths_tree(pkg, maxDepth, minInst):
    X, y = waves(400, 5)
    data = pkg.PartitionedData.parallelize(y, X, 3)
    eng = RegEngine(X, y)
    eng.pkg = pkg
    model = pkg.DecisionTree.trainRegressor(data, {}, "variance", maxDepth, 8, minInst, engine=eng)
    thr, nbins = pkg.find_splits(data, 8, engine=eng)
    same_tree(model, RT.train(X, y, thr, nbins, maxDepth, minInst), eng.err)
    assert model.algo == "Regression" and model.numClasses == 0 and model.prediction.dtype == np.float64
    assert model.depth <= maxDepth and "regressor" in model.toDebugString()
    grouped = pkg.DecisionTree.trainRegressor(data, {}, "variance", maxDepth, 8, minInst, engine=eng, scratchBudget=5 * 8 * 16)
    assert all(grouped.nodes[k].tobytes() == model.nodes[k].tobytes() for k in model.nodes)


def test_argument_refusals(pkg):
    I, U = pkg.IllegalArgumentException, pkg.UnsupportedOperationException
    X, y = waves(50, 3)
    data = pkg.PartitionedData.parallelize(y, X, 2)
    train = pkg.DecisionTree.trainRegressor
    for bad in (dict(categoricalFeaturesInfo={0: 3}), dict(maxDepth=31), dict(maxBins=257)):
        with pytest.raises(U):
            train(data, **bad, engine=RegEngine(X, y))
    for bad in (dict(impurity="gini"), dict(impurity="mse"), dict(maxDepth=-1), dict(maxBins=1), dict(minInstancesPerNode=0),
                dict(minInfoGain=-1.0)):
        with pytest.raises(I):
            train(data, **bad, engine=RegEngine(X, y))
    with pytest.raises(U):
        pkg.DecisionTree.trainClassifier(data, 2, impurity="variance", engine=RegEngine(X, y))


def test_plan_regression_mode_and_symbols(pkg):
    N = pkg._native
    for d, B, A in ((512, 32, 1), (17, 32, 64), (16, 32, 1), (40, 256, 3)):
        p = N.tree_plan("f32", d, B, 0, A, 10)
        cells = p["replication"] * p["slot_subgroup"] * p["feature_chunk"] * B
        assert p["lds_bytes"] == 12 * cells <= 65536 and p["scratch_bytes"] == p["group_slots"] * d * B * 16
    assert N.tree_plan("f32", 16, 32, 0, 1, 10)["replication"] == 2 and N.tree_plan("f32", 40, 256, 0, 3, 10)["feature_chunk"] == 16
    assert N.tree_plan("f32", 40, 32, 0, 5, 10, budget=2 * 40 * 32 * 16)["groups"] == 3
    for name in ("psgd_tree_label_range_device", "psgd_tree_targets_device", "psgd_tree_moments_device",
                 "psgd_tree_histogram_reg_device", "psgd_tree_best_split_reg_device"):
        assert name in N.EXPORTED and hasattr(N.lib(), name)
    assert pkg.target_scale(-1.5, 4.5) == 27 and pkg.target_scale(2.0, 2.0) == 0 and pkg.target_scale(0.0, 2.0 ** 30) == -1
