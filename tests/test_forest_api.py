"""The random forest's host side on the CPU: the refusals, m per strategy, the bag thresholds, the feature subsets, the
bindings; the truth's bag frequencies and its no-near-tie preconditions at the seeds the GPU tests train with."""
import ctypes
import math

import numpy as np
import pytest

import forest_truth as FT
from test_tree_api import NumpyEngine, blobs

TRAIN_SEEDS = (3, 11)        # tests/test_gpu_forest.py trains with these


def test_refusals(pkg):
    I, U = pkg.IllegalArgumentException, pkg.UnsupportedOperationException
    X, y = blobs()
    data = pkg.PartitionedData.parallelize(y, X, 2)
    train = pkg.RandomForest.trainClassifier
    for bad in (dict(categoricalFeaturesInfo={0: 3}), dict(impurity="variance"), dict(maxDepth=31), dict(numClasses=33),
                dict(maxBins=257)):
        with pytest.raises(U):
            train(data, **{"numClasses": 3, **bad}, engine=NumpyEngine(X, y))
    for bad in (dict(numTrees=0), dict(numTrees=2.5), dict(featureSubsetStrategy="half"), dict(subsamplingRate=0.0),
                dict(subsamplingRate=1.5), dict(numClasses=1), dict(maxBins=1)):
        with pytest.raises(I):
            train(data, **{"numClasses": 3, **bad}, engine=NumpyEngine(X, y))
    csr = pkg.PartitionedData([pkg.CsrPartition(np.zeros(1), np.array([0, 1], dtype=np.int64), np.zeros(1, dtype=np.int32), np.ones(1), 3)])
    with pytest.raises(U, match="dense"):
        train(csr, 2, engine=NumpyEngine(X, y))


def test_subset_sizes_cuts_and_subsets(pkg):
    want = {"all": (1, 2, 16, 17, 512), "sqrt": (1, 2, 4, 5, 23), "log2": (1, 1, 4, 5, 9), "onethird": (1, 1, 6, 6, 171)}
    for kind, ms in want.items():
        for d, m in zip((1, 2, 16, 17, 512), ms):
            assert pkg.forest_subset_size(kind, d, 5) == m == FT.subset_size(kind, d, 5), (kind, d)
    assert pkg.forest_subset_size("auto", 512, 1) == 512 and pkg.forest_subset_size("auto", 512, 2) == 23
    for T, rate in ((5, 1.0), (5, 0.5), (1, 0.6), (1, 1.0)):
        c = pkg.forest_cut(T, rate)
        assert c.dtype == np.uint64 and c.shape == (15,) and (np.diff(c.astype(object)) >= 0).all() and int(c[-1]) <= 1 << 53
        assert (c == FT.cut(T, rate)).all()
    assert int(pkg.forest_cut(1, 1.0)[0]) == 0 and int(pkg.forest_cut(1, 0.6)[1]) == 1 << 53
    assert int(pkg.forest_cut(5, 1.0)[0]) == math.ceil(math.exp(-1.0) * 2.0 ** 53)
    asked = [(t, nid) for t in range(3) for nid in (1, 2, 3, 6, 2 ** 30)]
    first = {k: pkg.forest_subset(9, *k, 17, 5) for k in asked}
    for k in reversed(asked):                       # sorted, distinct, and the same whatever was asked before
        s = pkg.forest_subset(9, *k, 17, 5)
        assert s.dtype == np.int32 and (np.diff(s) > 0).all() and 0 <= s[0] and s[-1] < 17
        assert (s == first[k]).all() and (s == FT.subset(9, *k, 17, 5)).all()
    assert len({first[k].tobytes() for k in asked}) > 1
    assert (pkg.forest_subset(9, 0, 1, 17, 17) == np.arange(17)).all()


def test_truth_bag_frequencies():
    """A condition on the truth, not the device: weights 0 .. 4 of 200,000 draws within 4 standard errors of e^-1 / k!."""
    n = 200_000
    w = FT.bag(20261126, 1, np.arange(n), FT.cut(2, 1.0))
    for k in range(5):
        p = math.exp(-1.0) / math.factorial(k)
        assert abs((w == k).mean() - p) <= 4 * math.sqrt(p * (1 - p) / n), k
    assert w.max() <= 15 and (FT.bag(5, 0, np.arange(50), FT.cut(1, 1.0)) == 1).all()
    assert set(FT.bag(5, 0, np.arange(500), FT.cut(1, 0.6))) == {0, 1}


@pytest.mark.parametrize("seed", TRAIN_SEEDS)
def test_truth_has_no_near_ties_at_the_training_seeds(pkg, seed):
    X, y = blobs()
    data = pkg.PartitionedData.parallelize(y, X, 3)
    thr, nbins = pkg.find_splits(data, 16, engine=NumpyEngine(X, y))
    forest = FT.train(X, y, 3, thr, nbins, 5, "sqrt", seed, maxDepth=4, min_inst=10)    # (best_split asserts inside)
    assert len(forest) == 5 and all(nodes[1]["feature"] >= 0 for nodes in forest)
    assert len({tuple(sorted(nodes)) for nodes in forest}) > 1                            # the bags differ


def test_plan_and_bindings(pkg):
    N = pkg._native
    p = N.forest_plan(512, 32, 2, 23, 320, 20, 39063, 10_000_000)      # the flagship's level 4: 21 nodes an item
    assert (p["subset_chunk"], p["node_subgroup"], p["groups"], p["group_trees"], p["tile_rows"]) == (23, 21, 1, 20, 32)
    assert p["lds_bytes"] <= 160 * 1024 and p["span_rows"] % 256 == 0 and p["span_rows"] * 15 < 2 ** 32
    p = N.forest_plan(40, 256, 32, 7, 2, 2, 1, 105)
    assert p["subset_chunk"] < 7 and p["node_subgroup"] == 1 and p["lds_bytes"] <= 160 * 1024
    assert N.forest_plan(300, 32, 2, 18, 20, 5, 1, 105, scratchBudget=10 * 18 * 64 * 8)["groups"] == 2
    assert N.forest_plan(3, 16, 3, 2, 1, 5, 2, 273, slotBudget=3 * 273 * 4)["group_trees"] == 3
    L = N.lib()
    out = np.zeros(11, dtype=np.int64)
    assert L.psgd_forest_plan(5, 32, 2, 6, 1, 1, 0, 0, 0, 0, out.ctypes.data) == N.PSGD_EINVAL       # m > d
    assert L.psgd_forest_plan(5, 32, 2, 2, 1, 1, 0, 0, 0, 0, None) == N.PSGD_EINVAL
    assert L.psgd_forest_plan(5, 257, 2, 2, 1, 1, 0, 0, 0, 0, out.ctypes.data) == N.PSGD_EUNSUPPORTED
    for name in ("psgd_forest_bag_device", "psgd_forest_histogram_device", "psgd_forest_best_split_device",
                 "psgd_forest_route_device", "psgd_forest_predict", "psgd_forest_predict_device", "psgd_forest_plan"):
        assert name in N.EXPORTED and getattr(L, name).argtypes and getattr(L, name).restype is ctypes.c_int32
    assert L.psgd_forest_bag_device(None, 1, None, 0, 0, 1, None, None) == N.PSGD_EINVAL
    for name in ("RandomForest", "RandomForestModel"):
        assert name in pkg.__all__
