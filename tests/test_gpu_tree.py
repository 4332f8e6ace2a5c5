"""The decision tree's passes on the GPU against tests/tree_truth.py, each alone and exactly (integers); the gains
and impurities meet tree_truth.bar. Then trainClassifier node for node, a second call byte for byte, bad labels, two ranks."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, has_gpu

import tree_truth as TT
from test_gpu_project import _free_port, dense_data, np_dtype, offsets
from test_tree_api import blobs, same_tree

pytestmark = pytest.mark.gpu
SIZES = (37, 0, 63, 5)
CASES = [(1, "f64", 2, 2, 1, None), (16, "f32", 32, 3, 5, None), (17, "f32", 32, 2, 11, 20), (40, "f64", 256, 32, 3, None),
         (40, "f32", 32, 3, 2, 48), (300, "f32", 32, 2, 2, None)]   # d, storage, maxBins, K, slots, zero-copy pitch


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not has_gpu():
        pytest.skip("no GPU")


@functools.lru_cache(maxsize=None)
def rows_case(d, storage, B, K, A):
    """Values on a grid of quarters (rows sit on thresholds), -0.0 among them; ragged nb_f, a single-bin last feature."""
    rng = np.random.default_rng(100 * d + B + K)
    n = sum(SIZES)
    X = (np.round(rng.standard_normal((n, d)) * 8) / 4).astype(np_dtype(storage))
    X[::7, 0] = -0.0
    thr, nbins = TT.ragged_thresholds(X, B, seed=K)
    t = np.unique(np.append(thr[0, : nbins[0] - 1], 0.0))      # -0.0 rows against a threshold of 0.0
    t = t[: B - 1] if 0.0 in t[: B - 1] else np.sort(np.append(t[: B - 2], 0.0))
    thr[0], nbins[0] = np.inf, len(t) + 1
    thr[0, : len(t)] = t
    if d > 1:
        nbins[d - 1] = 1
    y = rng.integers(0, K, n).astype(np.float64)
    slots = rng.integers(-1, A, n).astype(np.int32)
    return dict(X=X, y=y, thr=thr, nbins=nbins, slots=slots)


def engine_of(pkg, c, d, storage, ld):
    import torch
    if ld is None:
        return pkg.HipEngine(dense_data(pkg, c, SIZES))
    dev, o, parts = torch.device("cuda", 0), offsets(SIZES), []
    for a, b in zip(o[:-1], o[1:]):   # NaN in the pad columns: they must never be read
        X = torch.full((b - a, ld), float("nan"), dtype=torch.float32 if storage == "f32" else torch.float64, device=dev)
        X[:, :d] = torch.from_numpy(np.array(c["X"][a:b])).to(dev)
        parts.append(pkg.DevicePartition(torch.from_numpy(c["y"][a:b].copy()).to(dev), X, d))
    return pkg.HipEngine(pkg.PartitionedData(parts))


@pytest.mark.parametrize("d,storage,B,K,A,ld", CASES)
def test_bin_histogram_route(pkg, d, storage, B, K, A, ld):
    import torch
    c = rows_case(d, storage, B, K, A)
    plan = pkg._native.tree_plan(storage, d, B, K, A, 1)
    assert (d, B) not in ((40, 256), (300, 32)) or plan["feature_chunk"] < d      # more than one feature chunk
    assert A not in (11, 3) or plan["slot_subgroup"] < A                          # more than one slot sub-group
    eng = engine_of(pkg, c, d, storage, ld)
    bins = eng.tree_bin(c["thr"], c["nbins"])
    t_bins = TT.bin_rows(c["X"], c["thr"], c["nbins"])
    assert (bins.bins.cpu().numpy() == t_bins).all() and (bins.labels.cpu().numpy() == c["y"]).all()
    slots = torch.from_numpy(c["slots"].copy()).to(eng.dev)
    t_H = TT.histogram(t_bins, c["y"], c["slots"], d, B, K, 0, A)
    H = eng.tree_histogram(bins, slots, K, (0, A))
    assert H.dtype == torch.int64 and (H.cpu().numpy() == t_H).all()
    for repl in (1, 2):                              # either LDS layout, and a second call: the same bytes
        assert torch.equal(eng.tree_histogram(bins, slots, K, (0, A), replication=repl), H)
    if A > 1:                                        # a budget that forces two groups (from the plan): the same table
        p2 = pkg._native.tree_plan(storage, d, B, K, A, 1, budget=-(-A // 2) * d * B * K * 8)
        a1 = p2["group_slots"]
        assert p2["groups"] == 2 and 0 < a1 < A
        assert torch.equal(torch.cat([eng.tree_histogram(bins, slots, K, (0, a1)),
                                      eng.tree_histogram(bins, slots, K, (a1, A - a1))]), H)
    assert (eng.tree_histogram(bins, eng.tree_slots(), K).cpu().numpy() ==
            TT.histogram(t_bins, c["y"], np.zeros(len(c["y"])), d, B, K)).all()      # every slot starts at 0
    table = np.array([[s % d, (3 * s) % B, s + 1, -1] if s % 3 else [-1, 0, 0, 0] for s in range(A)], dtype=np.int32)
    eng.tree_route(bins, slots, table)
    assert (slots.cpu().numpy() == TT.route(t_bins, c["slots"], table)).all()
    assert (eng.tree_bin(c["thr"], c["nbins"]).bins.cpu().numpy() == t_bins).all()


@functools.lru_cache(maxsize=None)
def table_case(d, B, K, A):
    """Histograms with counts in the thousands (no near ties): feature f spreads class c's rows over its nb_f bins
    with weights of its own. Column 0 alone separates the classes (the lower half of them in its lower bins), so it
    holds the winner, and column d - 1 repeats it: a tie at bit-equal gain that the lower feature must win."""
    rng = np.random.default_rng(7 * d + B + K + A)
    nbins = np.array([1 + (f + K) % B for f in range(d)], dtype=np.int32)
    nbins[0] = B
    thr = np.cumsum(rng.uniform(0.5, 1.5, size=(d, B - 1)), axis=1)
    H = np.zeros((A, d, B, K), dtype=np.int64)
    for s in range(A):
        tot = rng.integers(2000, 9000, K)
        for f in range(d):
            for k in range(K):
                p = rng.dirichlet(np.ones(nbins[f]) * 0.7)
                if f == 0:
                    p = np.zeros(B)     # bin B / 2 stays empty: candidate B / 2 ties B / 2 - 1 from another lane of the wave
                    half = np.arange(0, B // 2) if k < (K + 1) // 2 else np.arange(B // 2 + (B >= 4), B)
                    p[half] = rng.dirichlet(np.ones(len(half)) * 0.7)
                H[s, f, : nbins[f], k] = rng.multinomial(tot[k], p)
    if d > 2:
        H[:, d - 1], nbins[d - 1], thr[d - 1] = H[:, 0], nbins[0], thr[0]
    return H, thr, nbins


@pytest.mark.parametrize("impurity", ["gini", "entropy"])
@pytest.mark.parametrize("d,B,K,A", [(1, 2, 2, 1), (17, 32, 3, 5), (40, 256, 32, 2), (70, 32, 2, 3)])   # the twin d - 1: column 0's wave (17), another
def test_best_split(pkg, d, B, K, A, impurity):
    import torch
    H, thr, nbins = table_case(d, B, K, A)
    c = dict(X=np.zeros((sum(SIZES), d), dtype=np.float32), y=np.zeros(sum(SIZES)))
    eng = pkg.HipEngine(dense_data(pkg, c, SIZES))
    bins = pkg.TreeBins(None, None, torch.from_numpy(thr).to(eng.dev), torch.from_numpy(nbins).to(eng.dev), B)
    Hd = torch.from_numpy(H).to(eng.dev)
    worst = 0.0
    for min_inst, min_gain in ((1, 0.0), (1500, 0.0), (10 ** 9, 0.0), (1, 10.0)):   # (1,500 < any class's rows)
        rec = eng.tree_best_split(Hd, bins, impurity, min_inst, min_gain).cpu().numpy()
        assert eng.tree_best_split(Hd, bins, impurity, min_inst, min_gain).cpu().numpy().tobytes() == rec.tobytes()
        for s in range(A):
            t = TT.best_split(H[s], thr, nbins, impurity, min_inst, min_gain)
            assert (rec[s, 0], rec[s, 1], rec[s, 2], rec[s, 5]) == (t["feature"], t["bin"], t["threshold"], t["n"]), (s, rec[s, :6], t)
            assert (rec[s, 6: 6 + K] == t["tot"]).all() and (rec[s, 6 + K:] == t["L"]).all()
            if min_inst < 10 ** 9 and min_gain == 0.0:   # column 0 wins, so its copy d - 1 ties it bit for bit and loses
                assert t["feature"] == 0 and t["bin"] < B // 2 and (d <= 2 or (H[s, d - 1] == H[s, 0]).all())
                assert B < 4 or not H[s, 0, t["bin"] + 1].any()   # ... and so does the next bin, from another lane
            worst = max(worst, abs(rec[s, 3] - float(t["gain"])) / TT.bar(K), abs(rec[s, 4] - float(t["impurity"])) / TT.bar(K))
        if min_inst == 10 ** 9 or min_gain > 0:
            assert (rec[:, 0] == -1).all()              # no valid candidate; a winner below minInfoGain
    print(f"d={d} B={B} K={K} {impurity}: worst gain / impurity error over the bar = {worst:.3g}")
    assert worst <= 1.0


@pytest.mark.parametrize("impurity", ["gini", "entropy"])
@pytest.mark.parametrize("maxDepth", [0, 4])
@pytest.mark.parametrize("storage", ["f32", "f64"])
def test_train_and_predict_match_the_truth(pkg, storage, maxDepth, impurity):
    X, y = blobs()
    data = pkg.PartitionedData.parallelize(y, X, 4, dtype=np_dtype(storage))
    model = pkg.DecisionTree.trainClassifier(data, 3, {}, impurity, maxDepth, 16, 10)
    thr, nbins = pkg.find_splits(data, 16)
    truth = TT.train(X, y, 3, thr, nbins, impurity, maxDepth, 10)   # (10 rows a node: no ties among tiny nodes)
    same_tree(model, truth, 3)
    pred = np.concatenate([t.cpu().numpy() for t in model.predict(data)])
    assert pred.dtype == np.int32 and (pred == TT.predict(X, truth)).all()
    eng = pkg.HipEngine(data)
    cls, prob = eng.tree_predict(model.nodes, probability=True)
    h_cls, h_prob = eng.ctx.tree_predict(model.nodes, probability=True)
    assert (cls.cpu().numpy() == pred).all() and (h_cls == pred).all() and (prob.cpu().numpy() == h_prob).all()
    again = pkg.DecisionTree.trainClassifier(data, 3, {}, impurity, maxDepth, 16, 10)
    assert all(again.nodes[k].tobytes() == model.nodes[k].tobytes() for k in model.nodes)


def test_refusals_on_the_device(pkg):
    """A label outside [0, K); thresholds that do not ascend; CSR rows; a node whose child is not a later node."""
    X, y = blobs()
    for bad in (7.0, 1.5, -1.0):
        yb = y.copy()
        yb[11] = bad
        with pytest.raises(pkg.IllegalArgumentException, match="labels"):
            pkg.DecisionTree.trainClassifier(pkg.PartitionedData.parallelize(yb, X, 2), 3, maxDepth=2)
    eng = pkg.HipEngine(pkg.PartitionedData.parallelize(y, X, 2))
    thr = np.array([[1.0, 1.0], [0.0, 1.0], [0.0, 1.0]])
    with pytest.raises(pkg.IllegalArgumentException, match="ascending"):
        eng.tree_bin(thr, np.array([3, 3, 3], dtype=np.int32))
    csr = pkg.CsrPartition(np.zeros(1), np.array([0, 1], dtype=np.int64), np.zeros(1, dtype=np.int32), np.ones(1), 3)
    with pytest.raises(pkg.UnsupportedOperationException):
        pkg.HipEngine(pkg.PartitionedData([csr])).tree_bin(thr, np.array([2, 2, 2], dtype=np.int32))
    L, h, N = pkg._native.lib(), eng.ctx.handle, pkg._native
    p = eng.tree_slots().data_ptr()                 # (any device pointer: the refusals come before a launch)
    assert L.psgd_tree_histogram_device(h, None, p, p, 2, 32, 0, 1, 0, p, p, None) == N.PSGD_EINVAL
    assert L.psgd_tree_histogram_device(h, p, p, p, 33, 32, 0, 1, 0, p, p, None) == N.PSGD_EUNSUPPORTED
    assert L.psgd_tree_best_split_device(h, p, p, None, 3, 32, 2, 1, 0, 1, 0.0, p, None) == N.PSGD_EINVAL
    assert L.psgd_tree_route_device(h, p, None, 1, p, None) == N.PSGD_EINVAL
    assert L.psgd_tree_bin_device(h, thr.ctypes.data, None, 3, p, p, p, p, None) == N.PSGD_EINVAL
    bad = dict(feature=[0, -1, -1], threshold=[0.0] * 3, left=[0, 0, 0], right=[2, 0, 0], prediction=[0] * 3, probability=[1.0] * 3)
    with pytest.raises(pkg.IllegalArgumentException, match="later node"):
        eng.tree_predict(bad)


def test_two_ranks(tmp_path, pkg):
    """Two ranks on cuda:0 over gloo, fresh child processes (tests/two_rank_tree.py), train one rank's tree byte for byte."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import two_rank_tree as T
    out = str(tmp_path / "res.json")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "two_rank_tree.py"), out], env=env,
                       capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    with open(out) as f:
        res = json.load(f)
    X, y = blobs()
    data = pkg.PartitionedData.parallelize(y, X, T.P, dtype=np.float32)
    one = pkg.DecisionTree.trainClassifier(data, 3, maxDepth=4, maxBins=16, minInstancesPerNode=10)
    want = {k: v.tolist() for k, v in one.nodes.items()}   # floats survive JSON exactly: identical bits
    assert res["0"]["nodes"] == res["1"]["nodes"] == want
