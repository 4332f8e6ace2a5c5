"""The random forest's passes on the GPU against tests/forest_truth.py, each alone and exactly (integers); gains meet
tree_truth.bar. Then trainClassifier tree for tree, a second call byte for byte, tree groups, two ranks."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, has_gpu

import forest_truth as FT
import tree_truth as TT
from test_forest_api import TRAIN_SEEDS
from test_gpu_project import _free_port, dense_data
from test_gpu_tree import SIZES, rows_case, table_case
from test_tree_api import blobs, same_tree

pytestmark = pytest.mark.gpu
N_ROWS = sum(SIZES)


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not has_gpu():
        pytest.skip("no GPU")


@pytest.mark.parametrize("T,rate", [(5, 1.0), (5, 0.5), (1, 0.6), (1, 1.0)])
def test_bag(pkg, T, rate):
    import torch
    eng = pkg.HipEngine(dense_data(pkg, dict(X=np.zeros((N_ROWS, 3), dtype=np.float32), y=np.zeros(N_ROWS)), SIZES))
    cut = pkg.forest_cut(T, rate)
    w = eng.forest_bag(77, cut, (2, 3)).cpu().numpy()                 # trees 2, 3, 4 of this rank's rows: row0 = 0
    assert w.dtype == np.uint8 and w.shape == (3, N_ROWS)
    far = torch.zeros(3 * N_ROWS, dtype=torch.uint8, device=eng.dev)  # ... and as a rank whose first row is 2^33 + 5
    eng.ctx.forest_bag_device(77, cut, 2 ** 33 + 5, 2, 3, far.data_ptr(), None)
    torch.cuda.synchronize()
    for i in range(3):
        assert (w[i] == FT.bag(77, 2 + i, np.arange(N_ROWS), FT.cut(T, rate))).all()
        assert (far.cpu().numpy()[i * N_ROWS: (i + 1) * N_ROWS] == FT.bag(77, 2 + i, 2 ** 33 + 5 + np.arange(N_ROWS), cut)).all()
    assert T > 1 or w.max() <= 1
    assert not (T, rate) == (5, 1.0) or w.max() >= 2


@functools.lru_cache(maxsize=None)
def frontier_case(d, B, K, m, T):
    """Tree t has 1 + (2 t + 1) % 4 open nodes (one when T is 1); slots in [-1, nodes); ascending random subsets."""
    rng = np.random.default_rng(d + B + K + m + T)
    c = rows_case(d, "f32", B, K, 1)
    sizes = [1 if T == 1 else 1 + (2 * t + 1) % 4 for t in range(T)]
    base = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    slots = np.stack([rng.integers(-1, s, N_ROWS) for s in sizes]).astype(np.int32)
    sub = np.stack([np.sort(rng.choice(d, m, replace=False)) for _ in range(base[-1])]).astype(np.int32)
    return c, sizes, base, slots, sub


@pytest.mark.parametrize("d,B,K,m,T", [(1, 2, 2, 1, 1), (17, 32, 3, 5, 3), (40, 256, 32, 7, 2), (300, 32, 2, 18, 5)])
def test_histogram(pkg, d, B, K, m, T):
    import torch
    c, sizes, base, slots, sub = frontier_case(d, B, K, m, T)
    A, cut, seed, tree0 = int(base[-1]), pkg.forest_cut(5, 1.0), 1234, 3
    plan = pkg._native.forest_plan(d, B, K, m, A, T, 1, N_ROWS)
    assert (d, B) != (40, 256) or plan["subset_chunk"] < m                  # one node's cells exceed the LDS table
    assert d != 300 or (plan["node_subgroup"] > max(sizes) and plan["groups"] == 1)    # a sub-group over several trees
    eng = pkg.HipEngine(dense_data(pkg, c, SIZES))
    bins = eng.tree_bin(c["thr"], c["nbins"])
    w = np.stack([FT.bag(seed, tree0 + t, np.arange(N_ROWS), cut) for t in range(T)])
    assert T == 1 or (w.max() >= 2 and (w == 0).any() and (slots < 0).any())
    want = FT.histogram(TT.bin_rows(c["X"], c["thr"], c["nbins"]), c["y"], slots, w, base, sub, B, K)
    fr = eng.forest_frontier(np.repeat(np.arange(T), sizes), base, sub)
    d_slots = torch.from_numpy(slots.copy()).to(eng.dev)
    H = eng.forest_histogram(bins, d_slots, K, fr, (seed, tree0, cut))
    assert H.dtype == torch.int64 and (H.cpu().numpy() == want).all()
    assert torch.equal(eng.forest_histogram(bins, d_slots, K, fr, (seed, tree0, cut)), H)      # a second call: the same bytes
    if A > 1:                                        # a budget that forces two node groups (from the plan): the same table
        p2 = pkg._native.forest_plan(d, B, K, m, A, T, 1, N_ROWS, scratchBudget=-(-A // 2) * m * B * K * 8)
        a1 = p2["group_nodes"]
        assert p2["groups"] == 2 and 0 < a1 < A
        assert torch.equal(torch.cat([eng.forest_histogram(bins, d_slots, K, fr, (seed, tree0, cut), (0, a1)),
                                      eng.forest_histogram(bins, d_slots, K, fr, (seed, tree0, cut), (a1, A - a1))]), H)
    # routing: every other node splits on its first subset feature; children are slots of the tree's next frontier
    table = np.array([[sub[a, 0], (3 * a) % B, a % 3, -1] if a % 2 == 0 else [-1, 0, 0, 0] for a in range(A)], dtype=np.int32)
    eng.forest_route(bins, d_slots, fr, table)
    t_bins = TT.bin_rows(c["X"], c["thr"], c["nbins"])
    for t in range(T):
        assert (d_slots[t].cpu().numpy() == TT.route(t_bins, slots[t], table[base[t]: base[t + 1]])).all()


@pytest.mark.parametrize("impurity", ["gini", "entropy"])
@pytest.mark.parametrize("d,B,K,A", [(17, 32, 3, 5), (40, 256, 32, 2)])
def test_best_split(pkg, d, B, K, A, impurity):
    """Even nodes hold column 0 and its bit-equal twin d - 1: the lower feature wins. Odd nodes hold neither: the
    winner comes from the subset although column 0 would beat it."""
    import torch
    H, thr, nbins = table_case(d, B, K, A)
    sub = np.array([[0, 2, 5, d - 1] if a % 2 == 0 else [1, 2, 3, 5] for a in range(A)], dtype=np.int32)
    Hc = np.stack([H[a][sub[a]] for a in range(A)])
    eng = pkg.HipEngine(dense_data(pkg, dict(X=np.zeros((N_ROWS, d), dtype=np.float32), y=np.zeros(N_ROWS)), SIZES))
    bins = pkg.TreeBins(None, None, torch.from_numpy(thr).to(eng.dev), torch.from_numpy(nbins).to(eng.dev), B)
    fr = eng.forest_frontier(np.zeros(A, dtype=np.int32), np.array([0, A], dtype=np.int32), sub)
    for node0 in (0, 1):
        rec = eng.forest_best_split(torch.from_numpy(Hc[node0:]).to(eng.dev), bins, fr, node0, impurity, 1500).cpu().numpy()
        for a in range(node0, A):
            t, r = TT.best_split(Hc[a], thr[sub[a]], nbins[sub[a]], impurity, 1500), rec[a - node0]
            assert t["feature"] >= 0 and (r[0], r[1], r[2], r[5]) == (sub[a][t["feature"]], t["bin"], t["threshold"], t["n"]), (a, r[:6], t)
            assert (r[6: 6 + K] == t["tot"]).all() and (r[6 + K:] == t["L"]).all()
            assert abs(r[3] - float(t["gain"])) <= TT.bar(K) and abs(r[4] - float(t["impurity"])) <= TT.bar(K)
            assert (r[0] == 0) == (a % 2 == 0)


def nodes_bytes(forest):
    return [{k: v.tobytes() for k, v in t.nodes.items()} for t in forest.trees]


def test_train_and_predict_match_the_truth(pkg):
    X, y = blobs()
    data = pkg.PartitionedData.parallelize(y, X, 4, dtype=np.float32)
    kw = dict(maxDepth=4, maxBins=16, minInstancesPerNode=10)
    one = pkg.RandomForest.trainClassifier(data, 3, {}, 1, "all", seed=TRAIN_SEEDS[0], **kw)
    tree = pkg.DecisionTree.trainClassifier(data, 3, seed=TRAIN_SEEDS[0], **kw)
    assert one.numTrees == 1 and nodes_bytes(one) == [{k: v.tobytes() for k, v in tree.nodes.items()}]
    thr, nbins = pkg.find_splits(data, 16)
    for seed in TRAIN_SEEDS:
        forest = pkg.RandomForest.trainClassifier(data, 3, {}, 5, "sqrt", seed=seed, **kw)
        truth = FT.train(X, y, 3, thr, nbins, 5, "sqrt", seed, maxDepth=4, min_inst=10)
        assert forest.numTrees == 5 and forest.totalNumNodes == sum(len(t) for t in truth) and forest.seed == seed
        for model, nodes in zip(forest.trees, truth):
            same_tree(model, nodes, 3)
        votes = FT.vote(X, truth, 3)
        pred = np.concatenate([t.cpu().numpy() for t in forest.predict(data)])
        assert pred.dtype == np.int32 and (pred == votes.argmax(axis=1)).all()
        eng = pkg.HipEngine(data)
        cls, vt = eng.forest_predict([t.nodes for t in forest.trees], 3, votes=True)
        h_cls, h_vt = eng.ctx.forest_predict([t.nodes for t in forest.trees], 3, votes=True)
        assert (cls.cpu().numpy() == pred).all() and (vt.cpu().numpy() == votes).all() and (h_cls == pred).all() and (h_vt == votes).all()
        assert nodes_bytes(pkg.RandomForest.trainClassifier(data, 3, {}, 5, "sqrt", seed=seed, **kw)) == nodes_bytes(forest)
        grouped = pkg.RandomForest.trainClassifier(data, 3, {}, 5, "sqrt", seed=seed, slotBudget=3 * len(y) * 4, **kw)
        assert nodes_bytes(grouped) == nodes_bytes(forest)           # tree groups of 3 and 2
    assert forest.toDebugString().count("Tree ") == 5


def test_refusals_on_the_device(pkg):
    X, y = blobs()
    yb = y.copy()
    yb[11] = 7.0
    with pytest.raises(pkg.IllegalArgumentException, match="labels"):
        pkg.RandomForest.trainClassifier(pkg.PartitionedData.parallelize(yb, X, 2), 3, numTrees=2, maxDepth=2, seed=1)
    eng = pkg.HipEngine(pkg.PartitionedData.parallelize(y, X, 2))
    with pytest.raises(pkg.IllegalArgumentException, match="frontier"):
        eng.forest_frontier([0], [0, 1], [[2, 1]])
    L, h, N = pkg._native.lib(), eng.ctx.handle, pkg._native
    p, cut = eng.forest_slots(1).data_ptr(), pkg.forest_cut(2, 1.0)
    c = cut.ctypes.data
    assert L.psgd_forest_histogram_device(h, None, p, p, 1, p, p, p, 1, 1, 2, 32, 0, 1, 1, c, 0, 0, p, p, None) == N.PSGD_EINVAL
    assert L.psgd_forest_histogram_device(h, p, p, p, 1, p, p, p, 1, 1, 33, 32, 0, 1, 1, c, 0, 0, p, p, None) == N.PSGD_EUNSUPPORTED
    assert L.psgd_forest_histogram_device(h, p, p, p, 1, p, p, p, 1, 1, 2, 32, 1, 1, 1, c, 0, 0, p, p, None) == N.PSGD_EINVAL
    assert L.psgd_forest_histogram_device(h, p, p, p, 1, p, p, p, 1, 1, 2, 32, 0, 1, 1, cut[::-1].copy().ctypes.data, 0, 0, p, p, None) == N.PSGD_EINVAL
    assert L.psgd_forest_best_split_device(h, p, p, p, None, 1, 32, 2, 1, 0, 1, 0.0, p, None) == N.PSGD_EINVAL
    assert L.psgd_forest_route_device(h, p, None, p, 1, p, None) == N.PSGD_EINVAL
    bad = dict(feature=[0, -1, -1], threshold=[0.0] * 3, left=[0, 0, 0], right=[2, 0, 0], prediction=[0] * 3)
    with pytest.raises(pkg.IllegalArgumentException, match="later node"):
        eng.forest_predict([bad], 3)


def test_two_ranks(tmp_path, pkg):
    """Two ranks on cuda:0 over gloo, fresh child processes (tests/two_rank_forest.py), train one rank's forest byte for byte."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import two_rank_forest as T
    out = str(tmp_path / "res.json")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "two_rank_forest.py"), out], env=env,
                       capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    with open(out) as f:
        res = json.load(f)
    X, y = blobs()
    one = pkg.RandomForest.trainClassifier(pkg.PartitionedData.parallelize(y, X, T.P, dtype=np.float32), 3, **T.ARGS)
    want = [{k: v.tolist() for k, v in t.nodes.items()} for t in one.trees]   # floats survive JSON exactly: identical bits
    assert res["0"]["trees"] == res["1"]["trees"] == want
