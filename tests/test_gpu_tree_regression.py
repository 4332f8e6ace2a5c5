"""The regression tree's passes on the GPU against tests/tree_reg_truth.py: targets, moments and histograms exactly
(integers), the split record with its gain within the truth's bar, then trainRegressor node for node and bit for bit."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, has_gpu

import tree_reg_truth as RT
import tree_truth as TT
from test_gpu_project import _free_port, dense_data, np_dtype
from test_tree_regression_api import same_tree, waves

pytestmark = pytest.mark.gpu
SIZES = (437, 563)          # 1,000 rows in 2 partitions: no multiple of 256


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not has_gpu():
        pytest.skip("no GPU")


@functools.lru_cache(maxsize=None)
def rows_case(d, storage, B, A):
    """Labels in [-3.7, 9.1] (a range that is no power of two), a third of them within 0.01 of ymax (q^2 >> 30 is
    large), one exactly at ymax; values on a grid of quarters, ragged nb_f, the last feature constant."""
    rng = np.random.default_rng(100 * d + B + A)
    n = sum(SIZES)
    X = (np.round(rng.standard_normal((n, d)) * 8) / 4).astype(np_dtype(storage))
    X[:, d - 1] = 0.75
    thr, nbins = TT.ragged_thresholds(X, B, seed=A)
    y = rng.uniform(-3.7, 9.1, n)
    y[::3] = 9.1 - rng.uniform(0.0, 0.01, len(y[::3]))
    y[5] = 9.1
    return dict(X=X, y=y, thr=thr, nbins=nbins, slots=rng.integers(-1, A, n).astype(np.int32))


@pytest.mark.parametrize("d,storage,B,A,slot0", [(17, "f32", 32, 3, 0), (40, "f32", 256, 3, 0), (16, "f64", 32, 1, 0),
                                                 (17, "f32", 32, 5, 2)])
def test_targets_moments_histogram(pkg, d, storage, B, A, slot0):
    import torch
    c = rows_case(d, storage, B, A)
    plan = pkg._native.tree_plan(storage, d, B, 0, A, 4)
    assert (d, B) != (16, 32) or plan["replication"] == 2          # two LDS copies
    assert (d, B) != (17, 32) or (plan["pitch"], plan["feature_chunk"]) == (32, 32)   # the second vector is partial
    eng = pkg.HipEngine(dense_data(pkg, c, SIZES))
    q, ymin, s = RT.targets(c["y"])
    t = eng.tree_targets()
    assert (t.ymin, t.s) == (ymin, s) and ymin < 0 and (t.q.cpu().numpy() == q).all() and q.max() > 2 ** 29
    assert torch.equal(eng.tree_targets(torch.from_numpy(c["y"].copy()).to(eng.dev)).q, t.q)   # a caller's labels
    slots = torch.from_numpy(c["slots"].copy()).to(eng.dev)
    mom = eng.tree_moments(t, slots, A).cpu().numpy()
    assert mom.tolist() == RT.moments(q, c["slots"], A) and (mom[:, 2] > 2 ** 30).all()
    assert eng.tree_moments(t, eng.tree_slots(), 1).cpu().numpy().tolist() == RT.moments(q, np.zeros(len(q), dtype=int), 1)
    bins = eng.tree_bin(c["thr"], c["nbins"])
    t_H = RT.histogram(TT.bin_rows(c["X"], c["thr"], c["nbins"]), q, c["slots"], d, B, slot0, A - slot0)
    assert t_H[0, d - 1, 0, 1] > 2 ** 32                           # the constant feature: a sum no uint32 cell holds
    H = eng.tree_histogram_reg(bins, t, slots, (slot0, A - slot0))
    assert H.dtype == torch.int64 and (H.cpu().numpy() == t_H).all()
    for repl in (1, 2):      # either LDS layout (two copies of B = 256 leave 8 features a chunk), and again: the same bytes
        assert torch.equal(eng.tree_histogram_reg(bins, t, slots, (slot0, A - slot0), replication=repl), H)


def test_constant_and_bad_labels(pkg):
    c = dict(rows_case(17, "f32", 32, 3), y=np.full(sum(SIZES), -2.75))
    eng = pkg.HipEngine(dense_data(pkg, c, SIZES))
    t = eng.tree_targets()
    assert (t.ymin, t.s) == (-2.75, 0) and not t.q.cpu().numpy().any()
    assert eng.tree_moments(t, eng.tree_slots(), 1).cpu().numpy().tolist() == [[sum(SIZES), 0, 0, 0]]
    for bad in (np.nan, np.inf):
        y = rows_case(17, "f32", 32, 3)["y"].copy()
        y[700] = bad
        with pytest.raises(pkg.IllegalArgumentException, match="labels"):
            pkg.DecisionTree.trainRegressor(dense_data(pkg, dict(c, y=y), SIZES), maxDepth=1)


@functools.lru_cache(maxsize=None)
def table_case(B, A):
    """Tables of 3,000 rows a slot whose targets step up where column 0's bin passes 0.6 B; column 1 is ragged noise
    and column 2 repeats column 0: a tie at bit-equal gain that the lower feature must win."""
    rng = np.random.default_rng(31 * B + A)
    n, s = 3000, 20
    nbins = np.array([B, max(2, B // 2 + 1), B], dtype=np.int32)
    thr = np.cumsum(rng.uniform(0.5, 1.5, size=(3, B - 1)), axis=1)
    bins = np.stack([rng.integers(0, B, n * A), rng.integers(0, nbins[1], n * A), np.zeros(n * A, dtype=np.int64)], axis=1)
    bins[:, 2] = bins[:, 0]
    q = (np.where(bins[:, 0] > (6 * B) // 10, 3 << 28, 1 << 27) + rng.integers(0, 1 << 26, n * A)).astype(np.int64)
    slots = np.repeat(np.arange(A), n)
    return RT.histogram(bins, q, slots, 3, B, 0, A), RT.moments(q, slots, A), thr, nbins, s, RT.bar(q, s)


@pytest.mark.parametrize("B,A", [(130, 2), (32, 3)])       # 130: the scan's carry crosses two steps of 64 bins
def test_best_split(pkg, B, A):
    import torch
    H, mom, thr, nbins, s, err = table_case(B, A)
    c = rows_case(17, "f32", 32, 3)
    eng = pkg.HipEngine(dense_data(pkg, c, SIZES))
    bins = pkg.TreeBins(None, None, torch.from_numpy(thr).to(eng.dev), torch.from_numpy(nbins).to(eng.dev), B)
    t = pkg.TreeTargets(None, 0.0, s)
    Hd, Md = torch.from_numpy(H).to(eng.dev), torch.tensor(mom, dtype=torch.int64, device=eng.dev)
    top = float(RT.best_split(H[0], mom[0][0], mom[0][1], thr, nbins, s, err)["gain"])
    for min_inst, min_gain in ((1, 0.0), (40, 0.0), (1400, 0.0), (10 ** 9, 0.0), (1, 4.0 * top)):
        rec = eng.tree_best_split_reg(Hd, Md, bins, t, min_inst, min_gain).cpu().numpy()
        assert eng.tree_best_split_reg(Hd, Md, bins, t, min_inst, min_gain).cpu().numpy().tobytes() == rec.tobytes()
        for a in range(A):
            w = RT.best_split(H[a], mom[a][0], mom[a][1], thr, nbins, s, err, min_inst, min_gain)
            assert (rec[a, 0], rec[a, 1], rec[a, 2]) == (w["feature"], w["bin"], w["threshold"]), (a, rec[a], w)
            assert abs(rec[a, 3] - float(w["gain"])) <= err
            assert min_inst > 40 or min_gain > 0 or (w["feature"] == 0 and (H[a, 2] == H[a, 0]).all())   # the twin loses
        assert (min_inst < 10 ** 9 and min_gain == 0.0) or (rec[:, 0] == -1).all()


def pure_corner(n=900, seed=11):
    """Rows of one feature in two clusters: the left one shares one label, so it becomes a leaf below the root."""
    rng = np.random.default_rng(seed)
    X = np.concatenate([rng.uniform(-3, -1, (n // 3, 1)), rng.uniform(1, 3, (n - n // 3, 1))]).astype(np.float32)
    y = np.where(X[:, 0] < 0, -6.5, 2.0 * X[:, 0] + 0.125 * rng.standard_normal(n))
    return X, y


@pytest.mark.parametrize("storage,maxDepth,rows", [("f32", 0, waves), ("f32", 4, waves), ("f64", 4, waves), ("f32", 3, pure_corner)])
def test_train_and_predict_match_the_truth(pkg, storage, maxDepth, rows):
    X, y = rows()
    d = X.shape[1]
    data = pkg.PartitionedData.parallelize(y, X, 4, dtype=np_dtype(storage))
    model = pkg.DecisionTree.trainRegressor(data, {}, "variance", maxDepth, 16, 10)
    thr, nbins = pkg.find_splits(data, 16)
    truth = RT.train(X, y, thr, nbins, maxDepth, 10)
    q, ymin, s = RT.targets(y)
    same_tree(model, truth, RT.bar(q, s))
    if rows is pure_corner:      # the cluster of one label: a leaf at depth 1 of impurity exactly 0, never examined for a split
        assert truth[2]["impurity"] == 0.0 and truth[2]["n"] > 200 and truth[2]["feature"] < 0 <= truth[3]["feature"]
    pred = np.concatenate([t.cpu().numpy() for t in model.predict(data)])
    assert pred.dtype == np.float64 and (pred == RT.predict(X, truth)).all()
    for t in truth.values():     # within a target's rounding of the mean of the raw labels
        assert abs(t["prediction"] - np.mean(y[t["rows"]], dtype=np.longdouble)) <= (y.max() - y.min()) * 2.0 ** -30
    grouped = pkg.DecisionTree.trainRegressor(data, {}, "variance", maxDepth, 16, 10, scratchBudget=d * 16 * 16)
    assert all(grouped.nodes[k].tobytes() == model.nodes[k].tobytes() for k in model.nodes)


def test_two_ranks(tmp_path, pkg):
    """Two ranks on cuda:0 over gloo, fresh child processes (tests/two_rank_tree_reg.py), train one rank's tree byte for byte."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import two_rank_tree_reg as T
    out = str(tmp_path / "res.json")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "two_rank_tree_reg.py"), out], env=env,
                       capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    with open(out) as f:
        res = json.load(f)
    X, y = waves()
    one = pkg.DecisionTree.trainRegressor(pkg.PartitionedData.parallelize(y, X, T.P, dtype=np.float32), maxDepth=4, maxBins=16,
                                          minInstancesPerNode=10)
    want = {k: v.tolist() for k, v in one.nodes.items()}   # floats survive JSON exactly: identical bits
    assert res["0"]["nodes"] == res["1"]["nodes"] == want
