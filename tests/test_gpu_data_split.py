"""randomSplit / kFold on the device (split.py; cell_select in psgd_kernels.hip, the gathers in
psgd_datasplit.hip) against the pure-Python restatement tests/split_truth.py: the selection is
exact, the compaction bit for bit, and a split trains and scores as the same rows built on the host.

Rows are tagged (column 1 of a dense row holds its position in its partition, a CSR row's label
does), so that a gathered partition names the source rows it holds."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import split_truth as T
from conftest import ROOT, has_gpu
from test_gpu_parity import assert_close
from test_split_api import SEEDS, SIZES

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not has_gpu():
        pytest.skip("no GPU")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


def host(t):
    return t.detach().cpu().numpy()


def tagged_dense(sizes, d, dtype=np.float64, seed=3):
    """[(labels, x)] with x[t, 1 % d] = t (exact in f32 below 2^24) and the rest random bits, a few
    of them -0.0 and NaNs with a payload: the gather must not touch any of it."""
    rng = np.random.default_rng(seed)
    out = []
    for p, n in enumerate(sizes):
        x = rng.standard_normal((n, d)).astype(dtype)
        if n:
            x[::7, 0] = -0.0
            if d > 2:
                nan = np.array([0x7FC00123 if dtype == np.float32 else 0x7FF8000000000123],
                               dtype=np.uint32 if dtype == np.float32 else np.uint64).view(dtype)[0]
                x[::11, d - 1] = nan
            x[:, 1 % d] = np.arange(n)
        y = (np.arange(n) % 2).astype(np.float64) + 2.0 * p
        out.append((y, x))
    return out


def tags(part, d):
    return host(part.x)[:, 1 % d].astype(np.int64)


# ---- 1. selection, exact ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sel(pkg):
    parts = tagged_dense(SIZES, 3)
    data = pkg.PartitionedData([pkg.DensePartition(y, x) for y, x in parts])
    return parts, data, pkg.HipEngine(data)


@pytest.mark.parametrize("weights", [[0.6, 0.4], [1, 1, 1], [0.5, 0, 0.5]])
@pytest.mark.parametrize("seed", SEEDS)
def test_selection_is_exact(pkg, sel, seed, weights):
    parts, data, engine = sel
    truth = T.random_split_rows(SIZES, weights, seed)
    b = T.split_bounds(weights)
    splits = pkg.randomSplit(data, weights, seed, engine=engine)
    assert len(splits) == len(weights)
    kept = [[] for _ in SIZES]
    for c, s in enumerate(splits):
        assert s.num_partitions == len(SIZES) and s.column_transform is None and s.num_features == 3
        assert list(s.partition_counts) == [len(r) for r in truth[c]]
        rows = engine.cell_rows(b[c], b[c + 1], False, seed, pkg._native.SEED_PLUS_INDEX)
        for p, (y, x) in enumerate(parts):
            want = truth[c][p]
            assert host(rows[p]).tolist() == want.tolist(), (c, p)
            part = s.partitions[p]
            assert isinstance(part, pkg.DevicePartition) and part.n_rows == len(want)
            assert tuple(part.x.shape) == (len(want), 4)
            assert tags(part, 3).tolist() == want.tolist(), (c, p)
            assert same_bits(host(part.x)[:, :3], x[want]) and same_bits(host(part.labels), y[want])
            assert not host(part.x)[:, 3:].any()
            kept[p].append(want)
    seeds = T.split_seeds(seed, len(SIZES))
    for p, n in enumerate(SIZES):
        union = np.concatenate(kept[p])
        assert len(np.unique(union)) == len(union), "the splits of a partition are disjoint"
        below = np.flatnonzero(T.draws(seeds[p], n) < b[-1])
        assert sorted(union.tolist()) == below.tolist()
    if weights == [0.6, 0.4]:
        for p, n in enumerate(SIZES):
            if n >= 63:
                assert splits[0].partitions[p].n_rows > 0 and splits[1].partitions[p].n_rows > 0
    if weights == [0.5, 0, 0.5]:
        assert splits[1].count() == 0


# ---- 2. closed and open ends ------------------------------------------------------------------------
@pytest.mark.parametrize("seeding", ["plus_index", "partitionwise"])
def test_cell_ends(pkg, sel, seeding):
    _, _, engine = sel
    N = pkg._native
    seed, p, t = 11, 5, 1234
    if seeding == "plus_index":
        mode, s_p = N.SEED_PLUS_INDEX, T.split_seeds(seed, len(SIZES))[p]
    else:
        mode, s_p = N.SEED_PARTITIONWISE, T.kfold_seeds(seed, len(SIZES))[p]
    x = T.draws(s_p, SIZES[p])
    lb = float(x[t])
    assert len(np.unique(x[:50])) == 50 and 0.0 < lb < 1.0
    upper = host(engine.cell_rows(lb, 1.0, False, seed, mode)[p])
    lower = host(engine.cell_rows(0.0, lb, False, seed, mode)[p])
    assert t in upper and t not in lower                       # lb is closed, ub is open
    assert upper.tolist() == T.cell(x, lb, 1.0, False).tolist()
    assert lower.tolist() == T.cell(x, 0.0, lb, False).tolist()
    mid = host(engine.cell_rows(0.25, lb, False, seed, mode)[p])
    out = host(engine.cell_rows(0.25, lb, True, seed, mode)[p])
    assert mid.tolist() == T.cell(x, 0.25, lb, False).tolist()
    assert sorted(mid.tolist() + out.tolist()) == list(range(SIZES[p])) and not set(mid) & set(out)
    for lo, hi in ((0.5, 0.5), (0.7, 0.2)):
        none = engine.cell_rows(lo, hi, False, seed, mode)
        every = engine.cell_rows(lo, hi, True, seed, mode)
        assert [int(r.numel()) for r in none] == [0] * len(SIZES)
        assert [host(r).tolist() for r in every] == [list(range(n)) for n in SIZES]
    with pytest.raises(pkg.IllegalArgumentException):
        engine.cell_rows(float("nan"), 1.0, False, seed, mode)
    with pytest.raises(pkg.IllegalArgumentException):
        engine.cell_rows(0.0, 1.0, False, seed, 7)


# ---- 3. gather_dense ---------------------------------------------------------------------------------
DENSE_SIZES = (0, 1, 70, 300)


@pytest.mark.parametrize("source", ["host", "device"])
@pytest.mark.parametrize("d", [1, 5, 13, 512, 1030])
@pytest.mark.parametrize("storage", [np.float32, np.float64])
def test_gather_dense(pkg, storage, d, source):
    import torch
    parts = tagged_dense(DENSE_SIZES, d, storage, seed=d)
    vec = 4 if storage == np.float32 else 2
    ld = (d + vec - 1) // vec * vec
    if source == "host":
        data = pkg.PartitionedData([pkg.DensePartition(y, x) for y, x in parts])
    else:
        wide = ld + 3 * vec   # a source pitch beyond the output's
        dev = []
        for y, x in parts:
            X = torch.zeros((len(y), wide), dtype=torch.float32 if storage == np.float32 else torch.float64,
                            device="cuda")
            X[:, :d] = torch.from_numpy(x).cuda()
            dev.append(pkg.DevicePartition(torch.from_numpy(y).cuda(), X, d))
        data = pkg.PartitionedData(dev)
    truth = T.random_split_rows(DENSE_SIZES, [0.6, 0.4], 5)
    splits = pkg.randomSplit(data, [0.6, 0.4], 5)
    for c, s in enumerate(splits):
        for p, (y, x) in enumerate(parts):
            want, part = truth[c][p], s.partitions[p]
            got = host(part.x)
            assert got.shape == (len(want), ld) and got.dtype == storage and part.d == d
            assert same_bits(got[:, :d], x[want]), (c, p)
            assert not bits(got[:, d:]).any(), "pad columns are +0.0"
            assert same_bits(host(part.labels), y[want])
    assert sum(s.count() for s in splits) == sum(DENSE_SIZES)


# ---- 4. gather_csr -------------------------------------------------------------------------------------
CSR_SIZES = (0, 1, 150, 400)
CSR_D = 1000


def csr_parts(dtype, seed=9):
    """Rows of 0, 1, 16, 17, 64 and 65 non-zeros, one row of 300; the label is the row's position."""
    rng = np.random.default_rng(seed)
    out = []
    for p, n in enumerate(CSR_SIZES):
        ptr, col, val = [0], [], []
        for t in range(n):
            m = (0, 1, 16, 17, 64, 65)[t % 6]
            if p == 3 and t == 77:
                m = 300
            col += np.sort(rng.choice(CSR_D, size=m, replace=False)).tolist()
            val += rng.standard_normal(m).astype(dtype).tolist()
            ptr.append(len(col))
        out.append((np.arange(n, dtype=np.float64), np.array(ptr, np.int64), np.array(col, np.int32),
                    np.array(val, dtype=dtype)))
    return out


def check_csr_partition(part, src, want):
    y, ptr, col, val = src
    rp, c, v = host(part.row_ptr), host(part.col), host(part.val)
    assert host(part.labels).tolist() == [float(t) for t in want]
    lens = ptr[want + 1] - ptr[want] if len(want) else np.zeros(0, np.int64)
    assert rp[0] == 0 and rp.tolist() == np.concatenate([[0], np.cumsum(lens)]).tolist()
    pick = np.concatenate([np.arange(ptr[t], ptr[t + 1]) for t in want] + [np.zeros(0, np.int64)]).astype(np.int64)
    assert len(c) == len(pick) == len(v) == rp[-1]
    assert np.array_equal(c, col[pick]) and same_bits(v, val[pick])


@pytest.mark.parametrize("source", ["host", "device"])
@pytest.mark.parametrize("storage", [np.float32, np.float64])
def test_gather_csr(pkg, storage, source):
    import torch
    parts = csr_parts(storage)
    if source == "host":
        data = pkg.PartitionedData([pkg.CsrPartition(y, ptr, col, val, CSR_D) for y, ptr, col, val in parts])
    else:
        # one arena, every partition's row_ptr absolute: row_ptr[0] is non-zero from the first on
        pad = 37
        col_all = np.concatenate([np.zeros(pad, np.int32)] + [q[2] for q in parts])
        val_all = np.concatenate([np.zeros(pad, storage)] + [q[3] for q in parts])
        C, V = torch.from_numpy(col_all).cuda(), torch.from_numpy(val_all).cuda()
        dev, base = [], pad
        for y, ptr, col, val in parts:
            dev.append(pkg.DeviceCsrPartition(torch.from_numpy(y).cuda(), torch.from_numpy(ptr + base).cuda(), C, V,
                                              CSR_D))
            base += len(col)
        assert int(host(dev[2].row_ptr)[0]) > 0
        data = pkg.PartitionedData(dev)
    engine = pkg.HipEngine(data)
    for weights in ([0.6, 0.4], [0.5, 0, 0.5]):
        truth = T.random_split_rows(CSR_SIZES, weights, 21)
        splits = pkg.randomSplit(data, weights, 21, engine=engine)
        for c, s in enumerate(splits):
            for p, src in enumerate(parts):
                part = s.partitions[p]
                assert isinstance(part, pkg.DeviceCsrPartition) and part.n_rows == len(truth[c][p])
                assert part.val.dtype == (torch.float32 if storage == np.float32 else torch.float64)
                check_csr_partition(part, src, truth[c][p])
    assert 77 in truth[0][3] or 77 in truth[2][3], "the 300-entry row is in a checked split"
    empty = splits[1]
    assert empty.count() == 0 and all(host(q.row_ptr).tolist() == [0] for q in empty.partitions)


# ---- 5. / 6. end to end --------------------------------------------------------------------------------
def test_end_to_end_dense(pkg, oracle):
    n, d, P = 6000, 20, 4
    rng = np.random.default_rng(17)
    X = rng.standard_normal((n, d))
    w_true = rng.standard_normal(d) / np.sqrt(d)
    y = ((X @ w_true + rng.logistic(size=n)) > 0).astype(np.float64)
    data = pkg.PartitionedData.parallelize(y, X, P)
    sizes = [q.n_rows for q in data.partitions]
    truth = T.random_split_rows(sizes, [0.6, 0.4], 11)
    train, test = pkg.randomSplit(data, [0.6, 0.4], 11)

    def subset(c):
        ys = [data.partitions[p].labels[truth[c][p]] for p in range(P)]
        xs = [data.partitions[p].x[truth[c][p]] for p in range(P)]
        return ys, xs, np.concatenate([[0], np.cumsum([len(v) for v in ys])]).astype(np.int64)

    ys, xs, offs = subset(0)
    w0 = np.zeros(d)
    w, h, counts = pkg.runParallelizedSGD(train, pkg.LogisticGradient(), pkg.SquaredL2SGDUpdater(), 1.0, 3, 0.01,
                                          1.0, w0, 0.0, return_chain_counts=True)
    wr, hr, cr = oracle.run(oracle.Matrix(np.concatenate(ys), np.concatenate(xs)), offs, "logistic", "squared_l2",
                            1.0, 3, 0.01, w0, tol=0.0, n_threads=4)
    assert [list(map(int, c)) for c in counts] == [list(map(int, c)) for c in cr]
    assert_close(w, wr, what="weights trained on the split")
    assert_close(h, hr, what="loss history on the split")

    ys, xs, _ = subset(1)
    ref = pkg.PartitionedData([pkg.DensePartition(a, b) for a, b in zip(ys, xs)])
    g, u = pkg.LogisticGradient(), pkg.SquaredL2SGDUpdater()
    a, b = pkg.evaluate(test, g, u, 0.01, w), pkg.evaluate(ref, g, u, 0.01, w)
    assert (a.lossSum, a.count, a.nCorrect, a.regVal) == (b.lossSum, b.count, b.nCorrect, b.regVal)
    assert a.partLoss.tolist() == b.partLoss.tolist() and a.partCorrect.tolist() == b.partCorrect.tolist()
    ma = pkg.BinaryClassificationMetrics.fromModel(test, w)
    mb = pkg.BinaryClassificationMetrics.fromModel(ref, w)
    assert (ma.areaUnderROC(), ma.areaUnderPR()) == (mb.areaUnderROC(), mb.areaUnderPR())
    assert all(np.array_equal(p, q) for p, q in zip(ma.cumulativeCounts(), mb.cumulativeCounts()))


def test_end_to_end_csr(pkg, oracle):
    n, d, P = 900, 300, 3
    rng = np.random.default_rng(23)
    ptr, col, val = [0], [], []
    for t in range(n):
        m = (0, 1, 16, 17, 40, 9)[t % 6]
        col += np.sort(rng.choice(d, size=m, replace=False)).tolist()
        val += rng.standard_normal(m).tolist()
        ptr.append(len(col))
    ptr, col, val = np.array(ptr, np.int64), np.array(col, np.int32), np.array(val)
    y = rng.integers(0, 2, size=n).astype(np.float64)
    data = pkg.PartitionedData.parallelize_csr(y, ptr, col, val, d, P)
    sizes = [q.n_rows for q in data.partitions]
    truth = T.random_split_rows(sizes, [0.6, 0.4], 11)
    train, test = pkg.randomSplit(data, [0.6, 0.4], 11)

    def subset(c):
        ys, ptrs, cols, vals = [], [0], [], []
        for p in range(P):
            q = data.partitions[p]
            for t in truth[c][p]:
                cols.append(q.col[q.row_ptr[t]: q.row_ptr[t + 1]])
                vals.append(q.val[q.row_ptr[t]: q.row_ptr[t + 1]])
                ptrs.append(ptrs[-1] + len(cols[-1]))
            ys.append(q.labels[truth[c][p]])
        offs = np.concatenate([[0], np.cumsum([len(v) for v in ys])]).astype(np.int64)
        return (np.concatenate(ys), np.array(ptrs, np.int64), np.concatenate(cols + [np.zeros(0, np.int32)]),
                np.concatenate(vals + [np.zeros(0)]), offs)

    ys, ptrs, cols, vals, offs = subset(0)
    w0 = np.zeros(d)
    w, h, counts = pkg.runParallelizedSGD(train, pkg.HingeGradient(), pkg.SimpleSGDUpdater(), 0.5, 3, 0.0, 1.0, w0,
                                          0.0, return_chain_counts=True)
    wr, hr, cr = oracle.run(oracle.Matrix(ys, row_ptr=ptrs, col=cols, val=vals, d=d), offs, "hinge", "simple", 0.5,
                            3, 0.0, w0, tol=0.0, n_threads=4)
    assert [list(map(int, c)) for c in counts] == [list(map(int, c)) for c in cr]
    assert_close(w, wr, what="weights trained on the CSR split")
    assert_close(h, hr, what="loss history on the CSR split")

    ys, ptrs, cols, vals, offs = subset(1)
    ref = pkg.PartitionedData([pkg.CsrPartition(ys[a:b], ptrs[a:b + 1] - ptrs[a], cols[ptrs[a]:ptrs[b]],
                                                vals[ptrs[a]:ptrs[b]], d) for a, b in zip(offs[:-1], offs[1:])])
    g, u = pkg.HingeGradient(), pkg.SimpleSGDUpdater()
    a, b = pkg.evaluate(test, g, u, 0.0, w), pkg.evaluate(ref, g, u, 0.0, w)
    assert (a.lossSum, a.count, a.nCorrect) == (b.lossSum, b.count, b.nCorrect)
    assert a.partLoss.tolist() == b.partLoss.tolist()


# ---- 7. kFold ------------------------------------------------------------------------------------------
def test_kfold_three_folds(pkg):
    n, P, d = 5000, 3, 4
    y, x = tagged_dense([n], d)[0]
    data = pkg.PartitionedData.parallelize(y, x, P)
    sizes = [q.n_rows for q in data.partitions]
    starts = np.concatenate([[0], np.cumsum(sizes)])
    folds = pkg.kFold(data, 3, 7)
    assert len(folds) == 3
    import psgd_ref
    seeds = [int(s) for s in psgd_ref.partition_seeds(7, P)]
    bounds = [(0.0, 0.3333333432674408), (0.3333333432674408, 0.6666666865348816), (0.6666666865348816, 1.0)]
    seen = [set() for _ in range(P)]
    for (training, validation), (lb, ub) in zip(folds, bounds):
        for p in range(P):
            xs = T.draws(seeds[p], sizes[p])
            va = tags(validation.partitions[p], d) - starts[p]
            tr = tags(training.partitions[p], d) - starts[p]
            assert va.tolist() == T.cell(xs, lb, ub, False).tolist(), p
            assert sorted(va.tolist() + tr.tolist()) == list(range(sizes[p])) and not set(va) & set(tr)
            assert not seen[p] & set(va.tolist()), "validation sets are pairwise disjoint"
            seen[p] |= set(va.tolist())
    assert [len(s) for s in seen] == sizes
    again = T.kfold_rows(sizes, 3, 7)
    assert again[1][1][2].tolist() == (tags(folds[1][1].partitions[2], d) - starts[2]).tolist()
    assert list(folds[1][0].partition_counts) == [len(v) for v in again[1][0]]


# ---- 8. repeatability and the scaler workflow ------------------------------------------------------------
def test_repeatable_and_scaler_workflow(pkg):
    n, P, d = 3000, 3, 6
    rng = np.random.default_rng(41)
    X = rng.standard_normal((n, d)) * np.arange(1, d + 1)
    X[:, 1] = np.arange(n)
    y = rng.integers(0, 2, size=n).astype(np.float64)
    source = pkg.PartitionedData.parallelize(y, X, P)
    a = pkg.randomSplit(source, [0.6, 0.4], 11)
    b = pkg.randomSplit(source, [0.6, 0.4], 11)
    for s, t in zip(a, b):
        for p, q in zip(s.partitions, t.partitions):
            assert same_bits(host(p.x), host(q.x)) and same_bits(host(p.labels), host(q.labels))
    train = a[0]
    model = pkg.StandardScaler(withMean=True, withStd=True).fit(train)
    with pytest.raises(pkg.IllegalArgumentException):
        model.transform(train)          # zero-copy partitions stay refused
    scaled = model.transform(source)
    c = pkg.randomSplit(scaled, [0.6, 0.4], 11)
    shift, factor = model.shift, model.factor
    sizes = [q.n_rows for q in source.partitions]
    starts = np.concatenate([[0], np.cumsum(sizes)])
    truth = T.random_split_rows(sizes, [0.6, 0.4], 11)
    for j, (s, t) in enumerate(zip(a, c)):
        assert t.column_transform is None
        for k, (p, q) in enumerate(zip(s.partitions, t.partitions)):
            idx = host(p.x)[:, 1].astype(np.int64)     # positions in the whole data set
            assert (idx - starts[k]).tolist() == truth[j][k].tolist()
            assert p.n_rows == q.n_rows and same_bits(host(p.labels), host(q.labels))
            want = (X[idx] - shift) * factor   # psgd_transform_columns: the subtraction first, one rounding each
            assert np.array_equal(host(q.x)[:, :d], want), (j, k)


# ---- 9. the epoch state is left alone ----------------------------------------------------------------------
def test_epoch_state_untouched(pkg):
    rng = np.random.default_rng(2)
    X = rng.standard_normal((800, 10))
    y = rng.integers(0, 2, size=800).astype(np.float64)
    data = pkg.PartitionedData.parallelize(y, X, 4)
    engine = pkg.HipEngine(data)
    pkg.runParallelizedSGD(data, pkg.LogisticGradient(), pkg.SimpleSGDUpdater(), 1.0, 1, 0.0, 1.0, np.zeros(10), 0.0,
                           engine=engine)
    ctx = engine.ctx
    before = (ctx.last_kernel(), ctx.chain_launches(), ctx.last_ring())
    assert before[0] != 0 and before[1] > 0
    pkg.randomSplit(data, [0.6, 0.4], 11, engine=engine)
    pkg.kFold(data, 2, 3, engine=engine)
    assert (ctx.last_kernel(), ctx.chain_launches(), ctx.last_ring()) == before


# ---- two ranks -----------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_two_ranks(tmp_path):
    """Two ranks sharing cuda:0 over gloo, each a fresh child process (tests/two_rank_split.py): each
    rank's own partitions equal the restatement at their global indices; partition_counts is the
    full table on both."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import two_rank_split as W
    out = str(tmp_path / "res.json")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "two_rank_split.py"), out], env=env,
                       capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    with open(out) as f:
        res = json.load(f)
    P = W.P
    sizes = [b - a for a, b in W.slices()]
    split = T.random_split_rows(sizes, W.WEIGHTS, W.SEED)
    folds = T.kfold_rows(sizes, W.FOLDS, W.FOLD_SEED)
    blocks = {"0": (0, 3), "1": (3, 5)}          # shard_range(5, r, 2)
    assert sorted(res) == ["0", "1"]
    for rank, (lo, hi) in blocks.items():
        got = res[rank]
        assert got["block"] == [lo, hi]
        for c in range(len(W.WEIGHTS)):
            assert got["split_counts"][c] == [len(v) for v in split[c]]
            for p in range(P):
                want = split[c][p].tolist() if lo <= p < hi else []
                assert got["split"][c][p] == want, (rank, c, p)
        for k in range(W.FOLDS):
            assert got["fold_counts"][k] == [[len(v) for v in folds[k][0]], [len(v) for v in folds[k][1]]]
            for p in range(P):
                for side in (0, 1):
                    want = folds[k][side][p].tolist() if lo <= p < hi else []
                    assert got["folds"][k][side][p] == want, (rank, k, side, p)
    assert res["0"]["split_counts"] == res["1"]["split_counts"] and res["0"]["fold_counts"] == res["1"]["fold_counts"]
