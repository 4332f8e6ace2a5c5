"""Scoring a multinomial logistic model on the device (psgd_evaluate_multinomial_device,
psgd_predict_multinomial_device, psgd_confusion*_device through HipEngine.evaluate_multinomial /
predict_classes / confusion, evaluate_multinomial() and MulticlassMetrics) against
tests/multiclass_truth.py.

Bars: |lossSum - truth| <= 1e-9 |truth| in total and per partition, the truth summed left to right
(the project's fp64 bar); every margin within nnz 2^-52 sum_i |x_i W_ci| of the truth's (a
reassociated f64 dot); count, nCorrect, every predicted class and the whole confusion table exactly.
Exactness is a guarantee, not luck: each case first asserts that, for every row with non-zeros, the
winning margin (0.0 for the pivot) is further than 1e-9 max_c sum_i |x_i W_ci| from the runner-up."""
import functools
import json
import math
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, has_gpu

import multiclass_truth as T

pytestmark = pytest.mark.gpu

ROWS = (0, 1, 65, 257, 1000)   # empty, single row, ragged tile tails, more than one tile


def need_gpu():
    if not has_gpu():
        pytest.skip("no GPU")


class Case:
    """Rows (an [n, d] array, or (idx, vals) pairs for CSR), labels covering 0 and K - 1, weights,
    and the truth's margins, classes and losses -- computed once and shared by the tests of a shape."""

    def __init__(self, rows, sizes, w, K, seed, X=None):
        rng = np.random.default_rng(seed)
        n = len(rows)
        self.rows, self.sizes, self.K, self.X = rows, list(sizes), K, X
        self.w = np.ascontiguousarray(w, dtype=np.float64)
        self.offs = np.concatenate([[0], np.cumsum(self.sizes)]).astype(int)
        self.y = rng.integers(0, K, size=n).astype(np.float64)
        if n >= 2:
            self.y[0], self.y[1] = 0.0, float(K - 1)
        if X is not None:   # dense: one matrix product for the whole case
            W = T.blocks(self.w, K)
            X64 = np.asarray(X, dtype=np.float64)
            self.M, self.A = X64 @ W.T, np.abs(X64) @ np.abs(W).T
            self.nnz = np.full(n, X.shape[1], dtype=np.int64)
        else:
            self.M, self.A, self.nnz = T.margins(rows, self.w, K), T.abs_margins(rows, self.w, K), T.nnz(rows)
        self.pred = T.predict(self.M)
        self.loss = T.losses(self.M, self.y)

    def gap_ok(self):
        """The precondition of exact classes: the winner of {0.0 (the pivot), m_0 .. m_{K-2}} is
        further than 1e-9 max_c sum|x_i W_ci| from the runner-up, for every row with non-zeros."""
        some = self.nnz > 0
        cand = np.sort(np.concatenate([self.M, np.zeros((len(self.M), 1))], axis=1), axis=1)
        gap = cand[:, -1] - cand[:, -2]
        return bool(np.all(gap[some] > 1e-9 * self.A[some].max(axis=1))) and bool(np.all(self.M[~some] == 0.0))

    def expected(self):
        """(lossSum, nCorrect, [lossSum_p], [nCorrect_p]); sums left to right."""
        pl, pc = [], []
        for a, b in zip(self.offs[:-1], self.offs[1:]):
            pl.append(T.sum_left_to_right(self.loss[a:b]))
            pc.append(int(np.sum(self.pred[a:b] == self.y[a:b])))
        return T.sum_left_to_right(pl), sum(pc), pl, pc


def within(got, want):
    return abs(got - want) <= 1e-9 * abs(want)


def check_case(pkg, case, data, what):
    assert case.gap_ok(), f"{what}: a winning margin is too close to the runner-up"
    K, w = case.K, case.w
    eng = pkg.HipEngine(data)
    got = eng.evaluate_multinomial(K, w)
    loss, correct, pl, pc = case.expected()
    print(f"{what}: lossSum {got.lossSum!r} truth {loss!r} rel {abs(got.lossSum - loss) / max(abs(loss), 1e-300):.3g} "
          f"nCorrect {got.nCorrect} truth {correct}")
    assert got.count == len(case.rows)
    assert within(got.lossSum, loss), (what, got.lossSum, loss)
    assert got.nCorrect == correct
    for p in range(len(pl)):
        assert within(got.partLoss[p], pl[p]), (what, p, got.partLoss[p], pl[p])
        assert int(got.partCorrect[p]) == pc[p], (what, p)
    worst = -np.inf
    for p in range(len(pl)):
        a, b = case.offs[p], case.offs[p + 1]
        classes, m = eng.predict_classes(p, K, w, margins=True)
        classes, m = classes.cpu().numpy(), m.cpu().numpy()
        assert classes.shape == (b - a,) and m.shape == (b - a, K - 1)
        assert np.array_equal(classes, case.pred[a:b]), (what, p)
        bound = case.nnz[a:b, None] * 2.0 ** -52 * case.A[a:b]
        err = np.abs(m - case.M[a:b])
        if b > a:
            worst = max(worst, float(np.max(err - bound)))
        assert np.all(err <= bound), (what, p, float(np.max(err - bound)))
        only = eng.predict_classes(p, K, w).cpu().numpy()   # classes alone: the same bits
        assert only.tobytes() == classes.tobytes()
    print(f"{what}: worst margin error minus its bound {worst:.3g}")
    table = eng.confusion(K, w)
    assert table.dtype == np.int64 and np.array_equal(table, T.confusion(case.pred, case.y, K)), what
    # a device tensor as the weights gives the same bits
    again = eng.evaluate_multinomial(K, eng.weights(w))
    assert again.lossSum == got.lossSum and again.nCorrect == got.nCorrect
    assert again.partLoss.tobytes() == got.partLoss.tobytes()
    return eng, got


# ---- dense ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dense_case(d, K, storage, sizes=ROWS, scale=1.0):
    rng = np.random.default_rng(2000 + 31 * d + K + (7 if storage == "f32" else 0))
    n = sum(sizes)
    X = rng.standard_normal((n, d)).astype(np.float32 if storage == "f32" else np.float64)
    w = scale * rng.standard_normal((K - 1) * d) / np.sqrt(d)
    return Case(list(range(n)), sizes, w, K, seed=d + K, X=X)


def dense_data(pkg, case):
    return pkg.PartitionedData([pkg.DensePartition(np.ascontiguousarray(case.y[a:b]), np.ascontiguousarray(case.X[a:b]))
                                for a, b in zip(case.offs[:-1], case.offs[1:])])


@pytest.mark.parametrize("storage", ["f32", "f64"])
@pytest.mark.parametrize("K", [3, 10])
@pytest.mark.parametrize("d", [1, 3, 100, 512, 1100])
def test_dense(pkg, d, K, storage):
    need_gpu()
    case = dense_case(d, K, storage)
    check_case(pkg, case, dense_data(pkg, case), f"dense d={d} K={K} {storage}")


@pytest.mark.parametrize("storage", ["f32", "f64"])
@pytest.mark.parametrize("side", ["within", "past"])
def test_dense_class_blocks_within_and_past_lds(pkg, side, storage):
    """(K - 1) d exactly the doubles of class blocks the kernel keeps in LDS, and one 16-byte row
    vector past it (the weights are then read from L2 / HBM); few rows."""
    need_gpu()
    budget = pkg._native.multiclass_switches()["lds_weights"]
    K = 3
    assert budget % (4 * (K - 1)) == 0
    d = budget // (K - 1) + (0 if side == "within" else 4)
    case = dense_case(d, K, storage, (0, 1, 70))
    check_case(pkg, case, dense_data(pkg, case), f"dense d={d} K={K} {storage} ({side} the LDS budget)")


@pytest.mark.parametrize("storage", ["f32", "f64"])
@pytest.mark.parametrize("extra", [0, 1])
def test_dense_softmax_switch(pkg, extra, storage):
    """K - 1 at the most classes whose softmax one lane takes, and one more (the wave then takes a
    row at a time, its lanes across the classes), at d = 16."""
    need_gpu()
    K = pkg._native.multiclass_switches()["lane_classes"] + 1 + extra
    case = dense_case(16, K, storage, (0, 1, 70))
    check_case(pkg, case, dense_data(pkg, case), f"dense d=16 K={K} {storage}")


@pytest.mark.parametrize("storage", ["f32", "f64"])
def test_dense_most_classes(pkg, storage):
    """K = 4,097, the most classes that train, at d = 2."""
    need_gpu()
    case = dense_case(2, 4097, storage, (0, 1, 70))
    check_case(pkg, case, dense_data(pkg, case), f"dense d=2 K=4097 {storage}")


def test_too_many_classes_is_unsupported(pkg):
    need_gpu()
    case = dense_case(1, 3, "f64")
    eng = pkg.HipEngine(dense_data(pkg, case))
    with pytest.raises(pkg.UnsupportedOperationException, match="4097"):
        eng.evaluate_multinomial(4098, np.zeros(4097))
    with pytest.raises(pkg.IllegalArgumentException):
        eng.evaluate_multinomial(2, np.zeros(1))
    with pytest.raises(pkg.IllegalArgumentException):
        eng.evaluate_multinomial(3, np.zeros(3))
    with pytest.raises(pkg.IllegalArgumentException):
        eng.predict_classes(9, 3, case.w)


def test_dense_device_resident_padded(pkg):
    """Device-resident partitions with ld > d (zero padding past the row's d features)."""
    need_gpu()
    import torch
    d, ld, K = 100, 112, 10
    case = dense_case(d, K, "f32")
    parts = []
    for a, b in zip(case.offs[:-1], case.offs[1:]):
        x = torch.zeros((b - a, ld), dtype=torch.float32, device="cuda")
        x[:, :d] = torch.from_numpy(np.ascontiguousarray(case.X[a:b])).cuda()
        parts.append(pkg.DevicePartition(torch.from_numpy(np.ascontiguousarray(case.y[a:b])).cuda(), x, d))
    torch.cuda.synchronize()
    check_case(pkg, case, pkg.PartitionedData(parts), f"dense device d={d} ld={ld} K={K}")


# ---- CSR ------------------------------------------------------------------------------------
def csr_rows(d, lengths, n, seed, dtype):
    rng = np.random.default_rng(seed)
    rows = []
    for k in range(n):
        m = lengths[k % len(lengths)]
        idx = np.sort(rng.choice(d, size=m, replace=False)).astype(np.int32)
        val = rng.standard_normal(m).astype(dtype)
        rows.append((idx.tolist(), [float(v) for v in val]))
    return rows


@functools.lru_cache(maxsize=None)
def csr_case(d, K, storage):
    """Three partitions by longest row: <= 16, <= 32 and 300 non-zeros (the three lane-group sizes),
    the last with rows of 0, 1, 16, 17, 128, 129 and 300."""
    dt = np.float32 if storage == "f32" else np.float64
    plan = [((1, 16, 7, 16), 120), ((1, 16, 17, 32, 5), 125), ((0, 1, 16, 17, 128, 129, 300), 259)]
    rows, sizes = [], []
    for k, (lengths, n) in enumerate(plan):
        rows += csr_rows(d, lengths, n, seed=37 * d % 1000 + 10 * K + k, dtype=dt)
        sizes.append(n)
    w = np.random.default_rng(5 + K).standard_normal((K - 1) * d) / np.sqrt(100.0)
    case = Case(rows, sizes, w, K, seed=d % 977 + K)
    case.dtype = dt
    return case


def csr_arrays(case, a, b):
    ptr = np.zeros(b - a + 1, dtype=np.int64)
    for k, r in enumerate(case.rows[a:b]):
        ptr[k + 1] = ptr[k] + len(r[0])
    col = np.array([i for r in case.rows[a:b] for i in r[0]], dtype=np.int32)
    val = np.array([v for r in case.rows[a:b] for v in r[1]], dtype=case.dtype)
    return ptr, col, val


def csr_data(pkg, case, d):
    parts = []
    for a, b in zip(case.offs[:-1], case.offs[1:]):
        ptr, col, val = csr_arrays(case, a, b)
        parts.append(pkg.CsrPartition(np.ascontiguousarray(case.y[a:b]), ptr, col, val, d))
    return pkg.PartitionedData(parts)


@pytest.mark.parametrize("storage", ["f32", "f64"])
@pytest.mark.parametrize("K", [3, 6])
def test_csr(pkg, K, storage):
    need_gpu()
    d = 47236
    case = csr_case(d, K, storage)
    eng, _ = check_case(pkg, case, csr_data(pkg, case, d), f"csr d={d} K={K} {storage}")
    # the rows without non-zeros: every margin 0.0, class 0
    a, b = case.offs[2], case.offs[3]
    empty = case.nnz[a:b] == 0
    assert empty.any()
    classes, m = eng.predict_classes(2, K, case.w, margins=True)
    assert np.all(classes.cpu().numpy()[empty] == 0.0) and np.all(m.cpu().numpy()[empty] == 0.0)


def test_csr_rows_without_nonzeros(pkg):
    """A partition of empty rows: class 0, every margin 0.0 and loss log(K) a row, as the truth
    computes it (log1p of K - 1 ones)."""
    need_gpu()
    K, d, n = 6, 47236, 5
    y = np.array([0.0, 5.0, 1.0, 0.0, 3.0])
    empty = pkg.CsrPartition(y, np.zeros(n + 1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0), d)
    eng = pkg.HipEngine(pkg.PartitionedData([empty]))
    w = np.random.default_rng(1).standard_normal((K - 1) * d)
    got = eng.evaluate_multinomial(K, w)
    want = T.sum_left_to_right([T.row_loss(np.zeros(K - 1), float(v)) for v in y])
    assert T.row_loss(np.zeros(K - 1), 0.0) == math.log1p(K - 1.0)
    assert got.count == n and got.nCorrect == 2 and within(got.lossSum, want)
    assert abs(got.lossSum - n * math.log(K)) <= 1e-9 * n * math.log(K)
    classes, m = eng.predict_classes(0, K, w, margins=True)
    assert np.all(classes.cpu().numpy() == 0.0) and np.all(m.cpu().numpy() == 0.0)


# ---- edge cases -----------------------------------------------------------------------------
def test_all_zero_weights(pkg):
    need_gpu()
    d, K = 100, 10
    case = dense_case(d, K, "f64")
    eng = pkg.HipEngine(dense_data(pkg, case))
    got = eng.evaluate_multinomial(K, np.zeros((K - 1) * d))
    n = len(case.rows)
    assert got.count == n and got.nCorrect == int(np.sum(case.y == 0.0))
    assert abs(got.lossSum - n * math.log(K)) <= 1e-9 * n * math.log(K)
    for p, (a, b) in enumerate(zip(case.offs[:-1], case.offs[1:])):
        assert np.all(eng.predict_classes(p, K, np.zeros((K - 1) * d)).cpu().numpy() == 0.0)
    table = eng.confusion(K, np.zeros((K - 1) * d))
    assert np.array_equal(table[:, 0], np.bincount(case.y.astype(int), minlength=K)) and not table[:, 1:].any()


@pytest.mark.parametrize("storage", ["f32", "f64"])
@pytest.mark.parametrize("d", [100, 1100])
def test_identical_weight_blocks_tie_to_the_lowest_class(pkg, d, storage):
    """Blocks c = 1 and c' = 3 hold the same bits and are scaled up so that they are the maximum
    for many rows: the margins of the two classes are the same bits, and those rows predict c + 1."""
    need_gpu()
    K = 6
    base = dense_case(d, K, storage)
    W = T.blocks(base.w, K).copy()
    W[1] *= 3.0
    W[3] = W[1]
    case = Case(base.rows, base.sizes, W.reshape(-1), K, seed=9, X=base.X)
    case.M[:, 3] = case.M[:, 1]   # (the truth's matrix product need not give the two columns the same bits)
    case.pred = T.predict(case.M)
    eng = pkg.HipEngine(dense_data(pkg, case))
    tied = (case.M[:, 1] == case.M.max(axis=1)) & (case.M[:, 1] > 0)
    # (the tied rows' other margins and 0.0 keep their distance: exact classes there too)
    others = np.delete(case.M, 3, axis=1)
    cand = np.sort(np.concatenate([others, np.zeros((len(others), 1))], axis=1), axis=1)
    assert np.all((cand[:, -1] - cand[:, -2])[tied] > 1e-9 * case.A[tied].max(axis=1))
    assert tied.sum() > 100 and np.all(case.pred[tied] == 2.0)
    for p, (a, b) in enumerate(zip(case.offs[:-1], case.offs[1:])):
        classes, m = eng.predict_classes(p, K, case.w, margins=True)
        classes, m = classes.cpu().numpy(), m.cpu().numpy()
        assert m[:, 1].tobytes() == m[:, 3].tobytes()
        assert np.all(classes[tied[a:b]] == 2.0)


@pytest.mark.parametrize("storage", ["f32", "f64"])
def test_margins_past_745(pkg, storage):
    """Weights scaled so that margins pass +-745 (exp overflows / underflows without the shift):
    finite, and within the bars."""
    need_gpu()
    case = dense_case(100, 10, storage, ROWS, 1000.0)
    assert case.M.max() > 745 and case.M.min() < -745
    _, got = check_case(pkg, case, dense_data(pkg, case), f"dense d=100 K=10 {storage} x1000")
    assert math.isfinite(got.lossSum) and np.all(np.isfinite(got.partLoss))


def test_labels_cover_the_first_and_last_class(pkg):
    need_gpu()
    case = dense_case(100, 10, "f64")
    assert 0.0 in case.y and 9.0 in case.y
    table = pkg.HipEngine(dense_data(pkg, case)).confusion(10, case.w)
    assert table[0].sum() == np.sum(case.y == 0.0) > 0 and table[9].sum() == np.sum(case.y == 9.0) > 0


# ---- determinism ----------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["dense", "csr"])
def test_partition_sum_is_independent_of_the_registry(pkg, layout):
    """A partition evaluated alone and as one of several gives a bit-identical partLoss; two calls
    in a row give bit-identical results."""
    need_gpu()
    if layout == "dense":
        case, K, k = dense_case(512, 10, "f32"), 10, 3
        data = dense_data(pkg, case)
    else:
        case, K, k = csr_case(47236, 6, "f64"), 6, 2
        data = csr_data(pkg, case, 47236)
    a = pkg.HipEngine(data).evaluate_multinomial(K, case.w)
    b = pkg.HipEngine(data).evaluate_multinomial(K, case.w)
    assert (a.lossSum, a.count, a.nCorrect) == (b.lossSum, b.count, b.nCorrect)
    assert a.partLoss.tobytes() == b.partLoss.tobytes()
    alone = pkg.HipEngine(pkg.PartitionedData([data.partitions[k]])).evaluate_multinomial(K, case.w)
    assert alone.partLoss[0].tobytes() == a.partLoss[k].tobytes()
    assert alone.count == data.partitions[k].n_rows and alone.partCorrect[0] == a.partCorrect[k]


# ---- non-interference with the epochs -----------------------------------------------------------
def drive(pkg, engine, params, w0, iters, between=None):
    """runParallelizedSGD's loop (tol = 0) by hand over engine.epoch; between(weights) runs after
    every iteration."""
    weights = engine.weights(w0)
    regVal = engine.initial_regval(params, w0)
    history = []
    for i in range(1, iters + 1):
        params.iteration = i
        folded, _ = engine.epoch(params, weights)
        avgRegVal, lossSum, batch = engine.scalars(folded)
        assert batch > 0
        history.append(lossSum / batch + regVal)
        weights = engine.adopt(folded)
        regVal = avgRegVal
        if between:
            between(weights)
    return engine.to_host(weights), np.array(history)


def test_scoring_does_not_disturb_training(pkg):
    need_gpu()
    d, K = 100, 3
    case = dense_case(d, K, "f64")
    data = dense_data(pkg, case)
    g, u = pkg.LogisticGradient(K), pkg.SquaredL2SGDUpdater()
    w0 = np.zeros((K - 1) * d)
    w_ref, h_ref = pkg.runParallelizedSGD(data, g, u, 0.5, 3, 0.01, 1.0, w0, 0.0)
    engine = pkg.HipEngine(data, weight_dim=(K - 1) * d)
    seen = []

    def between(weights):
        k0, n0 = engine.ctx.last_kernel(), engine.ctx.chain_launches()
        seen.append(engine.evaluate_multinomial(K, weights))
        engine.predict_classes(3, K, weights, margins=True)
        engine.confusion(K, weights)
        assert (engine.ctx.last_kernel(), engine.ctx.chain_launches()) == (k0, n0)

    params = pkg.make_params(g, u, 0.5, 0.01, 1.0, 0.0)
    w_plain, h_plain = drive(pkg, pkg.HipEngine(data, weight_dim=(K - 1) * d), params, w0, 3)
    w_eval, h_eval = drive(pkg, engine, params, w0, 3, between)
    assert w_eval.tobytes() == w_plain.tobytes() and h_eval.tobytes() == h_plain.tobytes()
    assert w_eval.tobytes() == w_ref.tobytes() and h_eval.tobytes() == h_ref.tobytes()
    assert len(seen) == 3 and all(s.count == len(case.rows) for s in seen)


def test_evaluation_objective_and_accuracy(pkg):
    need_gpu()
    d, K = 100, 10
    case = dense_case(d, K, "f32")
    sgd = pkg.ParallelizedSGD(pkg.LogisticGradient(K), pkg.SquaredL2SGDUpdater()).setRegParam(0.1)
    ev = sgd.evaluate_multinomial(dense_data(pkg, case), case.w)
    loss, correct, pl, pc = case.expected()
    want = ev.lossSum / ev.count + 0.5 * 0.1 * float(np.dot(case.w, case.w))   # UPD.scala:176-180
    assert abs(ev.objective - want) <= 1e-12 * abs(want)
    assert within(ev.lossSum, loss) and ev.count == len(case.rows)
    assert ev.accuracy == correct / len(case.rows)
    assert list(ev.partCorrect) == pc and len(ev.partLoss) == len(pl)


def test_host_pointer_forms(pkg):
    """psgd_evaluate_multinomial / psgd_predict_multinomial / psgd_confusion* (host buffers in and out)
    give the bits of the device forms; an unregistered partition is refused."""
    need_gpu()
    d, K = 100, 10
    case = dense_case(d, K, "f64")
    engine = pkg.HipEngine(dense_data(pkg, case))
    dev = engine.evaluate_multinomial(K, case.w)
    loss, count, correct, pl, pc = engine.ctx.evaluate_multinomial(K, case.w)
    assert (loss, count, correct) == (dev.lossSum, dev.count, dev.nCorrect)
    assert pl.tobytes() == dev.partLoss.tobytes() and [int(v) for v in pc] == [int(v) for v in dev.partCorrect]
    classes, m = engine.ctx.predict_multinomial(4, 1000, K, case.w)
    dc, dm = engine.predict_classes(4, K, case.w, margins=True)
    assert classes.tobytes() == dc.cpu().numpy().tobytes() and m.tobytes() == dm.cpu().numpy().tobytes()
    assert engine.ctx.predict_multinomial(0, 0, K, case.w)[0].shape == (0,)   # an empty partition writes nothing
    table, bad = engine.ctx.confusion_model(K, case.w)
    assert bad == 0 and np.array_equal(table, engine.confusion(K, case.w))
    t2, bad2 = engine.ctx.confusion(case.pred, case.y, K)
    assert bad2 == 0 and np.array_equal(t2, table)
    with pytest.raises(pkg.DeviceError, match="not registered"):
        engine.ctx.predict_multinomial(99, 1, K, case.w)


# ---- MulticlassMetrics ----------------------------------------------------------------------
def pairs(n, K, seed):
    rng = np.random.default_rng(seed)
    y = rng.integers(0, K, size=n).astype(np.float64)
    p = np.where(rng.random(n) < 0.6, y, rng.integers(0, K, size=n).astype(np.float64))
    return p, y


def table_of(p, y, K):
    t = np.zeros((K, K), dtype=np.int64)
    np.add.at(t, (y.astype(int), p.astype(int)), 1)
    return t


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 100000])
@pytest.mark.parametrize("K", [3, 64, 65])
def test_metrics_of_arrays(pkg, K, n):
    """K = 64 is the largest table the workgroups keep in LDS, K = 65 goes to global atomics."""
    need_gpu()
    import torch
    cells = pkg._native.multiclass_switches()["confusion_lds_cells"]
    assert 64 * 64 <= cells < 65 * 65
    p, y = pairs(n, K, seed=K + n)
    want = table_of(p, y, K)
    m = pkg.MulticlassMetrics(p, y, K)
    assert m.table.dtype == np.int64 and np.array_equal(m.table, want)
    md = pkg.MulticlassMetrics(torch.from_numpy(p).cuda(), torch.from_numpy(y).cuda(), K)   # device tensors
    assert np.array_equal(md.table, want)
    if n == 0:
        assert len(m.labels) == 0 and math.isnan(m.precision())
        assert pkg.MulticlassMetrics(p, y).numClasses == 1
        return
    t = T.Metrics(want)
    assert list(m.labels) == t.labels and m.precision() == t.accuracy()
    assert m.confusionMatrix().tolist() == t.confusionMatrix().tolist()
    c = t.labels[0]
    assert m.precision(c) == t.precision(c) and m.recall(c) == t.recall(c) and m.fMeasure(c) == t.fMeasure(c)
    assert m.weightedPrecision == t.weightedPrecision and m.weightedRecall == t.weightedRecall
    auto = pkg.MulticlassMetrics(p, y)   # numClasses = the largest value + 1
    k = auto.numClasses
    assert k == int(max(p.max(), y.max())) + 1 and np.array_equal(auto.table, want[:k, :k])


@pytest.mark.parametrize("K", [3, 65])
def test_metrics_refuse_values_outside_the_classes(pkg, K):
    need_gpu()
    p, y = pairs(300, K, seed=1)
    for bad in (2.5, float(K), -1.0):
        q = p.copy()
        q[17] = bad
        with pytest.raises(pkg.IllegalArgumentException, match="not a whole"):
            pkg.MulticlassMetrics(q, y, K)
        with pytest.raises(pkg.IllegalArgumentException, match="not a whole"):
            pkg.MulticlassMetrics(y, q, K)
    with pytest.raises(pkg.IllegalArgumentException, match="differ in length"):
        pkg.MulticlassMetrics(p[:-1], y, K)


@pytest.mark.parametrize("layout", ["dense", "csr"])
def test_metrics_from_model_equal_the_array_form(pkg, layout):
    need_gpu()
    import torch
    if layout == "dense":
        case, K = dense_case(100, 10, "f32"), 10
        data = dense_data(pkg, case)
    else:
        case, K = csr_case(47236, 6, "f32"), 6
        data = csr_data(pkg, case, 47236)
    model = pkg.MulticlassMetrics.fromModel(data, case.w, K)
    eng = pkg.HipEngine(data)
    classes = torch.cat([eng.predict_classes(p, K, case.w) for p in range(data.num_partitions)])
    arrays = pkg.MulticlassMetrics(classes, torch.from_numpy(case.y).cuda(), K)
    assert np.array_equal(model.table, arrays.table)
    assert np.array_equal(model.table, T.confusion(case.pred, case.y, K))
    assert model.precision() == arrays.precision() == case.expected()[1] / len(case.rows)
    assert model.weightedFMeasure() == T.Metrics(model.table).weightedFMeasure()


def test_model_form_refuses_a_label_outside_the_classes(pkg):
    need_gpu()
    d, K = 3, 3
    case = dense_case(d, K, "f64")
    y = case.y.copy()
    y[5] = 7.0
    data = pkg.PartitionedData([pkg.DensePartition(np.ascontiguousarray(y[a:b]), np.ascontiguousarray(case.X[a:b]))
                                for a, b in zip(case.offs[:-1], case.offs[1:])])
    with pytest.raises(pkg.IllegalArgumentException, match="labels are not whole numbers"):
        pkg.MulticlassMetrics.fromModel(data, case.w, K)


# ---- world size 2 -------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.parametrize("P", [5, 1])
def test_two_ranks(tmp_path, pkg, P):
    """Two ranks sharing cuda:0 over gloo, each a fresh child process (tests/two_rank_multiclass.py):
    both report the single-rank counts and table exactly and its lossSum within the bar; with P = 1
    rank 1 holds no partition."""
    need_gpu()
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import two_rank_multiclass as R
    out = str(tmp_path / "res.json")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), PSGD_TEST_P=str(P))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "two_rank_multiclass.py"), out], env=env,
                       capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    with open(out) as f:
        res = json.load(f)
    X, y, w, K = R.make_data()
    eng = pkg.HipEngine(pkg.PartitionedData.parallelize(y, X, P))
    one, table = eng.evaluate_multinomial(K, w), eng.confusion(K, w)
    assert len(res) == 2
    for rank in ("0", "1"):
        got = res[rank]
        assert within(got["lossSum"], one.lossSum), (rank, got["lossSum"], one.lossSum)
        assert got["count"] == one.count == X.shape[0] and got["nCorrect"] == one.nCorrect
        assert got["partCorrect"] == [int(v) for v in one.partCorrect]
        assert all(within(a, b) for a, b in zip(got["partLoss"], one.partLoss))
        assert got["table"] == table.tolist()
