"""Scoring at fixed weights on the device (psgd_evaluate_device / psgd_predict_device through
HipEngine.evaluate / predict and evaluate()): lossSum, count, nCorrect and per-row margins against
oracle/psgd_ref -- gradient(kind, row, label, w)[1] per row summed left to right, and _dot.

Bars: |lossSum - ref| <= 1e-9 |ref| in total and per partition (the project's fp64 bar); every margin
within d 2^-52 sum|x_i w_i| of the reference dot (a reassociated f64 dot; d the row's non-zero count
for CSR); count and nCorrect exactly. Exact nCorrect is a guarantee, not luck: each case first
asserts that every reference dot is further than 1e-9 sum|x_i w_i| from 0."""
import functools
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, has_gpu

pytestmark = pytest.mark.gpu

GRADS = {"logistic": 0, "least_squares": 1, "hinge": 2}
ROWS = (0, 1, 65, 257, 1000)   # empty, single row, ragged tile tails, more than one tile


def need_gpu():
    if not has_gpu():
        pytest.skip("no GPU")


def ref():
    import psgd_ref
    return psgd_ref


def grad_obj(pkg, name):
    return {"logistic": pkg.LogisticGradient, "least_squares": pkg.LeastSquaresGradient,
            "hinge": pkg.HingeGradient}[name]()


class Case:
    """Rows (python lists, or (idx, vals) tuples for CSR), labels per gradient family, weights, and
    the reference's per-row dots -- computed once and shared by the tests of a shape."""

    def __init__(self, rows, sizes, w, seed):
        R = ref()
        rng = np.random.default_rng(seed)
        n = len(rows)
        self.rows, self.sizes, self.w = rows, list(sizes), w
        self.offs = np.concatenate([[0], np.cumsum(self.sizes)]).astype(int)
        self.y01 = rng.integers(0, 2, size=n).astype(np.float64)
        self.yreal = rng.standard_normal(n)
        self.dots = np.array([R._dot(r, w) for r in rows])
        self.absum = np.array([self._absum(r) for r in rows])
        self.nnz = np.array([len(r[0]) if isinstance(r, tuple) else len(r) for r in rows])
        self._loss = {}

    def _absum(self, r):
        if isinstance(r, tuple):
            return float(sum(abs(v * self.w[i]) for i, v in zip(*r)))
        return float(sum(abs(v * wi) for v, wi in zip(r, self.w)))

    def labels(self, grad):
        return self.yreal if grad == "least_squares" else self.y01

    def losses(self, grad):
        if grad not in self._loss:
            R = ref()
            y = self.labels(grad)
            self._loss[grad] = [R.gradient(GRADS[grad], r, float(y[k]), self.w)[1] for k, r in enumerate(self.rows)]
        return self._loss[grad]

    def expected(self, grad):
        """(lossSum, nCorrect, [lossSum_p], [nCorrect_p]); sums left to right."""
        loss, y = self.losses(grad), self.labels(grad)
        pl, pc = [], []
        for a, b in zip(self.offs[:-1], self.offs[1:]):
            s = 0.0
            for k in range(a, b):
                s = s + loss[k]
            pl.append(s)
            pc.append(0 if grad == "least_squares" else
                      int(sum((1.0 if self.dots[k] > 0.0 else 0.0) == y[k] for k in range(a, b))))
        total = 0.0
        for s in pl:
            total = total + s
        return total, sum(pc), pl, pc


def check_case(pkg, case, data, grad, what):
    # the precondition of exact nCorrect: no reference dot within the kernels' error of 0. (A CSR
    # row without non-zeros adds no term: its dot is 0.0 exactly in the reference and on the device
    # alike, so its prediction cannot differ either; the strict inequality is asked of every other row.)
    some = case.nnz > 0
    assert np.all(np.abs(case.dots[some]) > 1e-9 * case.absum[some]), f"{what}: a reference dot is too close to 0"
    assert np.all(case.dots[~some] == 0.0) and np.all(case.absum[~some] == 0.0)
    eng = pkg.HipEngine(data)
    w = np.asarray(case.w, dtype=np.float64)
    got = eng.evaluate(grad_obj(pkg, grad), w)
    loss, correct, pl, pc = case.expected(grad)
    print(f"{what} {grad}: lossSum {got.lossSum!r} ref {loss!r} rel {abs(got.lossSum - loss) / max(abs(loss), 1e-300):.3g} "
          f"nCorrect {got.nCorrect} ref {correct}")
    assert got.count == len(case.rows)
    assert abs(got.lossSum - loss) <= 1e-9 * abs(loss), (what, got.lossSum, loss)
    assert got.nCorrect == correct
    for p in range(len(pl)):
        assert abs(got.partLoss[p] - pl[p]) <= 1e-9 * abs(pl[p]), (what, p, got.partLoss[p], pl[p])
        assert int(got.partCorrect[p]) == pc[p], (what, p)
    worst = -np.inf
    for p in range(len(pl)):
        a, b = case.offs[p], case.offs[p + 1]
        m = eng.predict(p, w).cpu().numpy()
        assert m.shape == (b - a,)
        bound = case.nnz[a:b] * 2.0 ** -52 * case.absum[a:b]
        err = np.abs(m - case.dots[a:b])
        if b > a:
            worst = max(worst, float(np.max(err - bound)))
        assert np.all(err <= bound), (what, p, float(np.max(err - bound)))
    print(f"{what}: worst margin error minus its bound {worst:.3g}")
    # a device tensor as the weights gives the same bits
    again = eng.evaluate(grad_obj(pkg, grad), eng.weights(w))
    assert again.lossSum == got.lossSum and again.nCorrect == got.nCorrect


# ---- dense ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dense_case(d, storage, sizes=ROWS):
    rng = np.random.default_rng(1000 + d + (7 if storage == "f32" else 0))
    n = sum(sizes)
    X = rng.standard_normal((n, d)).astype(np.float32 if storage == "f32" else np.float64)
    w = (rng.standard_normal(d) / np.sqrt(d)).tolist()
    case = Case([[float(v) for v in row] for row in X], sizes, w, seed=d)
    case.X = X
    return case


def dense_data(pkg, case, grad):
    y = case.labels(grad)
    return pkg.PartitionedData([pkg.DensePartition(np.ascontiguousarray(y[a:b]), np.ascontiguousarray(case.X[a:b]))
                                for a, b in zip(case.offs[:-1], case.offs[1:])])


@pytest.mark.parametrize("storage", ["f32", "f64"])
@pytest.mark.parametrize("d", [1, 3, 100, 512, 1100])
@pytest.mark.parametrize("grad", list(GRADS))
def test_dense(pkg, grad, d, storage):
    need_gpu()
    case = dense_case(d, storage)
    check_case(pkg, case, dense_data(pkg, case, grad), grad, f"dense d={d} {storage}")


@pytest.mark.parametrize("storage", ["f32", "f64"])
def test_dense_weights_past_lds(pkg, storage):
    """d = 4,100: past the 4,096 features whose weights the kernel keeps in LDS (they are read from
    HBM / L2 instead), ragged past whole 16-byte vectors per lane pass; few rows."""
    need_gpu()
    case = dense_case(4100, storage, (0, 1, 70))
    check_case(pkg, case, dense_data(pkg, case, "logistic"), "logistic", f"dense d=4100 {storage}")


def test_dense_device_resident_padded(pkg):
    """Device-resident partitions with ld > d (zero padding past the row's d features)."""
    need_gpu()
    import torch
    d, ld = 100, 112
    case = dense_case(d, "f32")
    grad = "logistic"
    y = case.labels(grad)
    parts = []
    for a, b in zip(case.offs[:-1], case.offs[1:]):
        x = torch.zeros((b - a, ld), dtype=torch.float32, device="cuda")
        x[:, :d] = torch.from_numpy(np.ascontiguousarray(case.X[a:b])).cuda()
        parts.append(pkg.DevicePartition(torch.from_numpy(np.ascontiguousarray(y[a:b])).cuda(), x, d))
    torch.cuda.synchronize()
    check_case(pkg, case, pkg.PartitionedData(parts), grad, f"dense device d={d} ld={ld}")


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
def csr_case(d, storage, n_scale=1):
    """Three partitions by longest row: <= 16, <= 32 and 300 non-zeros (the three lane-group
    sizes), the last with rows of 0, 1, 16, 17, 128, 129 and 300."""
    dt = np.float32 if storage == "f32" else np.float64
    plan = [((1, 16, 7, 16), 120 // n_scale), ((1, 16, 17, 32, 5), 125 // n_scale),
            ((0, 1, 16, 17, 128, 129, 300), 259 // n_scale)]
    rows, sizes = [], []
    for k, (lengths, n) in enumerate(plan):
        rows += csr_rows(d, lengths, n, seed=31 * d % 1000 + k, dtype=dt)
        sizes.append(n)
    rng = np.random.default_rng(5)
    w = rng.standard_normal(d) / np.sqrt(100.0)
    case = Case(rows, sizes, w, seed=d % 977)
    case.dtype = dt
    return case


def csr_arrays(case, a, b):
    ptr = np.zeros(b - a + 1, dtype=np.int64)
    for k, r in enumerate(case.rows[a:b]):
        ptr[k + 1] = ptr[k] + len(r[0])
    col = np.array([i for r in case.rows[a:b] for i in r[0]], dtype=np.int32)
    val = np.array([v for r in case.rows[a:b] for v in r[1]], dtype=case.dtype)
    return ptr, col, val


def csr_data(pkg, case, grad, d):
    y = case.labels(grad)
    parts = []
    for a, b in zip(case.offs[:-1], case.offs[1:]):
        ptr, col, val = csr_arrays(case, a, b)
        parts.append(pkg.CsrPartition(np.ascontiguousarray(y[a:b]), ptr, col, val, d))
    return pkg.PartitionedData(parts)


@pytest.mark.parametrize("storage", ["f32", "f64"])
@pytest.mark.parametrize("grad", list(GRADS))
def test_csr(pkg, grad, storage):
    need_gpu()
    d = 47236
    case = csr_case(d, storage)
    check_case(pkg, case, csr_data(pkg, case, grad, d), grad, f"csr d={d} {storage}")


@pytest.mark.parametrize("grad", ["hinge", "least_squares"])
def test_csr_wide(pkg, grad):
    """d = 2^22 (the reference's Logistic gradient builds a dense d-vector per row in pure Python:
    Hinge and LeastSquares keep the case at a second)."""
    need_gpu()
    d = 1 << 22
    case = csr_case(d, "f64", n_scale=2)
    check_case(pkg, case, csr_data(pkg, case, grad, d), grad, "csr d=2^22")


def test_csr_device_resident_offset_row_ptr(pkg):
    """A device-resident CSR registration whose row_ptr[0] != 0 (absolute offsets into col / val)."""
    need_gpu()
    import torch
    d = 47236
    case = csr_case(d, "f32")
    grad = "hinge"
    y = case.labels(grad)
    parts = []
    for k, (a, b) in enumerate(zip(case.offs[:-1], case.offs[1:])):
        ptr, col, val = csr_arrays(case, a, b)
        pad = 5 + 3 * k   # entries before the partition's first row
        col = np.concatenate([np.full(pad, d - 1, dtype=np.int32), col])
        val = np.concatenate([np.full(pad, 1e30, dtype=case.dtype), val])
        parts.append(pkg.DeviceCsrPartition(torch.from_numpy(np.ascontiguousarray(y[a:b])).cuda(),
                                            torch.from_numpy(ptr + pad).cuda(), torch.from_numpy(col).cuda(),
                                            torch.from_numpy(val).cuda(), d))
    torch.cuda.synchronize()
    check_case(pkg, case, pkg.PartitionedData(parts), grad, "csr device row_ptr[0] != 0")


# ---- determinism ----------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["dense", "csr"])
def test_partition_sum_is_independent_of_the_registry(pkg, layout):
    """A partition evaluated alone and as one of several gives a bit-identical partLoss; two calls
    in a row give bit-identical results."""
    need_gpu()
    if layout == "dense":
        case = dense_case(512, "f32")
        data = dense_data(pkg, case, "logistic")
        k = 3
    else:
        case = csr_case(47236, "f64")
        data = csr_data(pkg, case, "logistic", 47236)
        k = 2
    w = np.asarray(case.w)
    g = pkg.LogisticGradient()
    a = pkg.HipEngine(data).evaluate(g, w)
    b = pkg.HipEngine(data).evaluate(g, w)
    assert (a.lossSum, a.count, a.nCorrect) == (b.lossSum, b.count, b.nCorrect)
    assert a.partLoss.tobytes() == b.partLoss.tobytes()
    alone = pkg.HipEngine(pkg.PartitionedData([data.partitions[k]])).evaluate(g, w)
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


def test_evaluate_does_not_disturb_training(pkg):
    need_gpu()
    case = dense_case(100, "f64")
    data = dense_data(pkg, case, "logistic")
    g, u = pkg.LogisticGradient(), pkg.SquaredL2SGDUpdater()
    w0 = np.zeros(100)
    w_ref, h_ref = pkg.runParallelizedSGD(data, g, u, 0.5, 3, 0.01, 1.0, w0, 0.0)
    engine = pkg.HipEngine(data)
    seen = []

    def between(weights):
        k0, n0 = engine.ctx.last_kernel(), engine.ctx.chain_launches()
        seen.append(engine.evaluate(g, weights))
        engine.predict(3, weights)
        assert (engine.ctx.last_kernel(), engine.ctx.chain_launches()) == (k0, n0)

    params = pkg.make_params(g, u, 0.5, 0.01, 1.0, 0.0)
    w_plain, h_plain = drive(pkg, pkg.HipEngine(data), params, w0, 3)
    w_eval, h_eval = drive(pkg, engine, params, w0, 3, between)
    assert w_eval.tobytes() == w_plain.tobytes() and h_eval.tobytes() == h_plain.tobytes()
    assert w_eval.tobytes() == w_ref.tobytes() and h_eval.tobytes() == h_ref.tobytes()
    assert len(seen) == 3 and all(s.count == len(case.rows) for s in seen)


def test_evaluate_after_a_sampled_epoch_counts_every_row(pkg):
    need_gpu()
    case = dense_case(100, "f64")
    data = dense_data(pkg, case, "hinge")
    g, u = pkg.HingeGradient(), pkg.SimpleSGDUpdater()
    engine = pkg.HipEngine(data)
    params = pkg.make_params(g, u, 0.5, 0.0, 0.5, 0.0)
    params.iteration = 1
    w = engine.weights(np.asarray(case.w))
    folded, _ = engine.epoch(params, w)
    _, _, batch = engine.scalars(folded)
    assert 0 < batch < len(case.rows)
    got = engine.evaluate(g, w)
    loss, correct, _, _ = case.expected("hinge")
    assert got.count == len(case.rows) and got.nCorrect == correct
    assert abs(got.lossSum - loss) <= 1e-9 * abs(loss)


# ---- Evaluation arithmetic ----------------------------------------------------------------------
def test_evaluation_objective_and_accuracy(pkg):
    need_gpu()
    case = dense_case(100, "f32")
    w = np.asarray(case.w)
    sgd = pkg.ParallelizedSGD(pkg.LogisticGradient(), pkg.SquaredL2SGDUpdater()).setRegParam(0.1)
    ev = sgd.evaluate(dense_data(pkg, case, "logistic"), w)
    loss, correct, pl, pc = case.expected("logistic")
    want = ev.lossSum / ev.count + 0.5 * 0.1 * float(np.dot(w, w))   # UPD.scala:176-180
    assert abs(ev.objective - want) <= 1e-12 * abs(want)
    assert ev.meanLoss == ev.lossSum / ev.count and ev.count == len(case.rows)
    assert ev.accuracy == correct / len(case.rows)
    assert list(ev.partCorrect) == pc and len(ev.partLoss) == len(pl)
    ls = pkg.evaluate(dense_data(pkg, case, "least_squares"), pkg.LeastSquaresGradient(), pkg.SimpleSGDUpdater(),
                      0.0, w)
    assert ls.accuracy is None and ls.regVal == 0.0
    ref_ls = case.expected("least_squares")[0]
    assert abs(ls.lossSum - ref_ls) <= 1e-9 * abs(ref_ls)


def test_predict_refuses_a_partition_of_another_rank(pkg):
    need_gpu()
    case = dense_case(3, "f64")
    engine = pkg.HipEngine(dense_data(pkg, case, "logistic"))
    with pytest.raises(pkg.IllegalArgumentException):
        engine.predict(5, np.asarray(case.w))
    with pytest.raises(pkg.IllegalArgumentException):
        engine.evaluate(pkg.LogisticGradient(), np.zeros(4))


def test_host_pointer_forms(pkg):
    """psgd_evaluate / psgd_predict (host buffers in and out) give the bits of the device forms;
    an unregistered partition and an unknown gradient are refused."""
    need_gpu()
    case = dense_case(100, "f64")
    w = np.asarray(case.w)
    engine = pkg.HipEngine(dense_data(pkg, case, "logistic"))
    dev = engine.evaluate(pkg.LogisticGradient(), w)
    loss, count, correct, pl, pc = engine.ctx.evaluate(0, w)
    assert (loss, count, correct) == (dev.lossSum, dev.count, dev.nCorrect)
    assert pl.tobytes() == dev.partLoss.tobytes() and [int(v) for v in pc] == [int(v) for v in dev.partCorrect]
    m = engine.ctx.predict(4, 1000, w)
    assert m.tobytes() == engine.predict(4, w).cpu().numpy().tobytes()
    assert engine.ctx.predict(0, 0, w).shape == (0,)   # an empty partition writes nothing
    with pytest.raises(pkg.DeviceError, match="not registered"):
        engine.ctx.predict(99, 1, w)
    with pytest.raises(pkg.IllegalArgumentException, match="unknown gradient"):
        engine.ctx.evaluate(7, w)


# ---- world size 2 -------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.parametrize("P", [5, 1])
def test_two_ranks(tmp_path, pkg, P):
    """Two ranks sharing cuda:0 over gloo, each a fresh child process (tests/two_rank_evaluate.py):
    both report the single-rank sums; with P = 1 rank 1 holds no partition."""
    need_gpu()
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import two_rank_evaluate as T
    out = str(tmp_path / "res.json")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), PSGD_TEST_P=str(P))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "two_rank_evaluate.py"), out], env=env,
                       capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    with open(out) as f:
        res = json.load(f)
    X, y, w = T.make_data()
    one = pkg.HipEngine(pkg.PartitionedData.parallelize(y, X, P)).evaluate(pkg.LogisticGradient(), w)
    assert len(res) == 2
    for rank in ("0", "1"):
        got = res[rank]
        assert abs(got["lossSum"] - one.lossSum) <= 1e-12 * abs(one.lossSum), (rank, got["lossSum"], one.lossSum)
        assert got["count"] == one.count == X.shape[0] and got["nCorrect"] == one.nCorrect
        assert got["partLoss"] == [float(v) for v in one.partLoss]
        assert got["partCorrect"] == [int(v) for v in one.partCorrect]
