"""Column statistics and the column transform on the device (psgd_column_stats_device /
psgd_transform_columns_device through HipEngine.column_stats, StandardScaler and
StandardScalerModel.transform).

The reference is exact arithmetic in this file: math.fsum per column over the stored values widened
to double (for CSR over the column's non-zeros, the implicit zeros added in closed form).

Bars (n rows, u = 2^-53):
  count, numNonzeros, max, min    exact;
  |mean - ref| <= n 2^-52 max_i |x_ij|                (the worst case of any summation order);
  variance: exactly 0 where ref == 0, else |var - ref| <= 16 n 2^-52 kappa_j ref with
  kappa_j = sqrt(1 + mean_j^2 / var_j) from the reference (2 n u kappa is the first-order worst case
  of the stable one- and two-pass families; 16 is room for the choice of shift). At n = 1323 and a
  column of 1e6 + N(0, 1) the bar is 4.7e-6 relative; shifted tile sums with a Chan merge land near
  8e-12, the textbook sum(x^2) - sum(x)^2 / n near 3.5e-3;
  the constant-0.1 column: mean exactly 0.1 (float32(0.1) for f32 rows), variance exactly 0.0;
  dense rows: two calls give the same bits."""
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

pytestmark = pytest.mark.gpu

ROWS = (0, 1, 65, 257, 1000)   # empty, single row, ragged tile tails, more than one tile (f64: 512 rows)
N = sum(ROWS)
CSR_D = 47236


def need_gpu():
    if not has_gpu():
        pytest.skip("no GPU")


def np_dtype(storage):
    return np.float32 if storage == "f32" else np.float64


class Ref:
    """Exact per-column statistics (count n over all rows)."""

    def __init__(self, n, d):
        self.n, self.d = n, d
        self.mean, self.var = np.zeros(d), np.zeros(d)
        self.nnz = np.zeros(d, dtype=np.int64)
        self.max, self.min, self.absmax = np.zeros(d), np.zeros(d), np.zeros(d)

    def set_column(self, j, nonzeros, n_stored_nonzero):
        """Column j holds `nonzeros` (doubles, none 0.0) and n - len(nonzeros) zeros."""
        n = self.n
        zeros = n - len(nonzeros)
        mean = math.fsum(nonzeros) / n
        m2 = math.fsum([(v - mean) * (v - mean) for v in nonzeros] + [zeros * mean * mean])
        self.mean[j] = mean
        self.var[j] = m2 / (n - 1) if n > 1 else 0.0
        self.nnz[j] = n_stored_nonzero
        vals = list(nonzeros) + ([0.0] if zeros else [])
        self.max[j], self.min[j] = max(vals), min(vals)
        self.absmax[j] = max(abs(v) for v in vals)


def dense_ref(X):
    n, d = X.shape
    X64 = X.astype(np.float64)
    r = Ref(n, d)
    r.nnz = (X64 != 0.0).sum(axis=0).astype(np.int64)
    r.max, r.min, r.absmax = X64.max(axis=0), X64.min(axis=0), np.abs(X64).max(axis=0)
    cols = X64.T.tolist()
    r.mean = np.array([math.fsum(c) / n for c in cols])
    if n > 1:
        dev = X64 - r.mean            # each difference rounded once, as (v - mean) in Python would be
        r.var = np.array([math.fsum(c) for c in (dev * dev).T.tolist()]) / (n - 1)
    # a constant column's exact mean is the constant and its exact variance 0 (fsum(c) / n rounds twice)
    const = r.max == r.min
    r.mean[const] = r.max[const]
    r.var[const] = 0.0
    return r


def check_stats(got, ref, what, exact_columns=()):
    n = ref.n
    assert got.count == n
    assert got.numNonzeros.tolist() == ref.nnz.tolist(), what
    assert got.max.tolist() == ref.max.tolist() and got.min.tolist() == ref.min.tolist(), what
    mean_err = np.abs(got.mean - ref.mean)
    mean_bar = n * 2.0 ** -52 * ref.absmax
    zero = ref.var == 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        kappa = np.sqrt(1.0 + ref.mean ** 2 / ref.var)
        var_bar = np.where(zero, 0.0, 16.0 * n * 2.0 ** -52 * kappa * ref.var)
        rel = np.where(zero, 0.0, np.abs(got.variance - ref.var) / ref.var)
    print(f"{what}: worst mean error / bar {np.max(mean_err / np.where(mean_bar > 0, mean_bar, 1.0)):.3g}, "
          f"worst relative variance error {rel.max():.3g} (bar there "
          f"{(var_bar / np.where(zero, 1.0, ref.var))[np.argmax(rel)]:.3g})")
    assert np.all(mean_err <= mean_bar), (what, int(np.argmax(mean_err - mean_bar)))
    assert np.all(got.variance[zero] == 0.0), (what, got.variance[zero])
    assert np.all(np.abs(got.variance - ref.var) <= var_bar), (what, int(np.argmax(np.abs(got.variance - ref.var) - var_bar)))
    for j, value in exact_columns:
        assert got.mean[j] == value and got.variance[j] == 0.0, (what, j, got.mean[j], got.variance[j])


# ---- dense ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dense_case(d, storage, sizes=ROWS):
    """Random rows with engineered columns where d allows: an all-zero one, a constant 0.1 one,
    columns of 1e6 + N(0, 1); for d >= 100 a constant and a shifted column also end the row (its
    last, possibly partial, 16-byte vector and column chunk)."""
    dt = np_dtype(storage)
    rng = np.random.default_rng(2000 + d + (7 if storage == "f32" else 0))
    n = sum(sizes)
    X = rng.standard_normal((n, d)).astype(dt)
    X[rng.random((n, d)) < 0.05] = 0.0          # some zeros for numNonzeros
    const = dt(0.1)
    exact = []
    if d >= 3:
        X[:, 0] = 0.0
        X[:, 1] = const
        X[:, 2] = (1e6 + rng.standard_normal(n)).astype(dt)
        exact += [(0, 0.0), (1, float(const))]
    if d >= 5:
        X[:, 3] = (1e6 + rng.standard_normal(n)).astype(dt)
    if d >= 100:
        X[:, d - 2] = const
        X[:, d - 1] = (1e6 + rng.standard_normal(n)).astype(dt)
        exact.append((d - 2, float(const)))
    y = rng.integers(0, 2, size=n).astype(np.float64)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(int)
    return {"X": X, "y": y, "offs": offs, "ref": dense_ref(X), "exact": exact, "d": d}


def dense_data(pkg, case):
    X, y, offs = case["X"], case["y"], case["offs"]
    return pkg.PartitionedData([pkg.DensePartition(np.ascontiguousarray(y[a:b]), np.ascontiguousarray(X[a:b]))
                                for a, b in zip(offs[:-1], offs[1:])])


@pytest.mark.parametrize("storage", ["f32", "f64"])
@pytest.mark.parametrize("d", [1, 3, 100, 512, 1100, 4100])
def test_dense(pkg, d, storage):
    need_gpu()
    case = dense_case(d, storage)
    engine = pkg.HipEngine(dense_data(pkg, case))
    got = engine.column_stats()
    check_stats(got, case["ref"], f"dense d={d} {storage}", case["exact"])
    again = engine.column_stats()
    for a, b in zip(got[1:], again[1:]):
        assert a.tobytes() == b.tobytes()      # no atomics: the same bits from call to call
    # the host-pointer form gives the same bits
    raw = engine.ctx.column_stats(d)
    assert raw[0] == N and raw[1:1 + d].tobytes() == got.mean.tobytes()
    assert (raw[1 + d:1 + 2 * d] / (N - 1)).tobytes() == got.variance.tobytes()


def test_dense_device_resident_padded(pkg):
    """Zero-copy rows with a pitch beyond the padded d (statistics only read): columns [d, ld) play no part."""
    need_gpu()
    import torch
    case = dense_case(100, "f64")
    dev = torch.device("cuda", 0)
    ld = 104
    parts = []
    for a, b in zip(case["offs"][:-1], case["offs"][1:]):
        X = torch.full((b - a, ld), 7.0, dtype=torch.float64, device=dev)
        X[:, :100] = torch.from_numpy(case["X"][a:b]).to(dev)
        parts.append(pkg.DevicePartition(torch.from_numpy(case["y"][a:b]).to(dev), X, 100))
    check_stats(pkg.HipEngine(pkg.PartitionedData(parts)).column_stats(), case["ref"], "dense device ld=104",
                case["exact"])


@pytest.mark.parametrize("layout", ["dense", "csr"])
def test_single_row_has_variance_zero(pkg, layout):
    need_gpu()
    if layout == "dense":
        x = np.array([[3.0, 0.0, -2.5, 0.1]])
        data = pkg.PartitionedData([pkg.DensePartition(np.zeros(0), np.zeros((0, 4))),
                                    pkg.DensePartition(np.ones(1), x)])
        want = x[0]
    else:
        data = pkg.PartitionedData([pkg.CsrPartition(np.ones(1), np.array([0, 2], dtype=np.int64),
                                                     np.array([0, 2], dtype=np.int32), np.array([3.0, -2.5]), 4)])
        want = np.array([3.0, 0.0, -2.5, 0.0])
    got = pkg.column_stats(data)
    assert got.count == 1 and got.variance.tolist() == [0.0] * 4
    assert got.mean.tolist() == want.tolist() == got.max.tolist() == got.min.tolist()
    assert got.numNonzeros.tolist() == (want != 0).astype(int).tolist()
    model = pkg.StandardScaler().fit(data)
    assert model.factor.tolist() == [0.0] * 4


@pytest.mark.parametrize("layout", ["dense", "csr"])
def test_registry_of_empty_partitions(pkg, layout):
    need_gpu()
    if layout == "dense":
        part = pkg.DensePartition(np.zeros(0), np.zeros((0, 5), dtype=np.float32))
    else:
        part = pkg.CsrPartition(np.zeros(0), np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0), 5)
    engine = pkg.HipEngine(pkg.PartitionedData([part, part]))
    raw = engine.ctx.column_stats(5)
    assert raw.tolist() == [0.0] * 26                      # count 0, zeros elsewhere, PSGD_OK
    with pytest.raises(pkg.IllegalArgumentException, match="Nothing has been added to this summarizer"):
        engine.column_stats()


# ---- CSR ------------------------------------------------------------------------------------
PLAN = [((1, 16, 7, 16), 120), ((1, 16, 17, 32, 5), 125), ((0, 1, 16, 17, 128, 129, 300), 259),
        ((3, 40, 0, 129), N - 504)]


@functools.lru_cache(maxsize=None)
def csr_case(storage, bias):
    """The scoring tests' row-length plan (rows of 0, 1, 16, 17, 128, 129 and 300 non-zeros among
    them) over the partition sizes ROWS; random columns below d - 8, engineered ones above:
      d - 8   never stored (an all-zero column);
      d - 7   replaces the last entry of every third row that has one, holding an explicitly stored
              0.0 in half of them (row lengths unchanged);
    and with bias (every row then one to three entries longer):
      d - 5, d - 4   1e6 + N(0, 1) in every row;    d - 1   1.0 in every row (the appended bias)."""
    dt = np_dtype(storage)
    d = CSR_D
    rng = np.random.default_rng(77 + (1 if storage == "f32" else 0) + (2 if bias else 0))
    rows = []
    for lengths, count in PLAN:
        for k in range(count):
            m = lengths[k % len(lengths)]
            idx = np.sort(rng.choice(d - 8, size=m, replace=False)).astype(np.int64).tolist()
            val = [float(v) for v in rng.standard_normal(m).astype(dt)]
            val = [v if v != 0.0 else 1.0 for v in val]
            if m and len(rows) % 3 == 0:
                idx[-1] = d - 7
                if len(rows) % 2 == 0:
                    val[-1] = 0.0
            if bias:
                idx += [d - 5, d - 4, d - 1]
                val += [float(dt(1e6 + rng.standard_normal())), float(dt(1e6 + rng.standard_normal())), 1.0]
            rows.append((idx, val))
    assert len(rows) == N
    offs = np.concatenate([[0], np.cumsum(ROWS)]).astype(int)
    columns, stored_zero = {}, set()
    for idx, val in rows:
        for j, v in zip(idx, val):
            if v != 0.0:
                columns.setdefault(j, []).append(v)
            else:
                stored_zero.add(j)
    ref = Ref(N, d)
    for j, vals in columns.items():
        ref.set_column(j, vals, len(vals))
    assert stored_zero == {d - 7} and d - 8 not in columns
    lens = {len(r[0]) - (3 if bias else 0) for r in rows}
    assert {0, 1, 16, 17, 128, 129, 300} <= lens
    rngy = np.random.default_rng(5)
    return {"rows": rows, "offs": offs, "ref": ref, "dtype": dt, "d": d,
            "y": rngy.integers(0, 2, size=N).astype(np.float64)}


def csr_data(pkg, case):
    parts = []
    for a, b in zip(case["offs"][:-1], case["offs"][1:]):
        ptr = np.zeros(b - a + 1, dtype=np.int64)
        for k, r in enumerate(case["rows"][a:b]):
            ptr[k + 1] = ptr[k] + len(r[0])
        col = np.array([i for r in case["rows"][a:b] for i in r[0]], dtype=np.int32)
        val = np.array([v for r in case["rows"][a:b] for v in r[1]], dtype=case["dtype"])
        parts.append(pkg.CsrPartition(np.ascontiguousarray(case["y"][a:b]), ptr, col, val, case["d"]))
    return pkg.PartitionedData(parts)


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("storage", ["f32", "f64"])
def test_csr(pkg, storage, bias):
    need_gpu()
    case = csr_case(storage, bias)
    d = case["d"]
    got = pkg.HipEngine(csr_data(pkg, case)).column_stats()
    exact = [(d - 8, 0.0)] + ([(d - 1, 1.0)] if bias else [])
    check_stats(got, case["ref"], f"csr {storage} bias={bias}", exact)
    # the explicitly stored 0.0 does not count as a non-zero
    assert got.numNonzeros[d - 7] == case["ref"].nnz[d - 7] < sum(1 for r in case["rows"] if d - 7 in r[0])
    if bias:
        assert got.numNonzeros[d - 1] == N and got.max[d - 1] == got.min[d - 1] == 1.0


# ---- transform ----------------------------------------------------------------------------------
def unit(d, j):
    e = np.zeros(d)
    e[j] = 1.0
    return e


@pytest.mark.parametrize("storage", ["f32", "f64"])
@pytest.mark.parametrize("d", [3, 100])
def test_transform_dense(pkg, d, storage):
    """withMean and withStd: reading the transformed rows back through predict(p, e_j) (a dot with
    one non-zero term: exact) gives the NumPy transform, the constant column all 0.0; training on
    the transformed set equals training on the NumPy-transformed array bit for bit (d = 3 in f32
    has a pad column: touching it would change the bits)."""
    need_gpu()
    case = dense_case(d, storage)
    data = dense_data(pkg, case)
    model = pkg.StandardScaler(withMean=True, withStd=True).fit(data)
    assert model.factor[0] == 0.0 and model.factor[1] == 0.0       # the all-zero and the constant column
    scaled = model.transform(data)
    want = ((case["X"].astype(np.float64) - model.shift) * model.factor).astype(np_dtype(storage))
    engine = pkg.HipEngine(scaled)
    for j in sorted({0, 1, 2, d - 1}):
        for p, (a, b) in enumerate(zip(case["offs"][:-1], case["offs"][1:])):
            col = engine.predict(p, unit(d, j)).cpu().numpy()
            assert np.array_equal(col, want[a:b, j].astype(np.float64)), (j, p)
            if j == 1:
                assert np.all(col == 0.0)
    g, u = pkg.LogisticGradient(), pkg.SquaredL2SGDUpdater()
    w0 = np.zeros(d)
    w_dev, h_dev = pkg.runParallelizedSGD(scaled, g, u, 0.5, 3, 0.01, 1.0, w0, 0.0)
    host = pkg.PartitionedData([pkg.DensePartition(np.ascontiguousarray(case["y"][a:b]), np.ascontiguousarray(want[a:b]))
                                for a, b in zip(case["offs"][:-1], case["offs"][1:])])
    w_host, h_host = pkg.runParallelizedSGD(host, g, u, 0.5, 3, 0.01, 1.0, w0, 0.0)
    assert w_dev.tobytes() == w_host.tobytes() and np.asarray(h_dev).tobytes() == np.asarray(h_host).tobytes()


@pytest.mark.parametrize("storage", ["f32", "f64"])
def test_transform_csr(pkg, storage):
    need_gpu()
    case = csr_case(storage, True)
    d = case["d"]
    data = csr_data(pkg, case)
    model = pkg.StandardScaler().fit(data)
    f = model.factor
    assert f[d - 1] == 0.0 and f[d - 8] == 0.0 and model.shift is None
    scaled = model.transform(data)
    engine = pkg.HipEngine(scaled)
    dt = case["dtype"]
    for j in (d - 1, d - 5, d - 7, case["rows"][1][0][0]):
        for p, (a, b) in enumerate(zip(case["offs"][:-1], case["offs"][1:])):
            want = np.array([dt(dict(zip(*r)).get(j, 0.0) * f[j]) for r in case["rows"][a:b]], dtype=np.float64)
            got = engine.predict(p, unit(d, j)).cpu().numpy()
            assert np.array_equal(got, want.reshape(got.shape)), (j, p)
    # end to end against rows scaled on the host (the plan's own rows, empty ones included)
    case = csr_case(storage, False)
    data = csr_data(pkg, case)
    model = pkg.StandardScaler().fit(data)
    f = model.factor
    scaled = model.transform(data)
    g, u = pkg.LogisticGradient(), pkg.SquaredL2SGDUpdater()
    w0 = np.zeros(d)
    w_dev, h_dev = pkg.runParallelizedSGD(scaled, g, u, 0.5, 3, 0.01, 1.0, w0, 0.0)
    parts = []
    for part in data.partitions:
        val = (part.val.astype(np.float64) * f[part.col]).astype(dt)
        parts.append(pkg.CsrPartition(part.labels, part.row_ptr, part.col, val, d))
    w_host, h_host = pkg.runParallelizedSGD(pkg.PartitionedData(parts), g, u, 0.5, 3, 0.01, 1.0, w0, 0.0)
    assert w_dev.tobytes() == w_host.tobytes() and np.asarray(h_dev).tobytes() == np.asarray(h_host).tobytes()


def test_original_data_is_not_disturbed_and_unscale(pkg):
    """Training on the transformed set re-registers; the untransformed set then scores as before;
    and (withMean = False, f64 rows) the margins of the transformed rows at w are those of the
    original rows at model.unscale(w)."""
    need_gpu()
    d = 100
    case = dense_case(d, "f64")
    data = dense_data(pkg, case)
    g, u = pkg.LogisticGradient(), pkg.SquaredL2SGDUpdater()
    rng = np.random.default_rng(11)
    w_probe = rng.standard_normal(d) / np.sqrt(d)
    before = pkg.evaluate(data, g, u, 0.01, w_probe)
    model = pkg.StandardScaler().fit(data)
    scaled = model.transform(data)
    w, _ = pkg.runParallelizedSGD(scaled, g, u, 0.5, 3, 0.01, 1.0, np.zeros(d), 0.0)
    after = pkg.evaluate(data, g, u, 0.01, w_probe)
    assert (after.lossSum, after.count, after.nCorrect) == (before.lossSum, before.count, before.nCorrect)
    assert after.partLoss.tobytes() == before.partLoss.tobytes()
    e_scaled, e_orig = pkg.HipEngine(scaled), pkg.HipEngine(data)
    Xs = case["X"] * model.factor
    for p, (a, b) in enumerate(zip(case["offs"][:-1], case["offs"][1:])):
        m_scaled = e_scaled.predict(p, w).cpu().numpy()
        m_orig = e_orig.predict(p, model.unscale(w)).cpu().numpy()
        absum = np.abs(Xs[a:b] * w).sum(axis=1)
        bound = d * 2.0 ** -52 * absum + 2.0 ** -53 * absum
        assert np.all(np.abs(m_scaled - m_orig) <= bound), (p, float(np.max(np.abs(m_scaled - m_orig) - bound)))


def drive(pkg, engine, params, w0, iters, between=None):
    """runParallelizedSGD's loop (tol = 0) by hand over engine.epoch; between() runs after every iteration."""
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
            between()
    return engine.to_host(weights), np.array(history)


def test_column_stats_does_not_disturb_training(pkg):
    need_gpu()
    case = dense_case(100, "f64")
    data = dense_data(pkg, case)
    g, u = pkg.LogisticGradient(), pkg.SquaredL2SGDUpdater()
    w0 = np.zeros(100)
    w_ref, h_ref = pkg.runParallelizedSGD(data, g, u, 0.5, 3, 0.01, 1.0, w0, 0.0)
    engine = pkg.HipEngine(data)
    seen = []

    def between():
        k0, n0 = engine.ctx.last_kernel(), engine.ctx.chain_launches()
        seen.append(engine.column_stats())
        assert (engine.ctx.last_kernel(), engine.ctx.chain_launches()) == (k0, n0)

    params = pkg.make_params(g, u, 0.5, 0.01, 1.0, 0.0)
    w_plain, h_plain = drive(pkg, pkg.HipEngine(data), params, w0, 3)
    w_stat, h_stat = drive(pkg, engine, params, w0, 3, between)
    assert w_stat.tobytes() == w_plain.tobytes() and h_stat.tobytes() == h_plain.tobytes()
    assert w_stat.tobytes() == w_ref.tobytes() and h_stat.tobytes() == np.asarray(h_ref).tobytes()
    assert len(seen) == 3 and all(s.mean.tobytes() == seen[0].mean.tobytes() for s in seen)


def test_c_abi_refusals(pkg):
    need_gpu()
    import torch
    dev = torch.device("cuda", 0)
    X = torch.ones((8, 4), dtype=torch.float64, device=dev)
    y = torch.zeros(8, dtype=torch.float64, device=dev)
    engine = pkg.HipEngine(pkg.PartitionedData([pkg.DevicePartition(y, X, 4)]))
    with pytest.raises(pkg.DeviceError, match="zero-copy"):
        engine.ctx.transform_columns(None, np.full(4, 2.0))
    assert torch.all(X == 1.0).item()
    assert engine.column_stats().mean.tolist() == [1.0] * 4       # statistics only read: allowed
    part = pkg.CsrPartition(np.zeros(2), np.array([0, 1, 2], dtype=np.int64), np.array([0, 3], dtype=np.int32),
                            np.array([1.0, 2.0]), 4)
    engine = pkg.HipEngine(pkg.PartitionedData([part]))
    with pytest.raises(pkg.IllegalArgumentException, match="CSR"):
        engine.ctx.transform_columns(np.zeros(4), np.ones(4))
    # the host-pointer form, and twice is twice
    engine.ctx.transform_columns(None, np.array([2.0, 1.0, 1.0, 0.5]))
    engine.ctx.transform_columns(None, np.array([2.0, 1.0, 1.0, 0.5]))
    assert engine.column_stats().max.tolist() == [4.0, 0.0, 0.0, 0.5]
    engine.ctx.clear()
    engine.ctx.registered_token = None
    with pytest.raises(pkg.DeviceError, match="no partitions registered"):
        engine.ctx.transform_columns(None, np.ones(4))


# ---- world size 2 -------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.parametrize("P", [5, 1])
def test_two_ranks(tmp_path, pkg, P):
    """Two ranks sharing cuda:0 over gloo, each a fresh child process (tests/two_rank_colstats.py):
    both report the same statistics; the exact quantities equal the single-rank run, mean and
    variance stay within the bars; with P = 1 rank 1 holds no partition."""
    need_gpu()
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import two_rank_colstats as T
    out = str(tmp_path / "res.json")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), PSGD_TEST_P=str(P))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "two_rank_colstats.py"), out], env=env,
                       capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    with open(out) as f:
        res = json.load(f)
    X, y = T.make_data()
    one = pkg.HipEngine(pkg.PartitionedData.parallelize(y, X, P)).column_stats()
    ref = dense_ref(X)
    assert len(res) == 2 and res["0"] == res["1"]
    got = pkg.ColumnStats(res["0"]["count"], *(np.array(res["0"][k]) for k in ("mean", "variance", "numNonzeros", "max", "min")))
    assert got.count == one.count == X.shape[0]
    assert got.numNonzeros.tolist() == one.numNonzeros.tolist()
    assert got.max.tolist() == one.max.tolist() and got.min.tolist() == one.min.tolist()
    check_stats(got, ref, f"two ranks P={P}", [(1, 0.1)])
