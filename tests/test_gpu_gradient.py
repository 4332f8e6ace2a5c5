"""The batch gradient at fixed weights and GradientDescent on the device (psgd_gradient_sum_device /
psgd_gd_update_device through HipEngine.gradient_sum, HipEngine.gd_update and
GradientDescent.runMiniBatchSGD).

The reference is oracle/psgd_ref: gradient(kind, row, y, w) per row, the per-row gradients and
losses added left to right; updater(kind, w, g, step, it, reg, state); partition_seeds /
bernoulli_sample; is_converged. run_minibatch_ref below restates MLlib's runMiniBatchSGD from them.

Bars:
  every feature j: |G_j - Ref_j| <= 1e-9 A_j with A_j = sum_i |mult_i x_ij| from the oracle's per-row
  gradients (the project's fp64 bar on the sum of magnitudes: a gradient component cancels);
  lossSum within 1e-9 relative; count exact; no row or feature is left out.
Preconditions asserted on the oracle's numbers before each case (check_preconditions):
  every Hinge row has |1 - (2y - 1) dot| > 1e-9 (1 + sum|x w|): no row's branch can flip;
  for every j, sum_i nnz_i 2^-52 (sum|x_i w|) |x_ij| <= 1e-10 A_j: the multipliers' error from a
  reassociated dot cannot reach the bar.
Update kernel: w' within 1e-9 max(1, max|w'_ref|) per component, regVal within 1e-9 relative.
End to end: weights and loss history at rel 1e-9 (floor 1e-12) per entry, as the parity tests."""
import functools
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, has_gpu

import psgd_ref as R

pytestmark = pytest.mark.gpu

KINDS = {"logistic": R.GRAD_LOGISTIC, "least_squares": R.GRAD_LEAST_SQUARES, "hinge": R.GRAD_HINGE}
UPDS = {"simple": R.UPD_SIMPLE, "l2": R.UPD_SQUARED_L2, "l1": R.UPD_L1}
TILE = {"f32": 1024, "f64": 512}       # the dense kernels' tile_rows (the statistics passes' tiling)
FUSED_MAX = {"f32": 2048, "f64": 1024}  # the fused kernel's largest d


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not has_gpu():
        pytest.skip("no GPU")


def gradient_of(pkg, name):
    return {"logistic": pkg.LogisticGradient, "least_squares": pkg.LeastSquaresGradient,
            "hinge": pkg.HingeGradient}[name]()


def updater_of(pkg, name):
    return {"simple": pkg.SimpleSGDUpdater, "l2": pkg.SquaredL2SGDUpdater, "l1": pkg.L1SGDUpdater}[name]()


def np_dtype(storage):
    return np.float32 if storage == "f32" else np.float64


# ---- the oracle's batch sums ----------------------------------------------------------------------
def oracle_batch(kind, rows, ys, w, d):
    """(G, A, lossSum, count): the oracle's per-row gradients and losses added left to right, and
    A_j = sum_i |g_ij|. rows: dense lists or (indices, values) tuples."""
    G, A = np.zeros(d), np.zeros(d)
    loss = 0.0
    wl = [float(v) for v in w]
    for row, y in zip(rows, ys):
        g, l = R.gradient(kind, row, float(y), wl)
        loss = loss + l
        if isinstance(row, tuple):
            if g[0] == "dense":             # Logistic: a dense vector, zero off the row's indices
                idx, vals = row[0], [g[1][i] for i in row[0]]
            else:
                idx, vals = g[1], g[2]
            if not len(idx):
                continue
            idx, vals = np.asarray(idx, dtype=np.int64), np.asarray(vals, dtype=np.float64)
            G[idx] = G[idx] + vals          # (a row's indices are distinct)
            A[idx] = A[idx] + np.abs(vals)
        else:
            if g[0] != "dense":             # Hinge off the margin: the empty vector
                continue
            vals = np.asarray(g[1], dtype=np.float64)
            G = G + vals
            A = A + np.abs(vals)
    return G, A, loss, len(rows)


def check_preconditions(kind, rows, ys, w, d, A):
    w = np.asarray(w, dtype=np.float64)
    lhs = np.zeros(d)
    for row, y in zip(rows, ys):
        if isinstance(row, tuple):
            idx, x = np.asarray(row[0], dtype=np.int64), np.asarray(row[1], dtype=np.float64)
        else:
            idx, x = np.arange(d), np.asarray(row, dtype=np.float64)
        s = float(np.sum(np.abs(x * w[idx])))
        if kind == R.GRAD_HINGE:
            dot = R._dot(row, [float(v) for v in w]) if len(idx) <= 4096 else float(np.dot(x, w[idx]))
            assert abs(1.0 - (2.0 * y - 1.0) * dot) > 1e-9 * (1.0 + s), "a Hinge row sits on its margin"
        lhs[idx] += len(idx) * 2.0 ** -52 * s * np.abs(x)
    assert np.all(lhs <= 1e-10 * A), ("the multipliers' error could reach the bar", float(np.max(lhs / np.maximum(A, 1e-300))))


def check_sums(got, G, A, loss, count, what):
    d = len(G)
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == (d + 2,), what
    assert got[d + 1] == count, (what, got[d + 1], count)
    err = np.abs(got[:d] - G)
    worst = float(np.max(err / np.where(A > 0, A, 1.0))) if d else 0.0
    lrel = abs(got[d] - loss) / max(abs(loss), 1e-300) if loss != 0.0 else abs(got[d])
    print(f"{what}: worst |G - ref| / A {worst:.3g}, lossSum rel {lrel:.3g}, count {count}")
    assert np.all(err <= 1e-9 * A), (what, int(np.argmax(err - 1e-9 * A)), worst)
    assert lrel <= 1e-9, (what, got[d], loss)


# ---- dense --------------------------------------------------------------------------------------------
def dense_sizes(d, storage):
    if d <= 100:      # every ragged size, and a partition longer than three tiles
        return (0, 1, 65, 257, 1000, 3 * TILE[storage] + 37)
    if d <= 1000:
        return (0, 1, 65, 257)
    return (0, 1, 65, 70)   # (fewer rows at the fused path's limit: the oracle is pure Python)


@functools.lru_cache(maxsize=None)
def dense_case(d, storage, sizes=None):
    sizes = sizes or dense_sizes(d, storage)
    rng = np.random.default_rng(4100 + d + (9 if storage == "f32" else 0))
    n = sum(sizes)
    X = rng.standard_normal((n, d)).astype(np_dtype(storage))
    X[rng.random((n, d)) < 0.05] = 0.0
    w = 0.5 * rng.standard_normal(d) / np.sqrt(d)
    y = rng.integers(0, 2, size=n).astype(np.float64)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(int)
    return {"X": X, "y": y, "w": w, "offs": offs, "d": d, "rows": X.astype(np.float64).tolist()}


@functools.lru_cache(maxsize=None)
def dense_ref(d, storage, gname, sizes=None):
    c = dense_case(d, storage, sizes)
    G, A, loss, count = oracle_batch(KINDS[gname], c["rows"], c["y"], c["w"], d)
    check_preconditions(KINDS[gname], c["rows"], c["y"], c["w"], d, A)
    return G, A, loss, count


def dense_data(pkg, c, offs=None):
    offs = c["offs"] if offs is None else offs
    return pkg.PartitionedData([pkg.DensePartition(np.ascontiguousarray(c["y"][a:b]), np.ascontiguousarray(c["X"][a:b]))
                                for a, b in zip(offs[:-1], offs[1:])])


def run_dense(pkg, d, storage, gname):
    c = dense_case(d, storage)
    ref = dense_ref(d, storage, gname)
    engine = pkg.HipEngine(dense_data(pkg, c))
    g = gradient_of(pkg, gname)
    got = engine.gradient_sum(g, c["w"]).cpu().numpy()
    check_sums(got, *ref, f"dense d={d} {storage} {gname}")
    again = engine.gradient_sum(g, c["w"]).cpu().numpy()
    assert got.tobytes() == again.tobytes()          # no atomics: the same bits from call to call
    raw = engine.ctx.gradient_sum(KINDS[gname], c["w"])   # the host-pointer form gives the same bits
    assert raw.tobytes() == got.tobytes()
    return engine, got


@pytest.mark.parametrize("gname", list(KINDS))
@pytest.mark.parametrize("storage", ["f32", "f64"])
@pytest.mark.parametrize("d", [1, 3, 100, 512, 1000])
def test_dense(pkg, d, storage, gname):
    run_dense(pkg, d, storage, gname)


@pytest.mark.parametrize("gname", list(KINDS))
@pytest.mark.parametrize("storage", ["f32", "f64"])
@pytest.mark.parametrize("past", [0, 1])
def test_dense_fused_limit_and_two_pass(pkg, storage, gname, past):
    """The fused path's largest d, and one d just past it (the two-pass path)."""
    run_dense(pkg, FUSED_MAX[storage] + past * (5 if storage == "f32" else 1), storage, gname)


@pytest.mark.parametrize("d,storage,ld", [(101, "f32", 104), (100, "f64", 104), (3, "f32", 8), (2053, "f32", 2060)])
def test_dense_zero_copy_pitch(pkg, d, storage, ld):
    """psgd_register_dense_device rows with ld > d: the pad belongs to the caller (NaN here) and plays
    no part -- in the row's last, partial vector either."""
    import torch
    sizes = (0, 1, 65, 70)
    c = dense_case(d, storage, sizes)
    dev = torch.device("cuda", 0)
    tdt = torch.float32 if storage == "f32" else torch.float64
    parts = []
    for a, b in zip(c["offs"][:-1], c["offs"][1:]):
        X = torch.full((b - a, ld), float("nan"), dtype=tdt, device=dev)
        X[:, :d] = torch.from_numpy(c["X"][a:b]).to(dev)
        parts.append(pkg.DevicePartition(torch.from_numpy(c["y"][a:b]).to(dev), X, d))
    engine = pkg.HipEngine(pkg.PartitionedData(parts))
    for gname in KINDS:
        got = engine.gradient_sum(gradient_of(pkg, gname), c["w"]).cpu().numpy()
        check_sums(got, *dense_ref(d, storage, gname, sizes), f"zero-copy d={d} ld={ld} {gname}")


@pytest.mark.parametrize("storage", ["f32", "f64"])
def test_dense_one_or_several_partitions(pkg, storage):
    """The same rows registered as one partition or as several: the same totals within the bar (the
    tiling differs, so not bitwise)."""
    d = 100
    c = dense_case(d, storage)
    ref = dense_ref(d, storage, "logistic")
    one = np.array([0, c["offs"][-1]])
    g = pkg.LogisticGradient()
    a = pkg.HipEngine(dense_data(pkg, c, one)).gradient_sum(g, c["w"]).cpu().numpy()
    b = pkg.HipEngine(dense_data(pkg, c)).gradient_sum(g, c["w"]).cpu().numpy()
    check_sums(a, *ref, f"one partition {storage}")
    check_sums(b, *ref, f"several partitions {storage}")


@pytest.mark.parametrize("layout", ["dense", "csr"])
def test_registry_of_empty_partitions(pkg, layout):
    if layout == "dense":
        part = pkg.DensePartition(np.zeros(0), np.zeros((0, 5), dtype=np.float32))
    else:
        part = pkg.CsrPartition(np.zeros(0), np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0), 5)
    engine = pkg.HipEngine(pkg.PartitionedData([part, part]))
    assert engine.ctx.gradient_sum(0, np.ones(5)).tolist() == [0.0] * 7
    assert engine.gradient_sum(pkg.HingeGradient(), np.ones(5)).cpu().numpy().tolist() == [0.0] * 7


def test_errors(pkg):
    c = dense_case(3, "f64")
    engine = pkg.HipEngine(dense_data(pkg, c))
    L, ctx = pkg._native.lib(), engine.ctx
    w, out = np.zeros(3), np.zeros(5)
    EINVAL = pkg._native.PSGD_EINVAL
    assert L.psgd_gradient_sum(ctx.handle, 3, w.ctypes.data, 1.0, 1, out.ctypes.data) == EINVAL
    assert L.psgd_gradient_sum(ctx.handle, 0, None, 1.0, 1, out.ctypes.data) == EINVAL
    assert L.psgd_gradient_sum(ctx.handle, 0, w.ctypes.data, 1.0, 1, None) == EINVAL
    for f in (-0.1, 1.5, float("nan")):
        assert L.psgd_gradient_sum(ctx.handle, 0, w.ctypes.data, f, 1, out.ctypes.data) == EINVAL
        assert b"Sampling fraction" in L.psgd_last_error()
    gs = np.array([1.0, 1.0, 1.0, 0.0, 0.0])
    with pytest.raises(pkg.IllegalArgumentException, match="empty"):
        ctx.gd_update(0, w, gs, 1.0, 1, 0.0)                      # count 0
    gs[4] = 2.0
    with pytest.raises(pkg.IllegalArgumentException, match="iteration"):
        ctx.gd_update(0, w, gs, 1.0, 0, 0.0)
    for upd in (3, 4):
        with pytest.raises(pkg.UnsupportedOperationException, match="stateless"):
            ctx.gd_update(upd, w, gs, 1.0, 1, 0.0)
    ctx.clear()
    ctx.registered_token = None
    assert L.psgd_gradient_sum(ctx.handle, 0, w.ctypes.data, 1.0, 1, out.ctypes.data) == pkg._native.PSGD_ESTATE


# ---- CSR ----------------------------------------------------------------------------------------------
CSR_SIZES = (0, 1, 40, 90)


@functools.lru_cache(maxsize=None)
def csr_case(d, storage):
    """Rows of 0, 1, 64, 128 and 130 non-zeros (the lane groups' 64 and the 128-entry loop's edges)
    over an empty, a one-row and two longer partitions; column d - 1 is present in every row that
    has an entry, so every adder of a wave hits one address. The weights are small enough that
    every such row is inside the Hinge margin (|dot| < 1); the rows of 5 entries hold values 50 times
    larger in columns of the 64-entry row before them, so about a quarter of them are off the margin
    (multiplier 0) while every column they touch also has a row on it (the second precondition)."""
    dt = np_dtype(storage)
    rng = np.random.default_rng(900 + d % 1000 + (3 if storage == "f32" else 0))
    lengths = (1, 64, 0, 128, 130, 5)
    rows, last64 = [], None
    for k in range(sum(CSR_SIZES)):
        m = lengths[k % len(lengths)]
        if m == 5:
            idx = np.sort(rng.choice(last64[:-1], size=4, replace=False)).astype(np.int64).tolist() + [d - 1]
            val = [float(v) if v != 0 else 50.0 for v in (50.0 * rng.standard_normal(5)).astype(dt)]
        else:
            idx = np.sort(rng.choice(d - 1, size=max(m - 1, 0), replace=False)).astype(np.int64).tolist()
            if m:
                idx.append(d - 1)
            val = [float(v) if v != 0 else 1.0 for v in rng.standard_normal(len(idx)).astype(dt)]
        if m == 64:
            last64 = idx
        rows.append((idx, val))
    w = 0.1 * rng.standard_normal(d) / np.sqrt(64.0)
    y = rng.integers(0, 2, size=len(rows)).astype(np.float64)
    offs = np.concatenate([[0], np.cumsum(CSR_SIZES)]).astype(int)
    return {"rows": rows, "y": y, "w": w, "offs": offs, "d": d, "dtype": dt}


@functools.lru_cache(maxsize=None)
def csr_ref(d, storage, gname):
    c = csr_case(d, storage)
    G, A, loss, count = oracle_batch(KINDS[gname], c["rows"], c["y"], c["w"], d)
    check_preconditions(KINDS[gname], c["rows"], c["y"], c["w"], d, A)
    if gname == "hinge":   # rows on both sides of the margin
        wl = [float(v) for v in c["w"]]
        off = sum(1 for r, y in zip(c["rows"], c["y"]) if len(r[0]) and R.gradient(R.GRAD_HINGE, r, float(y), wl)[1] == 0.0)
        assert 0 < off < sum(1 for r in c["rows"] if len(r[0])) - off
    return G, A, loss, count


def csr_data(pkg, c, rows=None, y=None, offs=None):
    rows = c["rows"] if rows is None else rows
    y = c["y"] if y is None else y
    offs = c["offs"] if offs is None else offs
    parts = []
    for a, b in zip(offs[:-1], offs[1:]):
        ptr = np.zeros(b - a + 1, dtype=np.int64)
        for k, r in enumerate(rows[a:b]):
            ptr[k + 1] = ptr[k] + len(r[0])
        col = np.array([i for r in rows[a:b] for i in r[0]], dtype=np.int32)
        val = np.array([v for r in rows[a:b] for v in r[1]], dtype=c["dtype"])
        parts.append(pkg.CsrPartition(np.ascontiguousarray(y[a:b]), ptr, col, val, c["d"]))
    return pkg.PartitionedData(parts)


def lds_applies(pkg, d):
    import ctypes
    f = ctypes.CDLL(pkg._native.LIB_PATH)._ZN4psgd20grad_csr_lds_appliesEi
    f.restype, f.argtypes = ctypes.c_bool, [ctypes.c_int]
    return f(d)


@pytest.mark.parametrize("gname", list(KINDS))
@pytest.mark.parametrize("storage", ["f32", "f64"])
def test_csr_wide(pkg, storage, gname):
    d = 200000
    assert not lds_applies(pkg, d)
    c = csr_case(d, storage)
    engine = pkg.HipEngine(csr_data(pkg, c))
    got = engine.gradient_sum(gradient_of(pkg, gname), c["w"]).cpu().numpy()
    check_sums(got, *csr_ref(d, storage, gname), f"csr d={d} {storage} {gname}")
    again = engine.gradient_sum(gradient_of(pkg, gname), c["w"]).cpu().numpy()
    assert again[d:].tobytes() == got[d:].tobytes()      # lossSum and count are reproducible


@pytest.mark.parametrize("gname", list(KINDS))
@pytest.mark.parametrize("storage", ["f32", "f64"])
def test_csr_narrow_both_paths(pkg, storage, gname, monkeypatch):
    """A model inside the LDS path's range, and the same data forced down the global-atomic path."""
    d = 1000
    c = csr_case(d, storage)
    ref = csr_ref(d, storage, gname)
    engine = pkg.HipEngine(csr_data(pkg, c))
    monkeypatch.delenv("PSGD_GRAD_CSR_GLOBAL", raising=False)
    assert lds_applies(pkg, d)
    lds = engine.gradient_sum(gradient_of(pkg, gname), c["w"]).cpu().numpy()
    check_sums(lds, *ref, f"csr lds d={d} {storage} {gname}")
    monkeypatch.setenv("PSGD_GRAD_CSR_GLOBAL", "1")
    assert not lds_applies(pkg, d)
    glob = engine.gradient_sum(gradient_of(pkg, gname), c["w"]).cpu().numpy()
    check_sums(glob, *ref, f"csr global d={d} {storage} {gname}")
    assert glob[d:].tobytes() == lds[d:].tobytes()


# ---- sampling -----------------------------------------------------------------------------------------
def sampled(rows, ys, offs, fraction, iteration):
    """The rows of RDD.sample(false, fraction, 42 + iteration), partition by partition."""
    seeds = R.partition_seeds(42 + iteration, len(offs) - 1)
    keep = []
    for p, (a, b) in enumerate(zip(offs[:-1], offs[1:])):
        keep += [a + t for t in R.bernoulli_sample(seeds[p], b - a, fraction)]
    return [rows[i] for i in keep], [ys[i] for i in keep]


@pytest.mark.parametrize("iteration", [1, 2])
@pytest.mark.parametrize("fraction", [1e-9, 0.4, 0.999999])
@pytest.mark.parametrize("layout", ["dense", "two_pass", "csr"])
def test_sampled_batch(pkg, layout, fraction, iteration):
    if layout == "csr":
        c = csr_case(1000, "f32")
        data, d = csr_data(pkg, c), 1000
    else:
        d, storage = (100, "f64") if layout == "dense" else (1026, "f64")
        c = dense_case(d, storage)
        data = dense_data(pkg, c)
    rows, ys = sampled(c["rows"], c["y"], c["offs"], fraction, iteration)
    engine = pkg.HipEngine(data)
    # (a sampled CSR batch can lose the on-margin row of a column: Hinge's second precondition)
    for gname in (("logistic", "least_squares") if layout == "csr" else ("logistic", "hinge")):
        G, A, loss, count = oracle_batch(KINDS[gname], rows, ys, c["w"], d)
        check_preconditions(KINDS[gname], rows, ys, c["w"], d, A)
        got = engine.gradient_sum(gradient_of(pkg, gname), c["w"], fraction, iteration).cpu().numpy()
        check_sums(got, G, A, loss, count, f"sampled {layout} f={fraction} i={iteration} {gname}")
        if count == 0:
            assert got.tolist() == [0.0] * (d + 2)      # an all-empty batch: zeros and PSGD_OK
    assert engine.ctx.gradient_sum(0, c["w"], 0.0, iteration).tolist() == [0.0] * (d + 2)


# ---- the update kernel --------------------------------------------------------------------------------
@pytest.mark.parametrize("uname", list(UPDS))
@pytest.mark.parametrize("d", [1, 100, 4097])
def test_update(pkg, uname, d):
    import torch
    engine = pkg.HipEngine(dense_data(pkg, dense_case(3, "f64")))
    rng = np.random.default_rng(31 + d)
    w = rng.standard_normal(d)
    gs = np.concatenate([rng.standard_normal(d) * 37.0, [5.0, 37.0]])
    g = gs[:d] / gs[d + 1]
    for reg in (0.0, 0.1):
        for it in (1, 7):
            want = [float(v) for v in w]
            rv = R.updater(UPDS[uname], want, ("dense", [float(v) for v in g]), 0.7, it, reg, R.UpdaterState())
            got, grv = engine.ctx.gd_update(UPDS[uname], w, gs, 0.7, it, reg)
            want = np.array(want)
            assert np.all(np.abs(got - want) <= 1e-9 * max(1.0, np.max(np.abs(want)))), (uname, d, reg, it)
            assert abs(grv - rv) <= 1e-9 * abs(rv), (uname, d, reg, it, grv, rv)
            if reg == 0.0 or uname == "simple":
                assert grv == 0.0
            # in place (w_out = w) gives the same bits as out of place
            dev = torch.device("cuda", 0)
            wd = torch.from_numpy(w).to(dev)
            sd = torch.from_numpy(gs).to(dev)
            out, rv2 = engine.gd_update(updater_of(pkg, uname), wd, sd, 0.7, it, reg)
            buf = torch.cat([wd, torch.zeros(1, dtype=torch.float64, device=dev)])
            torch.cuda.synchronize()
            engine.ctx.gd_update_device(UPDS[uname], d, buf.data_ptr(), sd.data_ptr(), 0.7, it, reg, buf.data_ptr(),
                                        buf.data_ptr() + 8 * d, None)
            torch.cuda.synchronize()
            assert out.cpu().numpy().tobytes() == got.tobytes() == buf[:d].cpu().numpy().tobytes()
            assert rv2 == grv == float(buf[d].cpu())


def test_update_l1_threshold(pkg):
    """L1 with components on both sides of the soft threshold, and well away from it."""
    engine = pkg.HipEngine(dense_data(pkg, dense_case(3, "f64")))
    step, it, reg = 0.5, 4, 0.2
    s = step / np.sqrt(it)
    shrink = reg * s
    t = np.array([0.25, -0.25, 2.0, -2.0, 0.5, -3.0, 0.0]) * shrink     # w - s g
    g = np.linspace(-1.0, 1.0, len(t))
    w = t + s * g
    pre = w + (-s) * g
    assert np.all(np.abs(np.abs(pre) - shrink) > 0.4 * shrink)        # nothing near the threshold
    gs = np.concatenate([g * 8.0, [1.0, 8.0]])
    want = [float(v) for v in w]
    rv = R.updater(R.UPD_L1, want, ("dense", [float(v) for v in gs[:-2] / 8.0]), step, it, reg, R.UpdaterState())
    got, grv = engine.ctx.gd_update(R.UPD_L1, w, gs, step, it, reg)
    assert (np.array(want) == 0.0).tolist() == [True, True, False, False, True, False, True]
    assert (got == 0.0).tolist() == (np.array(want) == 0.0).tolist()
    assert np.all(np.abs(got - np.array(want)) <= 1e-9 * max(1.0, np.max(np.abs(want))))
    assert abs(grv - rv) <= 1e-9 * abs(rv) and rv > 0.0


# ---- end to end ---------------------------------------------------------------------------------------
def run_minibatch_ref(rows, ys, offs, kind, upd, step, iters, reg, fraction, w0, tol):
    """MLlib 1.6.1 GradientDescent.runMiniBatchSGD from the oracle's pieces -> (weights, history,
    the isConverged ratios ||prev - cur|| / max(||cur||, 1) of the tested iterations)."""
    d = len(w0)
    w = [float(v) for v in w0]
    hist, ratios = [], []
    reg_val = R.updater(upd, list(w), ("dense", [0.0] * d), 0.0, 1, reg, R.UpdaterState())
    prev = cur = None
    converged = False
    i = 1
    while not converged and i <= iters:
        brows, bys = sampled(rows, ys, offs, fraction, i)
        G, _, loss, count = oracle_batch(kind, brows, bys, w, d)
        if count > 0:
            hist.append(loss / count + reg_val)
            w = list(w)
            reg_val = R.updater(upd, w, ("dense", [float(v) for v in G / float(count)]), step, i, reg, R.UpdaterState())
            prev, cur = cur, list(w)
            if prev is not None:
                converged = R.is_converged(prev, cur, tol)
                diff = np.linalg.norm(np.array(prev) - np.array(cur))
                ratios.append(diff / max(np.linalg.norm(cur), 1.0))
        i += 1
    return np.array(w), np.array(hist), ratios


def assert_close(a, b, what, rel=1e-9, floor=1e-12):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    diff = np.abs(a - b)
    ok = (diff <= rel * np.maximum(np.abs(a), np.abs(b))) | (diff <= floor)
    assert ok.all(), (what, int(np.argmax(~ok)), a.flat[int(np.argmax(~ok))], b.flat[int(np.argmax(~ok))])


@functools.lru_cache(maxsize=None)
def small_case(layout):
    rng = np.random.default_rng(515)
    sizes = (0, 1, 65, 150)
    n, d = sum(sizes), 12
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(int)
    w_true = rng.standard_normal(d)
    if layout == "dense":
        X = rng.standard_normal((n, d))
        rows = X.tolist()
        y = (X @ w_true + 0.3 * rng.standard_normal(n) > 0).astype(np.float64)
        return {"X": X, "rows": rows, "y": y, "offs": offs, "d": d, "dtype": np.float64}
    rows, ys = [], []
    for k in range(n):
        m = (0, 3, 12, 5)[k % 4]
        idx = np.sort(rng.choice(d, size=m, replace=False)).astype(np.int64).tolist()
        val = [float(v) for v in rng.standard_normal(m)]
        rows.append((idx, val))
        ys.append(float(sum(v * w_true[i] for i, v in zip(idx, val)) > 0))
    return {"rows": rows, "y": np.array(ys), "offs": offs, "d": d, "dtype": np.float64}


def small_data(pkg, layout):
    c = small_case(layout)
    return dense_data(pkg, c) if layout == "dense" else csr_data(pkg, c)


@pytest.mark.parametrize("uname", list(UPDS))
@pytest.mark.parametrize("gname", list(KINDS))
def test_gradient_descent_matches_mllib_loop(pkg, gname, uname):
    for layout in ("dense", "csr"):
        c = small_case(layout)
        data = small_data(pkg, layout)
        w0 = np.linspace(-0.2, 0.2, c["d"])
        for fraction in (1.0, 0.5):
            w_ref, h_ref, _ = run_minibatch_ref(c["rows"], c["y"], c["offs"], KINDS[gname], UPDS[uname], 0.5, 6, 0.05,
                                                fraction, w0, 0.0)
            w, h = pkg.GradientDescent.runMiniBatchSGD(data, gradient_of(pkg, gname), updater_of(pkg, uname), 0.5, 6,
                                                       0.05, fraction, w0, 0.0)
            what = f"{layout} {gname} {uname} f={fraction}"
            assert len(h_ref) == 6
            assert_close(h, h_ref, what + " history")
            assert_close(w, w_ref, what + " weights")


def test_gradient_descent_converges_early(pkg):
    """convergenceTol stops the loop at the oracle's iteration (its ratio is not near the tolerance)."""
    c = small_case("dense")
    w0 = np.zeros(c["d"])
    tol = 0.05
    args = (KINDS["logistic"], UPDS["l2"], 1.0, 40, 0.1, 1.0, w0, tol)
    w_ref, h_ref, ratios = run_minibatch_ref(c["rows"], c["y"], c["offs"], *args)
    assert 2 <= len(h_ref) < 40
    assert all(abs(r - tol) > 1e-6 * tol for r in ratios) and ratios[-1] < tol
    gd = pkg.GradientDescent(pkg.LogisticGradient(), pkg.SquaredL2SGDUpdater()).setNumIterations(40) \
        .setRegParam(0.1).setConvergenceTol(tol)
    w, h = pkg.GradientDescent.runMiniBatchSGD(small_data(pkg, "dense"), gd.gradient, gd.updater, gd.stepSize,
                                               gd.numIterations, gd.regParam, gd.miniBatchFraction, w0,
                                               gd.convergenceTol)
    assert len(h) == len(h_ref)
    assert_close(h, h_ref, "early stop history")
    assert_close(w, w_ref, "early stop weights")
    assert_close(gd.optimize(small_data(pkg, "dense"), w0), w_ref, "optimize")


def test_gradient_descent_on_standardized_data(pkg):
    c = small_case("dense")
    data = small_data(pkg, "dense")
    model = pkg.StandardScaler().fit(data)
    scaled = model.transform(data)
    Xs = c["X"] * model.factor          # f64 storage: round_to_storage is the identity
    w0 = np.zeros(c["d"])
    w_ref, h_ref, _ = run_minibatch_ref(Xs.tolist(), c["y"], c["offs"], KINDS["logistic"], UPDS["simple"], 1.0, 5,
                                        0.0, 1.0, w0, 0.0)
    w, h = pkg.GradientDescent.runMiniBatchSGD(scaled, pkg.LogisticGradient(), pkg.SimpleSGDUpdater(), 1.0, 5, 0.0,
                                               1.0, w0, 0.0)
    assert_close(h, h_ref, "standardized history")
    assert_close(w, w_ref, "standardized weights")
    gs = pkg.gradient_sum(scaled, pkg.LogisticGradient(), w)
    G, A, loss, count = oracle_batch(KINDS["logistic"], Xs.tolist(), c["y"], w, c["d"])
    check_preconditions(KINDS["logistic"], Xs.tolist(), c["y"], w, c["d"], A)
    check_sums(np.concatenate([gs.gradient, [gs.lossSum, gs.count]]), G, A, loss, count, "standardized gradient_sum")


# ---- isolation ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("fraction", [1.0, 0.5])
def test_epoch_state_is_left_alone(pkg, fraction):
    c = small_case("dense")
    w0 = np.linspace(-0.2, 0.2, c["d"])
    g, u = pkg.LogisticGradient(), pkg.SquaredL2SGDUpdater()
    data_a, data_b = small_data(pkg, "dense"), small_data(pkg, "dense")
    plain = pkg.HipEngine(data_a)
    w_a, h_a = pkg.runParallelizedSGD(data_a, g, u, 1.0, 3, 0.01, fraction, w0, 0.0, engine=plain)
    before = (plain.ctx.last_kernel(), plain.ctx.chain_launches())
    plain.gradient_sum(g, w0, fraction, 1)
    plain.gradient_sum(g, w0, 1.0, 1)
    assert (plain.ctx.last_kernel(), plain.ctx.chain_launches()) == before
    # a gradient_sum between an engine's setup and its epochs changes none of their bits
    mixed = pkg.HipEngine(data_b)
    mixed.gradient_sum(g, w0, fraction, 1)
    w_b, h_b = pkg.runParallelizedSGD(data_b, g, u, 1.0, 3, 0.01, fraction, w0, 0.0, engine=mixed)
    assert w_a.tobytes() == w_b.tobytes() and h_a.tobytes() == h_b.tobytes()


# ---- world size 2 -------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.parametrize("P", [5, 1])
def test_two_ranks(tmp_path, pkg, P):
    """Two ranks sharing cuda:0 over gloo, each a fresh child process (tests/two_rank_gradient.py):
    both hold identical gradient_sum bits and identical GradientDescent weights; the sums are the
    oracle's within the bars, the weights the one-rank run's; with P = 1 rank 1 holds no partition."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import two_rank_gradient as T
    out = str(tmp_path / "res.json")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), PSGD_TEST_P=str(P))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "two_rank_gradient.py"), out], env=env,
                       capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    with open(out) as f:
        res = json.load(f)
    assert len(res) == 2 and res["0"] == res["1"]          # floats survive JSON exactly: identical bits
    X, y, w = T.make_data()
    d = X.shape[1]
    G, A, loss, count = oracle_batch(R.GRAD_LOGISTIC, X.tolist(), y, w, d)
    check_preconditions(R.GRAD_LOGISTIC, X.tolist(), y, w, d, A)
    check_sums(np.array(res["0"]["sum"]), G, A, loss, count, f"two ranks P={P}")
    data = pkg.PartitionedData.parallelize(y, X, P)
    w1, h1 = pkg.GradientDescent.runMiniBatchSGD(data, pkg.LogisticGradient(), pkg.SquaredL2SGDUpdater(),
                                                 *T.GD_ARGS, w, 0.0)
    assert_close(res["0"]["weights"], w1, "two-rank weights")
    assert_close(res["0"]["history"], h1, "two-rank history")
