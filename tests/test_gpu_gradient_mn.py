"""The multinomial batch gradient and GradientDescent for LogisticGradient(numClasses > 2) on the
device (psgd_gradient_sum_multinomial_device through HipEngine.gradient_sum_multinomial,
gradient_sum_multinomial and GradientDescent.runMiniBatchSGDMultinomial).

Truth: tests/multinomial_grad_truth.py, the numpy restatement that tests/test_multinomial_grad_truth.py
checks against oracle/psgd_ref.py::multinomial row by row.

Bar (check_sums): every (c, j): |G - ref| <= 1e-9 A[c, j] with A = sum_i |mult_ic x_ij|; lossSum
within 1e-9 relative; count exact; no class or feature is left out.
Precondition, asserted on the truth before each comparison (truth_of): sum_i e_ic |x_ij| <= 1e-10
A[c, j] with e_ic = 2 p_ic max_k(nnz_i 2^-52 sum_j |x_ij W_kj|) -- margins summed in another order
cannot move a multiplier far enough to reach the bar.

The two dense paths (fused, general) sum a row's margins in different lane orders: between them
`count` is byte-equal and lossSum and gradientSum agree within the bar -- no more is guaranteed. The
general path's results do not depend on its row ranges, bit for bit. CSR: lossSum and count are
byte-equal between the LDS and the global-atomic path."""
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

import multinomial_grad_truth as GT
import psgd_ref as R

pytestmark = pytest.mark.gpu

UPDS = {"simple": R.UPD_SIMPLE, "l2": R.UPD_SQUARED_L2, "l1": R.UPD_L1}


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not has_gpu():
        pytest.skip("no GPU")


@pytest.fixture(autouse=True)
def default_paths(monkeypatch):
    for name in ("PSGD_GRAD_MN_TWO_PASS", "PSGD_GRAD_MN_FUSE_ALL", "PSGD_GRAD_CSR_GLOBAL", "PSGD_GRAD_MN_RANGE"):
        monkeypatch.delenv(name, raising=False)


def updater_of(pkg, name):
    return {"simple": pkg.SimpleSGDUpdater, "l2": pkg.SquaredL2SGDUpdater, "l1": pkg.L1SGDUpdater}[name]()


def np_dtype(storage):
    return np.float32 if storage == "f32" else np.float64


def plan(pkg, *a):
    return pkg._native.gradient_multinomial_plan(*a)


def class_weights(rng, K, d):
    """w = 0.5 N(0, 1) / sqrt(d) per block."""
    return (0.5 * rng.standard_normal((K - 1, d)) / np.sqrt(d)).ravel()


def truth_of(rows, ys, w, K, d):
    t = GT.gradient(rows, ys, w, K, d)
    worst = float(np.max(t.pre / np.where(t.A > 0, t.A, 1.0))) if t.count else 0.0
    assert np.all(t.pre <= 1e-10 * t.A), ("the multipliers' error could reach the bar", worst)
    return t


def check_sums(got, t, what):
    n = t.G.size
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == (n + 2,), what
    assert got[n + 1] == t.count, (what, got[n + 1], t.count)
    err = np.abs(got[:n] - t.G.ravel())
    A = t.A.ravel()
    worst = float(np.max(err / np.where(A > 0, A, 1.0))) if n else 0.0
    lrel = abs(got[n] - t.lossSum) / max(abs(t.lossSum), 1e-300) if t.lossSum != 0.0 else abs(got[n])
    print(f"{what}: worst |G - ref| / A {worst:.3g}, lossSum rel {lrel:.3g}, count {t.count}")
    assert np.all(err <= 1e-9 * A), (what, int(np.argmax(err - 1e-9 * A)), worst)
    assert lrel <= 1e-9, (what, got[n], t.lossSum)


# ---- dense ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dense_case(d, storage, K, sizes, labels=None):
    rng = np.random.default_rng(5200 + 7 * d + K + (9 if storage == "f32" else 0))
    n = sum(sizes)
    X = rng.standard_normal((n, d)).astype(np_dtype(storage))
    X[rng.random((n, d)) < 0.05] = 0.0
    w = class_weights(rng, K, d)
    y = rng.integers(0, K, size=n).astype(np.float64)
    if labels is not None:
        y = np.array([labels[k % len(labels)] for k in range(n)], dtype=np.float64)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(int)
    return {"X": X, "y": y, "w": w, "offs": offs, "d": d, "K": K, "rows": X.astype(np.float64)}


@functools.lru_cache(maxsize=None)
def dense_truth(d, storage, K, sizes, labels=None):
    c = dense_case(d, storage, K, sizes, labels)
    return truth_of(c["rows"], c["y"], c["w"], K, d)


def dense_data(pkg, c):
    offs = c["offs"]
    return pkg.PartitionedData([pkg.DensePartition(np.ascontiguousarray(c["y"][a:b]), np.ascontiguousarray(c["X"][a:b]))
                                for a, b in zip(offs[:-1], offs[1:])])


def run_dense(pkg, d, storage, K, sizes, path=None, labels=None):
    c = dense_case(d, storage, K, sizes, labels)
    t = dense_truth(d, storage, K, sizes, labels)
    if path is not None:
        assert plan(pkg, "dense", storage, d, K)["path"] == path
    engine = pkg.HipEngine(dense_data(pkg, c))
    got = engine.gradient_sum_multinomial(K, c["w"]).cpu().numpy()
    check_sums(got, t, f"dense d={d} {storage} K={K} {path}")
    again = engine.gradient_sum_multinomial(K, c["w"]).cpu().numpy()
    assert got.tobytes() == again.tobytes()          # no atomics: the same bits from call to call
    raw = engine.ctx.gradient_sum_multinomial(K, c["w"])   # the host-pointer form gives the same bits
    assert raw.tobytes() == got.tobytes()
    return engine, c, t, got


def dense_sizes(pkg, d, storage):
    tile = plan(pkg, "dense", storage, d, 3)["tile_rows"]
    return (0, 1, 65, 257, 3 * tile + 37) if d <= 100 else (0, 1, 65, 257)


@pytest.mark.parametrize("storage", ["f32", "f64"])
@pytest.mark.parametrize("d", [1, 3, 100, 512])
@pytest.mark.parametrize("K", [3, 10])
def test_dense(pkg, K, d, storage):
    run_dense(pkg, d, storage, K, dense_sizes(pkg, d, storage))


def largest_fused_d(pkg, storage, K):
    lo, hi = 1, 1 << 16
    assert plan(pkg, "dense", storage, lo, K)["path"] == "fused"
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if plan(pkg, "dense", storage, mid, K)["path"] == "fused" else (lo, mid)
    return lo


SMALL = (0, 1, 65, 70)


@pytest.mark.parametrize("storage", ["f32", "f64"])
def test_fused_limit_and_forced_general(pkg, storage, monkeypatch):
    """The largest fused d for K = 3, the first d past it, and the fused shape down the general path."""
    K = 3
    dmax = largest_fused_d(pkg, storage, K)
    engine, c, t, fused = run_dense(pkg, dmax, storage, K, SMALL, "fused")
    run_dense(pkg, dmax + 1, storage, K, SMALL, "general")
    monkeypatch.setenv("PSGD_GRAD_MN_TWO_PASS", "1")
    assert plan(pkg, "dense", storage, dmax, K)["path"] == "general"
    general = engine.gradient_sum_multinomial(K, c["w"]).cpu().numpy()
    check_sums(general, t, f"forced general d={dmax} {storage}")
    assert general[-1:].tobytes() == fused[-1:].tobytes()     # count; the losses agree within the bar only


@pytest.mark.parametrize("K,d,storage", [(3, 100, "f32"), (5, 100, "f32"), (10, 30, "f64"), (10, 37, "f32"), (17, 9, "f64")])
def test_forced_general_on_fused_shapes(pkg, K, d, storage, monkeypatch):
    sizes = dense_sizes(pkg, d, storage)
    engine, c, t, fused = run_dense(pkg, d, storage, K, sizes, "fused")
    monkeypatch.setenv("PSGD_GRAD_MN_TWO_PASS", "1")
    general = engine.gradient_sum_multinomial(K, c["w"]).cpu().numpy()
    check_sums(general, t, f"forced general d={d} {storage} K={K}")
    assert general[-1:].tobytes() == fused[-1:].tobytes()
    assert general.tobytes() == engine.gradient_sum_multinomial(K, c["w"]).cpu().numpy().tobytes()


def test_class_blocks_within_and_past_lds(pkg):
    cap = pkg._native.multiclass_switches()["lds_weights"]
    K = 5
    d = cap // (K - 1)
    for dd, lds in ((d, 1), (d + 1, 0)):
        p = plan(pkg, "dense", "f32", dd, K)
        assert p["path"] == "general" and p["weights_in_lds"] == lds
        run_dense(pkg, dd, "f32", K, SMALL)


@pytest.mark.parametrize("storage", ["f32", "f64"])
@pytest.mark.parametrize("K", [65, 66])
def test_softmax_shapes(pkg, K, storage):
    """K - 1 = 64: a lane takes a row; K - 1 = 65: the lanes go across the classes."""
    assert plan(pkg, "dense", storage, 20, K)["wide_softmax"] == (1 if K == 66 else 0)
    run_dense(pkg, 20, storage, K, (0, 1, 65, 257), "general")


def test_most_classes_and_one_past(pkg):
    K = 4097
    engine, c, t, got = run_dense(pkg, 3, "f32", K, (70,), "general")
    with pytest.raises(pkg.UnsupportedOperationException, match="4097"):
        engine.ctx.gradient_sum_multinomial(K + 1, np.zeros(K * 3))


@pytest.mark.parametrize("storage", ["f32", "f64"])
def test_row_ranges_do_not_change_a_bit(pkg, storage, monkeypatch):
    """K - 1 = 39 classes: a record covers 4 tiles. The batch in one range, in ranges of 8 tiles (two
    spans), of 2 tiles (half a span: the items continue from the span's record) and of 1 tile."""
    K, d = 40, 20
    p = plan(pkg, "dense", storage, d, K)
    assert p["path"] == "general" and p["span"] == 4 and p["range"] > 16
    sizes = (5 * p["tile_rows"] + 37, 0, 2 * p["tile_rows"] + 1, 3)      # 6 + 0 + 3 + 1 tiles
    engine, c, t, whole = run_dense(pkg, d, storage, K, sizes)
    for r in (8, 2, 1):
        monkeypatch.setenv("PSGD_GRAD_MN_RANGE", str(r))
        assert plan(pkg, "dense", storage, d, K)["range"] == r
        assert engine.gradient_sum_multinomial(K, c["w"]).cpu().numpy().tobytes() == whole.tobytes(), r


@pytest.mark.parametrize("two_pass", [False, True])
@pytest.mark.parametrize("d,storage,ld", [(101, "f32", 104), (99, "f64", 104), (3, "f32", 8), (2051, "f32", 2060)])
def test_dense_zero_copy_pitch(pkg, d, storage, ld, two_pass, monkeypatch):
    """psgd_register_dense_device rows with ld > d: the pad belongs to the caller (NaN here) and plays
    no part -- in the row's last, partial 16-byte vector either."""
    import torch
    K = 3
    if two_pass:
        monkeypatch.setenv("PSGD_GRAD_MN_TWO_PASS", "1")
    assert plan(pkg, "dense", storage, d, K)["path"] == ("general" if two_pass or d > 2048 else "fused")
    c = dense_case(d, storage, K, SMALL)
    dev = torch.device("cuda", 0)
    tdt = torch.float32 if storage == "f32" else torch.float64
    parts = []
    for a, b in zip(c["offs"][:-1], c["offs"][1:]):
        X = torch.full((b - a, ld), float("nan"), dtype=tdt, device=dev)
        X[:, :d] = torch.from_numpy(c["X"][a:b]).to(dev)
        parts.append(pkg.DevicePartition(torch.from_numpy(c["y"][a:b]).to(dev), X, d))
    engine = pkg.HipEngine(pkg.PartitionedData(parts))
    got = engine.gradient_sum_multinomial(K, c["w"]).cpu().numpy()
    check_sums(got, dense_truth(d, storage, K, SMALL), f"zero-copy d={d} ld={ld} two_pass={two_pass}")


@pytest.mark.parametrize("layout", ["dense", "csr"])
def test_registry_of_empty_partitions(pkg, layout):
    if layout == "dense":
        part = pkg.DensePartition(np.zeros(0), np.zeros((0, 5), dtype=np.float32))
    else:
        part = pkg.CsrPartition(np.zeros(0), np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0), 5)
    engine = pkg.HipEngine(pkg.PartitionedData([part, part]))
    assert engine.ctx.gradient_sum_multinomial(3, np.ones(10)).tolist() == [0.0] * 12
    assert engine.gradient_sum_multinomial(3, np.ones(10)).cpu().numpy().tolist() == [0.0] * 12


# ---- CSR ------------------------------------------------------------------------------------------
CSR_SIZES = (0, 1, 40, 90)


@functools.lru_cache(maxsize=None)
def csr_case(d, storage, K):
    """Rows of 0, 1, 64, 128, 300 (longer than one hold of 64 lanes x 4 entries) and 5 non-zeros over
    an empty, a one-row and two longer partitions; column d - 1 is present in every row that has an
    entry, so every adder of a wave hits one address."""
    dt = np_dtype(storage)
    rng = np.random.default_rng(950 + d % 1000 + K + (3 if storage == "f32" else 0))
    lengths = (1, 64, 0, 128, 300, 5)
    rows = []
    for k in range(sum(CSR_SIZES)):
        m = min(lengths[k % len(lengths)], d)
        idx = np.sort(rng.choice(d - 1, size=max(m - 1, 0), replace=False)).astype(np.int64).tolist()
        if m:
            idx.append(d - 1)
        val = [float(v) if v != 0 else 1.0 for v in rng.standard_normal(len(idx)).astype(dt)]
        rows.append((idx, val))
    w = (0.5 * rng.standard_normal((K - 1, d)) / np.sqrt(64.0)).ravel()
    y = rng.integers(0, K, size=len(rows)).astype(np.float64)
    offs = np.concatenate([[0], np.cumsum(CSR_SIZES)]).astype(int)
    return {"rows": rows, "y": y, "w": w, "offs": offs, "d": d, "K": K, "dtype": dt}


@functools.lru_cache(maxsize=None)
def csr_truth(d, storage, K):
    c = csr_case(d, storage, K)
    return truth_of(c["rows"], c["y"], c["w"], K, d)


def csr_data(pkg, c):
    rows, y, offs = c["rows"], c["y"], c["offs"]
    parts = []
    for a, b in zip(offs[:-1], offs[1:]):
        ptr = np.zeros(b - a + 1, dtype=np.int64)
        for k, r in enumerate(rows[a:b]):
            ptr[k + 1] = ptr[k] + len(r[0])
        col = np.array([i for r in rows[a:b] for i in r[0]], dtype=np.int32)
        val = np.array([v for r in rows[a:b] for v in r[1]], dtype=c["dtype"])
        parts.append(pkg.CsrPartition(np.ascontiguousarray(y[a:b]), ptr, col, val, c["d"]))
    return pkg.PartitionedData(parts)


@pytest.mark.parametrize("storage", ["f32", "f64"])
@pytest.mark.parametrize("K", [3, 6])
def test_csr_narrow_both_paths(pkg, K, storage, monkeypatch):
    """(K - 1) d inside the LDS accumulator's range, and the same data forced down the global path."""
    d = 1000
    c, t = csr_case(d, storage, K), csr_truth(d, storage, K)
    n = (K - 1) * d
    engine = pkg.HipEngine(csr_data(pkg, c))
    assert plan(pkg, "csr", storage, d, K, 300)["path"] == "csr_lds"
    lds = engine.gradient_sum_multinomial(K, c["w"]).cpu().numpy()
    check_sums(lds, t, f"csr lds d={d} {storage} K={K}")
    again = engine.gradient_sum_multinomial(K, c["w"]).cpu().numpy()
    assert again[n:].tobytes() == lds[n:].tobytes()      # lossSum and count are reproducible
    monkeypatch.setenv("PSGD_GRAD_CSR_GLOBAL", "1")
    assert plan(pkg, "csr", storage, d, K, 300)["path"] == "csr_global"
    glob = engine.gradient_sum_multinomial(K, c["w"]).cpu().numpy()
    check_sums(glob, t, f"csr global d={d} {storage} K={K}")
    assert glob[n:].tobytes() == lds[n:].tobytes()
    raw = engine.ctx.gradient_sum_multinomial(K, c["w"])
    check_sums(raw, t, "csr host-pointer form")
    assert raw[n:].tobytes() == lds[n:].tobytes()


@pytest.mark.parametrize("storage", ["f32", "f64"])
def test_csr_wide_model(pkg, storage):
    d, K = 200000, 3
    assert plan(pkg, "csr", storage, d, K, 300)["path"] == "csr_global"
    c = csr_case(d, storage, K)
    engine = pkg.HipEngine(csr_data(pkg, c))
    got = engine.gradient_sum_multinomial(K, c["w"]).cpu().numpy()
    check_sums(got, csr_truth(d, storage, K), f"csr d={d} {storage}")


@pytest.mark.parametrize("K", [65, 66])
def test_csr_softmax_shapes(pkg, K, monkeypatch):
    d = 90                                         # (K - 1) d fits the LDS accumulator
    c, t = csr_case(d, "f64", K), csr_truth(d, "f64", K)
    engine = pkg.HipEngine(csr_data(pkg, c))
    p = plan(pkg, "csr", "f64", d, K, 90)
    assert p["path"] == "csr_lds" and p["wide_softmax"] == (1 if K == 66 else 0)
    lds = engine.gradient_sum_multinomial(K, c["w"]).cpu().numpy()
    check_sums(lds, t, f"csr lds K={K}")
    monkeypatch.setenv("PSGD_GRAD_CSR_GLOBAL", "1")
    glob = engine.gradient_sum_multinomial(K, c["w"]).cpu().numpy()
    check_sums(glob, t, f"csr global K={K}")
    assert glob[-2:].tobytes() == lds[-2:].tobytes()


# ---- sampling -------------------------------------------------------------------------------------
def sampled(rows, ys, offs, fraction, iteration):
    """The rows of RDD.sample(false, fraction, 42 + iteration), partition by partition."""
    seeds = R.partition_seeds(42 + iteration, len(offs) - 1)
    keep = []
    for p, (a, b) in enumerate(zip(offs[:-1], offs[1:])):
        keep += [a + t for t in R.bernoulli_sample(seeds[p], b - a, fraction)]
    return [rows[i] for i in keep], [ys[i] for i in keep]


@pytest.mark.parametrize("iteration", [1, 2])
@pytest.mark.parametrize("fraction", [1e-9, 0.4, 0.999999])
@pytest.mark.parametrize("layout", ["fused", "general", "csr"])
def test_sampled_batch(pkg, layout, fraction, iteration, monkeypatch):
    K = 3
    if layout == "csr":
        d = 1000
        c = csr_case(d, "f32", K)
        data = csr_data(pkg, c)
    else:
        d = 100
        c = dense_case(d, "f64", K, dense_sizes(pkg, d, "f64"))
        data = dense_data(pkg, c)
        if layout == "general":
            monkeypatch.setenv("PSGD_GRAD_MN_TWO_PASS", "1")
        assert plan(pkg, "dense", "f64", d, K)["path"] == layout
    rows, ys = sampled(list(c["rows"]), c["y"], c["offs"], fraction, iteration)
    t = truth_of(rows, ys, c["w"], K, d)
    engine = pkg.HipEngine(data)
    got = engine.gradient_sum_multinomial(K, c["w"], fraction, iteration).cpu().numpy()
    check_sums(got, t, f"sampled {layout} f={fraction} i={iteration}")
    if t.count == 0:
        assert got.tolist() == [0.0] * ((K - 1) * d + 2)      # an all-empty batch: zeros and PSGD_OK
    assert engine.ctx.gradient_sum_multinomial(K, c["w"], 0.0, iteration).tolist() == [0.0] * ((K - 1) * d + 2)


# ---- the per-row math -----------------------------------------------------------------------------
@pytest.mark.parametrize("two_pass", [False, True])
def test_labels_that_are_no_class(pkg, two_pass, monkeypatch):
    """Labels 0, K - 1 and K, -1, 2.5 (no indicator, and no error) in one partition."""
    if two_pass:
        monkeypatch.setenv("PSGD_GRAD_MN_TWO_PASS", "1")
    K = 4
    labels = (0.0, float(K - 1), float(K), -1.0, 2.5, 1.0, 2.0)
    engine, c, t, got = run_dense(pkg, 7, "f64", K, (150,), labels=labels)
    assert set(c["y"]) == set(labels)


@pytest.mark.parametrize("layout", ["fused", "general", "csr"])
def test_all_zero_weights(pkg, layout, monkeypatch):
    """Every mult_c = 1 / K - indicator; lossSum = n log(K)."""
    K = 4
    if layout == "csr":
        d = 1000
        c = csr_case(d, "f64", K)
        data, rows = csr_data(pkg, c), c["rows"]
    else:
        d = 12
        c = dense_case(d, "f64", K, (0, 1, 65, 257))
        data, rows = dense_data(pkg, c), c["rows"]
        if layout == "general":
            monkeypatch.setenv("PSGD_GRAD_MN_TWO_PASS", "1")
    w = np.zeros((K - 1) * d)
    t = truth_of(rows, c["y"], w, K, d)
    ind = (c["y"][:, None] == np.arange(1, K)[None, :]).astype(np.float64)
    assert np.array_equal(t.mult, 1.0 / K - ind)
    got = pkg.HipEngine(data).gradient_sum_multinomial(K, w).cpu().numpy()
    check_sums(got, t, f"zero weights {layout}")
    n = len(c["y"])
    assert abs(got[-2] - n * math.log(K)) <= 1e-12 * n * math.log(K)


@pytest.mark.parametrize("two_pass", [False, True])
def test_margins_past_745(pkg, two_pass, monkeypatch):
    """Margins of +-800 and +-1000: the shift keeps every output finite."""
    if two_pass:
        monkeypatch.setenv("PSGD_GRAD_MN_TWO_PASS", "1")
    K, d = 4, 2
    w = np.array([1.0, 0.0, 0.5, 0.0, -1.0, 0.0])      # margins of x = (t, 0): t, t / 2, -t
    ts = [800.0, -800.0, 1000.0, -1000.0, 3.0, -3.0, 0.0, 746.0, -746.0]
    X = np.array([[ts[k % len(ts)], float(k % 3) - 1.0] for k in range(90)])
    y = np.array([float(k % K) for k in range(90)])
    t = truth_of(X, y, w, K, d)
    assert np.isfinite(t.G).all() and math.isfinite(t.lossSum)
    engine = pkg.HipEngine(pkg.PartitionedData([pkg.DensePartition(y, X)]))
    got = engine.gradient_sum_multinomial(K, w).cpu().numpy()
    assert np.isfinite(got).all()
    check_sums(got, t, f"margins past 745 two_pass={two_pass}")
    score = engine.evaluate_multinomial(K, w)
    assert abs(score.lossSum - got[-2]) <= 1e-12 * abs(score.lossSum) and score.count == got[-1]


@pytest.mark.parametrize("layout", ["fused", "general", "csr"])
def test_consistent_with_scoring(pkg, layout, monkeypatch):
    """lossSum and count are evaluate_multinomial's on the same rows and weights."""
    K = 6
    if layout == "csr":
        c = csr_case(1000, "f32", K)
        data = csr_data(pkg, c)
    else:
        c = dense_case(100, "f32", K, dense_sizes(pkg, 100, "f32"))
        data = dense_data(pkg, c)
        if layout == "general":
            monkeypatch.setenv("PSGD_GRAD_MN_TWO_PASS", "1")
    engine = pkg.HipEngine(data)
    got = engine.gradient_sum_multinomial(K, c["w"]).cpu().numpy()
    score = engine.evaluate_multinomial(K, c["w"])
    assert score.count == got[-1]
    assert abs(score.lossSum - got[-2]) <= 1e-12 * abs(score.lossSum), (score.lossSum, got[-2])


def test_gradient_is_the_slope_of_the_scored_loss(pkg):
    """(loss(w + h e) - loss(w - h e)) / 2h from evaluate_multinomial against the gradient component,
    for the three largest components. h = 1e-4: the truncation error h^2 f''' / 6 and the rounding error
    2^-52 lossSum / h are both below 1e-7 of a component of this size."""
    K, d, n = 3, 5, 300
    c = dense_case(d, "f64", K, (n,))
    engine = pkg.HipEngine(dense_data(pkg, c))
    G = engine.gradient_sum_multinomial(K, c["w"]).cpu().numpy()[:-2]
    h = 1e-4
    for k in np.argsort(-np.abs(G))[:3]:
        e = np.zeros_like(c["w"])
        e[k] = h
        slope = (engine.evaluate_multinomial(K, c["w"] + e).lossSum
                 - engine.evaluate_multinomial(K, c["w"] - e).lossSum) / (2 * h)
        print(f"component {k}: gradient {G[k]:.12g}, slope {slope:.12g}")
        assert abs(slope - G[k]) <= 1e-6 * abs(G[k])


# ---- GradientDescent ------------------------------------------------------------------------------
def run_minibatch_ref(rows, ys, offs, K, upd, step, iters, reg, fraction, w0, tol):
    """MLlib 1.6.1 GradientDescent.runMiniBatchSGD with the truth module's batch sums and the oracle's
    updater -> (weights, history, the isConverged ratios of the tested iterations)."""
    n = len(w0)
    d = n // (K - 1)
    w = [float(v) for v in w0]
    hist, ratios = [], []
    reg_val = R.updater(upd, list(w), ("dense", [0.0] * n), 0.0, 1, reg, R.UpdaterState())
    prev = cur = None
    converged = False
    i = 1
    while not converged and i <= iters:
        brows, bys = sampled(rows, ys, offs, fraction, i)
        t = GT.gradient(brows, bys, np.array(w), K, d)
        if t.count > 0:
            hist.append(t.lossSum / t.count + reg_val)
            w = list(w)
            reg_val = R.updater(upd, w, ("dense", [float(v) for v in t.G.ravel() / float(t.count)]), step, i, reg,
                                R.UpdaterState())
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
def small_case(layout, K):
    rng = np.random.default_rng(616 + K)
    sizes = (0, 1, 65, 150)
    n, d = sum(sizes), 12
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(int)
    W = rng.standard_normal((K, d))
    if layout == "dense":
        X = rng.standard_normal((n, d))
        y = np.argmax(X @ W.T + 0.3 * rng.standard_normal((n, K)), axis=1).astype(np.float64)
        return {"X": X, "rows": list(X), "y": y, "offs": offs, "d": d, "K": K, "dtype": np.float64}
    rows, ys = [], []
    for k in range(n):
        m = (0, 3, 12, 5)[k % 4]
        idx = np.sort(rng.choice(d, size=m, replace=False)).astype(np.int64).tolist()
        val = [float(v) for v in rng.standard_normal(m)]
        rows.append((idx, val))
        ys.append(float(np.argmax(W[:, idx] @ np.array(val))) if m else 0.0)
    return {"rows": rows, "y": np.array(ys), "offs": offs, "d": d, "K": K, "dtype": np.float64}


def small_data(pkg, layout, K):
    c = small_case(layout, K)
    return dense_data(pkg, c) if layout == "dense" else csr_data(pkg, c)


@pytest.mark.parametrize("uname", list(UPDS))
@pytest.mark.parametrize("K", [3, 4])
def test_gradient_descent_matches_mllib_loop(pkg, K, uname):
    for layout in ("dense", "csr"):
        c = small_case(layout, K)
        data = small_data(pkg, layout, K)
        w0 = np.linspace(-0.2, 0.2, (K - 1) * c["d"])
        for fraction in (1.0, 0.5):
            w_ref, h_ref, _ = run_minibatch_ref(c["rows"], c["y"], c["offs"], K, UPDS[uname], 0.5, 5, 0.05, fraction,
                                                w0, 0.0)
            w, h = pkg.GradientDescent.runMiniBatchSGDMultinomial(data, pkg.LogisticGradient(K),
                                                                  updater_of(pkg, uname), 0.5, 5, 0.05, fraction, w0, 0.0)
            what = f"{layout} K={K} {uname} f={fraction}"
            assert len(h_ref) == 5
            assert_close(h, h_ref, what + " history")
            assert_close(w, w_ref, what + " weights")


def test_gradient_descent_converges_early(pkg):
    """convergenceTol stops the loop at the restatement's iteration (its ratios are not near the tolerance)."""
    K = 3
    c = small_case("dense", K)
    w0 = np.zeros((K - 1) * c["d"])
    tol = 0.05
    w_ref, h_ref, ratios = run_minibatch_ref(c["rows"], c["y"], c["offs"], K, UPDS["l2"], 1.0, 40, 0.1, 1.0, w0, tol)
    assert 2 <= len(h_ref) < 40
    assert all(abs(r - tol) > 1e-6 * tol for r in ratios) and ratios[-1] < tol
    gd = pkg.GradientDescent(pkg.LogisticGradient(K), pkg.SquaredL2SGDUpdater()).setNumIterations(40) \
        .setRegParam(0.1).setConvergenceTol(tol)
    data = small_data(pkg, "dense", K)
    w, h = pkg.GradientDescent.runMiniBatchSGDMultinomial(data, gd.gradient, gd.updater, gd.stepSize, gd.numIterations,
                                                          gd.regParam, gd.miniBatchFraction, w0, gd.convergenceTol)
    assert len(h) == len(h_ref)
    assert_close(h, h_ref, "early stop history")
    assert_close(w, w_ref, "early stop weights")
    assert_close(gd.optimize(data, w0), w_ref, "optimize")
    # ||gradient_sum / count + reg w|| at the result: the optimizer's own check
    gs = pkg.gradient_sum_multinomial(data, gd.gradient, w)
    t = GT.gradient(c["rows"], c["y"], w, K, c["d"])
    check_sums(np.concatenate([gs.gradient, [gs.lossSum, gs.count]]), t, "gradient_sum_multinomial at the result")


# ---- isolation, errors ----------------------------------------------------------------------------
@pytest.mark.parametrize("fraction", [1.0, 0.5])
def test_epoch_state_is_left_alone(pkg, fraction):
    K = 3
    c = small_case("dense", K)
    n = (K - 1) * c["d"]
    w0 = np.linspace(-0.2, 0.2, n)
    g, u = pkg.LogisticGradient(K), pkg.SquaredL2SGDUpdater()
    data_a, data_b = small_data(pkg, "dense", K), small_data(pkg, "dense", K)
    plain = pkg.HipEngine(data_a, weight_dim=n)
    w_a, h_a = pkg.runParallelizedSGD(data_a, g, u, 1.0, 3, 0.01, fraction, w0, 0.0, engine=plain)
    before = (plain.ctx.last_kernel(), plain.ctx.chain_launches())
    plain.gradient_sum_multinomial(K, w0, fraction, 1)
    plain.gradient_sum_multinomial(K, w0, 1.0, 1)
    plain.ctx.gradient_sum_multinomial(K, w0, fraction, 2)
    assert (plain.ctx.last_kernel(), plain.ctx.chain_launches()) == before
    # a gradient_sum_multinomial between an engine's setup and its epochs changes none of their bits
    mixed = pkg.HipEngine(data_b, weight_dim=n)
    mixed.gradient_sum_multinomial(K, w0, fraction, 1)
    w_b, h_b = pkg.runParallelizedSGD(data_b, g, u, 1.0, 3, 0.01, fraction, w0, 0.0, engine=mixed)
    assert w_a.tobytes() == w_b.tobytes() and h_a.tobytes() == h_b.tobytes()


def test_errors(pkg):
    K = 3
    c = dense_case(3, "f64", K, SMALL)
    engine = pkg.HipEngine(dense_data(pkg, c))
    L, ctx, N = pkg._native.lib(), engine.ctx, pkg._native
    w, out = np.zeros(6), np.zeros(8)
    call = L.psgd_gradient_sum_multinomial
    for bad_k in (2, 1, 0, -1):
        assert call(ctx.handle, bad_k, w.ctypes.data, 1.0, 1, out.ctypes.data) == N.PSGD_EINVAL
    assert call(ctx.handle, 4098, w.ctypes.data, 1.0, 1, out.ctypes.data) == N.PSGD_EUNSUPPORTED
    assert call(ctx.handle, K, None, 1.0, 1, out.ctypes.data) == N.PSGD_EINVAL
    assert call(ctx.handle, K, w.ctypes.data, 1.0, 1, None) == N.PSGD_EINVAL
    assert L.psgd_gradient_sum_multinomial_device(ctx.handle, K, None, 1.0, 1, None, None) == N.PSGD_EINVAL
    for f in (-0.1, 1.5, float("nan")):
        assert call(ctx.handle, K, w.ctypes.data, f, 1, out.ctypes.data) == N.PSGD_EINVAL
        assert b"Sampling fraction" in L.psgd_last_error()
    with pytest.raises(pkg.IllegalArgumentException, match="^requirement failed$"):
        engine.gradient_sum_multinomial(K, np.zeros(5))
    with pytest.raises(pkg.IllegalArgumentException, match="numClasses > 2"):
        engine.gradient_sum_multinomial(2, np.zeros(3))
    with pytest.raises(pkg.UnsupportedOperationException, match="gradient_sum_multinomial"):
        engine.gradient_sum(pkg.LogisticGradient(K), w)
    ctx.clear()
    ctx.registered_token = None
    assert call(ctx.handle, K, w.ctypes.data, 1.0, 1, out.ctypes.data) == N.PSGD_ESTATE


# ---- world size 2 ---------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.parametrize("P", [5, 1])
def test_two_ranks(tmp_path, pkg, P):
    """Two ranks sharing cuda:0 over gloo, each a fresh child process (tests/two_rank_gradient_mn.py):
    both hold identical gradient_sum_multinomial bits and identical GradientDescent weights; the sums
    are the truth's within the bar, the weights the one-rank run's; with P = 1 rank 1 holds no partition."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import two_rank_gradient_mn as T
    out = str(tmp_path / "res.json")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), PSGD_TEST_P=str(P))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "two_rank_gradient_mn.py"), out], env=env,
                       capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    with open(out) as f:
        res = json.load(f)
    assert len(res) == 2 and res["0"] == res["1"]          # floats survive JSON exactly: identical bits
    X, y, w = T.make_data()
    t = truth_of(X, y, w, T.K, X.shape[1])
    check_sums(np.array(res["0"]["sum"]), t, f"two ranks P={P}")
    data = pkg.PartitionedData.parallelize(y, X, P)
    w1, h1 = pkg.GradientDescent.runMiniBatchSGDMultinomial(data, pkg.LogisticGradient(T.K), pkg.SquaredL2SGDUpdater(),
                                                            *T.GD_ARGS, w, 0.0)
    assert_close(res["0"]["weights"], w1, "two-rank weights")
    assert_close(res["0"]["history"], h1, "two-rank history")
