"""psgd_gramian on the GPU: the augmented Gramian M = sum z z^T, z = [x, y, 1], from the fp64 MFMA
kernel over dense rows and the atomic kernel over CSR rows, against numpy's float64 Z^T Z.

Bars: |M_jk - truth_jk| <= 1e-9 A_jk for every entry (A = |Z|^T |Z|, the project's fp64 bar on the
sum of magnitudes), M == M^T exactly, the count exact. Whole-number data (-3 .. 3) makes every product
and sum exact in fp64 in any order, so there M equals the int64 truth bit for bit: a row or column
counted twice or not at all cannot hide behind a relative bar.

Shapes: d = 1, 13, 14, 15, 30 give a = 3, 15, exactly 16, 17 and two full blocks; 46 and 70 are the
2 x 4 rectangle with one and two group columns; 130 (nine blocks) first exceeds 2 x 4 and takes 4 x 8
with several groups both ways, 300 more of them. Partitions of 1, 3, 4, 5, 65 and tile + 37 rows with
an empty one in the middle: every remainder of the 4-row step and the 8-row stage, one tile boundary."""
import functools
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, has_gpu

import gram_truth as GT

pytestmark = pytest.mark.gpu

TILE = {"f32": 1024, "f64": 512}
DENSE_D = (1, 13, 14, 15, 30, 46, 70, 130, 300)


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not has_gpu():
        pytest.skip("no GPU")


def np_dtype(storage):
    return np.float32 if storage == "f32" else np.float64


def sizes_of(storage):
    return (1, 3, 0, 4, 5, 65, TILE[storage] + 37)


@functools.lru_cache(maxsize=None)
def dense_case(d, storage, whole=False):
    sizes = sizes_of(storage)
    rng = np.random.default_rng(7300 + d + (9 if storage == "f32" else 0) + (100000 if whole else 0))
    n = sum(sizes)
    if whole:
        X = rng.integers(-3, 4, size=(n, d)).astype(np_dtype(storage))
        y = rng.integers(-3, 4, size=n).astype(np.float64)
    else:
        X = (rng.standard_normal((n, d)) * rng.uniform(0.5, 2.0, size=d) + rng.uniform(-1.0, 1.0, size=d)).astype(np_dtype(storage))
        X[rng.random((n, d)) < 0.05] = 0.0
        y = rng.standard_normal(n) + 0.5
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(int)
    T, A = GT.gram_truth(X, y)
    return {"X": X, "y": y, "offs": offs, "d": d, "T": T, "A": A}


def dense_data(pkg, c):
    return pkg.PartitionedData([pkg.DensePartition(np.ascontiguousarray(c["y"][a:b]), np.ascontiguousarray(c["X"][a:b]))
                                for a, b in zip(c["offs"][:-1], c["offs"][1:])])


def matrix_of(engine, d):
    return engine.gramian().cpu().numpy().reshape(d + 2, d + 2)


@pytest.mark.parametrize("storage", ["f32", "f64"])
@pytest.mark.parametrize("d", DENSE_D)
def test_dense(pkg, d, storage):
    c = dense_case(d, storage)
    engine = pkg.HipEngine(dense_data(pkg, c))
    M = matrix_of(engine, d)
    GT.check_gramian(M, c["T"], c["A"], f"dense d={d} {storage}")
    again = matrix_of(engine, d)
    assert M.tobytes() == again.tobytes()          # no atomics: the same bits from call to call
    raw = engine.ctx.gramian(d)                    # the host-pointer form gives the same bits
    assert raw.tobytes() == M.tobytes()


@pytest.mark.parametrize("storage", ["f32", "f64"])
@pytest.mark.parametrize("d", DENSE_D)
def test_dense_whole_numbers_are_exact(pkg, d, storage):
    c = dense_case(d, storage, True)
    M = matrix_of(pkg.HipEngine(dense_data(pkg, c)), d)
    Ti = GT.gram_truth_int(c["X"], c["y"])
    assert (M == Ti).all(), f"{int((M != Ti).sum())} entries differ, first at {tuple(np.argwhere(M != Ti)[0])}"


def test_dense_more_than_two_spans(pkg):
    """Enough tiles that a span is several tiles long (read from the plan): whole-number rows in two
    partitions, more than two spans + 3 of them, bit for bit."""
    d, storage = 1, "f32"
    tile = TILE[storage]
    sizes = (4500 * tile + 5, 4600 * tile - 2)
    tiles = sum(-(-s // tile) for s in sizes)
    plan = pkg._native.gramian_plan("dense", storage, d, tiles)
    assert plan["span_tiles"] >= 2 and plan["spans"] > 2
    n = sum(sizes)
    assert n > 2 * plan["span_tiles"] * plan["tile_rows"] + 3
    rng = np.random.default_rng(31)
    X = rng.integers(-3, 4, size=(n, d)).astype(np.float32)
    y = rng.integers(-3, 4, size=n).astype(np.float64)
    parts = [pkg.DensePartition(y[:sizes[0]], X[:sizes[0]]), pkg.DensePartition(y[sizes[0]:], X[sizes[0]:])]
    M = matrix_of(pkg.HipEngine(pkg.PartitionedData(parts)), d)
    assert (M == GT.gram_truth_int(X, y)).all()


@pytest.mark.parametrize("d,storage,ld", [(13, "f32", 16), (30, "f64", 32), (101, "f32", 104), (130, "f32", 136)])
def test_dense_zero_copy_pitch(pkg, d, storage, ld):
    """psgd_register_dense_device rows with ld > d: the pad belongs to the caller (NaN here) and must
    not reach an MFMA, not even against a zero."""
    import torch
    c = dense_case(d, storage) if d in DENSE_D else None
    if c is None:
        rng = np.random.default_rng(d)
        sizes = sizes_of(storage)
        X = rng.standard_normal((sum(sizes), d)).astype(np_dtype(storage))
        y = rng.standard_normal(sum(sizes))
        T, A = GT.gram_truth(X, y)
        c = {"X": X, "y": y, "offs": np.concatenate([[0], np.cumsum(sizes)]).astype(int), "T": T, "A": A}
    dev = torch.device("cuda", 0)
    tdt = torch.float32 if storage == "f32" else torch.float64
    parts = []
    for a, b in zip(c["offs"][:-1], c["offs"][1:]):
        X = torch.full((b - a, ld), float("nan"), dtype=tdt, device=dev)
        X[:, :d] = torch.from_numpy(np.array(c["X"][a:b])).to(dev)
        parts.append(pkg.DevicePartition(torch.from_numpy(np.array(c["y"][a:b])).to(dev), X, d))
    M = matrix_of(pkg.HipEngine(pkg.PartitionedData(parts)), d)
    assert not np.isnan(M).any()
    GT.check_gramian(M, c["T"], c["A"], f"zero-copy d={d} ld={ld}")


@pytest.mark.parametrize("layout", ["dense", "csr"])
def test_registry_of_empty_partitions(pkg, layout):
    if layout == "dense":
        part = pkg.DensePartition(np.zeros(0), np.zeros((0, 5), dtype=np.float32))
    else:
        part = pkg.CsrPartition(np.zeros(0), np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0), 5)
    engine = pkg.HipEngine(pkg.PartitionedData([part, part]))
    assert (engine.ctx.gramian(5) == 0.0).all()
    assert (matrix_of(engine, 5) == 0.0).all()


def test_errors(pkg):
    import ctypes
    N = pkg._native
    c = dense_case(13, "f32")
    engine = pkg.HipEngine(dense_data(pkg, c))
    engine.gramian()
    L, h = N.lib(), engine.ctx.handle
    assert L.psgd_gramian(h, None) == N.PSGD_EINVAL
    assert L.psgd_gramian_device(h, None, None) == N.PSGD_EINVAL
    fresh = ctypes.c_void_p()
    assert L.psgd_ctx_create(0, ctypes.byref(fresh)) == 0
    try:
        buf = np.zeros(9)
        assert L.psgd_gramian(fresh, buf.ctypes.data) == N.PSGD_ESTATE
    finally:
        L.psgd_ctx_destroy(fresh)


# ---- CSR ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def csr_case(d, storage, whole=False):
    """Ragged rows of 0, 1, 2, 17 and d entries (capped at d), one explicitly stored 0.0 per six rows."""
    dt = np_dtype(storage)
    rng = np.random.default_rng(8800 + d + (3 if storage == "f32" else 0) + (100000 if whole else 0))
    sizes = (1, 3, 0, 4, 5, 65, 512 + 37)
    lengths = (0, 1, 2, 17, d, 2)
    rows = []
    for k in range(sum(sizes)):
        m = min(lengths[k % len(lengths)], d)
        idx = np.sort(rng.choice(d, size=m, replace=False)).astype(np.int64)
        if whole:
            val = rng.integers(-3, 4, size=m).astype(dt)
        else:
            val = (rng.standard_normal(m) + 0.25).astype(dt)
        if k % len(lengths) == 5 and m:
            val[0] = 0.0                         # stored, and zero
        rows.append((idx.tolist(), val))
    n = len(rows)
    y = rng.integers(-3, 4, size=n).astype(np.float64) if whole else rng.standard_normal(n) + 0.5
    X = GT.csr_to_dense(rows, d, dt)
    T, A = GT.gram_truth(X, y)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(int)
    return {"rows": rows, "X": X, "y": y, "offs": offs, "d": d, "dtype": dt, "T": T, "A": A}


def csr_data(pkg, c):
    parts = []
    for a, b in zip(c["offs"][:-1], c["offs"][1:]):
        rows = c["rows"][a:b]
        ptr = np.zeros(b - a + 1, dtype=np.int64)
        for k, r in enumerate(rows):
            ptr[k + 1] = ptr[k] + len(r[0])
        col = np.array([i for r in rows for i in r[0]], dtype=np.int32)
        val = np.array([v for r in rows for v in r[1]], dtype=c["dtype"])
        parts.append(pkg.CsrPartition(np.ascontiguousarray(c["y"][a:b]), ptr, col, val, c["d"]))
    return pkg.PartitionedData(parts)


@pytest.mark.parametrize("storage", ["f32", "f64"])
@pytest.mark.parametrize("d", [1, 13, 14, 15, 30, 130, 300])
def test_csr(pkg, d, storage):
    c = csr_case(d, storage)
    engine = pkg.HipEngine(csr_data(pkg, c))
    M = matrix_of(engine, d)
    GT.check_gramian(M, c["T"], c["A"], f"csr d={d} {storage}")
    again = matrix_of(engine, d)
    GT.check_gramian(again, c["T"], c["A"], f"csr d={d} {storage}, second call")
    # y^T y, sum y and the count are per-tile sums merged in tile order: the same bits
    assert M[d:, d:].tobytes() == again[d:, d:].tobytes()
    raw = engine.ctx.gramian(d)
    assert raw[d:, d:].tobytes() == M[d:, d:].tobytes()


@pytest.mark.parametrize("storage", ["f32", "f64"])
@pytest.mark.parametrize("d", [1, 15, 30, 300])
def test_csr_whole_numbers_are_exact(pkg, d, storage):
    c = csr_case(d, storage, True)
    M = matrix_of(pkg.HipEngine(csr_data(pkg, c)), d)
    Ti = GT.gram_truth_int(c["X"], c["y"])
    assert (M == Ti).all(), f"{int((M != Ti).sum())} entries differ, first at {tuple(np.argwhere(M != Ti)[0])}"


# ---- two independent kernels against each other -------------------------------------------------------
@pytest.mark.parametrize("layout,d,storage", [("dense", 30, "f32"), ("dense", 130, "f64"), ("csr", 30, "f32")])
def test_gradient_sum_agrees_with_the_gramian(pkg, layout, d, storage):
    """gradient_sum(LeastSquaresGradient, w) at an arbitrary w is G w - X^T y, its lossSum
    (w^T G w - 2 w^T X^T y + y^T y) / 2; at w* = normal_equations(data, lambda) the regularised mean
    gradient vanishes. Each bar is the sum of the two sides' bars."""
    c = dense_case(d, storage) if layout == "dense" else csr_case(d, storage)
    data = dense_data(pkg, c) if layout == "dense" else csr_data(pkg, c)
    engine = pkg.HipEngine(data)
    g = pkg.gramian(data, engine=engine)
    X = np.asarray(c["X"], dtype=np.float64)
    y, n = c["y"], X.shape[0]
    assert g.count == n
    G_abs, xty_abs = np.abs(c["T"][:d, :d]), np.abs(c["T"][:d, d])

    def bar(w):
        diff = X @ w - y
        a_grad = np.abs(X * diff[:, None]).sum(axis=0)
        return GT.BAR * (a_grad + G_abs @ np.abs(w) + xty_abs)

    rng = np.random.default_rng(17)
    w = rng.standard_normal(d) / np.sqrt(d)
    gs = pkg.gradient_sum(data, pkg.LeastSquaresGradient(), w, engine=engine)
    want = g.gram @ w - g.xty
    assert (np.abs(gs.gradient - want) <= bar(w)).all()
    loss = (w @ g.gram @ w - 2.0 * (w @ g.xty) + g.yty) / 2.0
    terms = np.abs(w) @ G_abs @ np.abs(w) + 2.0 * np.abs(w) @ xty_abs + c["T"][d, d]
    assert abs(gs.lossSum - loss) <= GT.BAR * terms
    assert gs.count == n
    lam = 0.05
    ws = pkg.normal_equations(data, lam, engine=engine)
    at = pkg.gradient_sum(data, pkg.LeastSquaresGradient(), ws, engine=engine)
    assert (np.abs(at.gradient / n + lam * ws) <= bar(ws) / n).all()


@pytest.mark.parametrize("layout,d,storage", [("dense", 30, "f32"), ("dense", 70, "f64"), ("csr", 15, "f64")])
def test_covariance_and_corr_end_to_end(pkg, layout, d, storage):
    c = dense_case(d, storage) if layout == "dense" else csr_case(d, storage)
    data = dense_data(pkg, c) if layout == "dense" else csr_data(pkg, c)
    X = np.asarray(c["X"], dtype=np.float64)
    n = X.shape[0]
    mean = X.mean(axis=0)
    bar = GT.BAR * (c["A"][:d, :d] / (n - 1) + n / (n - 1) * np.abs(np.outer(mean, mean)))
    want = np.cov(X, rowvar=False).reshape(d, d)
    cov = pkg.covariance(data)
    assert (np.abs(cov - want) <= bar).all()
    sigma = np.sqrt(np.diag(want))
    assert (sigma > 1e-3).all()
    cor = pkg.corr(data)
    ss = np.outer(sigma, sigma)
    err = np.abs(cor - np.corrcoef(X, rowvar=False).reshape(d, d))
    print(f"corr {layout} d={d}: worst error / bar = {(err / (bar / ss)).max():.3g}")
    assert (err <= bar / ss).all()
    assert (np.diag(cor) == 1.0).all()


# ---- world size 2 -------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.parametrize("P", [5, 1])
def test_two_ranks(tmp_path, pkg, P):
    """Two ranks sharing cuda:0 over gloo, each a fresh child process (tests/two_rank_gram.py): both
    hold identical bits, the truth within the bar; with P = 1 rank 1 holds no partition."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import two_rank_gram as T
    out = str(tmp_path / "res.json")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), PSGD_TEST_P=str(P))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "two_rank_gram.py"), out], env=env,
                       capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    with open(out) as f:
        res = json.load(f)
    assert len(res) == 2 and res["0"] == res["1"]          # floats survive JSON exactly: identical bits
    X, y = T.make_data()
    a = X.shape[1] + 2
    truth, A = GT.gram_truth(X, y)
    GT.check_gramian(np.array(res["0"]["matrix"]).reshape(a, a), truth, A, f"two ranks P={P}")
