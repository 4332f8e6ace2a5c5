"""The second-order passes on the GPU: psgd_row_curvature, the row-weighted Gramian (fp64 MFMA over
dense rows, atomics over CSR rows), hessian_sum and Newton's method over them, against the numpy truth
of tests/hessian_truth.py.

Bars: a curvature within 1e-9 of its truth (relative: the project's fp64 bar); every entry of M_w within
1e-9 A_w (A_w = |Z|^T diag|omega| |Z|), M_w == M_w^T exactly, the same bytes from call to call and from
the host-pointer form on dense rows; omega == 1.0 returns psgd_gramian's bytes; whole-number rows with
omega in {0, 0.5, 1, 2, 4} make every product and partial sum exact in any order, so 2 M_w equals the
int64 truth bit for bit. Newton: the weights within 1e-9 max(|w|, 1) of the numpy run, the numpy
gradient at them of norm <= 1e-10, the loss history within 1e-9 (relative) while the truth's ||g|| > 1e-6.

Partitions are test_gpu_gram's: 1, 3, 0, 4, 5, 65 and tile + 37 rows."""
import ctypes
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, has_gpu

import gram_truth as GT
import hessian_truth as HT
from test_gpu_gram import _free_port, csr_case, csr_data, dense_case, dense_data, np_dtype, sizes_of

pytestmark = pytest.mark.gpu

BAR = 1e-9
WEIGHTED_D = (1, 14, 15, 30, 70, 130)     # a = 3, 16, 17, two blocks, the 2 x 4 and the 4 x 8 rectangle


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not has_gpu():
        pytest.skip("no GPU")


def curvature_of(engine, gradient, w):
    return engine.row_curvature(gradient, w).cpu().numpy()


def weighted_of(engine, d, om):
    return engine.gramian(weights=engine.device_rows(om)).cpu().numpy().reshape(d + 2, d + 2)


@functools.lru_cache(maxsize=None)
def omega_of(n, seed, whole=False):
    """Finite weights in (0, 2] with 5 % zeros and a few negative ones; whole: {0, 0.5, 1, 2, 4}."""
    rng = np.random.default_rng(seed)
    if whole:
        om = rng.choice([0.0, 0.5, 1.0, 2.0, 4.0], size=n)
    else:
        om = 2.0 - rng.uniform(0.0, 2.0, size=n)
        om[rng.random(n) < 0.05] = 0.0
        om[rng.choice(n, size=min(4, n), replace=False)] *= -0.75
    om.setflags(write=False)
    return om


def check_weighted(M, T, A, what):
    assert M.shape == T.shape and not np.isnan(M).any(), what
    err = np.abs(M - T)
    bad = err > BAR * A
    assert not bad.any(), f"{what}: {int(bad.sum())} entries off, first at {tuple(np.argwhere(bad)[0])}, worst {err.max():.3g}"
    assert (M == M.T).all(), f"{what}: not symmetric"


# ---- curvature ----------------------------------------------------------------------------------------
def check_curvature(h, X, w, what):
    want = HT.curvature(X, w, "logistic")
    assert h.shape == want.shape, what
    err = np.abs(h - want)
    assert (err <= BAR * want).all(), f"{what}: worst relative error {(err / want).max():.3g}"


@pytest.mark.parametrize("storage", ["f32", "f64"])
@pytest.mark.parametrize("d", [1, 13, 130])
def test_curvature_dense(pkg, d, storage):
    c = dense_case(d, storage)
    engine = pkg.HipEngine(dense_data(pkg, c))
    n = c["X"].shape[0]
    assert engine.local_rows() == n and engine.ctx.local_rows() == n
    w = np.random.default_rng(40 + d).standard_normal(d) / np.sqrt(d)
    h = curvature_of(engine, pkg.LogisticGradient(), w)
    check_curvature(h, c["X"], w, f"dense d={d} {storage}")
    assert h.tobytes() == curvature_of(engine, pkg.LogisticGradient(), w).tobytes()
    assert engine.ctx.row_curvature(0, w).tobytes() == h.tobytes()           # the host-pointer form
    assert (curvature_of(engine, pkg.LogisticGradient(), np.zeros(d)) == 0.25).all()
    assert (curvature_of(engine, pkg.LeastSquaresGradient(), w) == 1.0).all()


@pytest.mark.parametrize("storage", ["f32", "f64"])
@pytest.mark.parametrize("d", [30, 300])
def test_curvature_csr(pkg, d, storage):
    c = csr_case(d, storage)
    engine = pkg.HipEngine(csr_data(pkg, c))
    w = np.random.default_rng(41 + d).standard_normal(d) / np.sqrt(d)
    h = curvature_of(engine, pkg.LogisticGradient(), w)
    check_curvature(h, c["X"], w, f"csr d={d} {storage}")
    empty = np.array([len(r[0]) == 0 for r in c["rows"]])
    assert empty.any() and (h[empty] == 0.25).all()                        # a row without entries: z = 0
    assert (curvature_of(engine, pkg.LogisticGradient(), np.zeros(d)) == 0.25).all()
    assert (curvature_of(engine, pkg.LeastSquaresGradient(), w) == 1.0).all()
    assert engine.ctx.row_curvature(0, w).tobytes() == h.tobytes()


@pytest.mark.parametrize("storage", ["f32", "f64"])
def test_curvature_underflows_to_zero_at_a_margin_of_800(pkg, storage):
    """Tagged rows (800, 0, ..) and (-800, 0, ..) against w = (1, ..): z = +-800 exactly, exp(-800)
    underflows, h == 0.0 and not NaN -- the first row of a partition, the last row of the data, and a
    row in the middle of the long partition."""
    d = 13
    c = dense_case(d, storage)
    X = np.array(c["X"])
    offs = c["offs"]
    tagged = [int(offs[3]), X.shape[0] - 1, int(offs[6]) + 300]
    for k, r in enumerate(tagged):
        X[r] = 0.0
        X[r, 0] = 800.0 if k % 2 == 0 else -800.0
    w = np.random.default_rng(5).standard_normal(d)
    w[0] = 1.0
    X[tagged, 1:] = 0.0
    data = dense_data(pkg, {"X": X, "y": c["y"], "offs": offs})
    h = curvature_of(pkg.HipEngine(data), pkg.LogisticGradient(), w)
    assert (h[tagged] == 0.0).all() and not np.isnan(h).any()
    check_curvature(np.delete(h, tagged), np.delete(X, tagged, axis=0), w, "the other rows")


def device_parts(pkg, c, d, storage, ld):
    import torch
    dev = torch.device("cuda", 0)
    tdt = torch.float32 if storage == "f32" else torch.float64
    parts = []
    for a, b in zip(c["offs"][:-1], c["offs"][1:]):
        X = torch.full((b - a, ld), float("nan"), dtype=tdt, device=dev)
        X[:, :d] = torch.from_numpy(np.array(c["X"][a:b])).to(dev)
        parts.append(pkg.DevicePartition(torch.from_numpy(np.array(c["y"][a:b])).to(dev), X, d))
    return pkg.PartitionedData(parts)


@pytest.mark.parametrize("d,storage,ld", [(13, "f32", 16), (130, "f32", 136)])
def test_zero_copy_pitch(pkg, d, storage, ld):
    """Rows registered in place with ld > d: the pad is the caller's (NaN here) and reaches neither a
    dot nor an MFMA."""
    c = dense_case(d, storage)
    engine = pkg.HipEngine(device_parts(pkg, c, d, storage, ld))
    w = np.random.default_rng(42 + d).standard_normal(d) / np.sqrt(d)
    h = curvature_of(engine, pkg.LogisticGradient(), w)
    assert not np.isnan(h).any()
    check_curvature(h, c["X"], w, f"zero-copy d={d} ld={ld}")
    om = omega_of(c["X"].shape[0], 900 + d)
    M = weighted_of(engine, d, om)
    assert not np.isnan(M).any()
    T, A = HT.weighted_gram(c["X"], c["y"], om)
    check_weighted(M, T, A, f"zero-copy weighted d={d} ld={ld}")


# ---- the weighted Gramian, dense ------------------------------------------------------------------------
@pytest.mark.parametrize("storage", ["f32", "f64"])
@pytest.mark.parametrize("d", WEIGHTED_D)
def test_weighted_dense(pkg, d, storage):
    c = dense_case(d, storage)
    n = c["X"].shape[0]
    engine = pkg.HipEngine(dense_data(pkg, c))
    om = omega_of(n, 600 + d)
    assert (om == 0.0).any() and (om < 0.0).any() and om.max() <= 2.0
    M = weighted_of(engine, d, om)
    T, A = HT.weighted_gram(c["X"], c["y"], om)
    check_weighted(M, T, A, f"weighted dense d={d} {storage}")
    assert M.tobytes() == weighted_of(engine, d, om).tobytes()               # the same bits from call to call
    assert engine.ctx.gramian_weighted(d, om).tobytes() == M.tobytes()       # ... and from the host-pointer form
    # unit weights: the unweighted pass's bytes (one plan, one order; x * 1.0 is x)
    plain = engine.gramian().cpu().numpy().reshape(d + 2, d + 2)
    assert weighted_of(engine, d, np.ones(n)).tobytes() == plain.tobytes()


@pytest.mark.parametrize("storage", ["f32", "f64"])
@pytest.mark.parametrize("d", WEIGHTED_D)
def test_weighted_dense_whole_numbers_are_exact(pkg, d, storage):
    c = dense_case(d, storage, True)
    n = c["X"].shape[0]
    engine = pkg.HipEngine(dense_data(pkg, c))
    om = omega_of(n, 700 + d, True)
    M = weighted_of(engine, d, om)
    T2 = HT.weighted_gram_int2(c["X"], c["y"], om)
    assert (2.0 * M == T2).all(), f"{int((2.0 * M != T2).sum())} entries differ, first at {tuple(np.argwhere(2.0 * M != T2)[0])}"
    # a row of weight 0 is a row that is not there
    keep = np.random.default_rng(d).random(n) < 0.7
    keep[[0, n - 1]] = [False, True]
    M01 = weighted_of(engine, d, keep.astype(np.float64))
    assert (M01 == GT.gram_truth_int(c["X"][keep], c["y"][keep])).all()


# ---- the weighted Gramian, CSR --------------------------------------------------------------------------
@pytest.mark.parametrize("storage", ["f32", "f64"])
@pytest.mark.parametrize("d", [30, 300])
def test_weighted_csr(pkg, d, storage):
    c = csr_case(d, storage)
    n = c["X"].shape[0]
    engine = pkg.HipEngine(csr_data(pkg, c))
    om = omega_of(n, 800 + d)
    T, A = HT.weighted_gram(c["X"], c["y"], om)
    M = weighted_of(engine, d, om)
    check_weighted(M, T, A, f"weighted csr d={d} {storage}")
    again = weighted_of(engine, d, om)
    check_weighted(again, T, A, f"weighted csr d={d} {storage}, second call")
    # sum w y^2, sum w y and sum w are per-tile sums merged in tile order: the same bits
    assert M[d:, d:].tobytes() == again[d:, d:].tobytes()
    assert engine.ctx.gramian_weighted(d, om)[d:, d:].tobytes() == M[d:, d:].tobytes()


@pytest.mark.parametrize("storage", ["f32", "f64"])
@pytest.mark.parametrize("d", [15, 300])
def test_weighted_csr_whole_numbers_are_exact(pkg, d, storage):
    c = csr_case(d, storage, True)
    n = c["X"].shape[0]
    engine = pkg.HipEngine(csr_data(pkg, c))
    om = omega_of(n, 810 + d, True)
    M = weighted_of(engine, d, om)
    T2 = HT.weighted_gram_int2(c["X"], c["y"], om)
    assert (2.0 * M == T2).all(), f"{int((2.0 * M != T2).sum())} entries differ, first at {tuple(np.argwhere(2.0 * M != T2)[0])}"
    keep = np.random.default_rng(d).random(n) < 0.7
    assert (weighted_of(engine, d, keep.astype(np.float64)) == GT.gram_truth_int(c["X"][keep], c["y"][keep])).all()


# ---- errors ---------------------------------------------------------------------------------------------
def test_errors(pkg):
    N = pkg._native
    c = dense_case(13, "f32")
    engine = pkg.HipEngine(dense_data(pkg, c))
    n = c["X"].shape[0]
    L, h = N.lib(), engine.ctx.handle
    w, om, out, big = np.zeros(13), np.ones(n), np.zeros(n), np.zeros(15 * 15)
    rows = ctypes.c_int64()
    assert L.psgd_local_rows(h, ctypes.byref(rows)) == 0 and rows.value == n
    assert L.psgd_local_rows(h, None) == N.PSGD_EINVAL and L.psgd_local_rows(None, ctypes.byref(rows)) == N.PSGD_EINVAL
    assert L.psgd_row_curvature(h, 0, None, out.ctypes.data) == N.PSGD_EINVAL
    assert L.psgd_row_curvature(h, 0, w.ctypes.data, None) == N.PSGD_EINVAL
    assert L.psgd_row_curvature_device(h, 0, None, None, None) == N.PSGD_EINVAL
    assert L.psgd_row_curvature(h, 2, w.ctypes.data, out.ctypes.data) == N.PSGD_EUNSUPPORTED      # Hinge
    assert L.psgd_row_curvature(h, 7, w.ctypes.data, out.ctypes.data) == N.PSGD_EINVAL
    assert L.psgd_gramian_weighted(h, None, big.ctypes.data) == N.PSGD_EINVAL
    assert L.psgd_gramian_weighted(h, om.ctypes.data, None) == N.PSGD_EINVAL
    assert L.psgd_gramian_weighted_device(h, None, None, None) == N.PSGD_EINVAL
    with pytest.raises(pkg.UnsupportedOperationException):
        engine.row_curvature(pkg.HingeGradient(), w)
    with pytest.raises(pkg.UnsupportedOperationException):
        engine.row_curvature(pkg.LogisticGradient(3), w)
    with pytest.raises(pkg.IllegalArgumentException):
        engine.gramian(weights=engine.device_rows(om[:-1]))
    fresh = ctypes.c_void_p()
    assert L.psgd_ctx_create(0, ctypes.byref(fresh)) == 0
    try:
        assert L.psgd_row_curvature(fresh, 0, w.ctypes.data, out.ctypes.data) == N.PSGD_ESTATE
        assert L.psgd_gramian_weighted(fresh, om.ctypes.data, big.ctypes.data) == N.PSGD_ESTATE
        assert L.psgd_local_rows(fresh, ctypes.byref(rows)) == 0 and rows.value == 0
    finally:
        L.psgd_ctx_destroy(fresh)


@pytest.mark.parametrize("layout", ["dense", "csr"])
def test_registry_of_empty_partitions(pkg, layout):
    if layout == "dense":
        part = pkg.DensePartition(np.zeros(0), np.zeros((0, 5), dtype=np.float32))
    else:
        part = pkg.CsrPartition(np.zeros(0), np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0), 5)
    engine = pkg.HipEngine(pkg.PartitionedData([part, part]))
    assert engine.local_rows() == 0
    assert curvature_of(engine, pkg.LogisticGradient(), np.ones(5)).shape == (0,)
    assert (weighted_of(engine, 5, np.zeros(0)) == 0.0).all()
    assert (engine.ctx.gramian_weighted(5, np.zeros(0)) == 0.0).all()


# ---- hessian_sum and Newton end to end ----------------------------------------------------------------------
NEWTON_CASES = ((13, 0.1, 0.0), (30, 0.01, 5.0), (130, 0.1, 3.0))     # d, regParam, every initial weight


@functools.lru_cache(maxsize=None)
def newton_case(d, lam, start):
    """Rows stretched by 2 so that a start away from the optimum backtracks; f64 storage. The numpy run
    is the reference: computed once."""
    sizes = sizes_of("f64")
    X, y = HT.planted_logistic(sum(sizes), d, 5000 + d, stretch=2.0)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(int)
    truth = HT.newton(X, y, np.full(d, start), lam, num_iterations=25)
    return {"X": X, "y": y, "offs": offs, "d": d, "truth": truth}


@pytest.mark.parametrize("d,lam,start", NEWTON_CASES)
def test_newton_logistic(pkg, d, lam, start):
    c = newton_case(d, lam, start)
    X, y, truth = c["X"], c["y"], c["truth"]
    n = X.shape[0]
    # conditions on the inputs, asserted on the truth itself
    halvings = sum(truth["halvings"])
    print(f"truth d={d}: halvings {truth['halvings']}, ||g|| {['%.1e' % g for g in truth['gnorm']]}")
    if start == 0.0:
        assert halvings == 0
    else:
        assert halvings >= 3
    live = [k for k, g in enumerate(truth["gnorm"]) if g > 1e-6]
    assert min(m for k in live for m in truth["margins"][k]) > 1e-6     # no Armijo decision near its flip
    # the last iteration starts below the bar on ||g|| checked further down: whatever its line search
    # makes of differences below f's rounding, a step t in [0, 1] along the Newton direction leaves ||g||
    # there
    assert truth["gnorm"][-1] <= 1e-10 and len(truth["history"]) < 25
    data = dense_data(pkg, c)
    w, hist = pkg.runNewton(data, pkg.LogisticGradient(), pkg.SquaredL2SGDUpdater(), 25, lam, np.full(d, start))
    err = np.abs(w - truth["weights"]).max()
    gnorm = np.linalg.norm(HT.gradient_sum(X, y, w, "logistic") / n + lam * w)
    print(f"device d={d}: {len(hist)} iterations, weight error {err:.3g}, ||g|| {gnorm:.3g}")
    assert err <= BAR * max(np.abs(truth["weights"]).max(), 1.0)
    assert gnorm <= 1e-10
    assert len(hist) > live[-1]
    np.testing.assert_allclose(hist[: live[-1] + 1], np.array(truth["history"])[: live[-1] + 1], rtol=BAR, atol=0)


@pytest.mark.parametrize("d,lam,start", NEWTON_CASES[:2])
def test_hessian_sum(pkg, d, lam, start):
    """hessian_sum at the start: the curvature within 1e-9 of its truth and the weighted pass within
    1e-9 A of its weights', so 2e-9 A = 2e-9 |X|^T diag(h) |X| in all."""
    c = newton_case(d, lam, start)
    X, n = c["X"], c["X"].shape[0]
    w = np.full(d, start) + 0.1
    hs = pkg.hessian_sum(dense_data(pkg, c), pkg.LogisticGradient(), w)
    h = HT.curvature(X, w, "logistic")
    A = np.abs(X).T @ (np.abs(X) * h[:, None])
    assert hs.count == n and hs.hessian.shape == (d, d)
    assert (np.abs(hs.hessian - HT.hessian_sum(X, w, "logistic")) <= 2.0 * BAR * A).all()
    assert abs(hs.curvatureSum - h.sum()) <= 2.0 * BAR * h.sum()
    assert (hs.hessian == hs.hessian.T).all()


@pytest.mark.parametrize("layout,d,storage", [("dense", 30, "f32"), ("dense", 130, "f64"), ("csr", 30, "f64")])
def test_newton_least_squares_is_the_normal_equations(pkg, layout, d, storage):
    c = dense_case(d, storage) if layout == "dense" else csr_case(d, storage)
    data = dense_data(pkg, c) if layout == "dense" else csr_data(pkg, c)
    lam = 0.05
    want = pkg.normal_equations(data, lam)
    w, hist = pkg.runNewton(data, pkg.LeastSquaresGradient(), pkg.SquaredL2SGDUpdater(), 10, lam, np.full(d, 2.0))
    assert np.abs(w - want).max() <= BAR * np.abs(want).max()
    assert 1 <= len(hist) <= 2
    nt = pkg.Newton(pkg.LeastSquaresGradient(), pkg.SquaredL2SGDUpdater()).setRegParam(lam).setNumIterations(10)
    assert np.abs(nt.optimize(data, np.zeros(d)) - want).max() <= BAR * np.abs(want).max()


def test_weighted_least_squares_through_stat(pkg):
    """stat.gramian(weights=) from a host array, and its normal equations against numpy's weighted
    least squares."""
    d = 30
    c = dense_case(d, "f64")
    X, y, n = c["X"], c["y"], c["X"].shape[0]
    om = np.abs(omega_of(n, 1234))
    g = pkg.gramian(dense_data(pkg, c), weights=om)
    T, A = HT.weighted_gram(X, y, om)
    check_weighted(g.matrix, T, A, "stat.gramian weighted")
    assert g.weighted and abs(g.weightSum - om.sum()) <= BAR * om.sum()
    lam = 0.1
    want = np.linalg.solve(T[:d, :d] / om.sum() + lam * np.eye(d), T[:d, d] / om.sum())
    assert np.abs(g.normal_equations(lam) - want).max() <= BAR * np.abs(want).max()


# ---- world size 2 -------------------------------------------------------------------------------------------
def test_two_ranks(tmp_path, pkg):
    """Two ranks sharing cuda:0 over gloo, each a fresh child process (tests/two_rank_hessian.py), one of
    them holding the empty partition: both hold identical bits, the single-rank truth within the bars."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import two_rank_hessian as T
    out = str(tmp_path / "res.json")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "two_rank_hessian.py"), out], env=env,
                       capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    with open(out) as f:
        res = json.load(f)
    assert len(res) == 2 and res["0"] == res["1"]          # floats survive JSON exactly: identical bits
    X, y, om = T.make_data()
    n, d = X.shape
    Tw, A = HT.weighted_gram(X, y, om)
    check_weighted(np.array(res["0"]["matrix"]).reshape(d + 2, d + 2), Tw, A, "two ranks, weighted Gramian")
    truth = HT.newton(X, y, np.full(d, T.START), T.LAM, num_iterations=25)
    assert sum(truth["halvings"]) >= 1 and truth["gnorm"][-1] <= 1e-10          # (conditions on the inputs)
    w = np.array(res["0"]["weights"])
    assert np.abs(w - truth["weights"]).max() <= BAR * max(np.abs(truth["weights"]).max(), 1.0)
    assert np.linalg.norm(HT.gradient_sum(X, y, w, "logistic") / n + T.LAM * w) <= 1e-10
    live = [k for k, g in enumerate(truth["gnorm"]) if g > 1e-6]
    hist = np.array(res["0"]["history"])
    np.testing.assert_allclose(hist[: live[-1] + 1], np.array(truth["history"])[: live[-1] + 1], rtol=BAR, atol=0)
