"""The multinomial batch gradient without a device: the C ABI's symbols and argument errors, the host
plan (psgd_gradient_multinomial_plan) at its path boundaries, the Python calls' refusals before any
device work, and GradientDescent.runMiniBatchSGDMultinomial's driver loop over a scripted engine."""
import ctypes
import logging
import os
import re

import numpy as np
import pytest

NEW_SYMBOLS = ("psgd_gradient_sum_multinomial", "psgd_gradient_sum_multinomial_device",
               "psgd_gradient_multinomial_plan")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_exported_bound_and_declared(pkg):
    lib = ctypes.CDLL(pkg._native.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "psgd.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in pkg._native.EXPORTED
        assert getattr(pkg._native.lib(), name).argtypes is not None
        assert re.search(r"\b%s\(" % name, header), name
    for name in ("gradient_sum_multinomial", "runMiniBatchSGDMultinomial"):
        assert name in pkg.__all__ and callable(getattr(pkg, name))


def test_argument_errors_need_no_device(pkg):
    L = pkg._native.lib()
    N = pkg._native
    w, out = np.zeros(8), np.zeros(10)
    assert L.psgd_gradient_sum_multinomial(None, 3, w.ctypes.data, 1.0, 1, out.ctypes.data) == N.PSGD_EINVAL
    assert b"ctx is null" in L.psgd_last_error()
    assert L.psgd_gradient_sum_multinomial_device(None, 3, w.ctypes.data, 1.0, 1, out.ctypes.data, None) == N.PSGD_EINVAL
    assert b"ctx is null" in L.psgd_last_error()
    plan = (ctypes.c_int32 * 12)()
    assert L.psgd_gradient_multinomial_plan(0, 1, 100, 3, 0, None) == N.PSGD_EINVAL
    for K in (2, 1, 0, -5):
        assert L.psgd_gradient_multinomial_plan(0, 1, 100, K, 0, plan) == N.PSGD_EINVAL
        assert b"num_classes" in L.psgd_last_error()
    assert L.psgd_gradient_multinomial_plan(0, 1, 100, 4097, 0, plan) == N.PSGD_OK
    assert L.psgd_gradient_multinomial_plan(0, 1, 100, 4098, 0, plan) == N.PSGD_EUNSUPPORTED
    assert b"4097" in L.psgd_last_error()
    for bad in ((2, 1, 100, 3, 0), (0, 2, 100, 3, 0), (0, 1, 0, 3, 0), (1, 1, 100, 3, -1)):
        assert L.psgd_gradient_multinomial_plan(*bad, plan) == N.PSGD_EINVAL


def plan(pkg, *a, **k):
    return pkg._native.gradient_multinomial_plan(*a, **k)


def largest_fused_d(pkg, storage, K, hi=1 << 16):
    """The largest d with a fused plan (the fused shapes of a K are d = 1 .. that)."""
    assert plan(pkg, "dense", storage, 1, K)["path"] == "fused"
    lo = 1
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if plan(pkg, "dense", storage, mid, K)["path"] == "fused":
            lo = mid
        else:
            hi = mid
    return lo


def test_plan_fused_and_forced_general(pkg, monkeypatch):
    monkeypatch.delenv("PSGD_GRAD_MN_TWO_PASS", raising=False)
    p = plan(pkg, "dense", "f32", 100, 3)
    assert p["path"] == "fused" and p["weights_in_lds"] == 1 and p["wide_softmax"] == 0
    assert p["tile_rows"] == 1024 and p["span"] == 1
    # a lane's accumulators: class_accumulators x nvl vectors, within the register budget
    assert p["class_accumulators"] >= 2 and p["class_accumulators"] * p["nvl"] <= 16
    assert plan(pkg, "dense", "f64", 100, 3)["tile_rows"] == 512
    monkeypatch.setenv("PSGD_GRAD_MN_TWO_PASS", "1")
    q = plan(pkg, "dense", "f32", 100, 3)
    assert q["path"] == "general" and q["col_chunks"] >= 1 and q["class_chunks"] >= 1 and q["range"] >= 1
    monkeypatch.setenv("PSGD_GRAD_MN_TWO_PASS", "0")
    assert plan(pkg, "dense", "f32", 100, 3)["path"] == "fused"
    # a shape that fits the registers but was measured slower fused: general, unless PSGD_GRAD_MN_FUSE_ALL=1
    monkeypatch.delenv("PSGD_GRAD_MN_FUSE_ALL", raising=False)
    assert plan(pkg, "dense", "f32", 100, 10)["path"] == "general"
    monkeypatch.setenv("PSGD_GRAD_MN_FUSE_ALL", "1")
    p = plan(pkg, "dense", "f32", 100, 10)
    assert p["path"] == "fused" and p["class_accumulators"] == 16 and p["nvl"] == 1
    assert plan(pkg, "dense", "f32", 512, 10)["path"] == "general"      # 16 x 2 vectors do not fit


def test_plan_fused_boundary(pkg, monkeypatch):
    monkeypatch.delenv("PSGD_GRAD_MN_TWO_PASS", raising=False)
    monkeypatch.delenv("PSGD_GRAD_MN_FUSE_ALL", raising=False)
    for storage in ("f32", "f64"):
        for K in (3, 10):
            dmax = largest_fused_d(pkg, storage, K)
            assert plan(pkg, "dense", storage, dmax, K)["path"] == "fused"
            assert plan(pkg, "dense", storage, dmax + 1, K)["path"] == "general"
            # the fused shapes are an interval from d = 1
            for d in (1, 2, dmax // 2, dmax - 1):
                assert plan(pkg, "dense", storage, max(d, 1), K)["path"] == "fused"
    # more classes leave room for fewer columns
    assert largest_fused_d(pkg, "f32", 3) > largest_fused_d(pkg, "f32", 10)
    # past 17 classes nothing is fused
    assert plan(pkg, "dense", "f32", 1, 18)["path"] == "general"


def test_plan_softmax_switch(pkg, monkeypatch):
    monkeypatch.delenv("PSGD_GRAD_MN_TWO_PASS", raising=False)
    lanes = pkg._native.multiclass_switches()["lane_classes"]
    assert lanes == 64
    for layout in ("dense", "csr"):
        assert plan(pkg, layout, "f32", 20, lanes + 1, 8)["wide_softmax"] == 0      # K - 1 = 64
        assert plan(pkg, layout, "f32", 20, lanes + 2, 8)["wide_softmax"] == 1      # K - 1 = 65


def test_plan_class_blocks_in_lds(pkg, monkeypatch):
    monkeypatch.setenv("PSGD_GRAD_MN_TWO_PASS", "1")
    cap = pkg._native.multiclass_switches()["lds_weights"]
    K = 5
    d = cap // (K - 1)          # (K - 1) d == cap with d a whole number of vectors
    assert d % 4 == 0
    assert plan(pkg, "dense", "f32", d, K)["weights_in_lds"] == 1
    assert plan(pkg, "dense", "f32", d + 1, K)["weights_in_lds"] == 0


def test_plan_csr_lds_boundary(pkg, monkeypatch):
    monkeypatch.delenv("PSGD_GRAD_CSR_GLOBAL", raising=False)
    f = ctypes.CDLL(pkg._native.LIB_PATH)._ZN4psgd20grad_csr_lds_appliesEi
    f.restype, f.argtypes = ctypes.c_bool, [ctypes.c_int]
    cells = 1
    while f(cells * 2):
        cells *= 2
    while f(cells + 1):
        cells += 1                       # kGradLdsFeatures, as the binary pass reports it
    for K in (3, 4, 7):
        d = cells // (K - 1)
        assert plan(pkg, "csr", "f32", d, K, 40)["path"] == "csr_lds"
        assert plan(pkg, "csr", "f32", d + 1, K, 40)["path"] == "csr_global"
    assert plan(pkg, "csr", "f64", 200000, 3, 40)["path"] == "csr_global"
    assert [plan(pkg, "csr", "f32", 100, 3, m)["group"] for m in (0, 16, 17, 32, 33, 5000)] == [16, 16, 32, 32, 64, 64]
    monkeypatch.setenv("PSGD_GRAD_CSR_GLOBAL", "1")
    assert plan(pkg, "csr", "f32", 10, 3, 40)["path"] == "csr_global"


def test_plan_scratch_is_bounded(pkg, monkeypatch):
    """A record covers `span` tiles with (K - 1) / span <= 16; a range's multipliers take at most
    2^25 doubles, or one tile's."""
    monkeypatch.delenv("PSGD_GRAD_MN_TWO_PASS", raising=False)
    for K in (3, 17, 18, 33, 66, 1000, 4097):
        for storage, d in (("f32", 3), ("f32", 5000), ("f64", 700)):
            p = plan(pkg, "dense", storage, d, K)
            assert (K - 1) <= 16 * p["span"] and p["span"] & (p["span"] - 1) == 0
            if p["path"] == "general":
                r = p["range"]
                assert r >= 1 and r & (r - 1) == 0
                assert r == 1 or r * p["tile_rows"] * (K - 1) <= 1 << 25


# ---- the Python calls ----
class NoEngine:
    def __getattr__(self, name):
        raise AssertionError("device work before the refusal: " + name)


def _data(pkg):
    return pkg.PartitionedData.parallelize(np.array([0.0, 1.0, 2.0, 1.0]), np.ones((4, 2)), 2)


def test_refusals_before_device_work(pkg):
    data = _data(pkg)
    g3 = pkg.LogisticGradient(3)
    upd = pkg.SimpleSGDUpdater()
    for bad in (pkg.LogisticGradient(), pkg.LeastSquaresGradient(), pkg.HingeGradient()):
        with pytest.raises(pkg.IllegalArgumentException, match="numClasses > 2"):
            pkg.gradient_sum_multinomial(data, bad, [0.0] * 4, engine=NoEngine())
        with pytest.raises(pkg.IllegalArgumentException, match="numClasses > 2"):
            pkg.GradientDescent.runMiniBatchSGDMultinomial(data, bad, upd, 1.0, 2, 0.0, 1.0, [0.0] * 4,
                                                           engine=NoEngine())
    for stateful in (pkg.AdaGradSGDUpdater(), pkg.AdamSGDUpdater()):
        with pytest.raises(pkg.UnsupportedOperationException, match="stateless"):
            pkg.GradientDescent.runMiniBatchSGDMultinomial(data, g3, stateful, 1.0, 2, 0.0, 1.0, [0.0] * 4,
                                                           engine=NoEngine())
    for f in (1.5, -0.1, float("nan")):
        with pytest.raises(pkg.IllegalArgumentException, match="Sampling fraction"):
            pkg.gradient_sum_multinomial(data, g3, [0.0] * 4, f, engine=NoEngine())
    # MLlib's require on weights.size: (K - 1) * num_features
    for size in (2, 3, 5, 6):
        with pytest.raises(pkg.IllegalArgumentException, match="^requirement failed$"):
            pkg.gradient_sum_multinomial(data, g3, [0.0] * size, engine=NoEngine())
        with pytest.raises(pkg.IllegalArgumentException, match="^requirement failed$"):
            pkg.GradientDescent.runMiniBatchSGDMultinomial(data, g3, upd, 1.0, 2, 0.0, 1.0, [0.0] * size,
                                                           engine=NoEngine())
    with pytest.raises(pkg.IllegalArgumentException, match="^requirement failed$"):
        pkg.gradient_sum_multinomial(data, g3, np.zeros((2, 2)), engine=NoEngine())
    # the binary-named calls keep refusing K > 2 and name the call that takes it
    with pytest.raises(pkg.UnsupportedOperationException, match="multinomial.*gradient_sum_multinomial"):
        pkg.gradient_sum(data, g3, [0.0] * 4, engine=NoEngine())
    with pytest.raises(pkg.UnsupportedOperationException, match="multinomial.*runMiniBatchSGDMultinomial"):
        pkg.GradientDescent.runMiniBatchSGD(data, g3, upd, 1.0, 2, 0.0, 1.0, [0.0] * 4, engine=NoEngine())
    # no partitions: an empty sum, no engine
    none = pkg.PartitionedData([])
    s = pkg.gradient_sum_multinomial(none, g3, [0.0] * 4, engine=NoEngine())
    assert s.count == 0 and s.lossSum == 0.0 and s.gradient.shape == (0,)


class ScriptedEngine:
    """Returns canned batch sums {gradientSum[n], lossSum, count} of n = (K - 1) d weights and updates
    by w' = w - g / count, regVal' = the next scripted one. It has no binary gradient_sum: the
    multinomial driver must not call it."""

    def __init__(self, sums, n, terms=(1.0, 1.0), rv0=0.25, regvals=()):
        self.sums, self.n, self.terms, self.rv0 = list(sums), n, terms, rv0
        self.regvals = list(regvals)
        self.batches, self.updates, self.conv_calls = [], [], 0

    def weights(self, w):
        return np.array(w, dtype=float)

    def initial_regval(self, params, w):
        assert params.num_classes == 3 and len(w) == self.n
        return self.rv0

    def gradient_sum_multinomial(self, K, w, fraction, iteration):
        self.batches.append((K, fraction, iteration, np.array(w)))
        return self.sums.pop(0)

    def batch_scalars(self, s):
        return float(s[self.n]), int(s[self.n + 1])

    def gd_update(self, updater, w, s, step, iteration, reg):
        self.updates.append((iteration, step, reg))
        return w - s[: self.n] / s[self.n + 1], self.regvals.pop(0)

    def convergence_terms(self, prev, cur):
        self.conv_calls += 1
        return self.terms

    def to_host(self, w):
        return np.array(w)


def run(pkg, eng, updater, iters, fraction=1.0, tol=0.001, w0=(0.0, 0.0, 0.0, 0.0), data=None, reg=0.1):
    return pkg.GradientDescent.runMiniBatchSGDMultinomial(data or _data(pkg), pkg.LogisticGradient(3), updater, 1.0,
                                                          iters, reg, fraction, list(w0), tol, engine=eng)


def test_driver_regval_lag_and_empty_batch(pkg, caplog):
    sums = [np.array([4.0, 8.0, 0.0, -4.0, 8.0, 4.0]),    # g = (1, 2, 0, -1), lossSum 8, count 4
            np.array([9.0, 9.0, 9.0, 9.0, 0.0, 0.0]),     # empty batch: weights kept, no history entry
            np.array([2.0, 2.0, 2.0, 2.0, 2.0, 2.0])]
    eng = ScriptedEngine(sums, 4, terms=(100.0, 1.0), rv0=0.25, regvals=[0.5, 0.7])
    with caplog.at_level(logging.WARNING):
        w, h = run(pkg, eng, pkg.SquaredL2SGDUpdater(), 3)
    # the loss of iteration i is at the weights, and with the regVal, of iteration i - 1
    assert list(h) == [8.0 / 4 + 0.25, 2.0 / 2 + 0.5]
    assert list(w) == [-1.0 - 1.0, -2.0 - 1.0, 0.0 - 1.0, 1.0 - 1.0]
    assert [b[0] for b in eng.batches] == [3, 3, 3]
    assert [b[2] for b in eng.batches] == [1, 2, 3]               # the batch of iteration i is seeded 42 + i
    assert np.array_equal(eng.batches[2][3], eng.batches[1][3])   # the empty batch kept the weights
    assert [u[0] for u in eng.updates] == [1, 3]                  # the update's iter is the loop's i
    assert all(u[1:] == (1.0, 0.1) for u in eng.updates)
    assert "Iteration (2/3). The size of sampled batch is zero" in caplog.text


def test_driver_convergence_and_tolerance_zero(pkg):
    one = np.array([1.0, 2.0, 3.0, 4.0, 8.0, 4.0])
    eng = ScriptedEngine([one.copy() for _ in range(5)], 4, terms=(0.0, 1.0), regvals=[0.0] * 5)   # ||diff|| = 0 < tol
    w, h = run(pkg, eng, pkg.SimpleSGDUpdater(), 5)
    assert len(h) == 2 and eng.conv_calls == 1    # no test after the first update, converged at the second
    # an empty batch between them does not count as an update
    eng = ScriptedEngine([one.copy(), np.zeros(6), one.copy(), one.copy()], 4, terms=(0.0, 1.0), regvals=[0.0] * 4)
    w, h = run(pkg, eng, pkg.L1SGDUpdater(), 4)
    assert len(h) == 2 and eng.conv_calls == 1 and len(eng.batches) == 3
    eng = ScriptedEngine([one.copy() for _ in range(4)], 4, terms=(0.0, 1.0), regvals=[0.0] * 4)
    _, h = run(pkg, eng, pkg.SimpleSGDUpdater(), 4, tol=0.0)
    assert len(h) == 4
    # sqrt(dsq) < tol * max(sqrt(nsq), 1) is strict
    eng = ScriptedEngine([one.copy() for _ in range(3)], 4, terms=(1e-6, 1.0), regvals=[0.0] * 3)
    _, h = run(pkg, eng, pkg.SimpleSGDUpdater(), 3, tol=0.001)
    assert len(h) == 3


def test_driver_empty_data_zero_iterations_and_warnings(pkg, caplog):
    empty = pkg.PartitionedData.parallelize(np.ones(0), np.ones((0, 2)), 2)
    eng = ScriptedEngine([], 4)
    with caplog.at_level(logging.WARNING):
        w, h = run(pkg, eng, pkg.SimpleSGDUpdater(), 3, w0=(0.5, -0.5, 0.25, 0.0), data=empty)
    assert list(w) == [0.5, -0.5, 0.25, 0.0] and len(h) == 0 and not eng.batches
    assert "returning initial weights, no data found" in caplog.text
    eng = ScriptedEngine([], 4)
    w, h = run(pkg, eng, pkg.SimpleSGDUpdater(), 0, w0=(0.5, -0.5, 0.25, 0.0))
    assert list(w) == [0.5, -0.5, 0.25, 0.0] and len(h) == 0 and not eng.batches
    caplog.clear()
    eng = ScriptedEngine([np.array([1.0, 2.0, 3.0, 4.0, 8.0, 4.0])], 4, regvals=[0.0])
    with caplog.at_level(logging.WARNING):
        run(pkg, eng, pkg.SimpleSGDUpdater(), 1, fraction=0.1)
    assert "Testing against a convergenceTol when using miniBatchFraction < 1.0 can be unstable" in caplog.text
    assert "The miniBatchFraction is too small" in caplog.text   # 4 rows * 0.1 < 1
    assert eng.batches[0][1] == 0.1


def test_optimize_chooses_by_num_classes(pkg, monkeypatch):
    calls = []
    monkeypatch.setattr(pkg.GradientDescent, "runMiniBatchSGD",
                        staticmethod(lambda *a, **k: (calls.append("binary"), (np.zeros(2), None))[1]))
    monkeypatch.setattr(pkg.GradientDescent, "runMiniBatchSGDMultinomial",
                        staticmethod(lambda *a, **k: (calls.append("multinomial"), (np.zeros(4), None))[1]))
    data = _data(pkg)
    pkg.GradientDescent(pkg.LogisticGradient(), pkg.SimpleSGDUpdater()).optimize(data, [0.0] * 2)
    pkg.GradientDescent(pkg.LogisticGradient(3), pkg.SimpleSGDUpdater()).optimize(data, [0.0] * 4)
    pkg.GradientDescent(pkg.HingeGradient(), pkg.SimpleSGDUpdater()).optimize(data, [0.0] * 2)
    assert calls == ["binary", "multinomial", "binary"]
