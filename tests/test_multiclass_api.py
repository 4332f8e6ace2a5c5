"""The multiclass scoring calls without a device: exported symbols, null-context errors, the refusals
that must come before any device work, MulticlassMetrics arithmetic from an injected table, and
evaluate_multinomial on a data set without partitions."""
import ctypes
import math

import numpy as np
import pytest

import multiclass_truth as T

NEW_SYMBOLS = ("psgd_evaluate_multinomial", "psgd_evaluate_multinomial_device", "psgd_predict_multinomial",
               "psgd_predict_multinomial_device", "psgd_confusion", "psgd_confusion_device", "psgd_confusion_model",
               "psgd_confusion_model_device", "psgd_multiclass_switches")


def test_symbols_exported_and_bound(pkg):
    lib = ctypes.CDLL(pkg._native.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in pkg._native.EXPORTED
        assert getattr(pkg._native.lib(), name).argtypes is not None
    for name in ("evaluate_multinomial", "MulticlassMetrics"):
        assert name in pkg.__all__ and hasattr(pkg, name)
    for name in ("evaluate_multinomial", "predict_classes", "confusion"):
        assert callable(getattr(pkg.HipEngine, name))
    assert callable(pkg.ParallelizedSGD.evaluate_multinomial)


def test_null_context_is_einval_with_a_message(pkg):
    L = pkg._native.lib()
    w, out = np.zeros(4), np.zeros(8)
    counts, bad = np.zeros(9, dtype=np.int64), ctypes.c_int64()
    calls = [
        lambda: L.psgd_evaluate_multinomial(None, 3, w.ctypes.data, out.ctypes.data, None),
        lambda: L.psgd_evaluate_multinomial_device(None, 3, w.ctypes.data, out.ctypes.data, None, None),
        lambda: L.psgd_predict_multinomial(None, 0, 3, w.ctypes.data, out.ctypes.data, None),
        lambda: L.psgd_predict_multinomial_device(None, 0, 3, w.ctypes.data, out.ctypes.data, None, None),
        lambda: L.psgd_confusion(None, w.ctypes.data, w.ctypes.data, 4, 3, counts.ctypes.data, ctypes.byref(bad)),
        lambda: L.psgd_confusion_device(None, w.ctypes.data, w.ctypes.data, 4, 3, counts.ctypes.data,
                                        ctypes.byref(bad), None),
        lambda: L.psgd_confusion_model(None, 3, w.ctypes.data, counts.ctypes.data, ctypes.byref(bad)),
        lambda: L.psgd_confusion_model_device(None, 3, w.ctypes.data, counts.ctypes.data, ctypes.byref(bad), None),
    ]
    for call in calls:
        assert call() == pkg._native.PSGD_EINVAL
        assert b"ctx is null" in L.psgd_last_error()


def test_path_switches_are_named(pkg):
    sw = pkg._native.multiclass_switches()
    assert set(sw) == {"lds_weights", "lane_classes", "confusion_lds_cells"}
    assert all(v > 0 for v in sw.values())
    assert pkg._native.lib().psgd_multiclass_switches(None) == pkg._native.PSGD_EINVAL


class NoEngine:
    def __getattr__(self, name):
        raise AssertionError("device work before the refusal: " + name)


def _data(pkg):
    return pkg.PartitionedData.parallelize(np.array([0.0, 1.0, 2.0, 1.0]), np.ones((4, 2)), 2)


def test_refusals_before_any_device_work(pkg):
    data = _data(pkg)
    g3, upd = pkg.LogisticGradient(3), pkg.SimpleSGDUpdater()
    # MLlib's require(weights.size % dataSize == 0 && numClasses == weights.size / dataSize + 1)
    for bad in (np.zeros(3), np.zeros(2), np.zeros(6), np.zeros((2, 2))):
        with pytest.raises(pkg.IllegalArgumentException) as e:
            pkg.evaluate_multinomial(data, g3, upd, 0.0, bad, engine=NoEngine())
        assert str(e.value) == "requirement failed"
        with pytest.raises(pkg.IllegalArgumentException) as e:
            pkg.MulticlassMetrics.fromModel(data, bad, 3, engine=NoEngine())
        assert str(e.value) == "requirement failed"
    with pytest.raises(pkg.IllegalArgumentException) as e:
        pkg.ParallelizedSGD(g3, upd).evaluate_multinomial(data, np.zeros(5), engine=NoEngine())
    assert str(e.value) == "requirement failed"
    # a binary gradient
    for g in (pkg.LogisticGradient(), pkg.LogisticGradient(2), pkg.HingeGradient(), pkg.LeastSquaresGradient()):
        with pytest.raises(pkg.IllegalArgumentException, match="numClasses > 2"):
            pkg.evaluate_multinomial(data, g, upd, 0.0, np.zeros(2), engine=NoEngine())
        with pytest.raises(pkg.IllegalArgumentException, match="numClasses > 2"):
            pkg.ParallelizedSGD(g, upd).evaluate_multinomial(data, np.zeros(2), engine=NoEngine())
    with pytest.raises(pkg.IllegalArgumentException, match="numClasses > 2"):
        pkg.MulticlassMetrics.fromModel(data, np.zeros(2), 2, engine=NoEngine())
    # the binary calls keep refusing the multinomial gradient, now with a pointer to the new call
    with pytest.raises(pkg.UnsupportedOperationException, match="evaluate_multinomial"):
        pkg.evaluate(data, g3, upd, 0.0, np.zeros(4), engine=NoEngine())


def test_evaluate_multinomial_without_partitions(pkg):
    empty = pkg.PartitionedData([])
    ev = pkg.evaluate_multinomial(empty, pkg.LogisticGradient(4), pkg.SimpleSGDUpdater(), 0.0, np.zeros(6),
                                  engine=NoEngine())
    assert ev.count == 0 and ev.lossSum == 0.0 and ev.nCorrect == 0
    assert ev.accuracy is None and math.isnan(ev.meanLoss)
    m = pkg.MulticlassMetrics.fromModel(empty, np.zeros(6), 4, engine=NoEngine())
    assert m.table.shape == (4, 4) and not m.table.any() and len(m.labels) == 0


def check_members(pkg, m, t):
    """Every member of pkg.MulticlassMetrics m against the truth's Metrics t."""
    assert list(m.labels) == t.labels
    assert m.confusionMatrix().tolist() == t.confusionMatrix().tolist()
    assert m.precision() == m.recall() == m.fMeasure() == t.accuracy()
    for c in t.labels:
        assert m.precision(c) == t.precision(c) and m.recall(c) == t.recall(c)
        assert m.fMeasure(c) == t.fMeasure(c) and m.fMeasure(c, 0.5) == t.fMeasure(c, 0.5)
        assert m.truePositiveRate(c) == t.truePositiveRate(c)
        assert m.falsePositiveRate(c) == t.falsePositiveRate(c)
    assert m.weightedPrecision == t.weightedPrecision and m.weightedRecall == t.weightedRecall
    assert m.weightedTruePositiveRate == t.weightedTruePositiveRate
    assert m.weightedFalsePositiveRate == t.weightedFalsePositiveRate
    assert m.weightedFMeasure() == t.weightedFMeasure() and m.weightedFMeasure(2.0) == t.weightedFMeasure(2.0)


def test_metrics_from_an_injected_table(pkg):
    table = [[2, 1, 1], [1, 3, 0], [0, 0, 1]]   # the nine-pair example of test_multiclass_truth.py
    m = pkg.MulticlassMetrics.fromTable(table)
    assert m.numClasses == 3 and m.table.dtype == np.int64
    assert m.precision(0.0) == 2 / 3 and m.recall(0.0) == 1 / 2 and m.precision() == 6 / 9
    check_members(pkg, m, T.Metrics(table))
    # a predicted class that never occurs as a label: no column, still a miss and a false positive
    t4 = T.confusion([0.0, 3.0, 1.0, 3.0, 1.0], [0.0, 0.0, 1.0, 1.0, 1.0], 4)
    m4 = pkg.MulticlassMetrics.fromTable(t4)
    assert list(m4.labels) == [0.0, 1.0] and m4.confusionMatrix().tolist() == [[1, 0], [0, 2]]
    assert m4.precision() == 3 / 5
    check_members(pkg, m4, T.Metrics(t4))
    for never in (2.0, 3.0, 4.0, -1.0, 0.5):
        with pytest.raises(pkg.IllegalArgumentException, match="does not occur"):
            m4.recall(never)
    # the guarded zero denominators
    m2 = pkg.MulticlassMetrics.fromTable([[1, 0], [1, 0]])
    assert m2.precision(1.0) == 0.0 and m2.recall(1.0) == 0.0 and m2.fMeasure(1.0) == 0.0
    rng = np.random.default_rng(3)
    big = rng.integers(0, 50, size=(7, 7))
    big[4, :] = 0   # class 4 never occurs as a label
    check_members(pkg, pkg.MulticlassMetrics.fromTable(big), T.Metrics(big))
    for bad in ([[1, 2, 3]], [[1, -1], [0, 2]]):
        with pytest.raises(pkg.IllegalArgumentException):
            pkg.MulticlassMetrics.fromTable(bad)
