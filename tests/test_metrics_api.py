"""BinaryClassificationMetrics' surface that needs no device: the curves and the F-measure from a
canned table, the one-class and empty cases, the numBins refusal, argument validation, and the C
ABI's exported symbols and null-pointer errors."""
import ctypes as C
import math
import os

import numpy as np
import pytest

SYMBOLS = ("psgd_binary_counts", "psgd_binary_counts_device", "psgd_binary_counts_model",
           "psgd_binary_counts_model_device", "psgd_metrics_sort_tile")

# scores 0.9 0.8 0.8 0.4 0.4 0.4 0.1 with labels 1 1 0 1 0 0 0
THR = [0.9, 0.8, 0.4, 0.1]
CUM_POS = [1, 2, 3, 3]
CUM_NEG = [0, 1, 3, 4]


def native(pkg):
    import spark_parallelized_sgd_amd._native as N
    if not os.path.exists(N.LIB_PATH):
        pytest.skip("libpsgd.so not built (__graft_entry__.build())")
    return N


def test_package_exports_the_class(pkg):
    assert pkg.BinaryClassificationMetrics is pkg.evaluation.BinaryClassificationMetrics
    assert "BinaryClassificationMetrics" in pkg.__all__


def test_curves_from_a_canned_table(pkg):
    m = pkg.BinaryClassificationMetrics.fromCounts(THR, CUM_POS, CUM_NEG)
    assert m.numPositives == 3 and m.numNegatives == 4 and m.numThresholds == 4
    assert m.thresholds().tolist() == THR
    recall = [1 / 3, 2 / 3, 3 / 3, 3 / 3]
    fpr = [0 / 4, 1 / 4, 3 / 4, 4 / 4]
    precision = [1 / 1, 2 / 3, 3 / 6, 3 / 7]
    assert m.roc().tolist() == [[0.0, 0.0]] + [[f, r] for f, r in zip(fpr, recall)] + [[1.0, 1.0]]
    assert m.pr().tolist() == [[0.0, 1.0]] + [[r, p] for r, p in zip(recall, precision)]
    assert m.precisionByThreshold().tolist() == [[t, p] for t, p in zip(THR, precision)]
    assert m.recallByThreshold().tolist() == [[t, r] for t, r in zip(THR, recall)]
    f1 = [2.0 * p * r / (p + r) for p, r in zip(precision, recall)]
    assert m.fMeasureByThreshold().tolist() == [[t, f] for t, f in zip(THR, f1)]
    f2 = [(1.0 + 4.0) * p * r / (4.0 * p + r) for p, r in zip(precision, recall)]
    assert m.fMeasureByThreshold(2.0).tolist() == [[t, f] for t, f in zip(THR, f2)]
    # rocNumerator = sum (cumNeg[g] - cumNeg[g-1]) (cumPos[g] + cumPos[g-1]) = 0*1 + 1*3 + 2*5 + 1*6
    assert m.rocNumerator == 19
    assert m.areaUnderROC() == 19 / (2.0 * 3 * 4)
    pts = m.pr()
    area = math.fsum((pts[i, 0] - pts[i - 1, 0]) * (pts[i, 1] + pts[i - 1, 1]) / 2.0 for i in range(1, len(pts)))
    assert abs(m.areaUnderPR() - area) <= 4 * 2.0 ** -52 * area
    # the trapezoid area of roc() is the integer form, up to the rounding of the fp64 sum
    r = m.roc()
    trap = math.fsum((r[i, 0] - r[i - 1, 0]) * (r[i, 1] + r[i - 1, 1]) / 2.0 for i in range(1, len(r)))
    assert abs(trap - m.areaUnderROC()) <= 8 * 2.0 ** -52


def test_f_measure_is_zero_where_precision_and_recall_are(pkg):
    m = pkg.BinaryClassificationMetrics.fromCounts([2.0, 1.0], [0, 1], [1, 1])
    assert m.fMeasureByThreshold().tolist() == [[2.0, 0.0], [1.0, 2.0 * 0.5 * 1.0 / 1.5]]


def test_one_class_and_empty(pkg):
    B = pkg.BinaryClassificationMetrics
    neg = B.fromCounts([1.0, 0.0], [0, 0], [2, 5])
    assert neg.numPositives == 0 and neg.areaUnderROC() == 0.0 and neg.areaUnderPR() == 0.0
    assert neg.recallByThreshold()[:, 1].tolist() == [0.0, 0.0]
    assert neg.roc().tolist() == [[0.0, 0.0], [2 / 5, 0.0], [1.0, 0.0], [1.0, 1.0]]
    assert neg.fMeasureByThreshold()[:, 1].tolist() == [0.0, 0.0]
    pos = B.fromCounts([1.0, 0.0], [2, 5], [0, 0])
    assert pos.numNegatives == 0 and pos.areaUnderROC() == 1.0 and pos.areaUnderPR() == 1.0
    assert pos.roc().tolist() == [[0.0, 0.0], [0.0, 2 / 5], [0.0, 1.0], [1.0, 1.0]]
    none = B.fromCounts([], [], [])
    assert none.numThresholds == 0 and math.isnan(none.areaUnderROC()) and none.areaUnderPR() == 0.0
    assert none.roc().tolist() == [[0.0, 0.0], [1.0, 1.0]] and none.pr().tolist() == [[0.0, 1.0]]
    assert none.thresholds().shape == (0,) and none.fMeasureByThreshold().shape == (0, 2)
    # a data set without partitions needs no device either
    empty = B.fromModel(pkg.PartitionedData([]), np.zeros(3))
    assert empty.numThresholds == 0 and math.isnan(empty.areaUnderROC()) and empty.pr().tolist() == [[0.0, 1.0]]


def test_num_bins_is_refused_before_any_device_work(pkg):
    B = pkg.BinaryClassificationMetrics
    with pytest.raises(pkg.UnsupportedOperationException):
        B(np.zeros(3), np.zeros(3), numBins=100)
    with pytest.raises(pkg.IllegalArgumentException):
        B(np.zeros(3), np.zeros(3), numBins=-1)


def test_argument_validation(pkg):
    B = pkg.BinaryClassificationMetrics
    with pytest.raises(pkg.IllegalArgumentException):
        B(np.zeros(3), np.zeros(4))
    with pytest.raises(pkg.IllegalArgumentException):
        B(np.zeros((3, 2)), np.zeros((3, 2)))
    with pytest.raises(pkg.IllegalArgumentException):
        B.fromCounts([1.0, 0.5], [1], [0, 1])
    with pytest.raises(pkg.IllegalArgumentException):
        B.fromCounts([1.0, 0.5], [2, 1], [0, 1])       # cumulative counts do not shrink
    with pytest.raises(pkg.IllegalArgumentException):
        B.fromCounts([1.0, 0.5], [1, 1], [0, 0])       # a group holds at least one row
    data = pkg.PartitionedData.parallelize(np.zeros(4), np.ones((4, 2)), 2)
    with pytest.raises(pkg.IllegalArgumentException):
        B.fromModel(data, np.zeros(2), score="rank")


def test_library_exports_the_metrics_symbols(pkg):
    N = native(pkg)
    raw = C.CDLL(N.LIB_PATH)
    for name in SYMBOLS:
        assert hasattr(raw, name), name
        assert name in N.EXPORTED


def test_sort_tile_is_the_library_constant(pkg):
    N = native(pkg)
    T = pkg.evaluation.SORT_TILE
    assert T == N.lib().psgd_metrics_sort_tile() and T >= 64 and T % 64 == 0


def test_null_context_is_einval(pkg):
    N = native(pkg)
    L = N.lib()
    s = (C.c_double * 4)()
    out4 = (C.c_int64 * 4)()
    out2 = (C.c_double * 2)()
    assert L.psgd_binary_counts(None, s, s, 4, None, None, None, out4, out2) == N.PSGD_EINVAL
    assert b"ctx is null" in L.psgd_last_error()
    assert L.psgd_binary_counts_device(None, None, None, 0, None, None, None, None, None, None) == N.PSGD_EINVAL
    assert L.psgd_binary_counts_model(None, s, None, None, None, out4, out2) == N.PSGD_EINVAL
    assert L.psgd_binary_counts_model_device(None, None, None, None, None, None, None, None) == N.PSGD_EINVAL
    assert b"ctx is null" in L.psgd_last_error()
