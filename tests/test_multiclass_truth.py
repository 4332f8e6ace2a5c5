"""tests/multiclass_truth.py (the GPU tests' numpy truth) against oracle/psgd_ref.py::multinomial, row by
row, and its MulticlassMetrics arithmetic on examples that can be checked by hand. No device."""
import math

import numpy as np
import pytest

import multiclass_truth as T


def ref():
    import psgd_ref
    return psgd_ref


def dense_rows(n, d, seed):
    rng = np.random.default_rng(seed)
    return [[float(v) for v in row] for row in rng.standard_normal((n, d))]


def sparse_rows(n, d, seed):
    rng = np.random.default_rng(seed)
    rows = []
    for k in range(n):
        m = k % (d + 1)   # 0 .. d non-zeros, an empty row among them
        idx = np.sort(rng.choice(d, size=m, replace=False))
        rows.append(([int(i) for i in idx], [float(v) for v in rng.standard_normal(m)]))
    return rows


def check_rows(rows, w, K, labels):
    R = ref()
    M = T.margins(rows, w, K)
    got = T.losses(M, labels)
    for k, row in enumerate(rows):
        want = R.multinomial(row, float(labels[k]), list(w), K)[1]
        assert abs(got[k] - want) <= 1e-12 * abs(want), (k, got[k], want)
        # the margins themselves, through the oracle's own summation
        d = len(w) // (K - 1)
        act = list(zip(*row)) if isinstance(row, tuple) else list(enumerate(row))
        for c in range(K - 1):
            m = 0.0
            for j, v in act:
                m += v * w[c * d + j]
            assert abs(M[k, c] - m) <= 1e-13 * max(sum(abs(v * w[c * d + j]) for j, v in act), 1e-300)


@pytest.mark.parametrize("K", [3, 4, 10])
@pytest.mark.parametrize("layout", ["dense", "sparse"])
def test_losses_and_margins_match_the_oracle(layout, K):
    d, n = 5, 3 * K + 2
    rows = dense_rows(n, d, 10 + K) if layout == "dense" else sparse_rows(n, d, 20 + K)
    w = np.random.default_rng(K).standard_normal((K - 1) * d)
    labels = [float(k % K) for k in range(n)]   # labels 0 .. K - 1
    check_rows(rows, w, K, labels)


def test_shift_by_a_margin_past_745_and_all_negative_margins():
    K, d = 4, 2
    w = np.array([1.0, 0.0, 0.5, 0.0, -1.0, 0.0])      # margins of x = (t, 0): t, t / 2, -t
    rows = [[800.0, 0.0], [-800.0, 0.0], [-3.0, 0.0], ([0], [1600.0]), ([], [])]
    M = T.margins(rows, w, K)
    assert M[0, 0] == 800.0 and M[0].max() > 745           # exp(800) overflows: the shift matters
    assert np.all(M[2, :2] < 0) and M[2, 2] == 3.0
    neg = [[-2.0, 0.0]]
    w_neg = np.array([1.0, 0.0, 0.5, 0.0, 2.0, 0.0])
    assert np.all(T.margins(neg, w_neg, K) < 0)            # a row of all-negative margins: no shift
    for labels in ([0.0, 1.0, 2.0, 3.0, 0.0], [3.0, 2.0, 1.0, 0.0, 2.0]):
        check_rows(rows, w, K, labels)
        got = T.losses(M, labels)
        assert all(math.isfinite(v) for v in got)
    check_rows(neg, w_neg, K, [0.0])
    check_rows(neg, w_neg, K, [2.0])
    assert T.predict(T.margins(neg, w_neg, K))[0] == 0.0
    # the empty row: every margin 0, class 0, loss log(K)
    assert T.predict(M)[4] == 0.0 and T.row_loss(M[4], 0.0) == math.log1p(K - 1.0)


def test_predict_point_rule():
    assert T.predict_point([-1.0, -2.0]) == 0          # no positive margin: the pivot
    assert T.predict_point([0.0, 0.0]) == 0            # zero is not positive
    assert T.predict_point([1.0, 2.0, 2.0]) == 2       # exact ties go to the lowest class
    assert T.predict_point([3.0, 3.0]) == 1
    assert T.predict_point([-1.0, 1e-300]) == 2
    assert T.predict_point([float("nan"), 1.0]) == 2   # a NaN compares false


NINE = [(0, 0), (0, 1), (0, 0), (1, 0), (1, 1), (1, 1), (1, 1), (2, 2), (2, 0)]   # (prediction, label)


def test_metrics_on_the_nine_pair_example():
    pred = [float(p) for p, _ in NINE]
    lab = [float(y) for _, y in NINE]
    t = T.confusion(pred, lab, 3)
    assert t.tolist() == [[2, 1, 1], [1, 3, 0], [0, 0, 1]]
    m = T.Metrics(t)
    assert m.labels == [0.0, 1.0, 2.0] and m.confusionMatrix().tolist() == t.tolist()
    assert m.precision(0.0) == 2 / 3 and m.recall(0.0) == 1 / 2 and m.accuracy() == 6 / 9
    assert m.precision() == m.recall() == m.fMeasure() == 6 / 9
    assert m.precision(1.0) == 3 / 4 and m.recall(1.0) == 3 / 4
    assert m.precision(2.0) == 1 / 2 and m.recall(2.0) == 1.0
    assert m.truePositiveRate(2.0) == 1.0
    assert m.falsePositiveRate(0.0) == 1 / 5 and m.falsePositiveRate(1.0) == 1 / 5 and m.falsePositiveRate(2.0) == 1 / 8
    f0 = 2 * (2 / 3) * (1 / 2) / (2 / 3 + 1 / 2)
    assert abs(m.fMeasure(0.0) - f0) < 1e-15
    f0b = (1 + 4) * (2 / 3) * (1 / 2) / (4 * (2 / 3) + 1 / 2)
    assert abs(m.fMeasure(0.0, 2.0) - f0b) < 1e-15
    assert abs(m.weightedRecall - (0.5 * 4 + 0.75 * 4 + 1.0 * 1) / 9) < 1e-15
    assert m.weightedTruePositiveRate == m.weightedRecall
    assert abs(m.weightedPrecision - ((2 / 3) * 4 + 0.75 * 4 + 0.5 * 1) / 9) < 1e-15
    assert abs(m.weightedFalsePositiveRate - (0.2 * 4 + 0.2 * 4 + 0.125) / 9) < 1e-15
    want = sum(m.fMeasure(c) * k for c, k in ((0.0, 4), (1.0, 4), (2.0, 1))) / 9
    assert abs(m.weightedFMeasure() - want) < 1e-15


def test_a_predicted_class_that_never_occurs_as_a_label():
    pred = [0.0, 3.0, 1.0, 3.0, 1.0]
    lab = [0.0, 0.0, 1.0, 1.0, 1.0]
    m = T.Metrics(T.confusion(pred, lab, 4))
    assert m.labels == [0.0, 1.0]                       # classes 2 and 3 never occur as labels
    assert m.confusionMatrix().tolist() == [[1, 0], [0, 2]]   # class 3 has no column
    assert m.accuracy() == 3 / 5                        # its two rows are misses all the same
    assert m.recall(0.0) == 1 / 2 and m.recall(1.0) == 2 / 3
    assert m.fp(3.0) == 2 and m.tp(3.0) == 0            # false positives of class 3
    assert m.precision(0.0) == 1.0 and m.falsePositiveRate(0.0) == 0.0
    # a class that is never predicted: precision guards tp + fp = 0, fMeasure p + r = 0
    m2 = T.Metrics(T.confusion([0.0, 0.0], [0.0, 1.0], 2))
    assert m2.precision(1.0) == 0.0 and m2.recall(1.0) == 0.0 and m2.fMeasure(1.0) == 0.0
