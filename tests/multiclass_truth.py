"""A numpy restatement of what the multiclass scoring calls compute, for the tests: the K - 1 margins
of a multinomial logistic model (class 0 the pivot, weights W[c * d + i]), MLlib 1.6.1's predictPoint
class, the loss of LogisticGradient.compute for numClasses > 2, a confusion table, and every member
of MulticlassMetrics. tests/test_multiclass_truth.py checks it against oracle/psgd_ref.py::multinomial
row by row; the GPU tests take their truth from here, so none needs the oracle's pure-Python loop.

A row is a dense sequence of d values or an (indices, values) pair."""
import math

import numpy as np


def _d2i(x: float) -> int:
    """Double.toInt."""
    if x != x:
        return 0
    if x >= 2147483647.0:
        return 2147483647
    if x <= -2147483648.0:
        return -2147483648
    return int(x)


def blocks(w, K: int) -> np.ndarray:
    """The weights as [K - 1, d]."""
    w = np.asarray(w, dtype=np.float64)
    assert w.ndim == 1 and w.shape[0] % (K - 1) == 0
    return w.reshape(K - 1, w.shape[0] // (K - 1))


def margins(rows, w, K: int) -> np.ndarray:
    """[n, K - 1]: margin_c = sum_i x_i W[c, i] (numpy's dot: its summation order is not the
    reference's; the tests' bars cover a reassociated sum)."""
    W = blocks(w, K)
    out = np.zeros((len(rows), K - 1))
    for r, row in enumerate(rows):
        if isinstance(row, tuple):
            idx = np.asarray(row[0], dtype=np.int64)
            out[r] = W[:, idx] @ np.asarray(row[1], dtype=np.float64) if len(idx) else 0.0
        else:
            out[r] = W @ np.asarray(row, dtype=np.float64)
    return out


def abs_margins(rows, w, K: int) -> np.ndarray:
    """[n, K - 1]: sum_i |x_i W[c, i]|, the scale of a margin's rounding error."""
    return margins([(r[0], np.abs(r[1])) if isinstance(r, tuple) else np.abs(r) for r in rows], np.abs(w), K)


def nnz(rows) -> np.ndarray:
    return np.array([len(r[0]) if isinstance(r, tuple) else len(r) for r in rows], dtype=np.int64)


def predict_point(m) -> int:
    """best = 0, max = 0.0; for c ascending, m_c > max sets best = c + 1: the pivot wins when no
    margin is positive, exact ties go to the lowest class."""
    best, top = 0, 0.0
    for c, v in enumerate(m):
        if v > top:
            best, top = c + 1, v
    return best


def predict(M) -> np.ndarray:
    return np.array([float(predict_point(m)) for m in M], dtype=np.float64)


def row_loss(m, label: float) -> float:
    """LogisticGradient.compute(x, label, w)._2 for numClasses > 2 from the row's K - 1 margins."""
    ly = _d2i(label) - 1
    margin_y, top, top_idx = 0.0, -math.inf, 0
    for c, v in enumerate(m):
        v = float(v)
        if c == ly:
            margin_y = v
        if v > top:
            top, top_idx = v, c
    s = 0.0
    if top > 0:
        for c, v in enumerate(m):
            s += math.exp(-top) if c == top_idx else math.exp(float(v) - top)
    else:
        for v in m:
            s += math.exp(float(v))
    loss = math.log1p(s) - margin_y if label > 0.0 else math.log1p(s)
    return loss + top if top > 0 else loss


def losses(M, labels) -> list:
    return [row_loss(m, float(y)) for m, y in zip(M, labels)]


def sum_left_to_right(values) -> float:
    s = 0.0
    for v in values:
        s = s + v
    return s


def confusion(predictions, labels, K: int) -> np.ndarray:
    """[K, K] int64: rows actual, columns predicted."""
    t = np.zeros((K, K), dtype=np.int64)
    for p, y in zip(predictions, labels):
        t[int(y), int(p)] += 1
    return t


class Metrics:
    """MulticlassMetrics from the K x K table: the definitions of MLlib 1.6.1 as this project restates
    them (labels = the classes that occur as a true label, ascending)."""

    def __init__(self, table):
        self.table = np.asarray(table, dtype=np.int64)
        self.K = self.table.shape[0]
        self.count = {c: int(self.table[c].sum()) for c in range(self.K)}
        self.n = int(self.table.sum())
        self.labels = [float(c) for c in range(self.K) if self.count[c] > 0]

    def confusionMatrix(self):
        idx = [int(c) for c in self.labels]
        return np.array([[self.table[a, b] for b in idx] for a in idx], dtype=np.int64).reshape(len(idx), len(idx))

    def tp(self, label):
        return int(self.table[int(label), int(label)])

    def fp(self, label):
        return int(self.table[:, int(label)].sum()) - self.tp(label)

    def precision(self, label=None):
        if label is None:
            return self.accuracy()
        tp, fp = self.tp(label), self.fp(label)
        return 0.0 if tp + fp == 0 else tp / (tp + fp)

    def recall(self, label=None):
        if label is None:
            return self.accuracy()
        return self.tp(label) / self.count[int(label)]

    def fMeasure(self, label=None, beta=1.0):
        if label is None:
            return self.accuracy()
        p, r = self.precision(label), self.recall(label)
        return 0.0 if p + r == 0 else (1 + beta * beta) * p * r / (beta * beta * p + r)

    def truePositiveRate(self, label):
        return self.recall(label)

    def falsePositiveRate(self, label):
        return self.fp(label) / (self.n - self.count[int(label)])

    def accuracy(self):
        return sum(self.tp(c) for c in range(self.K)) / self.n

    def weighted(self, member):
        return sum_left_to_right(member(c) * self.count[int(c)] / self.n for c in self.labels)

    @property
    def weightedPrecision(self):
        return self.weighted(self.precision)

    @property
    def weightedRecall(self):
        return self.weighted(self.recall)

    @property
    def weightedTruePositiveRate(self):
        return self.weightedRecall

    @property
    def weightedFalsePositiveRate(self):
        return self.weighted(self.falsePositiveRate)

    def weightedFMeasure(self, beta=1.0):
        return self.weighted(lambda c: self.fMeasure(c, beta))
