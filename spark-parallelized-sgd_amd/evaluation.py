"""Classification metrics on the device. MulticlassMetrics (the end of this file): the K x K
confusion table of psgd_confusion_device / psgd_confusion_model_device and MLlib 1.6.1's members
derived from it on the host.

Binary classification metrics: MLlib 1.6.1's BinaryClassificationMetrics with
numBins = 0 -- the step every classification example of the linear-methods guide ends with
(`new BinaryClassificationMetrics(scoreAndLabels).areaUnderROC()`).

The table {threshold, cumPos, cumNeg} per distinct score and the two areas come from the device
(psgd_binary_counts_device / psgd_binary_counts_model_device: a radix sort, a scan and a compaction;
include/psgd.h and DESIGN.md §3 have the definitions). The areas need no table read-back; the curves
are derived on the host from the table, which is copied once, when a curve is first asked for."""
from __future__ import annotations

import numpy as np

from . import _native as N
from ._native import IllegalArgumentException, UnsupportedOperationException

__all__ = ["BinaryClassificationMetrics", "MulticlassMetrics", "SORT_TILE"]


def __getattr__(name):
    # SORT_TILE: the number of pairs one workgroup of the metrics kernels takes -- the library's own
    # constant (psgd_metrics_sort_tile), read when first asked for: the kernels change path at its
    # multiples, and 256 tiles are one sweep of the sort's table scan.
    if name == "SORT_TILE":
        return N.metrics_sort_tile()
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def roc_area(rocNumerator: int, P: int, N_: int) -> float:
    """areaUnderROC from the exact integers: 0.0 without positives, 1.0 without negatives (what the
    guarded rates give), NaN without rows."""
    if P == 0 and N_ == 0:
        return float("nan")
    if P == 0:
        return 0.0
    if N_ == 0:
        return 1.0
    return float(rocNumerator) / (2.0 * float(P) * float(N_))


class DeviceCounts:
    """What a device call left: the table as device tensors of n entries (G are written), and the
    summary and areas on the host."""

    def __init__(self, thresholds, cumPos, cumNeg, summary, areas):
        self.thresholds, self.cumPos, self.cumNeg = thresholds, cumPos, cumNeg
        self.G, self.P, self.N, self.rocNumerator = (int(v) for v in summary)
        self.areaUnderROC, self.areaUnderPR = float(areas[0]), float(areas[1])

    def table(self):
        """(thresholds, cumPos, cumNeg) on the host: the G written rows."""
        G = self.G
        if self.thresholds is None or G == 0:
            return np.zeros(0), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
        return (self.thresholds[:G].cpu().numpy(), self.cumPos[:G].cpu().numpy(), self.cumNeg[:G].cpu().numpy())


EMPTY = ((0, 0, 0, 0), (float("nan"), 0.0))


def alloc_outputs(torch, dev, n: int):
    """The output tensors of a device call over n pairs: thresholds, cumPos, cumNeg [n] and one
    buffer of {summary[4] int64, areas[2] double}."""
    thr = torch.empty(max(n, 1), dtype=torch.float64, device=dev)
    cp = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
    cn = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
    small = torch.zeros(6, dtype=torch.int64, device=dev)
    return thr, cp, cn, small


def read_outputs(thr, cp, cn, small) -> DeviceCounts:
    """Copies the 48 bytes of summary and areas (waits for the call on the current stream)."""
    h = small.cpu().numpy()
    return DeviceCounts(thr, cp, cn, h[:4], h[4:].view(np.float64))


def counts_of_tensors(ctx, torch, stream, scores, labels) -> DeviceCounts:
    """psgd_binary_counts_device over two device tensors of doubles, on `stream` (which is current)."""
    n = int(scores.shape[0])
    thr, cp, cn, small = alloc_outputs(torch, scores.device, n)
    ctx.binary_counts_device(scores.data_ptr() if n else None, labels.data_ptr() if n else None, n,
                             thr.data_ptr(), cp.data_ptr(), cn.data_ptr(), small.data_ptr(),
                             small.data_ptr() + 32, stream.cuda_stream)
    return read_outputs(thr, cp, cn, small)


def _vector(torch, a, dev, what):
    if torch.is_tensor(a):
        t = a.detach().to(device=dev, dtype=torch.float64).contiguous()
    else:
        t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
    if t.dim() != 1:
        raise IllegalArgumentException(f"requirement failed: {what} must be one-dimensional, got shape {tuple(t.shape)}")
    return t


def _length(a):
    shape = tuple(a.shape) if hasattr(a, "shape") else np.asarray(a).shape
    if len(shape) != 1:
        raise IllegalArgumentException(f"requirement failed: scores and labels must be one-dimensional, got shape {shape}")
    return int(shape[0])


class BinaryClassificationMetrics:
    """Evaluator for binary classification: BinaryClassificationMetrics(scoreAndLabels, numBins = 0).

    scores and labels are host arrays or device tensors of equal length; a row is positive when
    label > 0.5. Scores are keys in java.lang.Double.compare order (-0.0 < 0.0); NaN scores are
    outside the contract. numBins > 0 (MLlib's down-sampling of the curves) is not built."""

    def __init__(self, scores, labels, numBins: int = 0):
        _check_bins(numBins)
        if _length(scores) != _length(labels):
            raise IllegalArgumentException(
                f"requirement failed: scores and labels differ in length: {_length(scores)} and {_length(labels)}")
        import torch
        from .optimization import get_context
        if not torch.cuda.is_available():
            raise N.DeviceError("BinaryClassificationMetrics needs a visible MI355X (torch.cuda.is_available() is False)")
        dev = scores.device if torch.is_tensor(scores) and scores.is_cuda else torch.device(
            "cuda", torch.cuda.current_device())
        ctx = get_context(dev.index if dev.index is not None else torch.cuda.current_device())
        caller = torch.cuda.current_stream(dev)
        stream = torch.cuda.Stream(device=dev)   # a real handle: NULL would select the library's own stream
        stream.wait_stream(caller)
        with torch.cuda.stream(stream):
            s, y = _vector(torch, scores, dev, "scores"), _vector(torch, labels, dev, "labels")
            self._set(counts_of_tensors(ctx, torch, stream, s, y))
        caller.wait_stream(stream)

    # construction ------------------------------------------------------------------------------
    def _set(self, counts):
        self._counts = counts
        self._table = None

    @classmethod
    def _of(cls, counts) -> "BinaryClassificationMetrics":
        self = cls.__new__(cls)
        self._set(counts)
        return self

    @classmethod
    def fromCounts(cls, thresholds, cumPos, cumNeg) -> "BinaryClassificationMetrics":
        """From a table already on the host (descending thresholds with their cumulative counts):
        the summary and the areas by the definitions, in Python integers and fp64 left to right.
        Needs no device."""
        thr = np.ascontiguousarray(thresholds, dtype=np.float64)
        cp = np.ascontiguousarray(cumPos, dtype=np.int64)
        cn = np.ascontiguousarray(cumNeg, dtype=np.int64)
        if not (thr.ndim == cp.ndim == cn.ndim == 1 and len(thr) == len(cp) == len(cn)):
            raise IllegalArgumentException("requirement failed: thresholds, cumPos and cumNeg differ in length")
        if len(cp) and (np.any(np.diff(cp) < 0) or np.any(np.diff(cn) < 0) or cp[0] < 0 or cn[0] < 0
                        or np.any(np.diff(cp + cn) <= 0) or cp[0] + cn[0] <= 0):
            raise IllegalArgumentException("requirement failed: cumulative counts must grow with every group")
        G = len(thr)
        P, Nn = (int(cp[-1]), int(cn[-1])) if G else (0, 0)
        num, pp, pn = 0, 0, 0
        area, rec_prev, prec_prev = 0.0, 0.0, 1.0
        for g in range(G):
            p, q = int(cp[g]), int(cn[g])
            num += (q - pn) * (p + pp)
            rec, prec = (p / P if P else 0.0), p / (p + q)
            area = area + (rec - rec_prev) * (prec + prec_prev) / 2.0
            pp, pn, rec_prev, prec_prev = p, q, rec, prec
        self = cls._of(DeviceCounts(None, None, None, (G, P, Nn, num), (roc_area(num, P, Nn), area)))
        self._table = (thr, cp, cn)
        return self

    @classmethod
    def fromModel(cls, data, weights, score: str = "margin", engine=None) -> "BinaryClassificationMetrics":
        """The metrics of a linear model on `data`: every row's score is its raw margin x . w
        (score="margin": what a model with its threshold cleared predicts for an SVM) or
        sigmoid(x . w) (score="probability": a LogisticRegressionModel's), the labels are the data's.
        The rows are scored where they are registered; with several ranks each scores its own
        partitions, the ranks all-gather scores and labels, and every rank holds the same result."""
        if score not in ("margin", "probability"):
            raise IllegalArgumentException(f"requirement failed: score must be 'margin' or 'probability', got {score!r}")
        if data.num_partitions == 0:
            return cls._of(DeviceCounts(None, None, None, *EMPTY))
        if engine is None:
            from .optimization import HipEngine, _dist
            rank, world, _ = _dist()
            engine = HipEngine(data, rank, world)
        return cls._of(engine.binary_counts(weights, score))

    # the table ---------------------------------------------------------------------------------
    def _host(self):
        if self._table is None:
            self._table = self._counts.table()
        return self._table

    @property
    def numPositives(self) -> int:
        return self._counts.P

    @property
    def numNegatives(self) -> int:
        return self._counts.N

    @property
    def numThresholds(self) -> int:
        return self._counts.G

    @property
    def rocNumerator(self) -> int:
        return self._counts.rocNumerator

    def cumulativeCounts(self):
        """(thresholds, cumPos, cumNeg): per distinct score in descending order, the positives and
        negatives scored at or above it."""
        return self._host()

    def thresholds(self) -> np.ndarray:
        return self._host()[0]

    def _rates(self):
        _, cp, cn = self._host()
        P, Nn = self._counts.P, self._counts.N
        cpf, cnf = cp.astype(np.float64), cn.astype(np.float64)
        recall = cpf / float(P) if P else np.zeros(len(cp))
        fpr = cnf / float(Nn) if Nn else np.zeros(len(cn))
        precision = cpf / (cpf + cnf)
        return recall, fpr, precision

    def roc(self) -> np.ndarray:
        """The points (false positive rate, recall), (0, 0) before them and (1, 1) after."""
        recall, fpr, _ = self._rates()
        return np.concatenate([[[0.0, 0.0]], np.stack([fpr, recall], axis=1), [[1.0, 1.0]]])

    def pr(self) -> np.ndarray:
        """The points (recall, precision) with (0.0, 1.0) before them (the 1.6.1 form)."""
        recall, _, precision = self._rates()
        return np.concatenate([[[0.0, 1.0]], np.stack([recall, precision], axis=1)])

    def precisionByThreshold(self) -> np.ndarray:
        return np.stack([self.thresholds(), self._rates()[2]], axis=1)

    def recallByThreshold(self) -> np.ndarray:
        return np.stack([self.thresholds(), self._rates()[0]], axis=1)

    def fMeasureByThreshold(self, beta: float = 1.0) -> np.ndarray:
        """(1 + beta^2) p r / (beta^2 p + r) per threshold; 0.0 where p + r = 0."""
        r, _, p = self._rates()
        b2 = float(beta) * float(beta)
        den = b2 * p + r
        f = np.where(p + r == 0.0, 0.0, (1.0 + b2) * p * r / np.where(den == 0.0, 1.0, den))
        return np.stack([self.thresholds(), f], axis=1)

    def areaUnderROC(self) -> float:
        """The trapezoid area of roc(), exact: rocNumerator / (2 P N) in integers, divided once."""
        return self._counts.areaUnderROC

    def areaUnderPR(self) -> float:
        """The trapezoid area of pr(), summed in fp64 in a fixed order."""
        return self._counts.areaUnderPR


def _check_bins(numBins):
    if numBins < 0:
        raise IllegalArgumentException("requirement failed: numBins must be nonnegative")
    if numBins > 0:
        raise UnsupportedOperationException(
            "numBins > 0 is not built: MLlib's down-sampling of the curves follows its range partitioning")


class MulticlassMetrics:
    """Evaluator for multiclass classification: MulticlassMetrics(predictionAndLabels).

    predictions and labels are host arrays or device tensors of equal length holding classes as
    doubles (whole numbers in [0, numClasses)); numClasses defaults to the largest value + 1, found
    on the device. The pairs are counted on the device into a K x K table of int64 (rows actual,
    columns predicted; psgd_confusion_device, integer atomics: exact); every member below is
    arithmetic on that table on the host. A value that is not a whole number in [0, numClasses)
    raises IllegalArgumentException.

    The definitions are this project's restatement of MLlib 1.6.1's MulticlassMetrics, not pinned to
    its source: `labels` are the classes that occur as a true label, ascending (MLlib takes them
    from labelCountByClass); confusionMatrix() is over those only, so a predicted class that never
    occurs as a label has no column, but it still counts as a false positive of its class and as a
    miss of the row's label. A zero denominator gives 0.0 where MLlib guards it (precision with
    tp + fp = 0, fMeasure with p + r = 0). The per-label members raise for a class that never occurs
    as a label (MLlib: NoSuchElementException)."""

    def __init__(self, predictions, labels, numClasses=None):
        if _length(predictions) != _length(labels):
            raise IllegalArgumentException(
                f"requirement failed: predictions and labels differ in length: {_length(predictions)} and "
                f"{_length(labels)}")
        import torch
        from .optimization import get_context
        if not torch.cuda.is_available():
            raise N.DeviceError("MulticlassMetrics needs a visible MI355X (torch.cuda.is_available() is False)")
        dev = predictions.device if torch.is_tensor(predictions) and predictions.is_cuda else torch.device(
            "cuda", torch.cuda.current_device())
        ctx = get_context(dev.index if dev.index is not None else torch.cuda.current_device())
        caller = torch.cuda.current_stream(dev)
        stream = torch.cuda.Stream(device=dev)   # a real handle: NULL would select the library's own stream
        stream.wait_stream(caller)
        with torch.cuda.stream(stream):
            p, y = _vector(torch, predictions, dev, "predictions"), _vector(torch, labels, dev, "labels")
            n = int(p.shape[0])
            if numClasses is None:
                top = float(torch.maximum(p.max(), y.max()).item()) if n else 0.0
                if not np.isfinite(top) or top < 0.0:
                    raise IllegalArgumentException(f"requirement failed: classes must be whole numbers >= 0, got {top!r}")
                numClasses = int(top) + 1
            K = int(numClasses)
            if K < 1:
                raise IllegalArgumentException(f"requirement failed: numClasses must be positive but got {K}")
            buf = torch.zeros(1 + K * K, dtype=torch.int64, device=dev)   # {n_bad, counts}
            ctx.confusion_device(p.data_ptr() if n else None, y.data_ptr() if n else None, n, K, buf.data_ptr() + 8,
                                 buf.data_ptr(), stream.cuda_stream)
            h = buf.cpu().numpy()
        caller.wait_stream(stream)
        if int(h[0]) > 0:
            raise IllegalArgumentException(
                f"requirement failed: {int(h[0])} (prediction, label) pairs hold a value that is not a whole "
                f"number in [0, {K})")
        self._set(h[1:].reshape(K, K))

    def _set(self, table):
        t = np.ascontiguousarray(table, dtype=np.int64)
        if t.ndim != 2 or t.shape[0] != t.shape[1] or np.any(t < 0):
            raise IllegalArgumentException("requirement failed: the confusion table must be square and non-negative")
        self.table = t                                   # [K, K] over every class
        self.numClasses = int(t.shape[0])
        self._label_count = t.sum(axis=1)                # labelCountByClass
        self._pred_count = t.sum(axis=0)
        self._n = int(t.sum())
        self.labels = np.flatnonzero(self._label_count > 0).astype(np.float64)

    @classmethod
    def fromTable(cls, table) -> "MulticlassMetrics":
        """From a K x K table already on the host (rows actual, columns predicted). Needs no device."""
        self = cls.__new__(cls)
        self._set(table)
        return self

    @classmethod
    def fromModel(cls, data, weights, numClasses: int, *, engine=None) -> "MulticlassMetrics":
        """The metrics of a multinomial logistic model ((numClasses - 1) * num_features weights) on
        `data`: the rows are scored where they are registered, the classes stay in device scratch
        and the labels are the registry's (psgd_confusion_model_device). With several ranks each
        counts its own partitions and the tables are added."""
        from .optimization import HipEngine, _dist, _weights_size, check_multinomial_weights, check_num_classes
        K = check_num_classes(numClasses)
        if data.num_partitions == 0:
            return cls.fromTable(np.zeros((K, K), dtype=np.int64))
        check_multinomial_weights(K, data.num_features, _weights_size(weights))
        if engine is None:
            rank, world, _ = _dist()
            engine = HipEngine(data, rank, world)
        return cls.fromTable(engine.confusion(K, weights))

    # the table ---------------------------------------------------------------------------------
    def confusionMatrix(self) -> np.ndarray:
        """Rows actual, columns predicted, over `labels` only."""
        idx = self.labels.astype(np.int64)
        return self.table[np.ix_(idx, idx)].copy()

    def _class(self, label) -> int:
        c = int(label)
        if c != label or not (0 <= c < self.numClasses) or self._label_count[c] == 0:
            raise IllegalArgumentException(f"requirement failed: class {label!r} does not occur as a label")
        return c

    def _tp(self, c: int) -> int:
        return int(self.table[c, c])

    def _fp(self, c: int) -> int:
        return int(self._pred_count[c]) - self._tp(c)

    # per label -----------------------------------------------------------------------------------
    def truePositiveRate(self, label) -> float:
        return self.recall(label)

    def falsePositiveRate(self, label) -> float:
        c = self._class(label)
        den = self._n - int(self._label_count[c])
        with np.errstate(divide="ignore", invalid="ignore"):
            return float(np.float64(self._fp(c)) / np.float64(den))

    def precision(self, label=None) -> float:
        if label is None:
            return self._accuracy()
        c = self._class(label)
        tp, fp = self._tp(c), self._fp(c)
        return 0.0 if tp + fp == 0 else tp / (tp + fp)

    def recall(self, label=None) -> float:
        if label is None:
            return self._accuracy()
        c = self._class(label)
        return self._tp(c) / int(self._label_count[c])

    def fMeasure(self, label=None, beta: float = 1.0) -> float:
        if label is None:
            return self._accuracy()
        p, r = self.precision(label), self.recall(label)
        b2 = float(beta) * float(beta)
        return 0.0 if p + r == 0 else (1 + b2) * p * r / (b2 * p + r)

    # over all rows -------------------------------------------------------------------------------
    def _accuracy(self) -> float:
        """Correct predictions / rows (NaN without rows: 0.0 / 0)."""
        return float(np.trace(self.table)) / self._n if self._n else float("nan")

    def _weighted(self, member) -> float:
        total = 0.0
        for label in self.labels:
            total = total + member(label) * int(self._label_count[int(label)]) / self._n
        return total

    @property
    def weightedTruePositiveRate(self) -> float:
        return self.weightedRecall

    @property
    def weightedFalsePositiveRate(self) -> float:
        return self._weighted(self.falsePositiveRate)

    @property
    def weightedRecall(self) -> float:
        return self._weighted(self.recall)

    @property
    def weightedPrecision(self) -> float:
        return self._weighted(self.precision)

    def weightedFMeasure(self, beta: float = 1.0) -> float:
        return self._weighted(lambda label: self.fMeasure(label, beta))
