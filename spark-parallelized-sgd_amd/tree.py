"""MLlib 1.6.1 tree.DecisionTree.trainClassifier for dense rows with continuous features, trained level by
level over the engine's device copy of the rows:

  model = DecisionTree.trainClassifier(data, numClasses=3, maxDepth=4, maxBins=32)
  model.numNodes, model.depth            # MLlib's counts: a lone root has depth 0
  model.predict(data)                    # per-partition device int32 tensors
  print(model.toDebugString())

find_splits picks each feature's thresholds on the host from a sample of the rows; the engine keeps a binned
copy of the rows (HipEngine.tree_bin: one byte a feature, a quarter of f32 rows), and a level is three
passes on the device (tree_histogram, tree_best_split, tree_route; include/psgd.h has the definitions). The
host reads back one small record a slot a level, names the nodes as MLlib does (root 1, children 2 i and
2 i + 1) and builds the next frontier: a child that is pure or at maxDepth is a finished leaf and gets no
slot; its class counts are its parent's L or tot - L, so no pass is spent on it. A frontier whose 64-bit
table exceeds scratchBudget bytes is processed in groups of slots (psgd_tree_plan).

The row sample of find_splits is this project's convention, as in KMeans: every row while n <=
max(maxBins^2, 10,000), else that many distinct positions from numpy.random.default_rng(seed), read as the
engine registered them. Regression trees, categorical features and forests are not built."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

from ._native import (TREE_IMPURITIES, TREE_MAX_BINS, TREE_MAX_CLASSES, IllegalArgumentException,
                      UnsupportedOperationException, tree_plan)
from .data import PartitionedData


class TreeBins(NamedTuple):
    """HipEngine.tree_bin's result: the engine-owned binned copy of the rows and what was binned against."""
    bins: object          # uint8 [local rows, pitch] on the device; the pad bytes are 0
    labels: object        # uint8 [local rows]: the label, 255 when it is no whole number in [0, 255)
    thresholds: object    # f64 [d, maxBins - 1] on the device
    nbins: object         # int32 [d] on the device
    max_bins: int


def _engine_for(data: PartitionedData, engine):
    if engine is not None:
        return engine
    from .optimization import HipEngine, _dist
    rank, world, _ = _dist()
    return HipEngine(data, rank, world)


def _check_dense(data: PartitionedData):
    from .data import CsrPartition, DeviceCsrPartition
    if any(isinstance(p, (CsrPartition, DeviceCsrPartition)) for p in data.partitions):
        raise UnsupportedOperationException("the decision tree needs dense rows (the partitions are CSR)")


def feature_splits(values: np.ndarray, maxBins: int) -> np.ndarray:
    """The thresholds of one feature from its sampled values: every distinct value when there are at most
    maxBins - 1 of them, else MLlib's stride walk over the sorted value counts (a value is taken when the
    running count passes the next multiple of n / maxBins more closely before it than after it)."""
    vals, counts = np.unique(np.asarray(values, dtype=np.float64), return_counts=True)
    num = maxBins - 1
    if len(vals) <= num:
        return vals
    stride = len(values) / (num + 1)
    out, current, target = [], int(counts[0]), stride
    for i in range(1, len(vals)):
        previous = current
        current += int(counts[i])
        if abs(previous - target) < abs(current - target):
            out.append(vals[i - 1])
            target += stride
    return np.array(out[:num], dtype=np.float64)


def find_splits(data: PartitionedData, maxBins: int = 32, seed=None, *, engine=None):
    """(thresholds [d, maxBins - 1] padded with +Inf, nbins [d] int32) for HipEngine.tree_bin."""
    if isinstance(maxBins, (bool, np.bool_)) or not 2 <= int(maxBins) <= TREE_MAX_BINS:
        raise IllegalArgumentException(f"requirement failed: maxBins must be in [2, {TREE_MAX_BINS}] (got {maxBins!r})")
    maxBins = int(maxBins)
    engine = _engine_for(data, engine)
    counts = getattr(data, "partition_counts", None)
    n = int(np.sum(counts)) if counts is not None else data.count()
    if n < 1:
        raise IllegalArgumentException("requirement failed: Cannot find splits on data without rows.")
    want = max(maxBins * maxBins, 10000)
    positions = np.arange(n) if n <= want else np.sort(np.random.default_rng(seed).choice(n, size=want, replace=False))
    rows = np.asarray(engine.registered_rows(positions), dtype=np.float64)
    d = rows.shape[1]
    thr = np.full((d, maxBins - 1), np.inf)
    nbins = np.ones(d, dtype=np.int32)
    for f in range(d):
        t = feature_splits(rows[:, f], maxBins)
        thr[f, : len(t)] = t
        nbins[f] = len(t) + 1
    return thr, nbins


def _impurity(counts: np.ndarray, kind: str) -> float:
    n = float(counts.sum())
    if n <= 0.0:
        return 0.0
    q = counts[counts > 0] / n
    return float(1.0 - np.sum(q * q)) if kind == "gini" else float(-np.sum(q * np.log(q) / np.log(2.0)))


class DecisionTreeModel:
    """A trained classifier as arrays, node 0 the root and a node's children after it: id (MLlib's), feature
    (-1: a leaf), threshold, left, right (indices into the arrays), prediction, probability, gain, impurity
    and counts [numNodes, numClasses]."""

    def __init__(self, nodes: dict, numClasses: int, numFeatures: int):
        self.nodes, self.numClasses, self.numFeatures = nodes, int(numClasses), int(numFeatures)
        for key, value in nodes.items():
            setattr(self, key, value)

    @property
    def numNodes(self) -> int:
        return int(len(self.nodes["id"]))

    @property
    def depth(self) -> int:
        return int(np.floor(np.log2(self.nodes["id"].max())))

    def predict(self, data: PartitionedData, *, engine=None):
        """The predicted class of every row: one device int32 tensor per partition of `data` (empty for another
        rank's partitions)."""
        if data.num_features != self.numFeatures:
            raise IllegalArgumentException(
                f"requirement failed: vector sizes do not match: Expected {self.numFeatures} but found {data.num_features}")
        _check_dense(data)
        engine = _engine_for(data, engine)
        cls, _ = engine.tree_predict(self.nodes)
        out, at = [], 0
        for p, part in enumerate(data.partitions):
            n = part.n_rows if engine.lo <= p < engine.hi else 0
            out.append(cls[at: at + n])
            at += n
        return out

    def toDebugString(self) -> str:
        lines = [f"DecisionTreeModel classifier of depth {self.depth} with {self.numNodes} nodes"]

        def walk(i: int, indent: int):
            pad = " " * indent
            if self.nodes["feature"][i] < 0:
                lines.append(f"{pad}Predict: {float(self.nodes['prediction'][i])}")
                return
            f, t = int(self.nodes["feature"][i]), float(self.nodes["threshold"][i])
            lines.append(f"{pad}If (feature {f} <= {t})")
            walk(int(self.nodes["left"][i]), indent + 1)
            lines.append(f"{pad}Else (feature {f} > {t})")
            walk(int(self.nodes["right"][i]), indent + 1)
        walk(0, 1)
        return "\n".join(lines) + "\n"


class DecisionTree:
    """MLlib 1.6.1 DecisionTree (the module docstring has the loop)."""

    @staticmethod
    def trainClassifier(data: PartitionedData, numClasses: int, categoricalFeaturesInfo=None, impurity: str = "gini",
                        maxDepth: int = 5, maxBins: int = 32, minInstancesPerNode: int = 1, minInfoGain: float = 0.0,
                        seed=None, *, engine=None, scratchBudget: int = 0) -> DecisionTreeModel:
        if categoricalFeaturesInfo:
            raise UnsupportedOperationException("categorical features are not built: categoricalFeaturesInfo must be empty")
        if impurity == "variance":
            raise UnsupportedOperationException("regression trees are not built: impurity is 'gini' or 'entropy'")
        if impurity not in TREE_IMPURITIES:
            raise IllegalArgumentException(f"requirement failed: unknown impurity {impurity!r}")
        K = numClasses
        if isinstance(K, (bool, np.bool_)) or not isinstance(K, (int, np.integer)) or K < 2:
            raise IllegalArgumentException(f"requirement failed: numClasses must be an integer >= 2 (got {K!r})")
        if K > TREE_MAX_CLASSES:
            raise UnsupportedOperationException(f"a tree takes at most {TREE_MAX_CLASSES} classes (got {K})")
        if isinstance(maxDepth, (bool, np.bool_)) or int(maxDepth) < 0:
            raise IllegalArgumentException(f"requirement failed: maxDepth must be nonnegative but got {maxDepth!r}")
        if int(maxDepth) > 30:
            raise UnsupportedOperationException(f"DecisionTree currently only supports maxDepth <= 30, but was given {maxDepth}")
        if int(maxBins) > TREE_MAX_BINS:
            raise UnsupportedOperationException(f"a tree takes at most {TREE_MAX_BINS} bins (got {maxBins}): a bin is a byte")
        if int(minInstancesPerNode) < 1 or not float(minInfoGain) >= 0.0:
            raise IllegalArgumentException("requirement failed: minInstancesPerNode must be >= 1 and minInfoGain >= 0")
        _check_dense(data)
        if data.num_partitions == 0:
            raise IllegalArgumentException("requirement failed: Cannot train a tree on data without partitions.")
        K, maxDepth, maxBins = int(K), int(maxDepth), int(maxBins)
        engine = _engine_for(data, engine)
        thr, nbins = find_splits(data, maxBins, seed, engine=engine)
        bins = engine.tree_bin(thr, nbins)
        slots = engine.tree_slots()
        d = data.num_features
        done = {}                       # MLlib id -> the node's fields
        frontier = [(1, None)]          # (id, class counts when the parent's record gave them)
        level = 0
        while frontier:
            A = len(frontier)
            plan = tree_plan("f32", d, maxBins, K, A, 0, scratchBudget)
            recs = []
            for s0 in range(0, A, plan["group_slots"]):
                hist = engine.tree_histogram(bins, slots, K, (s0, min(plan["group_slots"], A - s0)))
                recs.append(engine.tree_best_split(hist, bins, impurity, minInstancesPerNode, minInfoGain).cpu().numpy())
            rec = np.concatenate(recs)
            table = np.full((A, 4), -1, dtype=np.int32)
            nxt = []
            for s, (nid, _) in enumerate(frontier):
                r = rec[s]
                tot, L = r[6: 6 + K], r[6 + K: 6 + 2 * K]
                split = r[0] >= 0 and level < maxDepth
                done[nid] = dict(feature=int(r[0]) if split else -1, threshold=float(r[2]) if split else 0.0,
                                 gain=float(r[3]) if split else 0.0, impurity=float(r[4]), counts=tot.copy(),
                                 bin=int(r[1]) if split else -1)
                if not split:
                    continue
                table[s, 0], table[s, 1] = int(r[0]), int(r[1])
                for side, cnt in ((0, L), (1, tot - L)):
                    cid = 2 * nid + side
                    if level + 1 >= maxDepth or np.count_nonzero(cnt) <= 1:   # a finished leaf: no slot
                        done[cid] = dict(feature=-1, threshold=0.0, gain=0.0, impurity=_impurity(cnt, impurity),
                                         counts=cnt.copy(), bin=-1)
                    else:
                        table[s, 2 + side] = len(nxt)
                        nxt.append((cid, cnt))
            if nxt:
                engine.tree_route(bins, slots, table)
            frontier, level = nxt, level + 1
        return DecisionTreeModel(_node_arrays(done, K), K, d)


def _node_arrays(done: dict, K: int) -> dict:
    ids = sorted(done)                  # MLlib ids ascend level by level: a child lies after its parent
    at = {nid: i for i, nid in enumerate(ids)}
    n = len(ids)
    out = dict(id=np.array(ids, dtype=np.int64), feature=np.full(n, -1, dtype=np.int32), bin=np.full(n, -1, dtype=np.int32),
               threshold=np.zeros(n), left=np.zeros(n, dtype=np.int32), right=np.zeros(n, dtype=np.int32),
               prediction=np.zeros(n, dtype=np.int32), probability=np.zeros(n), gain=np.zeros(n), impurity=np.zeros(n),
               counts=np.zeros((n, K)))
    for nid, node in done.items():
        i = at[nid]
        for key in ("feature", "bin", "threshold", "gain", "impurity", "counts"):
            out[key][i] = node[key]
        cnt = node["counts"]
        out["prediction"][i] = int(np.argmax(cnt))          # the smallest class of the largest count
        out["probability"][i] = cnt.max() / cnt.sum() if cnt.sum() > 0 else 0.0
        if node["feature"] >= 0:
            out["left"][i], out["right"][i] = at[2 * nid], at[2 * nid + 1]
    return out
