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
engine registered them. Categorical features are not built.

DecisionTree.trainRegressor(data, maxDepth=5, maxBins=32) trains a variance tree over the same binned rows.
The labels become fixed-point targets once (HipEngine.tree_targets: q = rint((y - ymin) 2^s) below 2^30, 4 bytes
a row on the device; include/psgd.h has the definition), and a level is the node moments of every open node
(tree_moments: n, sum q and sum q^2 as integers), then, for the nodes that may split, the {count, sum}
histogram and the variance split (tree_histogram_reg, tree_best_split_reg) and the routing pass. The host
forms a node's value ymin + S / (n 2^s) and its variance from the integers as exact rationals, rounded once;
a node at maxDepth, of variance exactly 0 or of fewer than 2 minInstancesPerNode rows is a leaf and gets no
histogram pass (one routing pass closes up the slots of the others). Every child of a split gets a slot. The
model's algo is "Regression", its prediction float64, its counts replaced by n; predict gives float64 tensors.

RandomForest.trainClassifier trains numTrees such trees on bagged rows, each node looking at a random subset
of the features (include/psgd.h has the bag weight; forest_cut, forest_subset_size and forest_subset are the
host's part of the definitions):

  forest = RandomForest.trainClassifier(data, numClasses=3, numTrees=20, seed=7)
  forest.trees, forest.numTrees, forest.totalNumNodes
  forest.predict(data)                   # the trees' majority vote, ties to the lowest class

The rows are binned once; the trees train in groups of as many as slotBudget bytes of per-tree slots allow, a
group a level at a time through the forest passes (HipEngine.forest_histogram reads a row once for all trees
of a node sub-group, adds the bag weight, and counts only the node's feature subset). With more than one
rank, pass a seed: seed=None draws one on each host."""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np

from ._native import (TREE_IMPURITIES, TREE_MAX_BINS, TREE_MAX_CLASSES, IllegalArgumentException,
                      UnsupportedOperationException, forest_plan, tree_plan)
from .data import PartitionedData


class TreeBins(NamedTuple):
    """HipEngine.tree_bin's result: the engine-owned binned copy of the rows and what was binned against."""
    bins: object          # uint8 [local rows, pitch] on the device; the pad bytes are 0
    labels: object        # uint8 [local rows]: the label, 255 when it is no whole number in [0, 255)
    thresholds: object    # f64 [d, maxBins - 1] on the device
    nbins: object         # int32 [d] on the device
    max_bins: int


class TreeTargets(NamedTuple):
    """HipEngine.tree_targets' result: the rows' fixed-point regression targets and their unit."""
    q: object             # int32 [local rows] on the device: rint((y - ymin) 2^s), 0 .. 2^30
    ymin: float           # the smallest label over all ranks
    s: int                # a target's unit is 2^-s


def target_scale(ymin: float, ymax: float) -> int:
    """The largest integer s with (ymax - ymin) 2^s < 2^30, the difference as fp64 rounds it; 0 for a constant label."""
    r = float(ymax) - float(ymin)
    return 30 - math.frexp(r)[1] if r > 0.0 else 0       # r = m 2^e with 1/2 <= m < 1: m 2^30 < 2^30 <= m 2^31


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
    and counts [numNodes, numClasses]. A regression model (algo "Regression", numClasses 0) has a float64
    prediction, the same values in probability (the member the prediction kernel writes out), and the nodes' row
    counts n in place of counts."""

    def __init__(self, nodes: dict, numClasses: int, numFeatures: int, algo: str = "Classification"):
        self.nodes, self.numClasses, self.numFeatures, self.algo = nodes, int(numClasses), int(numFeatures), algo
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
        rank's partitions). A regression model gives float64 tensors of the leaves' values."""
        if data.num_features != self.numFeatures:
            raise IllegalArgumentException(
                f"requirement failed: vector sizes do not match: Expected {self.numFeatures} but found {data.num_features}")
        _check_dense(data)
        engine = _engine_for(data, engine)
        if self.algo == "Regression":
            nodes = dict(self.nodes, prediction=np.zeros(self.numNodes, dtype=np.int32))
            cls = engine.tree_predict(nodes, probability=True)[1]
        else:
            cls, _ = engine.tree_predict(self.nodes)
        out, at = [], 0
        for p, part in enumerate(data.partitions):
            n = part.n_rows if engine.lo <= p < engine.hi else 0
            out.append(cls[at: at + n])
            at += n
        return out

    def toDebugString(self) -> str:
        kind = "regressor" if self.algo == "Regression" else "classifier"
        lines = [f"DecisionTreeModel {kind} of depth {self.depth} with {self.numNodes} nodes"]

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


def _check_train_args(data, numClasses, categoricalFeaturesInfo, impurity, maxDepth, maxBins, minInstancesPerNode,
                      minInfoGain, regression=False):
    """trainClassifier's refusals, the tree's and the forest's alike; regression: trainRegressor's (no classes)."""
    if categoricalFeaturesInfo:
        raise UnsupportedOperationException("categorical features are not built: categoricalFeaturesInfo must be empty")
    K = numClasses
    if regression:
        if impurity != "variance":
            raise IllegalArgumentException(f"requirement failed: a regression tree's impurity is 'variance' (got {impurity!r})")
    else:
        if impurity == "variance":
            raise UnsupportedOperationException("a classifier's impurity is 'gini' or 'entropy': 'variance' is trainRegressor's")
        if impurity not in TREE_IMPURITIES:
            raise IllegalArgumentException(f"requirement failed: unknown impurity {impurity!r}")
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


class DecisionTree:
    """MLlib 1.6.1 DecisionTree (the module docstring has the loop)."""

    @staticmethod
    def trainClassifier(data: PartitionedData, numClasses: int, categoricalFeaturesInfo=None, impurity: str = "gini",
                        maxDepth: int = 5, maxBins: int = 32, minInstancesPerNode: int = 1, minInfoGain: float = 0.0,
                        seed=None, *, engine=None, scratchBudget: int = 0) -> DecisionTreeModel:
        _check_train_args(data, numClasses, categoricalFeaturesInfo, impurity, maxDepth, maxBins, minInstancesPerNode,
                          minInfoGain)
        K = numClasses
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

    @staticmethod
    def trainRegressor(data: PartitionedData, categoricalFeaturesInfo=None, impurity: str = "variance", maxDepth: int = 5,
                       maxBins: int = 32, minInstancesPerNode: int = 1, minInfoGain: float = 0.0, seed=None, *, engine=None,
                       scratchBudget: int = 0) -> DecisionTreeModel:
        """A level is the node moments of every open node, then the {count, sum} histogram and the variance split
        of those that may split (the module docstring has the loop)."""
        _check_train_args(data, 0, categoricalFeaturesInfo, impurity, maxDepth, maxBins, minInstancesPerNode, minInfoGain,
                          regression=True)
        maxDepth, maxBins, minInst = int(maxDepth), int(maxBins), int(minInstancesPerNode)
        counts = getattr(data, "partition_counts", None)
        if (int(np.sum(counts)) if counts is not None else data.count()) >= 1 << 33:
            raise UnsupportedOperationException("a regression tree takes fewer than 2^33 rows: its 64-bit sums must stay below 2^63")
        engine = _engine_for(data, engine)
        thr, nbins = find_splits(data, maxBins, seed, engine=engine)
        bins = engine.tree_bin(thr, nbins)
        targets = engine.tree_targets()
        slots = engine.tree_slots()
        d = data.num_features
        done = {}                       # MLlib id -> the node's fields
        frontier = [1]                  # the open nodes' ids, in slot order
        level = 0
        while frontier:
            mom_dev = engine.tree_moments(targets, slots, len(frontier))
            mom = mom_dev.cpu().numpy()
            keep = []                   # the slots that may split
            for s, nid in enumerate(frontier):
                n, S, S2 = int(mom[s, 0]), int(mom[s, 1]), (int(mom[s, 2]) << 30) + int(mom[s, 3])
                done[nid] = dict(_regression_stats(n, S, S2, targets.ymin, targets.s), feature=-1, bin=-1, threshold=0.0,
                                 gain=0.0)
                if level < maxDepth and n * S2 != S * S and n >= 2 * minInst:
                    keep.append(s)
            if not keep:
                break
            if len(keep) < len(frontier):   # the leaves' rows leave, the others' slots close up: one routing pass
                table = np.full((len(frontier), 4), -1, dtype=np.int32)
                for new, s in enumerate(keep):
                    table[s] = (0, 255, new, new)       # (every bin is <= 255: "left")
                engine.tree_route(bins, slots, table)
                frontier = [frontier[s] for s in keep]
                mom_dev = mom_dev[keep]
            A = len(frontier)
            plan = tree_plan("f32", d, maxBins, 0, A, 0, scratchBudget)
            recs = []
            for s0 in range(0, A, plan["group_slots"]):
                g = min(plan["group_slots"], A - s0)
                hist = engine.tree_histogram_reg(bins, targets, slots, (s0, g))
                recs.append(engine.tree_best_split_reg(hist, mom_dev[s0: s0 + g], bins, targets, minInst, minInfoGain).cpu().numpy())
            rec = np.concatenate(recs)
            table = np.full((A, 4), -1, dtype=np.int32)
            nxt = []
            for s, nid in enumerate(frontier):
                r = rec[s]
                if r[0] < 0:
                    continue
                done[nid].update(feature=int(r[0]), bin=int(r[1]), threshold=float(r[2]), gain=float(r[3]))
                table[s] = (int(r[0]), int(r[1]), len(nxt), len(nxt) + 1)    # both children get slots
                nxt += [2 * nid, 2 * nid + 1]
            if nxt:
                engine.tree_route(bins, slots, table)
            frontier, level = nxt, level + 1
        return DecisionTreeModel(_regression_arrays(done), 0, d, "Regression")


def _regression_stats(n: int, S: int, S2: int, ymin: float, s: int) -> dict:
    """A node's value ymin + S / (n 2^s) and variance (n S2 - S^2) / (n 2^s)^2 from its integer moments: exact
    rationals, each rounded once."""
    from fractions import Fraction
    if n == 0:
        return dict(n=0, prediction=float(ymin), impurity=0.0)
    unit = Fraction(1 << s) if s >= 0 else Fraction(1, 1 << -s)
    return dict(n=n, prediction=float(Fraction(ymin) + Fraction(S, n) / unit),
                impurity=float(Fraction(n * S2 - S * S, n * n) / (unit * unit)))


def _regression_arrays(done: dict) -> dict:
    ids = sorted(done)                  # MLlib ids ascend level by level: a child lies after its parent
    at = {nid: i for i, nid in enumerate(ids)}
    n = len(ids)
    out = dict(id=np.array(ids, dtype=np.int64), feature=np.full(n, -1, dtype=np.int32), bin=np.full(n, -1, dtype=np.int32),
               threshold=np.zeros(n), left=np.zeros(n, dtype=np.int32), right=np.zeros(n, dtype=np.int32),
               prediction=np.zeros(n), probability=np.zeros(n), gain=np.zeros(n), impurity=np.zeros(n),
               n=np.zeros(n, dtype=np.int64))
    for nid, node in done.items():
        i = at[nid]
        for key in ("feature", "bin", "threshold", "gain", "impurity", "n", "prediction"):
            out[key][i] = node[key]
        out["probability"][i] = node["prediction"]          # (the member the prediction kernel writes out)
        if node["feature"] >= 0:
            out["left"][i], out["right"][i] = at[2 * nid], at[2 * nid + 1]
    return out


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


# ---- random forest ----------------------------------------------------------------------------------------
FOREST_STRATEGIES = ("auto", "all", "sqrt", "log2", "onethird")


class ForestFrontier(NamedTuple):
    """HipEngine.forest_frontier's result: a level's open nodes of a group of trees, on the device."""
    node_tree: object     # int32 [A]: the node's tree within the group, ascending
    tree_base: object     # int32 [G + 1]: tree t's nodes are tree_base[t] .. tree_base[t + 1] - 1
    sub: object           # int32 [A, m]: the node's feature subset, ascending


def forest_cut(numTrees: int, subsamplingRate: float = 1.0) -> np.ndarray:
    """The 15 ascending uint64 thresholds of the bag weight, cut[k] = ceil(F(k) 2^53) (at most 2^53): Poisson(rate)
    for numTrees > 1, with F summed in fp64 from term_0 = exp(-rate), term_j = term_{j-1} * rate / j; one tree
    keeps a row with probability rate (weight 0 or 1), and every row when rate is 1."""
    top = 1 << 53
    cut = [top] * 15
    if numTrees > 1:
        term, F = math.exp(-float(subsamplingRate)), 0.0
        for k in range(15):
            F += term
            cut[k] = min(top, math.ceil(F * 2.0 ** 53))
            term = term * float(subsamplingRate) / (k + 1)
    else:
        cut[0] = min(top, math.ceil((1.0 - float(subsamplingRate)) * 2.0 ** 53))
    return np.array(cut, dtype=np.uint64)


def forest_subset_size(featureSubsetStrategy: str, d: int, numTrees: int) -> int:
    """m, the features a node looks at: d ("all"), ceil(sqrt d), max(1, ceil(log2 d)), ceil(d / 3); "auto" is "all"
    for one tree, else "sqrt"."""
    kind = featureSubsetStrategy
    if kind not in FOREST_STRATEGIES:
        raise IllegalArgumentException(f"requirement failed: unknown featureSubsetStrategy {kind!r}: one of {FOREST_STRATEGIES}")
    if kind == "auto":
        kind = "all" if numTrees == 1 else "sqrt"
    d = int(d)
    if kind == "sqrt":
        r = math.isqrt(d)
        return r if r * r == d else r + 1
    if kind == "log2":
        return max(1, (d - 1).bit_length())
    return d if kind == "all" else -(-d // 3)


def forest_subset(seed: int, tree: int, nid: int, d: int, m: int) -> np.ndarray:
    """The m features (ascending, int32) that node `nid` (MLlib's id) of tree `tree` looks at: a pure function
    of its arguments."""
    if m == d:
        return np.arange(d, dtype=np.int32)
    return np.sort(np.random.default_rng([int(seed), int(tree), int(nid)]).choice(d, m, replace=False)).astype(np.int32)


class RandomForestModel:
    """The trained trees (DecisionTreeModel each); predict is their majority vote, ties to the lowest class."""

    def __init__(self, trees, numClasses: int, numFeatures: int, seed: int):
        self.trees, self.numClasses, self.numFeatures, self.seed = list(trees), int(numClasses), int(numFeatures), int(seed)

    @property
    def numTrees(self) -> int:
        return len(self.trees)

    @property
    def totalNumNodes(self) -> int:
        return sum(t.numNodes for t in self.trees)

    def predict(self, data: PartitionedData, *, engine=None):
        """The voted class of every row: one device int32 tensor per partition of `data` (empty for another
        rank's partitions)."""
        if data.num_features != self.numFeatures:
            raise IllegalArgumentException(
                f"requirement failed: vector sizes do not match: Expected {self.numFeatures} but found {data.num_features}")
        _check_dense(data)
        engine = _engine_for(data, engine)
        cls, _ = engine.forest_predict([t.nodes for t in self.trees], self.numClasses)
        out, at = [], 0
        for p, part in enumerate(data.partitions):
            n = part.n_rows if engine.lo <= p < engine.hi else 0
            out.append(cls[at: at + n])
            at += n
        return out

    def toDebugString(self) -> str:
        lines = [f"TreeEnsembleModel classifier with {self.numTrees} trees", ""]
        for t, tree in enumerate(self.trees):
            lines.append(f"  Tree {t}:")
            lines += ["   " + line for line in tree.toDebugString().splitlines()[1:]]
        return "\n".join(lines) + "\n"


class RandomForest:
    """MLlib 1.6.1 RandomForest for classification (the module docstring has the loop)."""

    @staticmethod
    def trainClassifier(data: PartitionedData, numClasses: int, categoricalFeaturesInfo=None, numTrees: int = 20,
                        featureSubsetStrategy: str = "auto", impurity: str = "gini", maxDepth: int = 4, maxBins: int = 32,
                        seed=None, *, minInstancesPerNode: int = 1, minInfoGain: float = 0.0, subsamplingRate: float = 1.0,
                        engine=None, scratchBudget: int = 0, slotBudget: int = 0) -> RandomForestModel:
        _check_train_args(data, numClasses, categoricalFeaturesInfo, impurity, maxDepth, maxBins, minInstancesPerNode,
                          minInfoGain)
        if isinstance(numTrees, (bool, np.bool_)) or not isinstance(numTrees, (int, np.integer)) or numTrees < 1:
            raise IllegalArgumentException(f"requirement failed: numTrees must be an integer >= 1 (got {numTrees!r})")
        if not 0.0 < float(subsamplingRate) <= 1.0:
            raise IllegalArgumentException(f"requirement failed: subsamplingRate must be in (0, 1] (got {subsamplingRate!r})")
        K, T, maxDepth, maxBins, d = int(numClasses), int(numTrees), int(maxDepth), int(maxBins), data.num_features
        m = forest_subset_size(featureSubsetStrategy, d, T)
        seed = int(np.random.default_rng().integers(0, 1 << 63)) if seed is None else int(seed)
        cut = forest_cut(T, subsamplingRate)
        engine = _engine_for(data, engine)
        thr, nbins = find_splits(data, maxBins, seed, engine=engine)
        bins = engine.tree_bin(thr, nbins)
        counts = getattr(data, "partition_counts", None)
        n = int(np.sum(counts)) if counts is not None else data.count()
        # (the same tree groups on every rank: sized by all the rows, not this rank's)
        G = forest_plan(d, maxBins, K, m, 1, T, 0, n, scratchBudget, slotBudget)["group_trees"]
        trees = []
        for t0 in range(0, T, G):
            g = min(G, T - t0)
            slots = engine.forest_slots(g)
            done = [{} for _ in range(g)]           # per tree: MLlib id -> the node's fields
            frontier = [[1] for _ in range(g)]      # per tree: the open nodes' ids, in slot order
            level = 0
            while any(frontier):
                flat = [(t, nid) for t in range(g) for nid in frontier[t]]
                A = len(flat)
                base = np.concatenate([[0], np.cumsum([len(f) for f in frontier])]).astype(np.int32)
                sub = np.stack([forest_subset(seed, t0 + t, nid, d, m) for t, nid in flat])
                fr = engine.forest_frontier(np.array([t for t, _ in flat], dtype=np.int32), base, sub)
                plan = forest_plan(d, maxBins, K, m, A, g, 0, n, scratchBudget, slotBudget)
                recs = []
                for a0 in range(0, A, plan["group_nodes"]):
                    group = (a0, min(plan["group_nodes"], A - a0))
                    hist = engine.forest_histogram(bins, slots, K, fr, (seed, t0, cut), group)
                    recs.append(engine.forest_best_split(hist, bins, fr, a0, impurity, minInstancesPerNode,
                                                         minInfoGain).cpu().numpy())
                rec = np.concatenate(recs)
                table = np.full((A, 4), -1, dtype=np.int32)
                nxt = [[] for _ in range(g)]
                for a, (t, nid) in enumerate(flat):
                    r = rec[a]
                    tot, L = r[6: 6 + K], r[6 + K: 6 + 2 * K]
                    split = r[0] >= 0 and level < maxDepth
                    done[t][nid] = dict(feature=int(r[0]) if split else -1, threshold=float(r[2]) if split else 0.0,
                                        gain=float(r[3]) if split else 0.0, impurity=float(r[4]), counts=tot.copy(),
                                        bin=int(r[1]) if split else -1)
                    if not split:
                        continue
                    table[a, 0], table[a, 1] = int(r[0]), int(r[1])
                    for side, cnt in ((0, L), (1, tot - L)):
                        cid = 2 * nid + side
                        if level + 1 >= maxDepth or np.count_nonzero(cnt) <= 1:   # a finished leaf: no slot
                            done[t][cid] = dict(feature=-1, threshold=0.0, gain=0.0, impurity=_impurity(cnt, impurity),
                                                counts=cnt.copy(), bin=-1)
                        else:
                            table[a, 2 + side] = len(nxt[t])
                            nxt[t].append(cid)
                if any(nxt):
                    engine.forest_route(bins, slots, fr, table)
                frontier, level = nxt, level + 1
            trees += [DecisionTreeModel(_node_arrays(done[t], K), K, d) for t in range(g)]
        return RandomForestModel(trees, K, d, seed)
