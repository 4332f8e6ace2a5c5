"""MLlib 1.6.1 clustering.KMeans (runs = 1) over the engine's device copy of the rows:

  model = KMeans(k, maxIterations=20, epsilon=1e-4, seed=7).run(data)
  model.clusterCenters                 # [k, d] float64
  model.predict(data)                  # per-partition device int32 tensors
  model.computeCost(data)              # sum of squared distances to the closest centre
  step = kmeans_step(data, centres)    # one Lloyd step: sums, counts, cost, count

A Lloyd step is two passes on the device (HipEngine.kmeans_step: the assignment, then the centre
sums; include/psgd.h has the arithmetic), the update a third kernel (HipEngine.kmeans_update). The
centres stay on the device between iterations; the host reads back moved, cost and n.

The loop runs while iteration < maxIterations and some centre changed in the last step; a centre
counts as changed when ||c_new - c_old||^2 > epsilon^2. An empty cluster keeps its centre. The cost
reported is the last step's: the cost at the centres the step started from.

initializationMode "random" is this project's own convention: k distinct global row positions drawn
from numpy.random.default_rng(seed), read as the engine registered them (HipEngine.registered_rows).
"k-means||" is not built: give the initial centres with setInitialModel. trainingCost and
numIterations on the returned model are this project's additions."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

from ._native import KMEANS_MAX_K, IllegalArgumentException, UnsupportedOperationException
from .data import PartitionedData


class KMeansStep(NamedTuple):
    sums: np.ndarray      # [k, d]: the rows added by assigned centre
    counts: np.ndarray    # [k]: the rows of each centre
    cost: float           # the sum of the squared distances to the assigned centres
    count: int            # the rows


def _engine_for(data: PartitionedData, engine):
    if engine is not None:
        return engine
    from .optimization import HipEngine, _dist
    rank, world, _ = _dist()
    return HipEngine(data, rank, world)


def _check_centres(centres, d: int) -> np.ndarray:
    c = np.ascontiguousarray(centres, dtype=np.float64)
    if c.ndim != 2 or c.shape[1] != d or c.shape[0] < 1:
        raise IllegalArgumentException(
            f"requirement failed: the centres must be [k, {d}] with k >= 1 (got shape {c.shape})")
    if c.shape[0] > KMEANS_MAX_K:
        raise IllegalArgumentException(
            f"requirement failed: k-means takes at most {KMEANS_MAX_K} centres (got {c.shape[0]})")
    return c


def _split_step(h: np.ndarray, k: int, d: int) -> KMeansStep:
    return KMeansStep(h[: k * d].reshape(k, d), h[k * d: k * d + k], float(h[k * d + k]), int(h[k * d + k + 1]))


def kmeans_step(data: PartitionedData, centres, *, engine=None) -> KMeansStep:
    """One Lloyd step at `centres` [k, d] over every row of every partition, on all ranks
    (HipEngine.kmeans_step): the sibling of gradient_sum."""
    c = _check_centres(centres, data.num_features)
    engine = _engine_for(data, engine)
    return _split_step(engine.kmeans_step(c).cpu().numpy(), c.shape[0], c.shape[1])


class KMeansModel:
    """MLlib KMeansModel(clusterCenters)."""

    def __init__(self, clusterCenters):
        c = np.ascontiguousarray(clusterCenters, dtype=np.float64)
        if c.ndim != 2 or c.shape[0] < 1 or c.shape[0] > KMEANS_MAX_K:
            raise IllegalArgumentException(
                f"requirement failed: clusterCenters must be [k, d] with 1 <= k <= {KMEANS_MAX_K} (got shape {c.shape})")
        self.clusterCenters = c
        self.trainingCost = None
        self.numIterations = None

    @property
    def k(self) -> int:
        return int(self.clusterCenters.shape[0])

    def _check(self, data: PartitionedData):
        if data.num_features != self.clusterCenters.shape[1]:
            raise IllegalArgumentException(
                f"requirement failed: vector sizes do not match: Expected {self.clusterCenters.shape[1]} but found "
                f"{data.num_features}")

    def predict(self, data: PartitionedData, *, engine=None):
        """The closest centre of every row: one device int32 tensor per partition of `data` (empty for
        another rank's partitions), ties to the lowest index."""
        self._check(data)
        engine = _engine_for(data, engine)
        assign, _ = engine.kmeans_assign(self.clusterCenters)
        out, at = [], 0
        for p, part in enumerate(data.partitions):
            n = part.n_rows if engine.lo <= p < engine.hi else 0
            out.append(assign[at: at + n])
            at += n
        return out

    def computeCost(self, data: PartitionedData, *, engine=None) -> float:
        """The sum of the rows' squared distances to their closest centres, over all ranks."""
        self._check(data)
        return kmeans_step(data, self.clusterCenters, engine=engine).cost


class KMeans:
    """MLlib 1.6.1 KMeans with runs = 1 (the module docstring has the loop)."""

    def __init__(self, k: int = 2, maxIterations: int = 20, epsilon: float = 1e-4, initializationMode: str = "random",
                 seed=None):
        if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)) or int(k) < 1:
            raise IllegalArgumentException(f"requirement failed: Number of clusters must be positive but got {k!r}")
        if int(k) > KMEANS_MAX_K:
            raise IllegalArgumentException(f"requirement failed: k-means takes at most {KMEANS_MAX_K} centres (got {k})")
        if isinstance(maxIterations, (bool, np.bool_)) or int(maxIterations) < 0:
            raise IllegalArgumentException(
                f"requirement failed: Maximum of iterations must be nonnegative but got {maxIterations!r}")
        if not float(epsilon) >= 0.0:
            raise IllegalArgumentException(f"requirement failed: Distance threshold must be nonnegative but got {epsilon!r}")
        if initializationMode == "k-means||":
            raise UnsupportedOperationException(
                "the k-means|| initialisation is not built: use initializationMode='random' or give the "
                "initial centres with setInitialModel")
        if initializationMode != "random":
            raise IllegalArgumentException(f"requirement failed: unknown initializationMode {initializationMode!r}")
        self.k, self.maxIterations, self.epsilon = int(k), int(maxIterations), float(epsilon)
        self.initializationMode, self.seed = initializationMode, seed
        self.initialModel = None

    def setInitialModel(self, model: KMeansModel) -> "KMeans":
        if model.k != self.k:
            raise IllegalArgumentException("requirement failed: mismatched cluster count")
        self.initialModel = model
        return self

    def _initial_centres(self, data: PartitionedData, engine) -> np.ndarray:
        if self.initialModel is not None:
            return _check_centres(self.initialModel.clusterCenters, data.num_features)
        counts = getattr(data, "partition_counts", None)
        n = int(np.sum(counts)) if counts is not None else data.count()
        if n < self.k:
            raise IllegalArgumentException(
                f"requirement failed: random initialisation needs at least k = {self.k} rows (got {n})")
        positions = np.sort(np.random.default_rng(self.seed).choice(n, size=self.k, replace=False))
        return np.ascontiguousarray(engine.registered_rows(positions), dtype=np.float64)

    def run(self, data: PartitionedData, *, engine=None) -> KMeansModel:
        if data.num_partitions == 0:
            raise IllegalArgumentException("requirement failed: Cannot run k-means on data without partitions.")
        if self.initialModel is not None:   # (the refusal fires before any engine is touched)
            _check_centres(self.initialModel.clusterCenters, data.num_features)
        engine = _engine_for(data, engine)
        centres = self._initial_centres(data, engine)
        k, d = centres.shape
        c_dev = engine.device_rows(centres.reshape(-1)).reshape(k, d)
        eps2 = self.epsilon * self.epsilon
        iteration, changed, cost = 0, True, None
        while iteration < self.maxIterations and changed:
            step = engine.kmeans_step(c_dev)
            c_dev, moved = engine.kmeans_update(c_dev, step)
            cost = float(step[k * d + k:].cpu().numpy()[0])   # (the tail: cost, n)
            changed = bool(np.any(moved.cpu().numpy() > eps2))
            iteration += 1
        model = KMeansModel(np.array(c_dev.cpu().numpy(), dtype=np.float64).reshape(k, d))
        model.trainingCost, model.numIterations = cost, iteration
        return model

    @classmethod
    def train(cls, data: PartitionedData, k: int, maxIterations: int = 20, initializationMode: str = "random",
              seed=None, *, engine=None) -> KMeansModel:
        return cls(k, maxIterations, initializationMode=initializationMode, seed=seed).run(data, engine=engine)
