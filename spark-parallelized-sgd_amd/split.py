"""Train/test splits on the device: RDD.randomSplit and MLUtils.kFold of Spark / MLlib 1.6.1.

  train, test = randomSplit(data, [0.6, 0.4], seed=11)
  w, _ = runParallelizedSGD(train, ...)
  print(evaluate(test, gradient, updater, regParam, w).accuracy)

  for training, validation in kFold(data, 3, seed=7): ...

Both are BernoulliCellSampler passes over the rows the context holds in HBM (include/psgd.h,
psgd_cell_select: one XORShiftRandom draw a row, a row kept when its draw falls into the split's
cell), followed by one compaction launch into torch tensors (psgd_gather_dense_device /
psgd_gather_csr_device). The definitions are this project's statement of the behaviour (DESIGN.md
§3), not pinned to Spark's source.
"""
from __future__ import annotations

import math
from typing import List, Sequence, Tuple

import numpy as np

from . import _native as N
from .data import PartitionedData

IllegalArgumentException = N.IllegalArgumentException
SEED_PLUS_INDEX, SEED_PARTITIONWISE = N.SEED_PLUS_INDEX, N.SEED_PARTITIONWISE


def split_bounds(weights: Sequence[float]) -> List[float]:
    """The cell bounds of randomSplit(weights): sum = weights.sum (a left fold from 0.0), then
    weights.map(_ / sum).scanLeft(0.0)(_ + _) -- len(weights) + 1 doubles from 0.0; the last need not
    be exactly 1.0. Empty weights, a negative or NaN weight and a sum that is not a positive finite
    number raise IllegalArgumentException (this package's choice: Spark 1.6.1 checks none of it)."""
    ws = [float(w) for w in weights]
    if not ws:
        raise IllegalArgumentException("requirement failed: randomSplit needs at least one weight")
    total = 0.0
    for w in ws:
        if not w >= 0.0:
            raise IllegalArgumentException(f"requirement failed: Weights must be nonnegative, but got {ws}")
        total = total + w
    if not (total > 0.0 and math.isfinite(total)):
        raise IllegalArgumentException(f"requirement failed: Sum of weights must be positive, but got {total!r}")
    bounds = [0.0]
    for w in ws:
        bounds.append(bounds[-1] + w / total)
    return bounds


def kfold_bounds(numFolds: int) -> List[Tuple[float, float]]:
    """(lb, ub) of fold 1 .. numFolds: (fold - 1) / numFoldsF and fold / numFoldsF computed in float32
    (numFoldsF = numFolds.toFloat), then widened -- 3 folds give 0.3333333432674408 and
    0.6666666865348816. numFolds < 1 raises IllegalArgumentException (this package's choice)."""
    try:
        ok = not isinstance(numFolds, bool) and int(numFolds) == numFolds and int(numFolds) >= 1
    except (TypeError, ValueError, OverflowError):
        ok = False
    if not ok:
        raise IllegalArgumentException(f"requirement failed: numFolds must be a positive integer, but got {numFolds!r}")
    k = int(numFolds)
    f = np.float32(k)
    return [(float(np.float32(fold - 1) / f), float(np.float32(fold) / f)) for fold in range(1, k + 1)]


def _empty_like(data: PartitionedData) -> PartitionedData:
    out = PartitionedData([])
    out.partition_counts = np.zeros(0, dtype=np.int64)
    return out


def _engine_for(data: PartitionedData, engine):
    if engine is not None:
        return engine
    from .optimization import HipEngine, _dist
    rank, world, _ = _dist()
    return HipEngine(data, rank, world)


def randomSplit(data: PartitionedData, weights: Sequence[float], seed: int, engine=None) -> List[PartitionedData]:
    """data.randomSplit(weights, seed): one PartitionedData per weight. Split c keeps row t of
    partition p when b_c <= x_t < b_{c+1}, with b = split_bounds(weights) and x_t the t-th
    nextDouble() of XORShiftRandom(seed + p) (p the global partition index, the sum wrapping as a
    Java Long). A row whose draw is >= the last bound (the bounds need not end at exactly 1.0)
    belongs to no split, as in Spark.

    Every split has the source's number of partitions: partition p of a split holds the kept rows of
    source partition p, in order, possibly none, as DevicePartition / DeviceCsrPartition on the
    engine's device -- so the partition index is still the chain id. With several ranks each result
    lists all partitions, this rank's block filled and empty placeholders elsewhere, and carries
    `partition_counts`, every partition's row count on every rank.

    The rows are taken from the engine's registered copy: a source that carries a column_transform
    yields scaled splits, and the splits carry none. A split doubles the rows' HBM footprint until
    the source is re-registered away (training on a split does that: it registers the split in the
    source's place, zero-copy).

    A split depends only on (seed, partition index, row position), so it is repeatable:
      1. train, test = randomSplit(source, w, seed)
      2. model = StandardScaler().fit(train)        # read-only: works on device partitions
      3. scaled = model.transform(source)
      4. train, test = randomSplit(scaled, w, seed)  # the same rows, scaled
    model.transform on a split itself is refused, because its partitions are zero-copy.

    Empty weights, a negative or NaN weight and a sum of weights that is not positive raise
    IllegalArgumentException (this package's choice: Spark 1.6.1 checks none of it)."""
    bounds = split_bounds(weights)
    if data.num_partitions == 0:
        return [_empty_like(data) for _ in range(len(bounds) - 1)]
    engine = _engine_for(data, engine)
    return [engine.split_cell(bounds[c], bounds[c + 1], False, seed, SEED_PLUS_INDEX)
            for c in range(len(bounds) - 1)]


def kFold(data: PartitionedData, numFolds: int, seed: int, engine=None) -> List[Tuple[PartitionedData, PartitionedData]]:
    """MLUtils.kFold(data, numFolds, seed): a list of (training, validation), fold = 1 .. numFolds.
    validation keeps row t of partition p when lb <= x_t < ub and training is its complement, with
    (lb, ub) = kfold_bounds(numFolds)[fold - 1] and x_t the t-th nextDouble() of an XORShiftRandom
    seeded with the p-th java.util.Random(seed).nextLong() (PartitionwiseSampledRDD: the epoch
    sampler's seeding with `seed` in place of 42 + iteration). Partitions, placement and the column
    transform as for randomSplit. numFolds < 1 raises IllegalArgumentException."""
    cells = kfold_bounds(numFolds)
    if data.num_partitions == 0:
        return [(_empty_like(data), _empty_like(data)) for _ in cells]
    engine = _engine_for(data, engine)
    return [(engine.split_cell(lb, ub, True, seed, SEED_PARTITIONWISE),
             engine.split_cell(lb, ub, False, seed, SEED_PARTITIONWISE)) for lb, ub in cells]
