"""The train/test splits restated in pure Python (test code; DESIGN.md §3 has the definitions):
BernoulliCellSampler over XORShiftRandom draws, randomSplit's bounds and seeds, kFold's float32
bounds and PartitionwiseSampledRDD seeds. Uses oracle/psgd_ref.py (on the test path) for the
generators; nothing here calls the package under test."""
import functools

import numpy as np

import psgd_ref as R

M64 = (1 << 64) - 1


def java_long(v: int) -> int:
    """v wrapped to 64 bits, two's complement (a Java Long)."""
    v &= M64
    return v - (1 << 64) if v >= 1 << 63 else v


@functools.lru_cache(maxsize=None)
def draws(partition_seed: int, n: int) -> np.ndarray:
    """x_0 .. x_{n-1}: the first n nextDouble() of XORShiftRandom(partition_seed) (hashSeed inside)."""
    rng = R.XORShiftRandom(partition_seed)
    out = np.array([rng.next_double() for _ in range(n)], dtype=np.float64)
    out.setflags(write=False)
    return out


def cell(x: np.ndarray, lb: float, ub: float, complement: bool) -> np.ndarray:
    """The rows BernoulliCellSampler(lb, ub, complement) keeps, in order."""
    inside = (x >= lb) & (x < ub)
    return np.flatnonzero(~inside if complement else inside).astype(np.int64)


def split_bounds(weights):
    """sum = the left fold of the weights; scanLeft(0.0)(_ + _) over weights.map(_ / sum)."""
    total = 0.0
    for w in weights:
        total = total + float(w)
    b = [0.0]
    for w in weights:
        b.append(b[-1] + float(w) / total)
    return b


def kfold_bounds(num_folds: int):
    f = np.float32(num_folds)
    return [(float(np.float32(k - 1) / f), float(np.float32(k) / f)) for k in range(1, num_folds + 1)]


def split_seeds(seed: int, P: int):
    """randomSplit: s_p = seed + p as a Java Long."""
    return [java_long(seed + p) for p in range(P)]


def kfold_seeds(seed: int, P: int):
    """kFold: s_p = the p-th java.util.Random(seed).nextLong()."""
    return [int(s) for s in R.partition_seeds(seed, P)]


def random_split_rows(sizes, weights, seed):
    """[split][partition] -> kept row indices."""
    b = split_bounds(weights)
    seeds = split_seeds(seed, len(sizes))
    return [[cell(draws(seeds[p], n), b[c], b[c + 1], False) for p, n in enumerate(sizes)]
            for c in range(len(weights))]


def kfold_rows(sizes, num_folds, seed):
    """[fold] -> ([partition] -> training rows, [partition] -> validation rows)."""
    seeds = kfold_seeds(seed, len(sizes))
    out = []
    for lb, ub in kfold_bounds(num_folds):
        out.append(([cell(draws(seeds[p], n), lb, ub, True) for p, n in enumerate(sizes)],
                    [cell(draws(seeds[p], n), lb, ub, False) for p, n in enumerate(sizes)]))
    return out
