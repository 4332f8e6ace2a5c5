"""randomSplit / kFold without a device: the cell bounds, the argument checks, the null-context
errors of the new C entry points, empty data, and the restatement's own preconditions for the GPU
selection test (tests/test_gpu_data_split.py)."""
import ctypes

import numpy as np
import pytest

import split_truth as T


@pytest.fixture(scope="module")
def S(pkg):
    import importlib
    return importlib.import_module(pkg.__name__ + ".split")


def test_random_split_bounds(S):
    assert S.split_bounds([0.6, 0.4]) == [0.0, 0.6, 1.0]
    third = 1.0 / 3.0
    assert S.split_bounds([1, 1, 1]) == [0.0, third, third + third, third + third + third]
    assert S.split_bounds([0.5, 0, 0.5]) == [0.0, 0.5, 0.5, 1.0]
    for w in ([0.6, 0.4], [1, 1, 1], [0.5, 0, 0.5], [0.1] * 10, [3, 1e-3, 7.5]):
        assert S.split_bounds(w) == T.split_bounds(w)


def test_ten_tenths_are_a_left_fold(S):
    """Ten weights of 0.1: the left fold sums to 0.9999999999999999, every normalised weight is
    0.10000000000000002, and the scan of those gives exactly these doubles -- the last one 1.0."""
    total = 0.0
    for _ in range(10):
        total += 0.1
    assert total == 0.9999999999999999
    assert 0.1 / total == 0.10000000000000002
    assert S.split_bounds([0.1] * 10) == [
        0.0, 0.10000000000000002, 0.20000000000000004, 0.30000000000000004, 0.4000000000000001,
        0.5000000000000001, 0.6000000000000001, 0.7000000000000001, 0.8, 0.9, 1.0]


def test_kfold_bounds_are_float32(S):
    assert S.kfold_bounds(2) == [(0.0, 0.5), (0.5, 1.0)]
    assert S.kfold_bounds(3) == [(0.0, 0.3333333432674408), (0.3333333432674408, 0.6666666865348816),
                                 (0.6666666865348816, 1.0)]
    for k in (2, 3, 5, 10):
        got = S.kfold_bounds(k)
        f = np.float32(k)
        assert got == [(float(np.float32(i) / f), float(np.float32(i + 1) / f)) for i in range(k)]
        assert got == T.kfold_bounds(k)
        assert got[0][0] == 0.0 and got[-1][1] == 1.0
        assert all(a[1] == b[0] for a, b in zip(got, got[1:]))
    assert S.kfold_bounds(5)[2] == (0.4000000059604645, 0.6000000238418579)
    assert S.kfold_bounds(10)[6] == (0.6000000238418579, 0.699999988079071)


@pytest.mark.parametrize("weights", [[], [0.5, -0.1], [float("nan"), 1.0], [0.0, 0.0], [0.0]])
def test_random_split_refuses(pkg, weights):
    data = pkg.PartitionedData.parallelize(np.zeros(4), np.zeros((4, 2)), 2)
    with pytest.raises(pkg.IllegalArgumentException):
        pkg.randomSplit(data, weights, 1)
    with pytest.raises(pkg.IllegalArgumentException):
        pkg.randomSplit(pkg.PartitionedData([]), weights, 1)


@pytest.mark.parametrize("folds", [0, -3, 2.5])
def test_kfold_refuses(pkg, folds):
    data = pkg.PartitionedData.parallelize(np.zeros(4), np.zeros((4, 2)), 2)
    with pytest.raises(pkg.IllegalArgumentException):
        pkg.kFold(data, folds, 1)


def test_null_context_is_einval(pkg):
    N = pkg._native
    L = N.lib()
    buf = (ctypes.c_int64 * 4)()
    ptrs = (ctypes.c_uint64 * 4)()
    a = ctypes.addressof
    assert L.psgd_cell_select(None, 1, N.SEED_PLUS_INDEX, 0.0, 1.0, 0, None, a(buf), a(buf)) == N.PSGD_EINVAL
    assert b"ctx is null" in L.psgd_last_error()
    assert L.psgd_cell_select_device(None, 1, N.SEED_PARTITIONWISE, 0.0, 1.0, 0, None, a(buf), None,
                                     None) == N.PSGD_EINVAL
    assert L.psgd_gather_dense_device(None, None, a(buf), 4, a(ptrs), a(ptrs), None) == N.PSGD_EINVAL
    assert L.psgd_gather_csr_device(None, None, a(buf), a(buf), a(ptrs), a(ptrs), a(ptrs), a(ptrs),
                                    None) == N.PSGD_EINVAL
    assert b"ctx is null" in L.psgd_last_error()


def test_empty_data_splits_without_a_device(pkg):
    empty = pkg.PartitionedData([])
    parts = pkg.randomSplit(empty, [0.6, 0.4], 11)
    assert len(parts) == 2
    for s in parts:
        assert isinstance(s, pkg.PartitionedData) and s.num_partitions == 0 and s.count() == 0
        assert s.column_transform is None and len(s.partition_counts) == 0
    folds = pkg.kFold(empty, 3, 7)
    assert len(folds) == 3
    for tr, va in folds:
        assert tr.num_partitions == 0 and va.num_partitions == 0


def test_java_long_wrap():
    assert T.java_long(2**63 - 1 + 1) == -2**63
    assert T.split_seeds(2**63 - 1, 3) == [2**63 - 1, -2**63, -2**63 + 1]
    assert T.split_seeds(-3, 5) == [-3, -2, -1, 0, 1]


SIZES = (0, 1, 63, 64, 65, 16383, 16384, 16385, 40000)
SEEDS = (11, -3, 2**40 + 5)


@pytest.mark.parametrize("seed", SEEDS)
def test_selection_inputs_exercise_both_cells(seed):
    """What the GPU selection test relies on, checked on the restatement alone: with [0.6, 0.4] every
    partition of 63 rows or more has both cells non-empty; the zero-weight cell of [0.5, 0, 0.5] is
    empty everywhere; the cells of a partition are disjoint and cover the rows below the last bound."""
    two = T.random_split_rows(SIZES, [0.6, 0.4], seed)
    for p, n in enumerate(SIZES):
        if n >= 63:
            assert len(two[0][p]) > 0 and len(two[1][p]) > 0, (seed, n)
        assert len(two[0][p]) + len(two[1][p]) == n
    zero = T.random_split_rows(SIZES, [0.5, 0, 0.5], seed)
    assert all(len(r) == 0 for r in zero[1])
    for p, n in enumerate(SIZES):
        assert sorted(np.concatenate([zero[0][p], zero[2][p]]).tolist()) == list(range(n))
