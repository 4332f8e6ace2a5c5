"""The column-statistics and standardization surface that needs no device: exported symbols and
argument errors of the C ABI, StandardScalerModel's arithmetic, the refusals of transform, the
host-side merge of the ranks' statistics, and the checkpoint fingerprint of transformed data."""
import ctypes as C
import os
import types

import numpy as np
import pytest

SYMBOLS = ("psgd_column_stats", "psgd_column_stats_device", "psgd_transform_columns",
           "psgd_transform_columns_device")


def native(pkg):
    import spark_parallelized_sgd_amd._native as N
    if not os.path.exists(N.LIB_PATH):
        pytest.skip("libpsgd.so not built (__graft_entry__.build())")
    return N


def test_library_exports_the_symbols(pkg):
    N = native(pkg)
    raw = C.CDLL(N.LIB_PATH)
    for name in SYMBOLS:
        assert hasattr(raw, name), name
        assert name in N.EXPORTED


def test_null_context_is_einval(pkg):
    N = native(pkg)
    L = N.lib()
    buf = (C.c_double * 16)()
    assert L.psgd_column_stats(None, buf) == N.PSGD_EINVAL
    assert b"ctx is null" in L.psgd_last_error()
    assert L.psgd_column_stats_device(None, None, None) == N.PSGD_EINVAL
    assert L.psgd_transform_columns(None, None, buf) == N.PSGD_EINVAL
    assert L.psgd_transform_columns_device(None, None, None, None) == N.PSGD_EINVAL


def test_scaler_model_arithmetic(pkg):
    std = np.array([2.0, 0.0, 0.5, 1e-7])
    mean = np.array([1.0, 0.1, -3.0, 0.0])
    m = pkg.StandardScalerModel(std, mean, withStd=True, withMean=False)
    assert m.factor.tolist() == [0.5, 0.0, 2.0, 1.0 / 1e-7]   # std 0 gives 0, never 1 / tiny
    assert m.shift is None
    w = np.array([4.0, 7.0, -1.0, 2.0])
    assert m.unscale(w).tolist() == [2.0, 0.0, -2.0, 2.0 * (1.0 / 1e-7)]
    centred = pkg.StandardScalerModel(std, mean, withStd=False, withMean=True)
    assert centred.factor.tolist() == [1.0, 1.0, 1.0, 1.0]
    assert centred.shift.tolist() == mean.tolist()
    with pytest.raises(pkg.IllegalArgumentException):
        m.unscale(np.zeros(3))
    with pytest.raises(pkg.IllegalArgumentException):
        pkg.StandardScalerModel(std, None, withStd=True, withMean=True)
    assert (pkg.StandardScaler().withMean, pkg.StandardScaler().withStd) == (False, True)


def csr_data(pkg, d=4):
    part = pkg.CsrPartition(np.zeros(2), np.array([0, 1, 2], dtype=np.int64), np.array([0, 3], dtype=np.int32),
                            np.array([1.0, 2.0]), d)
    return pkg.PartitionedData([part])


def test_transform_refusals_and_sharing(pkg):
    x = np.arange(12.0).reshape(4, 3)
    data = pkg.PartitionedData.parallelize(np.zeros(4), x, 2)
    model = pkg.StandardScalerModel(np.ones(3), np.zeros(3), True, True)
    scaled = model.transform(data)
    assert scaled is not data and data.column_transform is None
    assert all(a is b for a, b in zip(scaled.partitions, data.partitions))   # the host rows are shared
    shift, factor = scaled.column_transform
    assert shift.tolist() == [0.0] * 3 and factor.tolist() == [1.0] * 3
    assert pkg.StandardScalerModel(np.ones(3), np.zeros(3), True, False).transform(data).column_transform[0] is None
    # a std of the wrong length
    with pytest.raises(pkg.IllegalArgumentException):
        pkg.StandardScalerModel(np.ones(4), np.zeros(4)).transform(data)
    # withMean on CSR rows (withStd alone is fine)
    with pytest.raises(pkg.IllegalArgumentException):
        pkg.StandardScalerModel(np.ones(4), np.zeros(4), True, True).transform(csr_data(pkg))
    assert pkg.StandardScalerModel(np.ones(4), np.zeros(4), True, False).transform(csr_data(pkg)).column_transform
    # device-resident partitions belong to the caller (no tensor is touched: the type decides)
    fake = types.SimpleNamespace(shape=(0,))
    for part in (pkg.DevicePartition(fake, fake, 3), pkg.DeviceCsrPartition(fake, fake, fake, fake, 3)):
        with pytest.raises(pkg.IllegalArgumentException):
            pkg.StandardScalerModel(np.ones(3), np.zeros(3)).transform(pkg.PartitionedData([part]))


def test_no_rows_is_the_summarizers_error(pkg):
    for data in (pkg.PartitionedData([]), pkg.PartitionedData.parallelize(np.zeros(0), np.zeros((0, 3)), 2)):
        with pytest.raises(pkg.IllegalArgumentException, match="Nothing has been added to this summarizer"):
            pkg.column_stats(data)
        with pytest.raises(pkg.IllegalArgumentException, match="Nothing has been added to this summarizer"):
            pkg.StandardScaler().fit(data)


def test_rank_merge_is_chans_formula(pkg):
    from spark_parallelized_sgd_amd.optimization import merge_column_stats
    rng = np.random.default_rng(3)
    d = 3
    blocks = [rng.standard_normal((5, d)) + 100.0, np.zeros((0, d)), rng.standard_normal((1, d)),
              rng.standard_normal((7, d))]

    def row(x):
        n = x.shape[0]
        if n == 0:
            return np.zeros(1 + 5 * d)
        mean = x.mean(axis=0)
        return np.concatenate([[n], mean, ((x - mean) ** 2).sum(axis=0), (x != 0).sum(axis=0), x.max(axis=0),
                               x.min(axis=0)])

    got = merge_column_stats(np.stack([row(b) for b in blocks]), d)
    allx = np.concatenate(blocks)
    assert got.count == 13 and got.numNonzeros.tolist() == [13] * d
    np.testing.assert_allclose(got.mean, allx.mean(axis=0), rtol=1e-14)
    np.testing.assert_allclose(got.variance, allx.var(axis=0, ddof=1), rtol=1e-12)
    assert got.max.tolist() == allx.max(axis=0).tolist() and got.min.tolist() == allx.min(axis=0).tolist()
    one = merge_column_stats(row(blocks[2])[None, :], d)
    assert one.count == 1 and one.variance.tolist() == [0.0] * d      # n = 1: variance 0
    # two ranks that each hold a constant column exactly (a plain sum / n in row() would not)
    rank = lambda n: np.concatenate([[n], np.full(d, 0.1), np.zeros(d), np.full(d, n), np.full(d, 0.1), np.full(d, 0.1)])
    const = merge_column_stats(np.stack([rank(4.0), rank(9.0)]), d)
    assert const.mean.tolist() == [0.1] * d and const.variance.tolist() == [0.0] * d
    with pytest.raises(pkg.IllegalArgumentException, match="Nothing has been added"):
        merge_column_stats(np.zeros((2, 1 + 5 * d)), d)


def test_fingerprint_depends_on_the_transform(pkg):
    from spark_parallelized_sgd_amd.optimization import _ckpt_fingerprint
    x = np.arange(12.0).reshape(4, 3)
    data = pkg.PartitionedData.parallelize(np.zeros(4), x, 2)
    params = pkg.make_params(pkg.LogisticGradient(), pkg.SimpleSGDUpdater(), 1.0, 0.0, 1.0, 0.0)
    w0 = np.zeros(3)
    plain = _ckpt_fingerprint(params, data, w0)
    assert plain.tobytes() == _ckpt_fingerprint(params, pkg.PartitionedData(data.partitions), w0).tobytes()
    a = pkg.StandardScalerModel(np.array([1.0, 2.0, 4.0]), np.zeros(3), True, False).transform(data)
    b = pkg.StandardScalerModel(np.array([1.0, 2.0, 8.0]), np.zeros(3), True, False).transform(data)
    c = pkg.StandardScalerModel(np.array([1.0, 2.0, 4.0]), np.zeros(3), True, True).transform(data)
    prints = [plain.tobytes()] + [_ckpt_fingerprint(params, t, w0).tobytes() for t in (a, b, c)]
    assert len(set(prints)) == 4
    again = pkg.StandardScalerModel(np.array([1.0, 2.0, 4.0]), np.zeros(3), True, False).transform(data)
    assert _ckpt_fingerprint(params, again, w0).tobytes() == prints[1]
