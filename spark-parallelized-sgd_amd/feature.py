"""Column statistics and feature standardization on the device: what MLlib 1.6.1's
GeneralizedLinearAlgorithm.run does between loading and optimizing (StandardScaler over
Statistics.colStats), on the rows the context already holds in HBM.

  stats = column_stats(data)                         # Statistics.colStats
  model = StandardScaler(withMean=False, withStd=True).fit(data)
  scaled = model.transform(data)                     # shares the host partitions
  w = runParallelizedSGD(scaled, ...)[0]
  w_original_space = model.unscale(w)                # what GeneralizedLinearAlgorithm returns

The statistics are one streaming fp64 pass over dense rows (two over CSR rows); the transform is
applied in place to the context's copy of the rows when an engine registers `scaled`
(HipEngine._register), so the host arrays are neither copied nor scaled.

  pca = PCA(k).fit(data)                             # mllib.feature.PCA over stat.covariance
  reduced = pca.transform(data)                      # new device rows of k features, labels kept

PCA is this project's restatement of MLlib 1.6.1's, not pinned to its source; the components' sign
convention and explainedVariance are stat.Gramian.principal_components'.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from ._native import PROJECT_MAX_K, IllegalArgumentException
from .data import CsrPartition, DeviceCsrPartition, DevicePartition, PartitionedData


def column_stats(data: PartitionedData, *, engine=None):
    """Statistics.colStats(data): ColumnStats(count, mean, variance, numNonzeros, max, min) over
    every row of every partition, on all ranks (HipEngine.column_stats). Data without rows raises
    the summarizer's IllegalArgumentException."""
    if data.num_partitions == 0 or data.count() == 0:
        raise IllegalArgumentException("requirement failed: Nothing has been added to this summarizer.")
    if engine is None:
        from .optimization import HipEngine, _dist
        rank, world, _ = _dist()
        engine = HipEngine(data, rank, world)
    return engine.column_stats()


class StandardScalerModel:
    """MLlib 1.6.1 StandardScalerModel(std, mean, withStd, withMean):
    x' = (x - shift) * factor with factor_j = 1 / std_j (0.0 where std_j == 0.0) under withStd, else
    1.0, and shift_j = mean_j under withMean, else no shift at all."""

    def __init__(self, std, mean, withStd: bool = True, withMean: bool = False):
        self.std = np.ascontiguousarray(std, dtype=np.float64)
        self.mean = None if mean is None else np.ascontiguousarray(mean, dtype=np.float64)
        self.withStd, self.withMean = bool(withStd), bool(withMean)
        if self.withMean:
            if self.mean is None:
                raise IllegalArgumentException("requirement failed: cannot center without a mean")
            if self.mean.shape != self.std.shape:
                raise IllegalArgumentException(
                    f"requirement failed: mean and std vector must have equal size if both are provided "
                    f"(got {self.mean.size} and {self.std.size})")

    @property
    def factor(self) -> np.ndarray:
        if not self.withStd:
            return np.ones_like(self.std)
        f = np.zeros_like(self.std)
        nz = self.std != 0.0
        f[nz] = 1.0 / self.std[nz]
        return f

    @property
    def shift(self) -> Optional[np.ndarray]:
        return self.mean.copy() if self.withMean else None

    def unscale(self, w) -> np.ndarray:
        """Weights trained on transform(data) as weights of the original features: w * factor
        (exact for withMean = False, where x' . w = x . (w * factor); what
        GeneralizedLinearAlgorithm.run returns)."""
        w = np.asarray(w, dtype=np.float64)
        if w.shape != self.std.shape:
            raise IllegalArgumentException(
                f"requirement failed: weights of size {w.size} do not match the model's {self.std.size} features")
        return w * self.factor

    def transform(self, data: PartitionedData) -> PartitionedData:
        """A new PartitionedData that shares `data`'s host partitions and carries this transform:
        an engine that registers it scales its device copy of the rows in place
        (psgd_transform_columns_device). Being a new object it has a registration of its own:
        training or scoring `data` afterwards registers the unscaled rows again."""
        if self.std.size != data.num_features:
            raise IllegalArgumentException(
                f"requirement failed: vector sizes do not match: Expected {self.std.size} but found "
                f"{data.num_features}")
        for p in data.partitions:
            if isinstance(p, (DevicePartition, DeviceCsrPartition)):
                raise IllegalArgumentException(
                    "requirement failed: device-resident (zero-copy) partitions belong to the caller, who "
                    "scales them itself; transform works on host partitions")
            if self.withMean and isinstance(p, (CsrPartition,)):
                raise IllegalArgumentException(
                    "requirement failed: cannot center sparse (CSR) rows: withMean would fill the absent entries")
        if getattr(data, "column_transform", None) is not None:
            raise IllegalArgumentException(
                "requirement failed: the data already carries a column transform; transform the original data")
        out = PartitionedData(data.partitions)
        out.column_transform = (self.shift, self.factor)
        return out


class StandardScaler:
    """MLlib 1.6.1 StandardScaler(withMean = false, withStd = true): fit computes the column
    statistics on the device and returns the model with std = sqrt(unbiased variance)."""

    def __init__(self, withMean: bool = False, withStd: bool = True):
        self.withMean, self.withStd = bool(withMean), bool(withStd)

    def fit(self, data: PartitionedData, *, engine=None) -> StandardScalerModel:
        stats = column_stats(data, engine=engine)
        return StandardScalerModel(np.sqrt(stats.variance), stats.mean, self.withStd, self.withMean)


class PCAModel:
    """MLlib PCAModel(k, pc): transform multiplies the rows by pc (d x k). As in MLlib it does not
    centre them. explainedVariance is MLlib 2.0's member."""

    def __init__(self, k, pc, explainedVariance=None):
        self.pc = np.ascontiguousarray(pc, dtype=np.float64)
        if self.pc.ndim != 2 or isinstance(k, bool) or int(k) != self.pc.shape[1]:
            raise IllegalArgumentException(
                f"requirement failed: pc must be [d, k] with k = {k} columns (got shape {self.pc.shape})")
        self.k = int(k)
        if not 1 <= self.k <= PROJECT_MAX_K:
            raise IllegalArgumentException(
                f"requirement failed: PCA takes 1 <= k <= {PROJECT_MAX_K} components (got {self.k})")
        self.explainedVariance = (None if explainedVariance is None
                                  else np.ascontiguousarray(explainedVariance, dtype=np.float64))

    def transform(self, data: PartitionedData, storage=None, *, engine=None) -> PartitionedData:
        """stat.multiply(data, pc): new dense device rows of k features with the rows' labels. A source
        column_transform is in the rows and is not carried over."""
        if self.pc.shape[0] != data.num_features:
            raise IllegalArgumentException(
                f"requirement failed: vector sizes do not match: Expected {self.pc.shape[0]} but found "
                f"{data.num_features}")
        from .stat import multiply
        return multiply(data, self.pc, storage, engine=engine)


class PCA:
    """MLlib 1.6.1 feature.PCA(k): fit computes the covariance on the device
    (stat.computePrincipalComponents) and returns the model of the top k components."""

    def __init__(self, k):
        if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)) or int(k) < 1:
            raise IllegalArgumentException(f"requirement failed: PCA requires a whole number of components k >= 1 (got {k!r})")
        if int(k) > PROJECT_MAX_K:
            raise IllegalArgumentException(
                f"requirement failed: PCA takes at most {PROJECT_MAX_K} components (got {k})")
        self.k = int(k)

    def fit(self, data: PartitionedData, *, engine=None) -> PCAModel:
        if self.k > data.num_features:
            raise IllegalArgumentException(
                f"requirement failed: source vector size is {data.num_features} must be greater than k={self.k}")
        from .stat import computePrincipalComponents
        pc, explained = computePrincipalComponents(data, self.k, engine=engine)
        return PCAModel(self.k, pc, explained)
