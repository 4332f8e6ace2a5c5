"""Second moments on the device: the augmented Gramian of the rows the context holds in HBM, and what
follows from it on the host -- RowMatrix.computeGramianMatrix / computeCovariance, Statistics.corr
(the sibling of feature.column_stats) and the normal equations of least squares.

  g = gramian(data)                  # one pass: sum z z^T, z = [x, y, 1]
  g.gram, g.xty, g.yty               # X^T X, X^T y, y^T y
  g.covariance(), g.corr()           # computeCovariance, Statistics.corr(., "pearson")
  w_star = g.normal_equations(regParam=0.1)

w_star is the point every run of ParallelizedSGD / GradientDescent with LeastSquaresGradient and
SquaredL2SGDUpdater converges toward. The pass is fp64 on the device (fp64 MFMA over dense rows, fp64
atomics over CSR rows; include/psgd.h has the semantics); everything after it is numpy fp64 on the
host over a (d + 2) x (d + 2) array, so `Gramian` can be built from any such array.

The definitions are this project's restatement of MLlib 1.6.1 (RowMatrix.computeCovariance,
PearsonCorrelation), not pinned to its source.
"""
from __future__ import annotations

import numpy as np

from ._native import IllegalArgumentException
from .data import PartitionedData


class Gramian:
    """A host object over M = sum_i z_i z_i^T, z_i = [x_i0 .. x_i,d-1, y_i, 1]: a symmetric
    (d + 2) x (d + 2) array of doubles."""

    def __init__(self, matrix):
        m = np.array(matrix, dtype=np.float64)
        if m.ndim == 1:
            a = int(round(np.sqrt(m.size)))
            if a * a != m.size:
                raise IllegalArgumentException(f"requirement failed: {m.size} values do not form a square matrix")
            m = m.reshape(a, a)
        if m.ndim != 2 or m.shape[0] != m.shape[1] or m.shape[0] < 3:
            raise IllegalArgumentException(
                f"requirement failed: the augmented Gramian is (d + 2) x (d + 2) with d >= 1 (got shape {m.shape})")
        self.matrix = m
        self.d = m.shape[0] - 2

    @property
    def count(self) -> int:
        return int(self.matrix[self.d + 1, self.d + 1])

    @property
    def gram(self) -> np.ndarray:
        """X^T X (RowMatrix.computeGramianMatrix), d x d."""
        return self.matrix[: self.d, : self.d]

    @property
    def xty(self) -> np.ndarray:
        return self.matrix[: self.d, self.d]

    @property
    def yty(self) -> float:
        return float(self.matrix[self.d, self.d])

    @property
    def columnSums(self) -> np.ndarray:
        return self.matrix[: self.d, self.d + 1]

    @property
    def labelSum(self) -> float:
        return float(self.matrix[self.d, self.d + 1])

    @property
    def mean(self) -> np.ndarray:
        n = self.count
        if n <= 0:
            raise IllegalArgumentException("requirement failed: Cannot compute the mean of a RowMatrix without rows.")
        return self.columnSums / float(n)

    def covariance(self) -> np.ndarray:
        """RowMatrix.computeCovariance: cov_jk = G_jk / (n - 1) - (n / (n - 1)) mean_j mean_k."""
        n = self.count
        if n <= 1:
            raise IllegalArgumentException(
                f"requirement failed: Cannot compute the covariance of a RowMatrix with <= 1 row. (got {n})")
        mean = self.mean
        return self.gram / (n - 1.0) - (n / (n - 1.0)) * np.outer(mean, mean)

    def corr(self) -> np.ndarray:
        """Statistics.corr(., "pearson"): sigma_j = sqrt(cov_jj), taken as 0 where |cov_jj| <= 1e-12;
        corr_jk = cov_jk / (sigma_j sigma_k), NaN where either sigma is 0; the diagonal is 1.0 always."""
        cov = self.covariance()
        var = np.diag(cov)
        with np.errstate(invalid="ignore"):
            sigma = np.where(np.abs(var) <= 1e-12, 0.0, np.sqrt(var))
        denom = np.outer(sigma, sigma)
        out = np.full_like(cov, np.nan)
        ok = denom != 0.0
        out[ok] = cov[ok] / denom[ok]
        np.fill_diagonal(out, 1.0)
        return out

    def normal_equations(self, regParam: float = 0.0) -> np.ndarray:
        """The minimiser of what LeastSquaresGradient with SquaredL2SGDUpdater minimises,
        (1 / n) sum (w . x - y)^2 / 2 + (regParam / 2) ||w||^2: (G / n + regParam I) w = X^T y / n,
        solved by Cholesky in fp64. A matrix that is not positive definite raises."""
        lam = float(regParam)
        if not lam >= 0.0:
            raise IllegalArgumentException(f"requirement failed: regParam must be nonnegative but got {regParam}")
        n = self.count
        if n <= 0:
            raise IllegalArgumentException("requirement failed: the normal equations need at least one row")
        A = self.gram / float(n) + lam * np.eye(self.d)
        b = self.xty / float(n)
        try:
            L = np.linalg.cholesky(A)
        except np.linalg.LinAlgError:
            raise IllegalArgumentException(
                "requirement failed: X^T X / n + regParam I is not positive definite (collinear or constant-zero "
                "columns): use regParam > 0 or drop the dependent columns") from None
        return np.linalg.solve(L.T, np.linalg.solve(L, b))

    def __repr__(self) -> str:
        return f"Gramian(d={self.d}, count={self.count})"


def gramian(data: PartitionedData, *, engine=None) -> Gramian:
    """The augmented Gramian of every row of every partition, on all ranks (HipEngine.gramian). Data
    without rows raises IllegalArgumentException, as column_stats does."""
    if data.num_partitions == 0 or data.count() == 0:
        raise IllegalArgumentException("requirement failed: Cannot compute the Gramian of data without rows.")
    if engine is None:
        from . import _native as N
        if data.num_features > N.GRAMIAN_MAX_D:
            raise IllegalArgumentException(
                f"requirement failed: the Gramian takes at most {N.GRAMIAN_MAX_D} features (got {data.num_features})")
        from .optimization import HipEngine, _dist
        rank, world, _ = _dist()
        engine = HipEngine(data, rank, world)
    a = data.num_features + 2
    return Gramian(engine.gramian().cpu().numpy().reshape(a, a))


def covariance(data: PartitionedData, *, engine=None) -> np.ndarray:
    """RowMatrix.computeCovariance over the rows of `data`."""
    return gramian(data, engine=engine).covariance()


def corr(data: PartitionedData, *, engine=None) -> np.ndarray:
    """Statistics.corr(rows, "pearson") over the rows of `data`."""
    return gramian(data, engine=engine).corr()


def normal_equations(data: PartitionedData, regParam: float = 0.0, *, engine=None) -> np.ndarray:
    """The least-squares optimum of `data` under SquaredL2 regularisation (Gramian.normal_equations)."""
    if not float(regParam) >= 0.0:
        raise IllegalArgumentException(f"requirement failed: regParam must be nonnegative but got {regParam}")
    return gramian(data, engine=engine).normal_equations(regParam)
