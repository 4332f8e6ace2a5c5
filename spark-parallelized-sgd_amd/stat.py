"""Second moments on the device: the augmented Gramian of the rows the context holds in HBM, and what
follows from it on the host -- RowMatrix.computeGramianMatrix / computeCovariance, Statistics.corr
(the sibling of feature.column_stats) and the normal equations of least squares.

  g = gramian(data)                  # one pass: sum z z^T, z = [x, y, 1]
  g.gram, g.xty, g.yty               # X^T X, X^T y, y^T y
  g.covariance(), g.corr()           # computeCovariance, Statistics.corr(., "pearson")
  w_star = g.normal_equations(regParam=0.1)
  gw = gramian(data, weights=omega)  # sum omega_i z z^T: weighted least squares (WeightedLeastSquares, "normal")
  gw.weightSum, gw.normal_equations(regParam=0.1)
  pc, explained = g.principal_components(k)   # RowMatrix.computePrincipalComponents
  s, V = g.svd(k)                             # RowMatrix.computeSVD, local-eigs mode
  projected = multiply(data, pc)              # RowMatrix.multiply: new rows on the device

w_star is the point every run of ParallelizedSGD / GradientDescent with LeastSquaresGradient and
SquaredL2SGDUpdater converges toward. The pass is fp64 on the device (fp64 MFMA over dense rows, fp64
atomics over CSR rows; include/psgd.h has the semantics); everything after it is numpy fp64 on the
host over a (d + 2) x (d + 2) array, so `Gramian` can be built from any such array. `multiply` is
the one function here that writes rows: Y = X B on the device (fp64 MFMA over dense rows,
HipEngine.project), the rows' labels kept beside them.

The definitions are this project's restatement of MLlib 1.6.1 (RowMatrix.computeCovariance,
PearsonCorrelation, RowMatrix.multiply / computePrincipalComponents / computeSVD), not pinned to its
source. Two things are this project's own: the sign of a principal component or singular vector is
fixed so that its largest-magnitude entry is positive (MLlib leaves it to LAPACK), and
explainedVariance is MLlib 2.0's member (1.6.1 returns the components alone).
"""
from __future__ import annotations

import numpy as np

from ._native import PROJECT_MAX_K, IllegalArgumentException
from .data import PartitionedData


def _check_k(k, d: int, what: str) -> int:
    """1 <= k <= d, a whole number (bool and float are refused)."""
    if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)):
        raise IllegalArgumentException(f"requirement failed: {what} takes a whole number k (got {k!r})")
    if not 1 <= int(k) <= d:
        raise IllegalArgumentException(f"requirement failed: {what} needs 1 <= k <= {d} (got {k})")
    return int(k)


def _fix_signs(V: np.ndarray) -> np.ndarray:
    """Each column's largest-magnitude entry (the first of equals) made positive."""
    V = np.array(V, dtype=np.float64)
    top = np.argmax(np.abs(V), axis=0)
    neg = V[top, np.arange(V.shape[1])] < 0.0
    V[:, neg] = -V[:, neg]
    return V


def _eigh_desc(A: np.ndarray):
    """Eigenvalues in descending order with their eigenvectors as columns, signs fixed (numpy fp64)."""
    A = 0.5 * (A + A.T)
    w, V = np.linalg.eigh(A)
    order = np.argsort(-w, kind="stable")
    return w[order], _fix_signs(V[:, order])


class Gramian:
    """A host object over M = sum_i z_i z_i^T, z_i = [x_i0 .. x_i,d-1, y_i, 1]: a symmetric
    (d + 2) x (d + 2) array of doubles. weighted: the matrix is M_w = sum_i omega_i z_i z_i^T of row
    weights omega (gramian(data, weights=)): M[d + 1, d + 1] is then their sum, weightSum, mean and
    normal_equations divide by it (weighted least squares), and the members that need the row count
    (covariance, corr, principal_components, svd) raise IllegalArgumentException."""

    def __init__(self, matrix, weighted: bool = False):
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
        self.weighted = bool(weighted)

    @property
    def count(self) -> int:
        return int(self.matrix[self.d + 1, self.d + 1])

    @property
    def weightSum(self) -> float:
        """M[d + 1, d + 1]: the sum of the row weights (the row count of an unweighted Gramian)."""
        return float(self.matrix[self.d + 1, self.d + 1])

    def _unweighted(self, what: str) -> None:
        if self.weighted:
            raise IllegalArgumentException(
                f"requirement failed: {what} needs the row count, which a weighted Gramian does not hold")

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
        if self.weighted:
            if not self.weightSum > 0.0:
                raise IllegalArgumentException("requirement failed: the weighted mean needs a positive weight sum")
            return self.columnSums / self.weightSum
        n = self.count
        if n <= 0:
            raise IllegalArgumentException("requirement failed: Cannot compute the mean of a RowMatrix without rows.")
        return self.columnSums / float(n)

    def covariance(self) -> np.ndarray:
        """RowMatrix.computeCovariance: cov_jk = G_jk / (n - 1) - (n / (n - 1)) mean_j mean_k."""
        self._unweighted("covariance")
        n = self.count
        if n <= 1:
            raise IllegalArgumentException(
                f"requirement failed: Cannot compute the covariance of a RowMatrix with <= 1 row. (got {n})")
        mean = self.mean
        return self.gram / (n - 1.0) - (n / (n - 1.0)) * np.outer(mean, mean)

    def corr(self) -> np.ndarray:
        """Statistics.corr(., "pearson"): sigma_j = sqrt(cov_jj), taken as 0 where |cov_jj| <= 1e-12;
        corr_jk = cov_jk / (sigma_j sigma_k), NaN where either sigma is 0; the diagonal is 1.0 always."""
        self._unweighted("corr")
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
        solved by Cholesky in fp64. A matrix that is not positive definite raises. On a weighted
        Gramian n is weightSum: the minimiser of (1 / W) sum omega_i (w . x_i - y_i)^2 / 2 + (regParam / 2)
        ||w||^2, weighted least squares."""
        lam = float(regParam)
        if not lam >= 0.0:
            raise IllegalArgumentException(f"requirement failed: regParam must be nonnegative but got {regParam}")
        if self.weighted:
            n = self.weightSum
            if not n > 0.0:
                raise IllegalArgumentException(
                    "requirement failed: the weighted normal equations need a positive weight sum")
        else:
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

    def principal_components(self, k):
        """RowMatrix.computePrincipalComponents(k): (pc, explainedVariance) from the
        eigen-decomposition of covariance() in numpy fp64. pc is d x k, its columns the eigenvectors
        in descending eigenvalue order, each with its largest-magnitude entry positive (this project's
        convention; MLlib leaves the sign to LAPACK); explainedVariance[j] is eigenvalue j over the
        trace (MLlib 2.0's member). Needs 1 <= k <= d and at least 2 rows."""
        self._unweighted("principal_components")
        k = _check_k(k, self.d, "computePrincipalComponents")
        w, V = _eigh_desc(self.covariance())
        total = float(np.sum(w))
        with np.errstate(invalid="ignore", divide="ignore"):
            explained = w / total
        return np.ascontiguousarray(V[:, :k]), explained[:k].copy()

    def svd(self, k, rCond: float = 1e-9):
        """RowMatrix.computeSVD(k, rCond = rCond) in its local-eigs mode: (s, V) with s the square roots
        of the leading eigenvalues of X^T X, descending, and V (d x len(s)) their eigenvectors (signs as
        in principal_components). Only sigma > rCond * sigma_0 are kept: fewer than k may be returned.
        An eigenvalue at or below the fp64 eigen-solver's noise floor, d * 2^-52 * sigma_0^2 (the
        tolerance of numpy.linalg.matrix_rank), counts as zero whatever rCond is: the square root of
        such noise is about 1e-8 sigma_0 and would pass rCond = 1e-9 as a singular value."""
        self._unweighted("svd")
        k = _check_k(k, self.d, "computeSVD")
        if not 0.0 <= float(rCond) <= 1.0:
            raise IllegalArgumentException(f"requirement failed: rCond must be within [0, 1] but got {rCond}")
        w, V = _eigh_desc(self.gram)
        w = np.where(w > self.d * np.finfo(np.float64).eps * w[0], w, 0.0)
        sigma = np.sqrt(np.maximum(w, 0.0))
        if not sigma[0] > 0.0:
            raise IllegalArgumentException("requirement failed: computeSVD needs a matrix with a non-zero entry")
        keep = 0
        while keep < k and sigma[keep] > float(rCond) * sigma[0]:
            keep += 1
        return sigma[:keep].copy(), np.ascontiguousarray(V[:, :keep])

    def __repr__(self) -> str:
        if self.weighted:
            return f"Gramian(d={self.d}, weightSum={self.weightSum})"
        return f"Gramian(d={self.d}, count={self.count})"


def _check_row_weights(data: PartitionedData, weights) -> np.ndarray:
    """One finite, non-negative double per row of `data`, in partition order."""
    om = np.ascontiguousarray(weights, dtype=np.float64)
    if om.ndim != 1 or om.shape[0] != data.count():
        raise IllegalArgumentException(
            f"requirement failed: weights must hold one value per row ({data.count()}; got shape {om.shape})")
    if not (np.all(np.isfinite(om)) and np.all(om >= 0.0)):
        raise IllegalArgumentException("requirement failed: weights must be finite and nonnegative")
    return om


def local_row_slice(data: PartitionedData, engine) -> slice:
    """The rows of the engine's partitions [lo, hi) within the data's rows in partition order."""
    sizes = [p.n_rows for p in data.partitions]
    return slice(sum(sizes[: engine.lo]), sum(sizes[: engine.hi]))


def gramian(data: PartitionedData, weights=None, *, engine=None) -> Gramian:
    """The augmented Gramian of every row of every partition, on all ranks (HipEngine.gramian). Data
    without rows raises IllegalArgumentException, as column_stats does. weights: a host array of
    data.count() non-negative doubles in partition order (each rank takes the slice of its
    partitions): the result is the weighted Gramian sum_i weights_i z_i z_i^T."""
    if data.num_partitions == 0 or data.count() == 0:
        raise IllegalArgumentException("requirement failed: Cannot compute the Gramian of data without rows.")
    om = None if weights is None else _check_row_weights(data, weights)
    if engine is None:
        from . import _native as N
        if data.num_features > N.GRAMIAN_MAX_D:
            raise IllegalArgumentException(
                f"requirement failed: the Gramian takes at most {N.GRAMIAN_MAX_D} features (got {data.num_features})")
        from .optimization import HipEngine, _dist
        rank, world, _ = _dist()
        engine = HipEngine(data, rank, world)
    a = data.num_features + 2
    if om is None:
        return Gramian(engine.gramian().cpu().numpy().reshape(a, a))
    local = engine.device_rows(om[local_row_slice(data, engine)])
    return Gramian(engine.gramian(weights=local).cpu().numpy().reshape(a, a), weighted=True)


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


def multiply(data: PartitionedData, B, storage=None, *, engine=None) -> PartitionedData:
    """RowMatrix.multiply(B) keeping the labels: the rows of `data` times B [d, k] (a numpy array or a
    device tensor) as a new PartitionedData of dense device partitions of k features, partition p
    the rows of source partition p in order (HipEngine.project; include/psgd.h has the semantics).
    storage ("f32" / "f64"; None keeps the source's) is the result's dtype."""
    shape = tuple(getattr(B, "shape", ())) or np.shape(B)
    if len(shape) != 2 or shape[0] != data.num_features:
        raise IllegalArgumentException(
            f"requirement failed: B must be [{data.num_features}, k] to multiply rows of {data.num_features} "
            f"features (got shape {tuple(shape)})")
    if not 1 <= shape[1] <= PROJECT_MAX_K:
        raise IllegalArgumentException(
            f"requirement failed: multiply takes 1 <= k <= {PROJECT_MAX_K} columns (got {shape[1]})")
    if storage not in (None, "f32", "f64"):
        raise IllegalArgumentException(f"requirement failed: storage must be 'f32', 'f64' or None (got {storage!r})")
    if engine is None:
        from .optimization import HipEngine, _dist
        rank, world, _ = _dist()
        engine = HipEngine(data, rank, world)
    return engine.project(B, storage)


def computePrincipalComponents(data: PartitionedData, k, *, engine=None):
    """RowMatrix.computePrincipalComponentsAndExplainedVariance(k) over the rows of `data`:
    Gramian.principal_components of one device pass."""
    _check_k(k, data.num_features, "computePrincipalComponents")
    return gramian(data, engine=engine).principal_components(k)


def computeSVD(data: PartitionedData, k, computeU: bool = False, rCond: float = 1e-9, *, engine=None):
    """RowMatrix.computeSVD(k, computeU, rCond), local-eigs mode only: (U, s, V) with U = None unless
    computeU, else the rows X V diag(1 / s) as multiply returns them (f64 whatever the source's storage:
    its columns are orthonormal to fp64 only there)."""
    _check_k(k, data.num_features, "computeSVD")
    s, V = gramian(data, engine=engine).svd(k, rCond)
    U = multiply(data, V / s[None, :], "f64", engine=engine) if computeU else None
    return U, s, V
