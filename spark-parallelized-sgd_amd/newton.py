"""Newton's method over the registered partitions -- the second-order sibling of GradientDescent, for
the smooth losses: LogisticGradient (binary) and LeastSquaresGradient, without a penalty
(SimpleSGDUpdater) or with SquaredL2SGDUpdater's. The objective is what evaluate().objective reports,

  f(w) = lossSum(w) / n + (regParam / 2) ||w||^2.

One iteration is three device passes at fixed weights and a d x d solve on the host:

  g = gradientSum / n + regParam w         HipEngine.gradient_sum
  H = hessian / n + regParam I             HipEngine.row_curvature, then HipEngine.gramian(weights=):
                                           sum_i h_i x_i x_i^T is the weighted Gramian's X^T W X block
  delta = H^-1 g                           Cholesky in numpy fp64
  w <- w - t delta                         t = 1, 1/2, 1/4, .. until the Armijo test passes, f through
                                           HipEngine.evaluate

For LeastSquaresGradient the first full step lands on stat.normal_equations(data, regParam); for
LogisticGradient the iteration reaches the optimum to rounding in about ten passes, which gives the
first-order optimizers the reference point least squares always had. This is this project's own
addition: MLlib 1.6.1 has no Newton optimizer (its second-order one is L-BFGS).
"""
from __future__ import annotations

import collections
import logging
import math
from typing import List

import numpy as np

from . import _native as N
from .data import PartitionedData
from .gradient import Gradient, HingeGradient, gradient_kind, num_classes
from .optimization import HipEngine, IllegalArgumentException, ParallelizedSGD, _dist, max_j
from .updater import SGDUpdater, SimpleSGDUpdater, SquaredL2SGDUpdater, updater_kind

log = logging.getLogger("org.apache.spark.mllib.optimization.Newton")

# sum_i h_i x_i x_i^T [d, d], sum_i h_i and the row count at fixed weights: gradient_sum's sibling
HessianSum = collections.namedtuple("HessianSum", "hessian curvatureSum count")

ARMIJO_C = 1e-4        # sufficient decrease: f(w - t delta) <= f(w) - ARMIJO_C t g . delta
MAX_HALVINGS = 30


def _check_gradient(gradient: Gradient) -> None:
    """What the second-order passes refuse, before any device work."""
    if num_classes(gradient) > 2:
        raise N.UnsupportedOperationException(
            "Newton's method takes a binary gradient: the multinomial LogisticGradient (numClasses > 2) "
            "has a matrix of curvatures per row")
    gradient_kind(gradient)
    if isinstance(gradient, HingeGradient):
        raise N.UnsupportedOperationException(
            "HingeGradient has no curvature: its second derivative is 0 almost everywhere")


def _check_updater(updater: SGDUpdater) -> None:
    updater_kind(updater)
    if not isinstance(updater, (SimpleSGDUpdater, SquaredL2SGDUpdater)):
        raise N.UnsupportedOperationException(
            f"Newton's method takes SimpleSGDUpdater (no penalty) or SquaredL2SGDUpdater: "
            f"{type(updater).__name__} is not a twice differentiable penalty")


def _check_size(nf: int, size: int) -> None:
    if size != nf:
        raise IllegalArgumentException(
            f"requirement failed: BLAS.dot(x: Vector, y: Vector) was given Vectors with "
            f"non-matching sizes: x.size = {nf}, y.size = {size}")


def _hessian(engine, gradient: Gradient, w, d: int):
    """(sum_i h_i x_i x_i^T [d, d], sum_i h_i): this rank's curvatures as the row weights of the
    Gramian over all ranks."""
    h = engine.row_curvature(gradient, w)
    M = engine.to_host(engine.gramian(weights=h)).reshape(d + 2, d + 2)
    return M[:d, :d].copy(), float(M[d + 1, d + 1])


def hessian_sum(data: PartitionedData, gradient: Gradient, weights, *, engine=None) -> HessianSum:
    """The Hessian of the loss sum at fixed `weights` (a host array or a device tensor of num_features
    doubles): hessian = sum_i h_i x_i x_i^T with h_i the loss's curvature along row i's margin
    (HipEngine.row_curvature), curvatureSum = sum_i h_i, count the rows. hessian / count is the
    Jacobian of gradient_sum().gradient / count. HingeGradient and LogisticGradient(numClasses > 2)
    raise UnsupportedOperationException."""
    _check_gradient(gradient)
    if data.num_partitions == 0:
        return HessianSum(np.zeros((0, 0)), 0.0, 0)
    nf = data.num_features
    shape = tuple(weights.shape) if hasattr(weights, "shape") else np.asarray(weights).shape
    _check_size(nf, int(shape[0]) if len(shape) == 1 else -1)
    if data.count() == 0:
        return HessianSum(np.zeros((nf, nf)), 0.0, 0)
    if engine is None:
        rank, world, _ = _dist()
        engine = HipEngine(data, rank, world)
    H, hsum = _hessian(engine, gradient, weights, nf)
    return HessianSum(H, hsum, data.count())


class Newton(ParallelizedSGD):
    """Newton(gradient, updater): ParallelizedSGD's validated setters (same messages) with the
    defaults numIterations 100, regParam 0.0, convergenceTol 1e-6; stepSize and miniBatchFraction are
    not used (the step comes from the line search, the batch is every row). optimize(data,
    initialWeights) -> weights. The arithmetic is fp64: setComputeDtype("f32") is refused."""

    def __init__(self, gradient: Gradient, updater: SGDUpdater):
        super().__init__(gradient, updater)
        self.convergenceTol = 1e-6

    def setComputeDtype(self, dtype: str) -> "Newton":
        if dtype != "f64":
            raise N.UnsupportedOperationException("Newton computes in fp64 only")
        return self

    def optimize(self, data: PartitionedData, initialWeights) -> np.ndarray:
        weights, _ = Newton.runNewton(data, self.gradient, self.updater, self.numIterations, self.regParam,
                                      initialWeights, self.convergenceTol)
        return weights

    @staticmethod
    def runNewton(data: PartitionedData, gradient: Gradient, updater: SGDUpdater, numIterations: int,
                  regParam: float, initialWeights, convergenceTol: float = 1e-6, *, engine=None):
        """Damped Newton iterations from initialWeights -> (weights, lossHistory). lossHistory[k] is
        f at the weights iteration k started from (GradientDescent's convention). An iteration whose
        line search finds no step (MAX_HALVINGS halvings: the decrease f could still show is below
        its rounding) ends the run with the weights unchanged; otherwise the run ends when
        ||w_new - w|| < convergenceTol * max(||w_new||, 1), GradientDescent's test, or after
        numIterations. L1, AdaGrad and Adam updaters, HingeGradient and numClasses > 2 raise before any
        device work; empty data returns the initial weights. A Hessian that is not positive definite
        raises IllegalArgumentException."""
        _check_gradient(gradient)
        _check_updater(updater)
        if not float(regParam) >= 0.0:
            raise IllegalArgumentException(f"requirement failed: regParam must be nonnegative but got {regParam}")
        lam = float(regParam) if isinstance(updater, SquaredL2SGDUpdater) else 0.0
        history: List[float] = []
        w = np.ascontiguousarray(np.asarray(initialWeights, dtype=np.float64))

        n = data.count()
        if n == 0:
            log.warning("Newton.runNewton returning initial weights, no data found")
            return w, np.array(history)
        d = data.num_features
        _check_size(d, w.shape[0] if w.ndim == 1 else -1)

        if engine is None:
            rank, world, _ = _dist()
            engine = HipEngine(data, rank, world)

        def objective(v: np.ndarray) -> float:
            return engine.evaluate(gradient, v).lossSum / n + 0.5 * lam * float(v @ v)

        # every f is engine.evaluate's, so the line search compares sums made in one order; an accepted
        # candidate's f is the next iteration's f(w)
        f0 = objective(w) if int(numIterations) >= 1 else 0.0
        for i in range(1, int(numIterations) + 1):
            gsum = engine.to_host(engine.gradient_sum(gradient, w))
            g = gsum[:d] / n + lam * w
            history.append(f0)
            hess, _ = _hessian(engine, gradient, w, d)
            H = hess / n + lam * np.eye(d)
            try:
                L = np.linalg.cholesky(H)
            except np.linalg.LinAlgError:
                raise IllegalArgumentException(
                    "requirement failed: hessian / n + regParam I is not positive definite (collinear or "
                    "constant-zero columns, or every curvature underflowed): use regParam > 0 or drop the "
                    "dependent columns") from None
            delta = np.linalg.solve(L.T, np.linalg.solve(L, g))
            slope = float(g @ delta)
            t, w_new = 1.0, None
            for _ in range(MAX_HALVINGS + 1):
                cand = w - t * delta
                f1 = objective(cand)
                if f1 <= f0 - ARMIJO_C * t * slope:
                    w_new, f0 = cand, f1
                    break
                t *= 0.5
            if w_new is None:
                log.info("Newton iteration %d: no step passes the line search (the rounding floor)", i)
                break
            diff = math.sqrt(float((w_new - w) @ (w_new - w)))
            w = w_new
            if diff < convergenceTol * max_j(math.sqrt(float(w @ w)), 1.0):
                break
        log.info("Newton.runNewton finished. Last 10 losses %s", ", ".join(str(v) for v in history[-10:]))
        return w, np.array(history)


runNewton = Newton.runNewton
