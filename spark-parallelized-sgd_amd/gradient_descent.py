"""GradientDescent -- MLlib 1.6.1's mini-batch gradient descent, the optimizer ParallelizedSGD was
written to replace, over the same registered partitions: one batch gradient at fixed weights per
iteration (psgd_gradient_sum_device, or psgd_gradient_sum_multinomial_device for
LogisticGradient(numClasses > 2): a HIP pass, the treeAggregate of runMiniBatchSGD) and one
stateless update (psgd_gd_update_device). Registering the data once, a user runs both optimizers on
the same device copy and compares loss histories and time per outer iteration.

[ext] MLlib 1.6.1 org/apache/spark/mllib/optimization/GradientDescent.scala
  class GradientDescent(gradient, updater)   -> class GradientDescent below
  object GradientDescent.runMiniBatchSGD     -> GradientDescent.runMiniBatchSGD, statement for statement
"""
from __future__ import annotations

import collections
import logging
import math
from typing import List

import numpy as np

from . import _native as N
from .data import PartitionedData
from .gradient import Gradient, LogisticGradient, gradient_kind, num_classes
from .optimization import (HipEngine, IllegalArgumentException, ParallelizedSGD, _dist, _weights_size,
                           check_multinomial_weights, check_num_classes, make_params, max_j)
from .updater import AdaGradSGDUpdater, AdamSGDUpdater, SGDUpdater, updater_kind

log = logging.getLogger("org.apache.spark.mllib.optimization.GradientDescent")

# treeAggregate's (gradientSum, lossSum, miniBatchSize) at fixed weights
GradientSum = collections.namedtuple("GradientSum", "gradient lossSum count")


def _check_updater(updater: SGDUpdater) -> None:
    if isinstance(updater, (AdaGradSGDUpdater, AdamSGDUpdater)):
        raise N.UnsupportedOperationException(
            f"GradientDescent takes a stateless updater (Simple, SquaredL2, L1): "
            f"{type(updater).__name__} keeps a status per chain")
    updater_kind(updater)


def _check_batch_kinds(gradient: Gradient, updater: SGDUpdater = None, call: str = "gradient_sum_multinomial") -> None:
    """What the binary batch passes refuse, before any device work."""
    if num_classes(gradient) > 2:
        raise N.UnsupportedOperationException(
            f"the multinomial LogisticGradient (numClasses > 2) goes through {call}")
    gradient_kind(gradient)
    if updater is not None:
        _check_updater(updater)


def _check_multinomial_kinds(gradient: Gradient, updater: SGDUpdater = None) -> int:
    """What the multinomial batch passes refuse, before any device work -> K."""
    if not isinstance(gradient, LogisticGradient) or num_classes(gradient) < 3:
        raise IllegalArgumentException(
            "requirement failed: the multinomial batch gradient needs LogisticGradient(numClasses > 2); "
            "a binary gradient goes through gradient_sum / runMiniBatchSGD")
    if updater is not None:
        _check_updater(updater)
    return check_num_classes(num_classes(gradient))


def _check_fraction(miniBatchFraction: float) -> None:
    if not (0.0 <= miniBatchFraction <= 1.0):
        raise IllegalArgumentException(
            f"requirement failed: Sampling fraction ({miniBatchFraction}) must be on interval [0, 1]")


def gradient_sum(data: PartitionedData, gradient: Gradient, weights, miniBatchFraction: float = 1.0,
                 iteration: int = 0, *, engine=None) -> GradientSum:
    """The gradient of the loss at fixed `weights` (a host array or a device tensor of num_features
    doubles) summed over the batch: every row, or RDD.sample(false, miniBatchFraction, 42 +
    iteration) per partition. gradient / count is the slope of evaluate()'s meanLoss; its norm at an
    optimizer's result is the standard check that it finished. The engine reuses the device
    context's registration as evaluate() does. LogisticGradient(numClasses > 2) raises
    UnsupportedOperationException: gradient_sum_multinomial takes it."""
    _check_batch_kinds(gradient)
    _check_fraction(miniBatchFraction)
    if data.num_partitions == 0:
        return GradientSum(np.zeros(0), 0.0, 0)
    if engine is None:
        rank, world, _ = _dist()
        engine = HipEngine(data, rank, world)
    h = engine.to_host(engine.gradient_sum(gradient, weights, miniBatchFraction, iteration))
    return GradientSum(h[:-2].copy(), float(h[-2]), int(h[-1]))


def gradient_sum_multinomial(data: PartitionedData, gradient: Gradient, weights, miniBatchFraction: float = 1.0,
                             iteration: int = 0, *, engine=None) -> GradientSum:
    """gradient_sum() for LogisticGradient(numClasses = K > 2): `weights` are (K - 1) * num_features
    doubles in K - 1 class blocks (class 0 the pivot), and so is the gradient -- the slope of
    evaluate_multinomial()'s lossSum (psgd_gradient_sum_multinomial). A binary gradient raises
    IllegalArgumentException."""
    K = _check_multinomial_kinds(gradient)
    _check_fraction(miniBatchFraction)
    if data.num_partitions == 0:
        return GradientSum(np.zeros(0), 0.0, 0)
    check_multinomial_weights(K, data.num_features, _weights_size(weights))
    if engine is None:
        rank, world, _ = _dist()
        engine = HipEngine(data, rank, world, weight_dim=(K - 1) * data.num_features)
    h = engine.to_host(engine.gradient_sum_multinomial(K, weights, miniBatchFraction, iteration))
    return GradientSum(h[:-2].copy(), float(h[-2]), int(h[-1]))


class GradientDescent(ParallelizedSGD):
    """MLlib 1.6.1 GradientDescent(gradient, updater): the defaults (stepSize 1.0, numIterations 100,
    regParam 0.0, miniBatchFraction 1.0, convergenceTol 0.001) and this package's validated setters
    (ParallelizedSGD's, same messages); optimize(data, initialWeights) -> weights. The arithmetic is
    fp64: setComputeDtype("f32") is refused."""

    def setComputeDtype(self, dtype: str) -> "GradientDescent":
        if dtype != "f64":
            raise N.UnsupportedOperationException("GradientDescent computes in fp64 only")
        return self

    def optimize(self, data: PartitionedData, initialWeights) -> np.ndarray:
        run = (GradientDescent.runMiniBatchSGDMultinomial if num_classes(self.gradient) > 2
               else GradientDescent.runMiniBatchSGD)
        weights, _ = run(
            data, self.gradient, self.updater, self.stepSize, self.numIterations, self.regParam,
            self.miniBatchFraction, initialWeights, self.convergenceTol)
        return weights

    @staticmethod
    def runMiniBatchSGD(data: PartitionedData, gradient: Gradient, updater: SGDUpdater, stepSize: float,
                        numIterations: int, regParam: float, miniBatchFraction: float, initialWeights,
                        convergenceTol: float = 0.001, *, engine=None):
        """GradientDescent.runMiniBatchSGD -> (weights, stochasticLossHistory). The weights stay on
        the device; the host reads lossSum, count and regVal per iteration. AdaGrad / Adam updaters
        raise before any device work, and so does numClasses > 2: runMiniBatchSGDMultinomial takes it."""
        _check_batch_kinds(gradient, updater, "runMiniBatchSGDMultinomial")

        def check_size(nf, size):
            if size != nf:
                raise IllegalArgumentException(
                    f"requirement failed: BLAS.dot(x: Vector, y: Vector) was given Vectors with "
                    f"non-matching sizes: x.size = {nf}, y.size = {size}")

        return _mini_batch_sgd(data, gradient, updater, stepSize, numIterations, regParam, miniBatchFraction,
                               initialWeights, convergenceTol, engine, check_size, lambda nf: nf,
                               lambda eng, w, i: eng.gradient_sum(gradient, w, miniBatchFraction, i))

    @staticmethod
    def runMiniBatchSGDMultinomial(data: PartitionedData, gradient: Gradient, updater: SGDUpdater, stepSize: float,
                                   numIterations: int, regParam: float, miniBatchFraction: float, initialWeights,
                                   convergenceTol: float = 0.001, *, engine=None):
        """runMiniBatchSGD for LogisticGradient(numClasses = K > 2), the same loop: the weights are
        (K - 1) * num_features doubles (MLlib's require on weights.size), the batch pass is
        HipEngine.gradient_sum_multinomial. Simple, SquaredL2 and L1 updaters; a binary gradient
        raises IllegalArgumentException before any device work."""
        K = _check_multinomial_kinds(gradient, updater)
        return _mini_batch_sgd(data, gradient, updater, stepSize, numIterations, regParam, miniBatchFraction,
                               initialWeights, convergenceTol, engine,
                               lambda nf, size: check_multinomial_weights(K, nf, size), lambda nf: (K - 1) * nf,
                               lambda eng, w, i: eng.gradient_sum_multinomial(K, w, miniBatchFraction, i))


def _mini_batch_sgd(data, gradient, updater, stepSize, numIterations, regParam, miniBatchFraction, initialWeights,
                    convergenceTol, engine, check_size, weight_dim, batch_sum):
    """The body of GradientDescent.runMiniBatchSGD, statement for statement; check_size(num_features,
    weights.size) is the gradient's require, batch_sum(engine, weights, i) its treeAggregate."""
    if miniBatchFraction < 1.0 and convergenceTol > 0.0:
        log.warning("Testing against a convergenceTol when using miniBatchFraction "
                    "< 1.0 can be unstable because of the stochasticity in sampling.")
    history: List[float] = []
    w0 = np.ascontiguousarray(np.asarray(initialWeights, dtype=np.float64))

    numExamples = data.count()
    if numExamples == 0:
        log.warning("GradientDescent.runMiniBatchSGD returning initial weights, no data found")
        return w0, np.array(history)
    if numExamples * miniBatchFraction < 1:
        log.warning("The miniBatchFraction is too small")
    nf = data.num_features
    check_size(nf, w0.shape[0] if w0.ndim == 1 else -1)

    if engine is None:
        rank, world, _ = _dist()
        engine = HipEngine(data, rank, world, weight_dim=weight_dim(nf))

    weights = engine.weights(w0)
    # regVal = updater.compute(weights, zeros, 0, 1, regParam)._2
    regVal = engine.initial_regval(make_params(gradient, updater, stepSize, regParam, miniBatchFraction,
                                               convergenceTol), w0)
    previousWeights = None
    currentWeights = None
    converged = False
    i = 1
    while not converged and i <= numIterations:
        # data.sample(false, miniBatchFraction, 42 + i).treeAggregate(..)
        gsum = batch_sum(engine, weights, i)
        lossSum, miniBatchSize = engine.batch_scalars(gsum)
        if miniBatchSize > 0:
            # lossSum is computed with the weights of the previous iteration: so is regVal
            history.append(lossSum / miniBatchSize + regVal)
            weights, regVal = engine.gd_update(updater, weights, gsum, stepSize, i, regParam)
            previousWeights = currentWeights
            currentWeights = weights
            if previousWeights is not None and currentWeights is not None:
                dsq, nsq = engine.convergence_terms(previousWeights, currentWeights)
                converged = math.sqrt(dsq) < convergenceTol * max_j(math.sqrt(nsq), 1.0)
        else:
            log.warning("Iteration (%d/%d). The size of sampled batch is zero", i, numIterations)
        i += 1
    log.info("GradientDescent.runMiniBatchSGD finished. Last 10 stochastic losses %s",
             ", ".join(str(v) for v in history[-10:]))
    return engine.to_host(weights), np.array(history)


runMiniBatchSGD = GradientDescent.runMiniBatchSGD
runMiniBatchSGDMultinomial = GradientDescent.runMiniBatchSGDMultinomial
