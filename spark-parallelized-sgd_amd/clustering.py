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

from ._native import GMM_MAX_D, GMM_MAX_K, KMEANS_MAX_K, IllegalArgumentException, UnsupportedOperationException
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


# ---- MLlib 1.6.1 clustering.GaussianMixture ----
#
#   model = GaussianMixture(k, convergenceTol=0.01, maxIterations=100, seed=7).run(data)
#   model.weights, model.gaussians       # [k], k stat.MultivariateGaussian
#   model.predict(data), model.predictSoft(data)     # per-partition device tensors
#   GaussianMixture(k).setInitialModel(GaussianMixtureModel.fromKMeans(kmeans_model, data)).run(data)
#
# An EM step is two passes on the device (HipEngine.gmm_step: the responsibilities, then the k weighted
# moment matrices; include/psgd.h has the arithmetic). The host makes the next model from the moments S_j:
# W_j = S_j[d][d], mu_j = S_j[:d, d] / W_j, Sigma_j = S_j[:d, :d] / W_j - mu_j mu_j^T, w_j = W_j / sum W, and
# the constants of each component (stat.MultivariateGaussian: k eigh calls). The loop is MLlib's: while
# iter < maxIterations and |llh - llhPrev| > convergenceTol, llhPrev starting at the most negative double.
# Without an initial model 5 k distinct row positions are drawn from numpy.random.default_rng(seed) (this
# project's convention, not Spark's) and read as the engine registered them; consecutive fives are
# grouped, mu_j their mean, Sigma_j the diagonal of their sample variance, w_j = 1 / k.
# logLikelihood and numIterations on the returned model are this project's additions.

class GaussianMixtureStep(NamedTuple):
    moments: np.ndarray       # [k, d + 1, d + 1]: sum r_j z z^T, z = [x, 1]
    logLikelihood: float      # the sum of ln P over the rows
    count: int                # the rows


def _check_mixture(weights, gaussians, d: int):
    from .stat import MultivariateGaussian
    w = np.ascontiguousarray(weights, dtype=np.float64)
    gaussians = list(gaussians)
    k = len(gaussians)
    if w.ndim != 1 or w.shape[0] != k or k < 1:
        raise IllegalArgumentException(
            f"requirement failed: Length of weight and Gaussian arrays must match (got {w.shape} and {k})")
    if k > GMM_MAX_K:
        raise IllegalArgumentException(f"requirement failed: a mixture takes at most {GMM_MAX_K} components (got {k})")
    if not np.all(w > 0.0):
        raise IllegalArgumentException("requirement failed: the weights of a mixture must be positive")
    for g in gaussians:
        if not isinstance(g, MultivariateGaussian):
            raise IllegalArgumentException("requirement failed: the components must be stat.MultivariateGaussian")
        if d is not None and g.mu.shape[0] != d:
            raise IllegalArgumentException(
                f"requirement failed: vector sizes do not match: Expected {g.mu.shape[0]} but found {d}")
    return w, gaussians


def _check_dense(data: PartitionedData):
    from .data import CsrPartition, DeviceCsrPartition
    if any(isinstance(p, (CsrPartition, DeviceCsrPartition)) for p in data.partitions):
        raise IllegalArgumentException("requirement failed: the Gaussian mixture needs dense rows (the partitions are CSR)")
    if data.num_features > GMM_MAX_D:
        raise IllegalArgumentException(
            f"requirement failed: the Gaussian mixture takes at most {GMM_MAX_D} features (got {data.num_features})")


def _split_gmm_step(h: np.ndarray, k: int, d: int) -> GaussianMixtureStep:
    a = d + 1
    return GaussianMixtureStep(h[: k * a * a].reshape(k, a, a), float(h[k * a * a]), int(h[k * a * a + 1]))


def _m_step(moments: np.ndarray):
    """(weights, gaussians) from the moments [k, d + 1, d + 1]: MLlib's updateWeightsAndGaussians."""
    from .stat import MultivariateGaussian
    d = moments.shape[1] - 1
    W = moments[:, d, d]
    gaussians = []
    for S, Wj in zip(moments, W):
        mu = S[:d, d] / Wj
        gaussians.append(MultivariateGaussian(mu, S[:d, :d] / Wj - np.outer(mu, mu)))
    return W / np.sum(W), gaussians


def gmm_step(data: PartitionedData, weights, gaussians, *, engine=None) -> GaussianMixtureStep:
    """One EM step of the mixture over every row of every partition, on all ranks (HipEngine.gmm_step):
    the sibling of kmeans_step."""
    _check_dense(data)
    w, gaussians = _check_mixture(weights, gaussians, data.num_features)
    engine = _engine_for(data, engine)
    return _split_gmm_step(engine.gmm_step(w, gaussians).cpu().numpy(), len(gaussians), data.num_features)


class GaussianMixtureModel:
    """MLlib GaussianMixtureModel(weights, gaussians)."""

    def __init__(self, weights, gaussians):
        self.weights, self.gaussians = _check_mixture(weights, gaussians, None)
        self.logLikelihood = None
        self.numIterations = None

    @property
    def k(self) -> int:
        return len(self.gaussians)

    def _per_partition(self, data: PartitionedData, engine, rows):
        out, at = [], 0
        for p, part in enumerate(data.partitions):
            n = part.n_rows if engine.lo <= p < engine.hi else 0
            out.append(rows[at: at + n])
            at += n
        return out

    def predictSoft(self, data: PartitionedData, *, engine=None):
        """The responsibilities of every row: one device [n, k] f64 tensor per partition of `data` (empty for
        another rank's partitions)."""
        _check_dense(data)
        _check_mixture(self.weights, self.gaussians, data.num_features)
        engine = _engine_for(data, engine)
        resp, _, _ = engine.gmm_responsibilities(self.weights, self.gaussians)
        return self._per_partition(data, engine, resp)

    def predict(self, data: PartitionedData, *, engine=None):
        """The component of the largest responsibility of every row, the first of equals: one device int32
        tensor per partition."""
        import torch
        return [r.argmax(dim=1).to(torch.int32) if r.shape[0] else r.new_zeros(0, dtype=torch.int32)
                for r in self.predictSoft(data, engine=engine)]

    @classmethod
    def fromKMeans(cls, model: KMeansModel, data: PartitionedData, *, engine=None) -> "GaussianMixtureModel":
        """The usual warm start: the means are the k-means centres, the covariances and weights those of
        the clusters (one gmm_moments call on the one-hot responsibilities of the assignment). Every
        cluster must hold rows that span a covariance."""
        import torch
        _check_dense(data)
        engine = _engine_for(data, engine)
        assign, _ = engine.kmeans_assign(model.clusterCenters)
        onehot = torch.nn.functional.one_hot(assign.to(torch.int64), model.k).to(torch.float64)
        d = data.num_features
        S = engine.gmm_moments(onehot).cpu().numpy().reshape(model.k, d + 1, d + 1)
        if not np.all(S[:, d, d] > 0.0):
            raise IllegalArgumentException("requirement failed: fromKMeans needs rows in every cluster")
        weights, gaussians = _m_step(S)
        return cls(weights, gaussians)


class GaussianMixture:
    """MLlib 1.6.1 GaussianMixture (the comment above has the loop and the initialisation)."""

    N_SAMPLES = 5   # rows drawn a component (MLlib's nSamples)

    def __init__(self, k: int = 2, convergenceTol: float = 0.01, maxIterations: int = 100, seed=None):
        if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)) or int(k) < 1:
            raise IllegalArgumentException(f"requirement failed: Number of Gaussians must be positive but got {k!r}")
        if int(k) > GMM_MAX_K:
            raise IllegalArgumentException(f"requirement failed: a mixture takes at most {GMM_MAX_K} components (got {k})")
        if isinstance(maxIterations, (bool, np.bool_)) or int(maxIterations) < 0:
            raise IllegalArgumentException(
                f"requirement failed: Maximum of iterations must be nonnegative but got {maxIterations!r}")
        if not float(convergenceTol) >= 0.0:
            raise IllegalArgumentException(
                f"requirement failed: Convergence tolerance must be nonnegative but got {convergenceTol!r}")
        self.k, self.convergenceTol, self.maxIterations = int(k), float(convergenceTol), int(maxIterations)
        self.seed = seed
        self.initialModel = None

    def setInitialModel(self, model: GaussianMixtureModel) -> "GaussianMixture":
        if model.k != self.k:
            raise IllegalArgumentException(
                f"requirement failed: Mismatched cluster count (model.k {model.k} != k {self.k})")
        self.initialModel = model
        return self

    def _initial_model(self, data: PartitionedData, engine):
        from .stat import MultivariateGaussian
        if self.initialModel is not None:
            return _check_mixture(self.initialModel.weights, self.initialModel.gaussians, data.num_features)
        counts = getattr(data, "partition_counts", None)
        n = int(np.sum(counts)) if counts is not None else data.count()
        m = self.N_SAMPLES
        if n < m * self.k:
            raise IllegalArgumentException(
                f"requirement failed: the initialisation needs at least 5 k = {m * self.k} rows (got {n})")
        positions = np.random.default_rng(self.seed).choice(n, size=m * self.k, replace=False)
        rows = np.ascontiguousarray(engine.registered_rows(positions), dtype=np.float64)
        gaussians = []
        for j in range(self.k):
            x = rows[j * m: (j + 1) * m]
            mu = x.sum(axis=0) / m                                   # vectorMean
            var = ((x * x).sum(axis=0) - m * mu * mu) / (m - 1)      # initCovariance: diag(ss / n - mu^2) n / (n - 1)
            gaussians.append(MultivariateGaussian(mu, np.diag(var)))
        return np.full(self.k, 1.0 / self.k), gaussians

    def run(self, data: PartitionedData, *, engine=None) -> GaussianMixtureModel:
        if data.num_partitions == 0:
            raise IllegalArgumentException("requirement failed: Cannot fit a mixture on data without partitions.")
        _check_dense(data)
        if self.initialModel is not None:   # (the refusal fires before any engine is touched)
            _check_mixture(self.initialModel.weights, self.initialModel.gaussians, data.num_features)
        engine = _engine_for(data, engine)
        weights, gaussians = self._initial_model(data, engine)
        k, d = self.k, data.num_features
        llh, llh_prev = -np.finfo(np.float64).max, 0.0
        iteration = 0
        while iteration < self.maxIterations and abs(llh - llh_prev) > self.convergenceTol:
            step = _split_gmm_step(engine.gmm_step(weights, gaussians).cpu().numpy(), k, d)
            weights, gaussians = _m_step(step.moments)
            llh_prev, llh = llh, step.logLikelihood
            iteration += 1
        model = GaussianMixtureModel(weights, gaussians)
        model.logLikelihood = llh if iteration else None
        model.numIterations = iteration
        return model
