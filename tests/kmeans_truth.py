"""K-means in numpy long double: the restatement the GPU tests compare against (include/psgd.h has
the definitions). s_j = ||c_j||^2 - 2 x . c_j, the assignment the first j that minimises s_j,
dist2 = max(||x||^2 + s_a, 0); a step is {sums, counts, cost, n}; an empty cluster keeps its centre."""
import numpy as np

LD = np.longdouble

# ---- the dense shapes tests/test_gpu_kmeans.py runs: d around the 4-, 8- and 16-feature steps and a
# stage of four steps, k around one, two and three centre blocks and four chunks of four blocks; every
# built rectangle of the sums (1, 2, 4 centre blocks x 2, 8 feature blocks of [x, 1]) ----
DENSE_DKS = ((1, 2, "f64"), (3, 1, "f32"), (4, 16, "f32"), (5, 17, "f64"), (8, 15, "f64"), (15, 33, "f32"),
             (16, 2, "f32"), (17, 16, "f64"), (33, 17, "f32"), (63, 15, "f32"), (64, 33, "f64"), (65, 1, "f64"),
             (300, 33, "f32"), (40, 256, "f64"), (20, 256, "f32"))
DENSE_OFF_LDS = (4096, 48)   # 4,096 x 48 doubles do not fit a CU's LDS
SIZES = (1, 3, 0, 15, 16, 17, 65, 3 * 16 + 5)


def scores(X, C):
    X, C = np.asarray(X, dtype=LD), np.asarray(C, dtype=LD)
    return (C * C).sum(axis=1)[None, :] - 2 * (X @ C.T)


def assign(X, C):
    """(assign [n], dist2 [n] long double)."""
    S = scores(X, C)
    a = np.argmin(S, axis=1)   # (the first minimum: ties to the lowest index)
    X = np.asarray(X, dtype=LD)
    d2 = np.maximum((X * X).sum(axis=1) + S[np.arange(len(a)), a], 0)
    return a.astype(np.int32), d2


def step(X, C):
    """(sums [k, d], counts [k], cost, n, assign, dist2) in long double."""
    a, d2 = assign(X, C)
    k = np.shape(C)[0]
    X = np.asarray(X, dtype=LD)
    sums = np.zeros((k, X.shape[1]), dtype=LD)
    np.add.at(sums, a, X)
    return sums, np.bincount(a, minlength=k), d2.sum(), len(a), a, d2


def update(C, sums, counts):
    C = np.asarray(C, dtype=LD)
    new = C.copy()
    live = counts > 0
    new[live] = sums[live] * (1 / counts[live].astype(LD))[:, None]
    return new, ((new - C) ** 2).sum(axis=1)


def lloyd(X, C0, maxIterations, epsilon):
    """KMeans.run: (centres, cost of the last step, iterations)."""
    C, it, changed, cost = np.asarray(C0, dtype=LD), 0, True, None
    while it < maxIterations and changed:
        sums, counts, cost, _, _, _ = step(X, C)
        C, moved = update(C, sums, counts)
        changed = bool((moved > LD(epsilon) ** 2).any())
        it += 1
    return C, cost, it


def bars(X, C, a):
    """The fp64 bar of dist2 on the sum of magnitudes, a row: 1e-9 (||x||^2 + ||c_a||^2 + 2 |x| . |c_a|)."""
    X, C = np.abs(np.asarray(X, dtype=np.float64)), np.abs(np.asarray(C, dtype=np.float64))
    return 1e-9 * ((X * X).sum(axis=1) + (C * C).sum(axis=1)[a] + 2 * (X * C[a]).sum(axis=1))


def check_gaps(X, C):
    """Every row's second-best score exceeds its best by more than twice the row's bar: the assignment is
    then decided whatever the order of the fp64 sums. Returns (assign, dist2, bars)."""
    S = scores(X, C)
    a, d2 = assign(X, C)
    bar = bars(X, C, a)
    if S.shape[1] > 1:
        part = np.partition(S, 1, axis=1)
        gap = (part[:, 1] - part[:, 0]).astype(np.float64)
        assert (gap > 2 * bar).all(), f"a tie within the bar: smallest gap / bar = {np.min(gap / bar):.3g}"
    return a, d2, bar
