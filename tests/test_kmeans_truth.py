"""tests/kmeans_truth.py against a plain triple loop (no GPU): the restatement the GPU tests trust."""
import numpy as np
import pytest

import kmeans_truth as KT


def loop_step(X, C):
    n, d = X.shape
    k = C.shape[0]
    a, d2 = np.zeros(n, dtype=np.int32), np.zeros(n)
    sums, counts = np.zeros((k, d)), np.zeros(k, dtype=np.int64)
    for i in range(n):
        best = None
        for j in range(k):
            dist = 0.0
            for f in range(d):
                dist += (float(X[i, f]) - float(C[j, f])) ** 2
            if best is None or dist < best:   # strict: ties to the lowest index
                best, a[i] = dist, j
        d2[i] = best
        sums[a[i]] += X[i]
        counts[a[i]] += 1
    return a, d2, sums, counts


@pytest.mark.parametrize("whole", [True, False])
def test_step_matches_the_loop(whole):
    rng = np.random.default_rng(5)
    X = rng.integers(-3, 4, size=(40, 3)).astype(np.float64) if whole else rng.standard_normal((40, 3))
    C = rng.integers(-3, 4, size=(5, 3)).astype(np.float64) if whole else rng.standard_normal((5, 3))
    if whole:
        C[3] = C[1]   # two equal centres: the higher index gets nothing
    a, d2, sums, counts = loop_step(X, C)
    t_sums, t_counts, t_cost, t_n, t_a, t_d2 = KT.step(X, C)
    assert (t_a == a).all() and (t_counts == counts).all() and t_n == 40
    assert np.allclose(t_d2.astype(np.float64), d2, rtol=1e-12, atol=1e-12)
    assert np.allclose(t_sums.astype(np.float64), sums, rtol=1e-12, atol=1e-12)
    assert abs(float(t_cost) - d2.sum()) <= 1e-10
    if whole:
        assert t_counts[3] == 0 and (t_d2 == d2).all()
    new, moved = KT.update(C, t_sums, t_counts)
    for j in range(5):
        want = sums[j] / counts[j] if counts[j] else C[j]
        assert np.allclose(new[j].astype(np.float64), want, rtol=1e-12, atol=1e-12)
        assert abs(float(moved[j]) - ((want - C[j]) ** 2).sum()) <= 1e-10
