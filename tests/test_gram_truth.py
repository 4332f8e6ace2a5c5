"""tests/gram_truth.py against a plain Python triple loop."""
import numpy as np

import gram_truth as GT


def test_truth_matches_triple_loop():
    rng = np.random.default_rng(5)
    n, d = 7, 3
    X = rng.standard_normal((n, d)).astype(np.float32)
    y = rng.standard_normal(n)
    M, A = GT.gram_truth(X, y)
    a = d + 2
    assert M.shape == A.shape == (a, a)
    rows = [[float(v) for v in X[i]] + [float(y[i]), 1.0] for i in range(n)]
    for j in range(a):
        for k in range(a):
            s = m = 0.0
            for i in range(n):
                s += rows[i][j] * rows[i][k]
                m += abs(rows[i][j] * rows[i][k])
            assert abs(M[j, k] - s) <= 1e-14 * m + 1e-300
            assert abs(A[j, k] - m) <= 1e-14 * m + 1e-300
    assert M[a - 1, a - 1] == n
    assert M[d, a - 1] == sum(r[d] for r in rows) or abs(M[d, a - 1] - sum(r[d] for r in rows)) < 1e-14 * A[d, a - 1]


def test_integer_truth_is_exact():
    rng = np.random.default_rng(6)
    X = rng.integers(-3, 4, size=(50, 4)).astype(np.float32)
    y = rng.integers(-3, 4, size=50).astype(np.float64)
    Ti = GT.gram_truth_int(X, y)
    M, _ = GT.gram_truth(X, y)
    assert (M == Ti).all()


def test_csr_to_dense_and_check():
    rows = [([0, 2], [1.5, -2.0]), ([], []), ([1], [0.0])]
    X = GT.csr_to_dense(rows, 3)
    assert X.tolist() == [[1.5, 0.0, -2.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]]
    M, A = GT.gram_truth(X, [1.0, 2.0, 3.0])
    GT.check_gramian(M, M, A)
    bad = M.copy()
    bad[0, 1] += 1.0
    try:
        GT.check_gramian(bad, M, A)
    except AssertionError:
        pass
    else:
        raise AssertionError("a wrong entry passed the check")
