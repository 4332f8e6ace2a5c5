"""tests/multinomial_grad_truth.py (the GPU tests' numpy truth of the multinomial batch gradient) against
oracle/psgd_ref.py::multinomial, row by row and summed. No device.

The two differ in summation order only (numpy's dot against the oracle's left-to-right loop), so G
and the loss agree within 1e-12 of their magnitude sums."""
import numpy as np
import pytest

import multinomial_grad_truth as GT


def ref():
    import psgd_ref
    return psgd_ref


def dense_rows(n, d, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d))
    x[rng.random((n, d)) < 0.1] = 0.0
    return [[float(v) for v in row] for row in x]


def sparse_rows(n, d, seed):
    rng = np.random.default_rng(seed)
    rows = []
    for k in range(n):
        m = k % (d + 1)   # 0 .. d non-zeros, an empty row among them
        idx = np.sort(rng.choice(d, size=m, replace=False))
        rows.append(([int(i) for i in idx], [float(v) for v in rng.standard_normal(m)]))
    return rows


def labels_for(n, K):
    """0, K - 1 and the labels that are no class (K, -1, 2.5) among the classes in turn."""
    special = [0.0, float(K - 1), float(K), -1.0, 2.5]
    return [special[k] if k < len(special) else float(k % K) for k in range(n)]


def check(rows, labels, w, K, d):
    """Row by row and over the whole batch: G within 1e-12 A, the loss within 1e-12 of its terms'
    magnitudes."""
    R = ref()
    C1 = K - 1
    total = np.zeros(C1 * d)
    loss_total = 0.0
    saw_shift = saw_no_shift = False
    for k, row in enumerate(rows):
        (kind, g), loss = R.multinomial(row, float(labels[k]), [float(v) for v in w], K)
        assert kind == "dense"
        one = GT.gradient([row], [labels[k]], w, K, d)
        g = np.array(g).reshape(C1, d)
        assert np.all(np.abs(one.G - g) <= 1e-12 * one.A), (k, np.max(np.abs(one.G - g)))
        assert abs(one.lossSum - loss) <= 1e-12 * one.lossAbs, (k, one.lossSum, loss)
        assert one.count == 1
        top = GT.T.margins([row], w, K).max()
        saw_shift |= bool(top > 0)
        saw_no_shift |= bool(top <= 0)
        total += g.ravel()
        loss_total += loss
    t = GT.gradient(rows, labels, w, K, d)
    assert np.all(np.abs(t.G.ravel() - total) <= 1e-12 * t.A.ravel())
    assert abs(t.lossSum - loss_total) <= 1e-12 * t.lossAbs
    assert t.count == len(rows)
    assert np.array_equal(GT.flat(t)[-2:], [t.lossSum, float(len(rows))])
    return saw_shift, saw_no_shift


@pytest.mark.parametrize("K", [3, 4, 10, 66])
@pytest.mark.parametrize("layout", ["dense", "sparse"])
def test_gradient_and_loss_match_the_oracle(layout, K):
    d, n = 5, 14
    rows = dense_rows(n, d, 10 + K) if layout == "dense" else sparse_rows(n, d, 20 + K)
    w = np.random.default_rng(K).standard_normal((K - 1) * d)
    labels = labels_for(n, K)
    # a row whose maximum margin is <= 0 (the zero row: every margin is 0) among rows with a positive one
    rows[5] = [0.0] * d if layout == "dense" else ([], [])
    shift, no_shift = check(rows, labels, w, K, d)
    assert shift and no_shift


@pytest.mark.parametrize("K", [3, 10])
def test_negative_margins_without_shift(K):
    d = 4
    rng = np.random.default_rng(K)
    rows = [[float(v) for v in np.abs(rng.standard_normal(d))] for _ in range(6)]
    w = -np.abs(rng.standard_normal((K - 1) * d))       # every margin < 0: no shift
    shift, no_shift = check(rows, labels_for(6, K), w, K, d)
    assert no_shift and not shift


@pytest.mark.parametrize("K", [3, 4, 66])
def test_identical_class_blocks_are_exact_ties(K):
    d, n = 3, 7
    rows = dense_rows(n, d, 5)
    block = np.random.default_rng(9).standard_normal(d)
    w = np.tile(block, K - 1)
    labels = labels_for(n, K)
    check(rows, labels, w, K, d)
    t = GT.gradient(rows, labels, w, K, d)
    # every class has the same probability; the first index holds the maximum
    assert np.all(t.p == t.p[:, :1])
    R = ref()
    for k, row in enumerate(rows):
        (_, g), _ = R.multinomial(row, 0.0, [float(v) for v in w], K)
        g = np.array(g).reshape(K - 1, d)
        assert np.all(g == g[:1])    # the oracle's blocks are bit-identical too


def test_precondition_quantity_by_hand():
    # one row x = (2, 0, -1), K = 3, W = [[1, 5, 1], [0, 0, 0]]: margins (1, 0), shifted (0, -1),
    # sum = exp(-1) + exp(-1), p = (1, exp(-1)) / (sum + 1)
    w = np.array([1.0, 5.0, 1.0, 0.0, 0.0, 0.0])
    t = GT.gradient([[2.0, 0.0, -1.0]], [2.0], w, 3, 3)
    s = 2.0 * np.exp(-1.0)
    p = np.array([1.0, np.exp(-1.0)]) / (s + 1.0)
    assert np.allclose(t.p[0], p, rtol=1e-15)
    assert np.allclose(t.mult[0], p - np.array([0.0, 1.0]), rtol=1e-15)
    # nnz counts the stored values (3), the margins' magnitude sums are (3, 0)
    e = 2.0 * p * (3 * 2.0 ** -52 * 3.0)
    assert np.allclose(t.pre, np.outer(e, [2.0, 0.0, 1.0]), rtol=1e-15)
    assert np.allclose(t.A, np.outer(np.abs(t.mult[0]), [2.0, 0.0, 1.0]), rtol=1e-15)
    # an (indices, values) row gives the same sums with nnz = 2
    ts = GT.gradient([([0, 2], [2.0, -1.0])], [2.0], w, 3, 3)
    assert np.array_equal(ts.G, t.G) and np.array_equal(ts.A, t.A) and ts.lossSum == t.lossSum
    assert np.allclose(ts.pre, t.pre * 2 / 3, rtol=1e-15)


def test_empty_batch():
    t = GT.gradient([], [], np.zeros(6), 3, 3)
    assert t.count == 0 and t.lossSum == 0.0 and not t.G.any() and t.G.shape == (2, 3)
