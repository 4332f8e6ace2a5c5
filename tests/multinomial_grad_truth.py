"""A numpy restatement of the multinomial batch gradient (LogisticGradient.compute for numClasses =
K > 2 summed over a batch), on top of multiclass_truth.py, for the tests: the gradient sum G[c, j] =
sum_i mult_ic x_ij, its magnitude sum A[c, j] = sum_i |mult_ic x_ij|, lossSum, count, and the quantity
the GPU tests' precondition bounds. tests/test_multinomial_grad_truth.py checks it against
oracle/psgd_ref.py::multinomial row by row; the GPU tests take their truth from here.

A row is a dense sequence of d values or an (indices, values) pair."""
import collections

import numpy as np

import multiclass_truth as T

GradTruth = collections.namedtuple("GradTruth", "G A lossSum lossAbs count pre mult p")


def multipliers(Mg, labels):
    """From the margins [n, K - 1]: (mult [n, K - 1], p [n, K - 1], loss [n], lossAbs [n]).
    M = the maximum margin, first index on ties; when M > 0 every margin is shifted by M and the sum
    takes exp(-M) in the maximum's place; p_c = exp(m_c [- M]) / (sum + 1); mult_c = p_c - [y != 0 and
    y == c + 1]; the loss is multiclass_truth.row_loss's. lossAbs adds the magnitudes of the loss's terms."""
    Mg = np.asarray(Mg, dtype=np.float64)
    labels = np.asarray(labels, dtype=np.float64)
    n, C1 = Mg.shape
    top = Mg.max(axis=1)
    idx = Mg.argmax(axis=1)          # the first index among equals
    shift = top > 0
    sh = np.where(shift[:, None], Mg - top[:, None], Mg)
    e = np.exp(sh)
    es = e.copy()
    es[shift, idx[shift]] = np.exp(-top[shift])
    s = es.sum(axis=1)
    p = e / (s + 1.0)[:, None]
    classes = np.arange(1, C1 + 1, dtype=np.float64)
    ind = (labels[:, None] != 0.0) & (labels[:, None] == classes[None, :])
    mult = p - ind
    ly = np.array([T._d2i(float(y)) - 1 for y in labels], dtype=np.int64)
    has = (ly >= 0) & (ly < C1)
    margin_y = np.where(has, Mg[np.arange(n), np.clip(ly, 0, C1 - 1)], 0.0)
    pos = labels > 0.0
    loss = np.log1p(s) - np.where(pos, margin_y, 0.0) + np.where(shift, top, 0.0)
    loss_abs = np.abs(np.log1p(s)) + np.where(pos, np.abs(margin_y), 0.0) + np.where(shift, np.abs(top), 0.0)
    return mult, p, loss, loss_abs


def _scatter(coef, rows, d):
    """sum_i coef[i, c] * x_ij -> [K - 1, d]."""
    C1 = coef.shape[1]
    if len(rows) and not isinstance(rows[0], tuple):
        return coef.T @ np.asarray(rows, dtype=np.float64).reshape(len(rows), d)
    out = np.zeros((C1, d))
    for i, (idx, val) in enumerate(rows):
        if len(idx):
            np.add.at(out, (slice(None), np.asarray(idx, dtype=np.int64)),
                      np.outer(coef[i], np.asarray(val, dtype=np.float64)))
    return out


def _abs_rows(rows):
    return [(r[0], np.abs(np.asarray(r[1], dtype=np.float64))) if isinstance(r, tuple)
            else np.abs(np.asarray(r, dtype=np.float64)) for r in rows]


def gradient(rows, labels, w, K: int, d: int) -> GradTruth:
    """The batch sums over `rows` at weights w ((K - 1) * d). pre[c, j] = sum_i e_ic |x_ij| with
    e_ic = 2 p_ic max_k(nnz_i 2^-52 sum_j |x_ij W_kj|): the bound on what margins summed in another
    order can move G[c, j] (a multiplier's derivative in any margin is at most p_ic in magnitude, and
    up to two margins -- its own and the maximum's -- carry the error)."""
    rows = list(rows)
    n = len(rows)
    C1 = K - 1
    if n == 0:
        z = np.zeros((C1, d))
        return GradTruth(z, z.copy(), 0.0, 0.0, 0, z.copy(), np.zeros((0, C1)), np.zeros((0, C1)))
    Mg = T.margins(rows, w, K)
    mult, p, loss, loss_abs = multipliers(Mg, labels)
    G = _scatter(mult, rows, d)
    ar = _abs_rows(rows)
    A = _scatter(np.abs(mult), ar, d)
    am = T.abs_margins(rows, w, K).max(axis=1)
    e = 2.0 * p * (T.nnz(rows) * 2.0 ** -52 * am)[:, None]
    pre = _scatter(e, ar, d)
    return GradTruth(G, A, T.sum_left_to_right(loss), float(loss_abs.sum()), n, pre, mult, p)


def flat(t: GradTruth) -> np.ndarray:
    """{gradientSum[(K - 1) d], lossSum, count} as the calls return it."""
    return np.concatenate([t.G.ravel(), [t.lossSum, float(t.count)]])
