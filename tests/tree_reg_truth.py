"""Plain restatements of the regression tree's passes (include/psgd.h has the definitions): every sum a Python or
int64 integer, every gain an exact fractions.Fraction. best_split asserts its precondition: a runner-up has the
winner's (nL, SL) or trails by more than 1,000 bars."""
from fractions import Fraction

import numpy as np

import tree_truth as TT


def unit(s):
    return Fraction(1 << s) if s >= 0 else Fraction(1, 1 << -s)


def targets(y):
    """(q int64 [n], ymin, s): s by search over the exact value of the fp64 difference ymax - ymin."""
    y = np.asarray(y, dtype=np.float64)
    ymin, ymax = float(y.min()) + 0.0, float(y.max()) + 0.0
    r, s = Fraction(ymax - ymin), 0
    if r > 0:
        while r * unit(s + 1) < 1 << 30:
            s += 1
        while r * unit(s) >= 1 << 30:
            s -= 1
    return np.rint(np.ldexp(y - ymin, s)).astype(np.int64), ymin, s


def bar(q, s):
    """The device's worst gain error. gain = (((SL SL) / nL + (SR SR) / nR - (S S) / n) / n) 2^-2s: three terms of two
    conversions, a product and a quotient each (4 roundings a term, relative 2^-53, the conversions counted
    once a factor), two sums and the last quotient: 15 roundings, 16 with a margin, of values no larger than
    n qmax^2 before, qmax^2 after the division by n -- the square of the label range, since the targets are
    offset from ymin and not centred. The scaling by 2^-2s is exact."""
    return 16 * 2.0 ** -53 * float(Fraction(int(np.max(q))) / unit(s)) ** 2


def moments(q, slots, A):
    out = [[0, 0, 0, 0] for _ in range(A)]
    for t, s in zip(q.tolist(), np.asarray(slots).tolist()):
        if 0 <= s < A:
            out[s] = [out[s][0] + 1, out[s][1] + t, out[s][2] + (t * t >> 30), out[s][3] + (t * t & ((1 << 30) - 1))]
    return out


def histogram(bins, q, slots, d, B, slot0=0, n_slots=1):
    H = np.zeros((n_slots, d, B, 2), dtype=np.int64)
    for r in range(len(q)):
        if 0 <= int(slots[r]) - slot0 < n_slots:
            H[int(slots[r]) - slot0, np.arange(d), bins[r, :d]] += (1, int(q[r]))
    return H


def stats(n, S, S2, ymin, s):
    """(prediction, impurity): exact rationals, rounded once each."""
    return float(Fraction(ymin) + Fraction(S, n) / unit(s)), float(Fraction(n * S2 - S * S, n * n) / unit(s) ** 2)


def best_split(H, n, S, thr, nbins, s, err, min_inst=1, min_gain=0.0):
    """H [d, B, 2] of one slot -> dict(feature, bin, threshold, gain); feature -1: a leaf. err: bar()."""
    cands = []
    for f in range(H.shape[0]):
        L = np.cumsum(H[f], axis=0)
        for b in range(nbins[f] - 1):
            nL, SL = int(L[b, 0]), int(L[b, 1])
            if nL >= min_inst and n - nL >= min_inst and nL > 0 and n - nL > 0:
                g = (Fraction(SL * SL, nL) + Fraction((S - SL) ** 2, n - nL) - Fraction(S * S, n)) / n / unit(s) ** 2
                cands.append((g, f, b, nL, SL))
    out = dict(feature=-1, bin=-1, threshold=0.0, gain=Fraction(0))
    if not cands:
        return out
    g, f, b, nL, SL = min(cands, key=lambda c: (-c[0], c[1], c[2]))
    for g2, f2, b2, nL2, SL2 in cands:
        assert (nL2, SL2) == (nL, SL) or g - g2 > 1000 * err, f"near tie: ({f}, {b}) against ({f2}, {b2}): {float(g - g2)}"
    assert abs(g) > 1000 * err or g == 0, g              # (the leaf rules too must not hang on the device's last bits)
    assert abs(g - Fraction(min_gain)) > 1000 * err or min_gain == 0.0, (g, min_gain)
    out["gain"] = g
    if g > 0 and g >= min_gain:
        out.update(feature=f, bin=b, threshold=float(thr[f, b]))
    return out


def train(X, y, thr, nbins, maxDepth=5, min_inst=1, min_gain=0.0):
    """The tree as {MLlib id: dict(feature, bin, threshold, gain, n, prediction, impurity, rows)}, each node from its own rows."""
    bins, B, d = TT.bin_rows(X, thr, nbins), thr.shape[1] + 1, X.shape[1]
    q, ymin, s = targets(y)
    err = bar(q, s)
    nodes, todo = {}, [(1, np.arange(len(y)), 0)]
    while todo:
        nid, rows, depth = todo.pop()
        (n, S, hi, lo), = moments(q[rows], np.zeros(len(rows), dtype=np.int32), 1)
        S2 = (hi << 30) + lo
        assert S2 == sum(t * t for t in q[rows].tolist())
        pred, imp = stats(n, S, S2, ymin, s)
        leaf = depth >= maxDepth or n * S2 == S * S or n < 2 * min_inst
        if not leaf:
            H = histogram(bins[rows], q[rows], np.zeros(len(rows), dtype=np.int32), d, B)[0]
            sp = best_split(H, n, S, thr, nbins, s, err, min_inst, min_gain)
            leaf = sp["feature"] < 0
        nodes[nid] = dict(feature=-1 if leaf else sp["feature"], bin=-1 if leaf else sp["bin"],
                          threshold=0.0 if leaf else sp["threshold"], gain=Fraction(0) if leaf else sp["gain"], n=n,
                          prediction=pred, impurity=imp, rows=rows)
        if not leaf:
            left = bins[rows, sp["feature"]] <= sp["bin"]
            todo += [(2 * nid, rows[left], depth + 1), (2 * nid + 1, rows[~left], depth + 1)]
    return nodes


def predict(X, nodes):
    out = np.zeros(len(X))
    for r in range(len(X)):
        nid = 1
        while nodes[nid]["feature"] >= 0:
            nid = 2 * nid + (0 if float(X[r, nodes[nid]["feature"]]) <= nodes[nid]["threshold"] else 1)
        out[r] = nodes[nid]["prediction"]
    return out
