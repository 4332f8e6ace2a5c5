"""Plain numpy restatements of the decision tree's passes (include/psgd.h has the definitions): integer counts, gains in
numpy.longdouble. best_split asserts its precondition: a runner-up has the winner's count vector or trails by > 1,000 bars."""
import numpy as np

LD = np.longdouble


def bar(K):
    """The device's worst gain error: about 4 K + 10 rounded operations on values of size <= max(1, log2 K)."""
    return 64 * K * 2.0 ** -53 * max(1.0, np.log2(K))


def ragged_thresholds(X, maxBins, seed=0):
    """(thr [d, maxBins - 1] padded with +Inf, nbins [d]): 1 + (f + seed) % (maxBins - 1) of feature f's own values."""
    n, d = X.shape
    thr, nbins = np.full((d, maxBins - 1), np.inf), np.ones(d, dtype=np.int32)
    for f in range(d):
        vals = np.unique(X[:, f].astype(np.float64))
        t = np.unique(vals[np.linspace(0, len(vals) - 1, min(len(vals), 1 + (f + seed) % (maxBins - 1))).astype(int)])
        thr[f, : len(t)], nbins[f] = t, len(t) + 1
    return thr, nbins


def bin_rows(X, thr, nbins):
    n, d = X.shape
    out = np.zeros((n, 16 * ((d + 15) // 16)), dtype=np.uint8)
    for f in range(d):
        t = thr[f, : nbins[f] - 1]
        out[:, f] = (X[:, f].astype(np.float64)[:, None] > t[None, :]).sum(axis=1)
    return out


def histogram(bins, y, slots, d, B, K, slot0=0, n_slots=1):
    H = np.zeros((n_slots, d, B, K), dtype=np.int64)   # (labels are whole numbers in [0, K) here)
    for r in range(len(y)):
        if 0 <= int(slots[r]) - slot0 < n_slots:
            H[int(slots[r]) - slot0, np.arange(d), bins[r, :d], int(y[r])] += 1
    return H


def impurity(c, kind):
    c = np.asarray(c, dtype=LD)
    n = c.sum()
    if n == 0:
        return LD(0)
    q = c[c > 0] / n
    return 1 - (q * q).sum() if kind == "gini" else -(q * np.log(q)).sum() / np.log(LD(2))


def best_split(H, thr, nbins, kind="gini", min_inst=1, min_gain=0.0):
    """H [d, B, K] of one slot -> dict(feature, bin, threshold, gain, impurity, n, tot, L); feature -1: a leaf."""
    d, B, K = H.shape
    tot = H[0].sum(axis=0)
    n = int(tot.sum())
    imp_t = impurity(tot, kind)
    cands = []
    for f in range(d):
        L = np.cumsum(H[f], axis=0)
        for b in range(nbins[f] - 1):
            nL = int(L[b].sum())
            if nL >= min_inst and n - nL >= min_inst and nL > 0 and n - nL > 0:
                gain = imp_t - LD(nL) / n * impurity(L[b], kind) - LD(n - nL) / n * impurity(tot - L[b], kind)
                cands.append((gain, f, b, L[b]))
    out = dict(feature=-1, bin=-1, threshold=0.0, gain=LD(0), impurity=imp_t, n=n, tot=tot, L=np.zeros(K, dtype=np.int64))
    if not cands:
        return out
    g, f, b, L = min(cands, key=lambda c: (-c[0], c[1], c[2]))
    for g2, f2, b2, L2 in cands:
        assert (L2 == L).all() or g - g2 > 1000 * bar(K), f"near tie: ({f}, {b}) {g} against ({f2}, {b2}) {g2}"
    assert abs(g) > 1000 * bar(K) or g == 0, g         # (the leaf rules too must not hang on the device's last bits)
    assert abs(g - min_gain) > 1000 * bar(K) or min_gain == 0.0, (g, min_gain)
    out["gain"] = g
    if g > 0 and g >= min_gain:
        out.update(feature=f, bin=b, threshold=float(thr[f, b]), L=L)
    return out


def route(bins, slots, table):
    out = np.full(len(slots), -1, dtype=np.int32)
    for r, s in enumerate(slots):
        if 0 <= s < len(table) and table[s][0] >= 0:
            f, b, left, right = table[s]
            out[r] = left if bins[r, f] <= b else right
    return out


def train(X, y, K, thr, nbins, kind="gini", maxDepth=5, min_inst=1, min_gain=0.0):
    """The tree as {MLlib id: dict(feature, bin, threshold, gain, counts)}, each node from its own rows."""
    bins, B = bin_rows(X, thr, nbins), thr.shape[1] + 1
    nodes, todo = {}, [(1, np.arange(len(y)), 0)]
    while todo:
        nid, rows, depth = todo.pop()
        H = histogram(bins[rows], y[rows], np.zeros(len(rows), dtype=np.int32), X.shape[1], B, K)
        tot = H[0, 0].sum(axis=0)
        leaf = depth >= maxDepth or (np.count_nonzero(tot) <= 1 and nid > 1)   # (a finished child is not examined)
        s = None if leaf else best_split(H[0], thr, nbins, kind, min_inst, min_gain)
        leaf = leaf or s["feature"] < 0
        nodes[nid] = dict(feature=-1 if leaf else s["feature"], bin=-1 if leaf else s["bin"],
                          threshold=0.0 if leaf else s["threshold"], gain=LD(0) if leaf else s["gain"], counts=tot)
        if not leaf:
            go_left = bins[rows, s["feature"]] <= s["bin"]
            todo += [(2 * nid, rows[go_left], depth + 1), (2 * nid + 1, rows[~go_left], depth + 1)]
    return nodes


def predict(X, nodes):
    out = np.zeros(len(X), dtype=np.int32)
    for r in range(len(X)):
        nid = 1
        while nodes[nid]["feature"] >= 0:
            nid = 2 * nid + (0 if float(X[r, nodes[nid]["feature"]]) <= nodes[nid]["threshold"] else 1)
        out[r] = int(np.argmax(nodes[nid]["counts"]))
    return out
