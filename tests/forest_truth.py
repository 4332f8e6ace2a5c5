"""Plain numpy restatements of the random forest's definitions (include/psgd.h): the bag weight in uint64 arithmetic, the
feature subsets, weighted integer histograms, and a forest trained node by node from each node's own rows. Bins,
impurities and best_split (with its no-near-tie assertions) are tree_truth's."""
import math

import numpy as np

import tree_truth as TT

GOLD = np.uint64(0x9E3779B97F4A7C15)


def mix(x):
    x = np.asarray(x, dtype=np.uint64).copy()
    x ^= x >> np.uint64(30)
    x *= np.uint64(0xBF58476D1CE4E5B9)
    x ^= x >> np.uint64(27)
    x *= np.uint64(0x94D049BB133111EB)
    x ^= x >> np.uint64(31)
    return x


def cut(numTrees, rate):
    F = []
    if numTrees > 1:
        term, acc = math.exp(-rate), 0.0
        for k in range(15):
            acc += term
            F.append(acc)
            term = term * rate / (k + 1)
    else:
        F = [1.0 - rate] + [1.0] * 14
    return np.array([min(1 << 53, math.ceil(f * 2.0 ** 53)) for f in F], dtype=np.uint64)


def bag(seed, tree, rows, cuts):
    """The weights of global rows `rows` in tree `tree`."""
    with np.errstate(over="ignore"):
        key = mix(np.uint64(seed) + np.uint64(tree + 1) * GOLD)
        u = mix(key + (np.asarray(rows, dtype=np.uint64) + np.uint64(1)) * GOLD) >> np.uint64(11)
    return (u[:, None] >= np.asarray(cuts, dtype=np.uint64)[None, :]).sum(axis=1)


def subset_size(kind, d, numTrees):
    kind = ("all" if numTrees == 1 else "sqrt") if kind == "auto" else kind
    return {"all": d, "sqrt": math.ceil(math.sqrt(d)), "log2": max(1, math.ceil(math.log2(d))), "onethird": math.ceil(d / 3)}[kind]


def subset(seed, tree, nid, d, m):
    return np.arange(d) if m == d else np.sort(np.random.default_rng([seed, tree, nid]).choice(d, m, replace=False))


def histogram(bins, y, slots, w, tree_base, sub, B, K):
    """H [A, m, B, K]: slots and w are [G, n]; a row of tree t with slot s >= 0 adds w to node tree_base[t] + s."""
    A, m = sub.shape
    H = np.zeros((A, m, B, K), dtype=np.int64)
    for t in range(len(slots)):
        for r in range(len(y)):
            if slots[t][r] >= 0:
                a = tree_base[t] + slots[t][r]
                H[a, np.arange(m), bins[r, sub[a]], int(y[r])] += int(w[t][r])
    return H


def train(X, y, K, thr, nbins, numTrees, strategy, seed, rate=1.0, kind="gini", maxDepth=4, min_inst=1):
    """The trees as tree_truth.train's dicts, each node from its own rows and its own subset."""
    n, d = X.shape
    bins, B, m, cuts = TT.bin_rows(X, thr, nbins), thr.shape[1] + 1, subset_size(strategy, d, numTrees), cut(numTrees, rate)
    forest = []
    for t in range(numTrees):
        w = bag(seed, t, np.arange(n), cuts)
        nodes, todo = {}, [(1, np.flatnonzero(w > 0), 0)]
        while todo:
            nid, rows, depth = todo.pop()
            sub = subset(seed, t, nid, d, m)
            H = np.zeros((m, B, K), dtype=np.int64)
            for r in rows:
                H[np.arange(m), bins[r, sub], int(y[r])] += w[r]
            tot = H[0].sum(axis=0)
            leaf = depth >= maxDepth or (np.count_nonzero(tot) <= 1 and nid > 1)
            s = None if leaf else TT.best_split(H, thr[sub], nbins[sub], kind, min_inst)
            leaf = leaf or s["feature"] < 0
            f = -1 if leaf else int(sub[s["feature"]])
            nodes[nid] = dict(feature=f, bin=-1 if leaf else s["bin"], threshold=0.0 if leaf else s["threshold"],
                              gain=TT.LD(0) if leaf else s["gain"], counts=tot)
            if not leaf:
                left = bins[rows, f] <= s["bin"]
                todo += [(2 * nid, rows[left], depth + 1), (2 * nid + 1, rows[~left], depth + 1)]
        forest.append(nodes)
    return forest


def vote(X, forest, K):
    votes = np.zeros((len(X), K), dtype=np.int32)
    for nodes in forest:
        votes[np.arange(len(X)), TT.predict(X, nodes)] += 1
    return votes
