"""Tagged rows: data in which chosen rows own a feature column nobody else touches (helper, no tests).

A tag is a column that is zero in every other row of the data set, with w0[tag] = 0. It leaves its
row's margin alone and receives exactly one gradient update of the chain, so after one outer
iteration the folded weight w[tag] = (n_p / N) (-s_t mult_t x_t,tag) (what the updater does to that
coordinate afterwards) reads out ONE row's step and multiplier at working precision, undiluted by
the other d - 1 coordinates and by max|w|. A row the chain never applied (unsampled, after a
per-sample break, an inactive Hinge row) leaves its tag at exactly 0.0. The fp64 oracle predicts
every such coordinate; tests/test_tagged_rows.py (CPU) fixes the bar from a plain float32
restatement and shows that one-row errors exceed it, tests/test_gpu_row_coefficients.py holds the
kernels to it.

Contents: where the tags go (required_positions, place), the dense and CSR generators, a plain
sequential numpy restatement of one chain (chain) and of the driver around it (run) in a chosen
dtype with one-row mutations, the per-coordinate error scale (tag_scale), the statistic, and the
case table both test modules share (CASES).

`python tests/tagged_rows.py` recomputes the CPU section of profiles/row_coefficients.json.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(ROOT, "profiles", "row_coefficients.json")

EPS = {"f32": 2.0 ** -24, "f64": 2.0 ** -53}
MUTATIONS = ("step_late", "swap", "stale", "drop", "dup")
GUARD = 64 * 2.0 ** -24          # Hinge guard band, in units of (||x|| ||w|| + 1)
REWRITES_ALL = ("squared_l2", "l1", "adam")   # updaters that rewrite every coordinate per sample


def _oracle():
    if os.path.join(ROOT, "oracle") not in sys.path:
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle as O
    return O


# ------------------------------------------------------------------------------------------------
# Where the tags go
# ------------------------------------------------------------------------------------------------
def required_positions(n, R=None, thread=None):
    """Positions (0-based, in processing order) of a chain of n processed rows that must carry a
    tag: every position of the first, a middle and the last full 8-row Gram block, every row of
    the tail block, row 0 and the last row, both sides of every wrap of an R-slot LDS ring (R - 1,
    R, R + 1, 2R - 1, ...), and both sides of every `thread` draws of the sampler (a sampler
    thread owns 64 consecutive draws; its round of 16,384 draws is past every chain here)."""
    if n <= 0:
        return []
    pos = {0, n - 1}
    full = n // 8
    for b in {0, full // 2, full - 1} if full else ():
        pos.update(range(8 * b, 8 * b + 8))
    pos.update(range(8 * full, n))
    for step in (R, thread):
        if step:
            for m in range(step, n + 1, step):
                pos.update((m - 1, m, m + 1))
    return sorted(p for p in pos if 0 <= p < n)


def place(rng, d, vec, rows_required, rows_optional, cap=None, cover=True):
    """Tag rows and columns. Every 16-byte vector of the row (vec elements; vector v belongs to
    lane v % 64, slot v // 64) gets at least one tag, the last, partly filled one included; at most
    `cap` (default d // 2) columns become tags, so that half the row stays shared. Rows: all the
    required ones, then optional ones until every vector is covered (cover=False: kernels that
    do not hold the row in lane vectors; only the required rows and as many again)."""
    cap = d // 2 if cap is None else cap
    nvec = (d + vec - 1) // vec
    rows = list(rows_required)
    assert len(rows) <= cap, f"{len(rows)} required tag rows but room for {cap}: a smaller case is needed"
    have = set(rows)
    extra = [r for r in rows_optional if r not in have]
    rng.shuffle(extra)
    want = min(cap, max(len(rows), nvec)) if cover else min(cap, 2 * len(rows))
    rows += extra[: max(want - len(rows), 0)]
    assert not cover or len(rows) >= nvec, f"{len(rows)} rows for {nvec} vectors: the case needs more rows"
    order = rng.permutation(len(rows))
    cols, used = np.zeros(len(rows), np.int64), set()
    for k, i in enumerate(order):
        v = k if (cover and k < nvec) else int(rng.integers(nvec))
        free = [c for c in range(v * vec, min(v * vec + vec, d)) if c not in used]
        while not free:
            v = int(rng.integers(nvec))
            free = [c for c in range(v * vec, min(v * vec + vec, d)) if c not in used]
        cols[i] = free[int(rng.integers(len(free)))]
        used.add(int(cols[i]))
    return np.array(rows, np.int64), cols


def sampled_rows(offs, fraction, iteration=1):
    """The rows (absolute) each chain processes in outer iteration `iteration`, in order."""
    P = len(offs) - 1
    if fraction >= 1.0:
        return [np.arange(offs[p], offs[p + 1]) for p in range(P)]
    O = _oracle()
    seeds = O.partition_seeds(42 + iteration, P)
    return [offs[p] + O.sample_partition(int(seeds[p]), offs[p + 1] - offs[p], fraction).astype(np.int64)
            for p in range(P)]


def _tag_rows(rng, offs, R, fraction):
    """(required, optional) absolute rows for the tags of a data set."""
    seqs = sampled_rows(offs, fraction)
    req, opt = [], []
    for p, seq in enumerate(seqs):
        n_p = offs[p + 1] - offs[p]
        thread = 64 if 0.0 < fraction <= 0.4 else None
        req += [int(seq[k]) for k in required_positions(len(seq), R, thread)]
        if 0.4 < fraction < 1.0:   # the filter sampler draws once per row: threads change at rows 64 m
            req += [offs[p] + r for m in range(64, n_p, 64) for r in (m - 1, m)]
        missed = np.setdiff1d(np.arange(offs[p], offs[p + 1]), seq)
        req += [int(r) for r in missed[:: max(len(missed) // 12, 1)]]   # rows the epoch skips: exact zeros
        opt += [int(r) for r in seq]
    return sorted(set(req)), opt


# ------------------------------------------------------------------------------------------------
# Generators
# ------------------------------------------------------------------------------------------------
def _labels(rng, z, grad):
    if grad == "least_squares":
        return z + 0.1 * rng.standard_normal(len(z))
    return ((z + rng.logistic(size=len(z))) > 0).astype(np.float64)


def dense_data(seed, sizes, d, grad, recipe="block", storage=np.float32, R=None, fraction=1.0, K=2, cover=True):
    """Dense rows with tags. Shared columns as test_gpu_block.synth (recipe "block": N(0, 1)
    entries) or test_gpu_split.synth ("split": N(0, 1) / sqrt(d)); tag columns zero outside their
    row, tag values of magnitude in [0.5, 2] with random sign; w0 non-zero on the shared columns
    (a noisy 1.5 x the labels' model, so that Hinge has inactive rows too) and zero on the tags.
    K > 2: labels 0..K-1 for the multinomial gradient, w0 of (K - 1) d.
    Returns dict(X float64 holding the stored values, y, w0, tags (rows, cols), offs, d)."""
    rng = np.random.default_rng(seed)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(int)
    n = int(offs[-1])
    vec = 16 // np.dtype(storage).itemsize
    req, opt = _tag_rows(rng, offs, R, fraction)
    rows, cols = place(rng, d, vec, req, opt, cover=cover)
    X = rng.standard_normal((n, d))
    wt = rng.standard_normal(d)
    if recipe == "block":
        wt /= np.sqrt(d)
    else:
        X /= np.sqrt(d)
    X[:, cols] = 0.0
    wt[cols] = 0.0
    X = X.astype(storage).astype(np.float64)
    z = X @ wt
    X[rows, cols] = rng.uniform(0.5, 2.0, len(rows)) * rng.choice([-1.0, 1.0], len(rows))
    X = X.astype(storage).astype(np.float64)
    if K > 2:
        W = 1.5 * rng.standard_normal((K, d)) / np.sqrt(d)   # margins of order 1: no multiplier near 0
        W[:, cols] = 0.0
        y = np.argmax(X @ W.T + rng.gumbel(size=(n, K)), 1).astype(np.float64)
        w0 = 0.5 * W[1:] + 0.1 * rng.standard_normal((K - 1, d)) / np.sqrt(d)
        w0[:, cols] = 0.0
        w0 = w0.reshape(-1)
    else:
        y = _labels(rng, z, grad)
        w0 = 1.5 * wt + 0.3 * rng.standard_normal(d) * np.std(wt)
        w0[cols] = 0.0
    return dict(X=X, y=y, w0=w0, tags=(rows, cols), offs=offs.tolist(), d=d, K=K)


def csr_data(seed, sizes, d, grad, kmin, kmax, n_tags, storage=np.float32, fraction=1.0, d_shared=None):
    """CSR rows with tags. d columns, of which n_tags random ones are tags and the rest (or the
    first d_shared of the rest) shared; shared features as test_gpu_sparse.synth_csr (kmin..kmax
    uniform(0.1, 1) values on random shared columns, the row normalised); each tagged row has one
    extra non-zero in a column of its own. Tag columns are drawn over the whole range, so with an
    LDS head of d / 3 features they fall in the head and in the HBM tail."""
    rng = np.random.default_rng(seed)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(int)
    n = int(offs[-1])
    req, opt = _tag_rows(rng, offs, None, fraction)
    assert len(req) <= n_tags, (len(req), n_tags)
    have = set(req)
    extra = [r for r in opt if r not in have]
    rng.shuffle(extra)
    rows = np.array(req + extra[: n_tags - len(req)], np.int64)
    cols = np.sort(rng.choice(d, size=len(rows), replace=False))[rng.permutation(len(rows))]
    assert cols.min() < d // 3 <= cols.max()
    shared = np.setdiff1d(np.arange(d), cols)
    if d_shared:
        shared = shared[:d_shared]
    tag_of = dict(zip(rows.tolist(), cols.tolist()))
    wt = np.zeros(d)
    wt[shared] = rng.standard_normal(len(shared))
    rp, col, val, z = [0], [], [], []
    for r in range(n):
        k = min(int(rng.integers(kmin, kmax + 1)), len(shared))
        idx = np.sort(rng.choice(shared, size=k, replace=False))
        v = rng.uniform(0.1, 1.0, size=k)
        v = (v / max(np.linalg.norm(v), 1e-12)).astype(np.float32).astype(np.float64)
        z.append(float(v @ wt[idx]))
        if r in tag_of:
            t = float(rng.uniform(0.5, 2.0) * rng.choice([-1.0, 1.0]))
            idx, v = np.append(idx, tag_of[r]), np.append(v, np.float64(np.dtype(storage).type(t)))
            o = np.argsort(idx)
            idx, v = idx[o], v[o]
        col += idx.tolist()
        val += v.tolist()
        rp.append(len(col))
    y = _labels(rng, np.array(z), grad)
    w0 = np.zeros(d)
    w0[shared] = 1.5 * wt[shared] + 0.3 * rng.standard_normal(len(shared))
    return dict(rp=np.array(rp, np.int64), col=np.array(col, np.int32), val=np.array(val, np.float64), y=y,
                w0=w0, tags=(rows, cols), offs=offs.tolist(), d=d, K=2)


def hinge_pivot(data, c):
    """Hinge's multiplier is +-1, so a margin computed from weights one update stale changes a
    tag only where it flips the row's decision. One tagged row per Hinge data set is therefore put
    where it does: its shared features are scaled (its margins from the current and from the stale
    weights scale alike; the tag is outside both) so that 1 lies midway between the two, the
    current margin on the active side. Among the tagged rows with both margins between 0.3 and 3
    the one where they differ most, and at least three guard bands to either side. Returns the row."""
    storage = np.float32 if (is_csr(data) and c["compute"] == "f32") else c["storage"] if not is_csr(data) else np.float64
    _, _, traces = run(data, "hinge", c["upd"], c["step"], c["reg"], 1, c["fraction"], stale_trace=True)
    tagged = dict(zip(*[a.tolist() for a in data["tags"]]))
    wn = np.linalg.norm(data["w0"])
    best = None
    for tr in traces:
        for k, (r, j, z, act, zs) in enumerate(tr):
            ys = 2 * data["y"][r] - 1
            a, b = ys * z, ys * zs
            xn = np.linalg.norm(data["val"][data["rp"][r]:data["rp"][r + 1]] if is_csr(data) else data["X"][r])
            far = 0.3 < a < b < 3.0 and (b - a) / (a + b) > 3 * GUARD * (2.0 / (a + b) * xn * wn + 1.0)
            if 1 <= k < len(tr) - 1 and r in tagged and far and (best is None or (b - a) / (a + b) > best[0]):
                best = ((b - a) / (a + b), r, 2.0 / (a + b))
    assert best is not None, "no tagged Hinge row can be put between its current and its stale margin"
    _, r, alpha = best
    if is_csr(data):
        a, b = data["rp"][r], data["rp"][r + 1]
        m = data["col"][a:b] != tagged[r]
        data["val"][a:b][m] = (data["val"][a:b][m] * alpha).astype(storage).astype(np.float64)
    else:
        m = np.ones(data["d"], bool)
        m[tagged[r]] = False
        data["X"][r, m] = (data["X"][r, m] * alpha).astype(storage).astype(np.float64)
    data["pivot_row"] = r
    return r


def is_csr(data):
    return "rp" in data


def matrix(data):
    O = _oracle()
    if is_csr(data):
        return O.Matrix(data["y"], row_ptr=data["rp"], col=data["col"], val=data["val"], d=data["d"])
    return O.Matrix(data["y"], data["X"])


# ------------------------------------------------------------------------------------------------
# The restatement: one chain, sample by sample, in one dtype
# ------------------------------------------------------------------------------------------------
def _dot(x, w, order):
    """order 0: left fold (the reference's ddot); 1: 64 strided partial sums and a pairwise tree
    (a wavefront's order). Two equally valid evaluations in the working precision."""
    p = x * w
    if order == 0 or p.size <= 1:
        return np.cumsum(p)[-1] if p.size else p.dtype.type(0)
    pad = np.zeros((-p.size) % 64, p.dtype)
    part = np.concatenate([p, pad]).reshape(-1, 64)
    acc = part[0].copy()
    for k in range(1, part.shape[0]):
        acc = acc + part[k]
    h = 32
    while h >= 1:
        acc = acc[:h] + acc[h:2 * h]
        h //= 2
    return acc[0]


def _row(data, r, T):
    if is_csr(data):
        a, b = data["rp"][r], data["rp"][r + 1]
        return data["col"][a:b], data["val"][a:b].astype(T)
    return None, data["X"][r].astype(T)


def chain(data, seq, w_in, grad, upd, step, reg, dtype=np.float64, order=0, mutate=None, at=None,
          beta=0.9, gamma=0.999, eps=1e-8, stale_trace=False, read=None):
    """ParallelizedSGD's chain (gradient, updater, iter += 1 per sample; no per-sample test: the
    caller truncates `seq` where the oracle breaks) over rows `seq` in order, every operation in
    `dtype`: the three binary gradients, the multinomial LogisticGradient (data["K"] > 2) and the
    five updaters, dense and CSR rows. stepSize / sqrt(iter) is formed in double and rounded once.

    mutate (at = position in seq) makes one row wrong: "step_late" takes iter + 1 for it, "swap"
    processes it after its successor, "stale" computes its margin from the weights before the
    previous update, "drop" does not apply it, "dup" applies it twice.

    read (binary gradients; default None: no effect): read(k, row, idx, wv, w) is called before the
    margin of position k with the row's columns (None: dense), the weights wv the margin is about to
    take for them and the whole current vector w, and returns the weights the margin takes: an
    observer, or a mutation of single reads (tests/reuse_schedule.py).

    Returns (w, trace) with trace[k] = (row, iter, z, active, z_stale) per position (z in double;
    z_stale, with stale_trace, the margin the row would get from the weights before the previous
    update, else z)."""
    T = np.dtype(dtype).type
    seq = [int(r) for r in seq]
    if mutate == "swap":
        seq[at], seq[at + 1] = seq[at + 1], seq[at]
    K = data.get("K", 2)
    d = data["d"]
    w = np.asarray(w_in, np.float64).astype(T)
    w_prev = w.copy()
    acc_a = acc_b = None
    trace = []
    j = 1
    for k, r in enumerate(seq):
        if mutate == "drop" and k == at:
            trace.append((r, j, 0.0, False, 0.0))
            j += 1
            continue
        idx, x = _row(data, r, T)
        y = T(data["y"][r])
        for rep in range(2 if (mutate == "dup" and k == at) else 1):
            it = j + 1 if (mutate == "step_late" and k == at) else j
            s = T(step / np.sqrt(float(it)))
            wm = w_prev if (mutate == "stale" and k == at and rep == 0) else w
            before = w.copy() if (mutate == "stale" or stale_trace) else None
            z_stale = None
            if K > 2:
                W = wm.reshape(K - 1, d)
                m = np.array([_dot(x, (W[i] if idx is None else W[i][idx]), order) for i in range(K - 1)], T)
                mx = m.max()
                if mx > 0:
                    e = np.exp(m - mx)      # the pivot class stands in the sum as exp(-max)
                    tot = e.sum() - e[int(np.argmax(m))] + np.exp(-mx)
                    mult = e / (tot + T(1))
                else:
                    tot = np.exp(m).sum()
                    mult = np.exp(m) / (tot + T(1))
                ly = int(data["y"][r]) - 1
                if ly >= 0:
                    mult[ly] = mult[ly] - T(1)
                z, active = float(m[0]), True
                if idx is None:
                    g = (mult[:, None] * x[None, :]).reshape(-1)
                    gi = None
                else:
                    gi = (np.arange(K - 1)[:, None] * d + idx[None, :]).reshape(-1)
                    g = (mult[:, None] * x[None, :]).reshape(-1)
            else:
                wv = wm if idx is None else wm[idx]
                if read is not None:
                    wv = read(k, r, idx, wv, w)
                zz = _dot(x, wv, order)
                z = float(zz)
                if stale_trace:
                    z_stale = float(_dot(x, w_prev if idx is None else w_prev[idx], order))
                active = True
                if grad == "logistic":
                    mult = T(1) / (T(1) + np.exp(-zz)) - y
                elif grad == "least_squares":
                    mult = zz - y
                else:
                    ls = T(2) * y - T(1)
                    active = bool(T(1) > ls * zz)
                    mult = -ls if active else T(0)
                g, gi = mult * x, idx
            # the updater
            if upd == "squared_l2":
                w = w * T(1.0 - float(s) * reg)
            if upd in ("simple", "squared_l2", "l1"):
                if active:
                    if gi is None:
                        w = w + (-s) * g
                    else:
                        w = w.copy()
                        w[gi] = w[gi] + (-s) * g
                if upd == "l1":
                    w = np.sign(w) * np.maximum(T(0), np.abs(w) - T(reg * float(s)))
            else:
                gd = g if gi is None else np.zeros(w.size, T)
                if gi is not None:
                    gd[gi] = g
                if not active:
                    gd = np.zeros(w.size, T)
                if upd == "adagrad":
                    acc_a = gd * gd if acc_a is None else acc_a + gd * gd
                    w = w + (-s) * (gd / np.sqrt(acc_a + T(1)))
                else:
                    if acc_a is None:
                        acc_a, acc_b = gd * T(1 - beta), (gd * gd) * T(1 - gamma)
                    else:
                        acc_a = acc_a * T(beta) + gd * T(1 - beta)
                        acc_b = acc_b * T(gamma) + (gd * gd) * T(1 - gamma)
                    lr = s / (T(1) - np.power(T(beta), T(it)))
                    fix = np.sqrt(T(1) - np.power(acc_b, T(it))) + T(eps)
                    w = w + (-lr) * (acc_a / fix)
            w_prev = before if before is not None else w_prev
        trace.append((r, j, z, active, z if z_stale is None else z_stale))
        j += 1
    return w, trace


def fold(ws, counts):
    """ParallelizedSGD.scala:271-276 in double: the count-weighted left fold of the chains."""
    acc, c = None, 0
    for w, n in zip(ws, counts):
        if acc is None:
            acc, c = np.asarray(w, np.float64).copy(), n
        else:
            acc = (acc * float(c) + np.asarray(w, np.float64) * float(n)) / float(c + n)
            c += n
    return acc


def run(data, grad, upd, step, reg, iters=1, fraction=1.0, limits=None, dtype=np.float64, order=0,
        mutate=None, at=None, stale_trace=False, read=None):
    """`iters` outer iterations of chain() over the partitions and the fold in double, as the
    device does it. limits[p]: the number of rows chain p applies (the oracle's break counts;
    first iteration only). mutate / at = (chain, position): first iteration only. read[p]: chain()'s
    `read` for chain p (a dict; first iteration only).
    Returns (folded weights, per-chain weights of the last iteration, traces of the first)."""
    offs = data["offs"]
    w = np.asarray(data["w0"], np.float64)
    first = None
    for i in range(1, iters + 1):
        seqs = sampled_rows(offs, fraction, i)
        if limits is not None and i == 1:
            seqs = [s[: int(n)] for s, n in zip(seqs, limits)]
        ws, traces = [], []
        for p, seq in enumerate(seqs):
            mut = mutate if (mutate and i == 1 and at[0] == p) else None
            wp, tr = chain(data, seq, w, grad, upd, step, reg, dtype, order, mut, at[1] if mut else None,
                           stale_trace=stale_trace and i == 1, read=read.get(p) if (read and i == 1) else None)
            ws.append(wp.astype(np.float64))
            traces.append(tr)
        first = traces if first is None else first
        counts = [len(s) for s in seqs]
        if sum(counts):
            w = fold(ws, counts)
    return w, ws, first


# ------------------------------------------------------------------------------------------------
# The per-coordinate scale and the statistic
# ------------------------------------------------------------------------------------------------
def tag_index(data):
    """Weight indices of the tags: one per tag, or one per tag and class block (K > 2), with the
    tag number of each."""
    rows, cols = data["tags"]
    K, d = data.get("K", 2), data["d"]
    blocks = np.arange(K - 1 if K > 2 else 1)
    which = np.tile(np.arange(len(rows)), len(blocks))
    return which, (blocks[:, None] * d + cols[None, :]).reshape(-1)


def tag_info(data, traces):
    """Per tag, from the float64 restatement's traces: chain, position (-1: not processed), iter,
    z, active, the rows after it in its chain, ||x|| and |y|."""
    rows, cols = data["tags"]
    where = {}
    for p, tr in enumerate(traces):
        for k, (r, j, z, act, zs) in enumerate(tr):
            where[r] = (p, k, j, z, act, len(tr) - 1 - k, zs)
    offs = np.asarray(data["offs"])
    out = []
    for r, c in zip(rows.tolist(), cols.tolist()):
        if is_csr(data):
            a, b = data["rp"][r], data["rp"][r + 1]
            xn = float(np.linalg.norm(data["val"][a:b]))
            xt = float(data["val"][a:b][list(data["col"][a:b]).index(c)])
        else:
            xn, xt = float(np.linalg.norm(data["X"][r])), float(data["X"][r, c])
        p, k, j, z, act, after, zs = where.get(r, (int(np.searchsorted(offs, r, "right") - 1), -1, 1, 0.0, False,
                                                   0, 0.0))
        out.append(dict(row=r, col=c, chain=p, pos=k, iter=j, z=z, active=act, after=after, xnorm=xn, xtag=xt,
                        y=float(data["y"][r]), z_stale=zs))
    return out


def tag_scale(data, info, upd, step, w_norm, w_tag_ref, compute="f32", share=None):
    """The error scale of every tag coordinate (array over tag_index(data)):

        eps ( s_t |x_tag| (||x_t|| ||w|| + |y_t| + 1) + k_after |w_ref[tag]| ),

    eps = 2^-24 (fp32 compute) or 2^-53; s_t = stepSize / sqrt(iter_t); ||w|| the largest weight
    norm of the row's chain (w_norm[chain]: the larger of what it started from and what it ended
    with); the first term is the rounding of the margin (a dot of ||x|| ||w|| in magnitude), of the
    multiplier and of the update itself. k_after is the number of later samples of the chain when
    the updater rewrites every coordinate at every sample (SquaredL2, L1, Adam), else 0: each
    rounds the tag once more.

    Refinement of the plain form (k_after for SquaredL2 on dense rows only): it counts on CSR
    rows too. The plain restatement multiplies every coordinate by 1 - s lambda at each sample whatever the layout,
    and a kernel that keeps the product of those factors aside (the alpha-scaled CSR form) rounds
    that product once per sample all the same, so the tag carries k_after roundings either way.
    share[chain] = n_p / N scales the chain's coordinates to the folded vector's (the fold is in
    double)."""
    e = EPS[compute]
    which, _ = tag_index(data)
    out = np.zeros(len(which))
    for q, t in enumerate(which):
        i = info[t]
        s = step / np.sqrt(float(i["iter"]))
        k_after = i["after"] if upd in REWRITES_ALL else 0
        v = e * (s * abs(i["xtag"]) * (i["xnorm"] * w_norm[i["chain"]] + abs(i["y"]) + 1.0)
                 + k_after * abs(w_tag_ref[q]))
        out[q] = v * (share[i["chain"]] if share is not None else 1.0)
    return out


def hinge_guard(info, w_norm, grad):
    """Tags left out of the comparison: Hinge rows whose oracle |1 - (2y - 1) z| is within
    64 x 2^-24 (||x|| ||w|| + 1) of the decision (either side may be taken in fp32)."""
    if grad != "hinge":
        return np.zeros(len(info), bool)
    return np.array([i["pos"] >= 0 and abs(1.0 - (2 * i["y"] - 1) * i["z"]) <
                     GUARD * (i["xnorm"] * w_norm[i["chain"]] + 1.0) for i in info])


def expected_zero(info):
    """Tags whose row the oracle did not apply: not processed, or an inactive Hinge row."""
    return np.array([i["pos"] < 0 or not i["active"] for i in info])


def statistic(w, w_ref, scale, idx, keep):
    """max over the kept tag coordinates of |w - w_ref| / scale, and the coordinate it is at."""
    err = np.abs(np.asarray(w)[idx] - np.asarray(w_ref)[idx]) / scale
    err = np.where(keep, err, 0.0)
    q = int(np.argmax(err)) if err.size else 0
    return (float(err[q]) if err.size else 0.0), q


# ------------------------------------------------------------------------------------------------
# The case table (shared by the CPU and the GPU module)
# ------------------------------------------------------------------------------------------------
GRADS = ("logistic", "least_squares", "hinge")
BLOCK_SHAPES = [(1, 251, np.float32), (2, 512, np.float32), (4, 1019, np.float32), (8, 2048, np.float32),
                (4, 300, np.float64)]   # NV, d, storage: d = 300 doubles are 150 vectors, NV 4


def _block_step(grad, d):
    return {"least_squares": 0.5 / d, "logistic": 2.0 / d, "hinge": 1.0 / d}[grad]


def _sizes(n_min, P, tail):
    """One chain, or five ragged ones: 1, 7, 8 and 9 rows and a long one; the long chain ends in a
    tail block of `tail` rows."""
    long = (n_min + 7) // 8 * 8 + tail
    return [long] if P == 1 else [9, 1, long, 7, 8]


def _cases():
    C = []

    def add(id, **kw):
        base = dict(id=id, layout="dense", compute="f32", reg=0.0, fraction=1.0, tol=0.0, iters=1, env={},
                    K=2, recipe="block", storage=np.float32, budget=None)
        base.update(kw)
        C.append(base)

    # chain_block: 300 + NV
    k = 0
    for nv, d, st in BLOCK_SHAPES:
        vec = 16 // np.dtype(st).itemsize
        for grad in GRADS:
            for upd in ("simple", "squared_l2"):
                for P in (1, 5):
                    k += 1
                    add(f"block-nv{nv}-d{d}-{np.dtype(st).name}-{grad}-{upd}-P{P}", family="block", nv=nv, d=d,
                        storage=st, grad=grad, upd=upd, step=_block_step(grad, d), reg=0.05 if upd == "squared_l2" else 0.0,
                        sizes=_sizes(max(296, (d + vec - 1) // vec + 24), P, 1 + k % 7), variant=300 + nv, seed=100 + k)
    add("block-min-ring", family="block", nv=2, d=512, grad="logistic", upd="squared_l2", step=2.0 / 512, reg=0.05,
        sizes=[93, 70, 35], variant=302, seed=201, budget=256)
    for f in (0.3, 0.7):
        add(f"block-sampled-f{f}", family="block", nv=2, d=512, grad="least_squares", upd="simple", step=0.5 / 512,
            sizes=[430, 301] if f < 0.5 else [260, 171], variant=302, seed=202, fraction=f)
    add("block-break", family="block", nv=2, d=512, grad="logistic", upd="simple", step=4.0 / 512, tol=0.01,
        sizes=[45 + (p % 3) for p in range(8)], variant=342, seed=203)
    add("block-two-iterations", family="block", nv=2, d=512, grad="logistic", upd="squared_l2", step=2.0 / 512,
        reg=0.05, sizes=[203, 150], variant=302, seed=204, iters=2)

    # chain_split fp32: 800 + 10 H + NV (H = min(NV, 4); d = 500 is the H = 2 instance). L1's
    # regParam is small enough that the later samples' soft thresholds (sum of reg s_j) do not
    # shrink an applied row's tag to zero.
    k = 0
    for d, nv in ((500, 2), (700, 4), (1024, 4), (2048, 8)):
        for upd in ("adagrad", "l1", "adam"):
            k += 1
            grad = GRADS[k % 3]
            add(f"split-d{d}-{upd}-{grad}", family="split", nv=nv, d=d, grad=grad, upd=upd, recipe="split",
                # s ||x||^2 = 0.5 as in the blocked cases for Adam (its momentum smooths one stale update
                # away at a short step) and for L1's Hinge rows (the pivot needs margins that move)
                step=0.05 if upd == "adagrad" else 0.5,
                reg=0.0002 if upd == "l1" else 0.0, sizes=[max(150, d // 4 + 30) + k % 5, 57],
                variant=800 + 10 * min(nv, 4) + nv, seed=300 + k)
    add("split-sampled", family="split", nv=4, d=700, grad="logistic", upd="adam", recipe="split", step=0.5,
        sizes=[500, 333], variant=844, seed=320, fraction=0.3)
    add("split-two-iterations", family="split", nv=4, d=700, grad="least_squares", upd="adagrad", recipe="split",
        step=0.05, sizes=[180, 121], variant=844, seed=321, iters=2)

    # chain_dense fp32 on request: 100 + NV
    for d, nv, upd in ((60, 1, "simple"), (512, 2, "squared_l2")):
        for grad in GRADS:
            add(f"dense-d{d}-{grad}-{upd}", family="dense", nv=nv, d=d, grad=grad, upd=upd, step=_block_step(grad, d),
                reg=0.05 if upd == "squared_l2" else 0.0, sizes=[19, 9] if d == 60 else [182, 43], variant=100 + nv,
                seed=400 + d + len(grad), env={"PSGD_PER_SAMPLE": "1"})
    add("dense-two-iterations", family="dense", nv=2, d=512, grad="logistic", upd="simple", step=2.0 / 512,
        sizes=[160, 77], variant=102, seed=420, iters=2, env={"PSGD_PER_SAMPLE": "1"})

    # CSR fp32: each on every kernel of test_gpu_sparse.KERNELS
    k = 0
    for grad in GRADS:
        for upd in ("simple", "squared_l2"):
            k += 1
            reg = 0.05 if upd == "squared_l2" else 0.0
            add(f"csr-narrow-{grad}-{upd}", layout="csr", family="csr", grad=grad, upd=upd, step=0.2, reg=reg,
                d=172, d_shared=12, kmin=1, kmax=9, n_tags=160, sizes=[300, 203, 97], seed=500 + k)
            add(f"csr-wide-{grad}-{upd}", layout="csr", family="csr", grad=grad, upd=upd, step=0.5, reg=reg,
                d=3000, d_shared=None, kmin=0, kmax=40, n_tags=400, sizes=[500, 0, 1, 499], seed=520 + k)
    add("csr-sampled", layout="csr", family="csr", grad="hinge", upd="simple", step=0.5, d=500, d_shared=None, kmin=0,
        kmax=30, n_tags=200, sizes=[600, 400], seed=540, fraction=0.3)
    add("csr-rows-over-128", layout="csr", family="csr-plain", grad="logistic", upd="simple", step=0.5, d=1000,
        d_shared=None, kmin=100, kmax=300, n_tags=150, sizes=[120, 81], seed=541, variant=401)
    add("csr-two-iterations", layout="csr", family="csr", grad="logistic", upd="simple", step=0.2,
        d=172, d_shared=12, kmin=1, kmax=9, n_tags=160, sizes=[300, 201], seed=542, iters=2)

    # the fp64 kernels, once each, at the 2^-53 scale
    f64 = dict(compute="f64")
    add("block64", family="block64", nv=2, d=512, grad="logistic", upd="squared_l2", step=2.0 / 512, reg=0.05,
        sizes=[203, 9, 1, 150], variant=712, seed=600, **f64)
    add("block64-break", family="block64", nv=2, d=512, grad="logistic", upd="simple", step=4.0 / 512, tol=0.01,
        sizes=[45 + (p % 3) for p in range(8)], variant=752, seed=203, **f64)
    add("split64", family="split", nv=4, d=700, grad="hinge", upd="adam", recipe="split", step=0.5,
        sizes=[205, 57], variant=844, seed=601, **f64)
    for head in ("all", "third"):
        add(f"sparse-lds64-{head}", layout="csr", family="csr64", grad="logistic", upd="squared_l2", step=0.3, reg=0.05,
            d=3000, d_shared=None, kmin=0, kmax=40, n_tags=300, sizes=[300, 201], seed=602, variant=620,
            env={"PSGD_SPARSE_LDS_HEAD": "1000"} if head == "third" else {}, **f64)
    add("sparse64-d200000", layout="csr", family="csr64", grad="least_squares", upd="simple", step=0.4, d=200_000,
        d_shared=None, kmin=0, kmax=120, n_tags=300, sizes=[300, 0, 1, 120], seed=603, variant=420, **f64)
    add("general-dense", family="general", nv=0, d=3000, grad="logistic", upd="simple", step=2.0 / 3000,
        sizes=[60, 41], variant=200, seed=604, **f64)
    add("general-csr", layout="csr", family="csr64", grad="logistic", upd="squared_l2", step=1.0, reg=1.0, d=300,
        d_shared=None, kmin=1, kmax=20, n_tags=120, sizes=[150, 101], seed=605, variant=201, **f64)
    for K, d, sizes in ((3, 200, [90, 45]), (70, 100, [30, 9])):
        add(f"multinomial-K{K}", family="multinomial", nv=0, d=d, K=K, grad="logistic", upd="simple", step=0.2,
            storage=np.float64, sizes=sizes, variant=500, seed=606 + K, **f64)
    return C


CASES = _cases()
CASE_IDS = [c["id"] for c in CASES]


def ring_rows(pkg, c):
    """R of the LDS ring the case's kernel gets (the dense families; None elsewhere)."""
    import test_ring_geometry as RG
    fam = {"dense": RG.DENSE, "split": RG.SPLIT, "block": RG.BLOCK, "block64": RG.BLOCK64}.get(c["family"])
    if fam is None:
        return None
    compute = RG.F32 if c["compute"] == "f32" else RG.F64
    budget = c["budget"] if c["budget"] else RG.spread_budget(len(c["sizes"]))
    return RG.ring_geometry(pkg, fam, c["nv"], compute, c["tol"] > 0, budget)[0]


_BUILT = {}


def build(pkg, c):
    """The case's data (cached) and its reference: dict(data, R, wr folded oracle weights of
    c["iters"] iterations, hr, cr, margins, chains (oracle.run_chains of the first epoch), info,
    w_norm, share, scale, idx, which, keep, zero)."""
    if c["id"] in _BUILT:
        return _BUILT[c["id"]]
    O = _oracle()
    R = ring_rows(pkg, c)
    if c.get("make"):
        data = c["make"](c)     # a case that brings its own generator (tests/reuse_schedule.py)
    elif c["layout"] == "csr":
        data = csr_data(c["seed"], c["sizes"], c["d"], c["grad"], c["kmin"], c["kmax"], c["n_tags"],
                        storage=np.float32 if c["compute"] == "f32" else np.float64, fraction=c["fraction"],
                        d_shared=c["d_shared"])
    else:
        data = dense_data(c["seed"], c["sizes"], c["d"], c["grad"], c["recipe"], c["storage"], R, c["fraction"],
                          K=c["K"], cover=c["nv"] > 0)
    if c["grad"] == "hinge" and not c.get("make"):
        hinge_pivot(data, c)
    mat = matrix(data)
    kw = dict(num_classes=c["K"]) if c["K"] > 2 else {}
    if c["fraction"] < 1.0:
        kw["fraction"] = c["fraction"]
    args = (mat, data["offs"], c["grad"], c["upd"], c["step"])
    if c["tol"] > 0:
        wr, hr, cr, mg = O.run_with_margins(*args, c["iters"], c["reg"], data["w0"], tol=c["tol"], **kw)
    else:
        wr, hr, cr = O.run(*args, c["iters"], c["reg"], data["w0"], tol=0.0, **kw)
        mg = None
    limits = [int(v) for v in cr[0]]
    # the float64 restatement: which rows were applied, their iter, margin and decision
    _, ws64, traces = run(data, c["grad"], c["upd"], c["step"], c["reg"], 1, c["fraction"], limits,
                          stale_trace=c["K"] == 2)
    info = tag_info(data, traces)
    which, idx = tag_index(data)
    total = float(sum(limits))
    share = [n / total for n in limits]
    w_norm = [max(np.linalg.norm(data["w0"]), np.linalg.norm(w)) for w in ws64]
    ref = dict(data=data, R=R, wr=wr, hr=hr, cr=cr, margins=mg, limits=limits, info=info, which=which, idx=idx,
               share=share, w_norm=w_norm, ws64=ws64, kw=kw)
    guard = hinge_guard(info, w_norm, c["grad"])
    ref["guard"] = guard
    ref["keep"] = ~guard[which]
    ref["zero"] = expected_zero(info)[which]
    _BUILT[c["id"]] = ref
    return ref


def chain_scale(c, ref, chain_w):
    """tag_scale against per-chain weights (CPU: one chain's own coordinates, no share)."""
    w_tag = np.array([chain_w[ref["info"][t]["chain"]][i] for t, i in zip(ref["which"], ref["idx"])])
    return tag_scale(ref["data"], ref["info"], c["upd"], c["step"], ref["w_norm"], w_tag, c["compute"]), w_tag


def folded_scale(c, ref):
    """tag_scale of the folded weights after c["iters"] iterations. One iteration: the chain's scale
    times its share n_p / N. Two: the second epoch starts from the folded tags (rounded to the
    working precision on the way in: eps |w|), every chain carries every tag through its updater
    (k_all = the longest chain's rows more roundings where the updater rewrites every coordinate),
    and the tag's row adds an update of the first epoch's size with its own rounding; so
    2 x the one-iteration scale + eps (1 + k_all) |w_ref[tag]|."""
    data = ref["data"]
    first = np.array([ref["ws64"][ref["info"][t]["chain"]][i] for t, i in zip(ref["which"], ref["idx"])])
    one = tag_scale(data, ref["info"], c["upd"], c["step"], ref["w_norm"], first, c["compute"], ref["share"])
    if c["iters"] == 1:
        return one
    k_all = max(ref["limits"]) if c["upd"] in REWRITES_ALL else 0
    return 2.0 * one + EPS[c["compute"]] * (1 + k_all) * np.abs(ref["wr"][ref["idx"]])


def load_profile():
    with open(PROFILE) as f:
        return json.load(f)


def bars():
    """(BAR, BAR64) of the committed CPU section."""
    cpu = load_profile()["cpu"]
    return cpu["BAR"], cpu["BAR64"]


def cpu_statistics(pkg, c):
    """S of the float32 (or, for an fp64 case, float64) restatement against the oracle on the
    case, per evaluation order of the dot; plus oracle.run_f32 orders 0 and 1 where it applies
    (dense Simple / SquaredL2, unsampled, tol = 0, fp32)."""
    O = _oracle()
    ref = build(pkg, c)
    data = ref["data"]
    dtype = np.float32 if c["compute"] == "f32" else np.float64
    out = {}
    for order in (0, 1):
        w, _, _ = run(data, c["grad"], c["upd"], c["step"], c["reg"], c["iters"], c["fraction"], ref["limits"],
                      dtype=dtype, order=order)
        out[f"restatement_order{order}"] = statistic(w, ref["wr"], folded_scale(c, ref), ref["idx"], ref["keep"])[0]
    if (c["compute"] == "f32" and c["layout"] == "dense" and c["upd"] in ("simple", "squared_l2")
            and c["fraction"] >= 1.0 and c["tol"] == 0.0):
        for order in (0, 1):
            w, _, _ = O.run_f32(matrix(data), data["offs"], c["grad"], c["upd"], c["step"], c["iters"], c["reg"],
                                data["w0"], order=order, tol=0.0)
            out[f"oracle_f32_order{order}"] = statistic(w, ref["wr"], folded_scale(c, ref), ref["idx"], ref["keep"])[0]
    return out


def write_cpu_profile(pkg):
    per_case = {c["id"]: cpu_statistics(pkg, c) for c in CASES}
    s32 = max(max(v.values()) for c, v in zip(CASES, per_case.values()) if c["compute"] == "f32")
    s64 = max(max(v.values()) for c, v in zip(CASES, per_case.values()) if c["compute"] == "f64")
    prof = load_profile() if os.path.exists(PROFILE) else {}
    prof["what"] = ("max over tag coordinates of |w - w_oracle| / tag_scale (tests/tagged_rows.py). 'cpu': numpy "
                    "restatements and oracle.run_f32 on a host CPU, no device involved; BAR = 4 S_ref is what "
                    "tests/test_gpu_row_coefficients.py holds the kernels to. 'device': what the kernels gave "
                    "on an MI355X, per test case.")
    prof["cpu"] = dict(S_ref=s32, BAR=4 * s32, S_ref64=s64, BAR64=4 * s64, cases=per_case)
    prof.setdefault("device", {})
    with open(PROFILE, "w") as f:
        json.dump(prof, f, indent=1, sort_keys=True)
    return prof


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import __graft_entry__ as g
    p = write_cpu_profile(g.load_package())
    print({k: v for k, v in p["cpu"].items() if k != "cases"})
