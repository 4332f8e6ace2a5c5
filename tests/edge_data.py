"""Data sets that put the chain kernels' per-sample math at saturated margins and exact ties
(tests/test_gpu_saturation.py runs the kernels on them; tests/test_edge_data.py checks, on the
CPU, that each set is conditioned well enough for the GPU bars to mean something). A plain helper
module.

Margin ladder: a unit direction g, rows x_i = t_i g + noise (noise orthogonal to g), w0 = g, so
row i's first margin is t_i; t is 0 and +- log-spaced 1e-3 .. T in every partition (T = 800 for
fp64, past exp's overflow at 709.78 and the sigmoid's clamps; 120 for fp32, past expf's at 88.7).
Labels are sign(t) with 5 % flipped among |t| < 30; step 0.05; partitions of 300, 1, 0, 299 rows.
"""
import numpy as np

STEP = 0.05
SIZES = (300, 1, 0, 299)
REGIMES = ((0.0, 1.0), (1.0, 20.0), (20.0, 88.0), (88.0, 709.0), (709.0, np.inf))


SEED_CSR = 3   # chosen by the CPU conditions (test_edge_data.py): Hinge's on/off decisions are
#                discontinuous, and other seeds put one within fp32 rounding of flipping


class EdgeSet:
    """y, the partition offsets, w0, the first margins t, and the rows: dense X, or CSR
    (row_ptr, col, val, d). Values are exactly representable in `dtype` (the storage type)."""

    def __init__(self, name, y, offs, w0, t, dtype, X=None, csr=None, d=None):
        self.name, self.y, self.offs, self.w0, self.t, self.dtype = name, y, list(offs), w0, t, dtype
        self.X, self.csr, self.d = X, csr, d if d is not None else X.shape[1]
        self.step = STEP

    def oracle_matrix(self, O, dense=False):
        if self.X is not None:
            return O.Matrix(self.y, self.X.astype(np.float64))
        rp, col, val = self.csr
        if dense:
            X = np.zeros((len(self.y), self.d))
            for i in range(len(self.y)):
                X[i, col[rp[i]:rp[i + 1]]] = val[rp[i]:rp[i + 1]]
            return O.Matrix(self.y, X)
        return O.Matrix(self.y, row_ptr=rp, col=col, val=val.astype(np.float64), d=self.d)

    def partitions(self, pkg):
        offs = self.offs
        if self.X is not None:
            return pkg.PartitionedData([pkg.DensePartition(self.y[a:b], self.X[a:b]) for a, b in zip(offs[:-1], offs[1:])])
        rp, col, val = self.csr
        return pkg.PartitionedData([pkg.CsrPartition(self.y[a:b], rp[a:b + 1] - rp[a], col[rp[a]:rp[b]], val[rp[a]:rp[b]], self.d)
                                    for a, b in zip(offs[:-1], offs[1:])])

    def first_margins(self):
        """x_i . w0 in longdouble."""
        w = self.w0.astype(np.longdouble)
        if self.X is not None:
            return np.asarray(self.X.astype(np.longdouble) @ w, np.float64)
        rp, col, val = self.csr
        return np.array([float(val[rp[i]:rp[i + 1]].astype(np.longdouble) @ w[col[rp[i]:rp[i + 1]]]) for i in range(len(self.y))])


def _offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def ladder_t(rng, sizes, T):
    """Per partition: 0 and +- log-spaced 1e-3 .. T, shuffled (a 1-row partition gets t = 1.5)."""
    out = []
    for m in sizes:
        if m == 0:
            continue
        if m == 1:
            out.append(np.array([1.5]))   # not 1: Hinge ties are exact_ties()
            continue
        k = (m - 1) // 2
        mag = np.exp(np.linspace(np.log(1e-3), np.log(T), k))
        t = np.concatenate([[0.0], mag, -mag, [0.5] * (m - 1 - 2 * k)])
        out.append(rng.permutation(t))
    return np.concatenate(out)


def labels_for(rng, t, flip):
    y = (t >= 0).astype(np.float64)
    if flip:
        f = (np.abs(t) < 30) & (rng.uniform(size=t.size) < 0.05)
        y[f] = 1 - y[f]
    return y


def _direction(rng, d, dtype):
    g = rng.standard_normal(d)
    return (g / np.linalg.norm(g)).astype(dtype).astype(np.float64)


def dense_rows(rng, t, g, dtype, noise=0.3):
    n, d = t.size, g.size
    gg = g @ g
    N = rng.standard_normal((n, d))
    N -= np.outer(N @ g / gg, g)
    N *= noise / np.linalg.norm(N, axis=1, keepdims=True)
    return (np.outer(t / gg, g) + N).astype(dtype)


def dense_ladder(d, dtype, T, seed=0, sizes=SIZES):
    rng = np.random.default_rng(seed)
    t = ladder_t(rng, sizes, T)
    g = _direction(rng, d, dtype)
    X = dense_rows(rng, t, g, dtype)
    return EdgeSet(f"dense_ladder_d{d}_{np.dtype(dtype).name}_T{T}", labels_for(rng, t, True), _offsets(sizes), g, t, dtype, X=X)


def csr_rows(rng, t, g, dtype, kmin, kmax):
    d = g.size
    rp, col, val = [0], [], []
    for ti in t:
        S = np.sort(rng.choice(d, size=int(rng.integers(kmin, kmax + 1)), replace=False))
        gs = g[S]
        col += S.tolist()
        val += (ti * gs / (gs @ gs)).tolist()
        rp.append(len(col))
    return np.array(rp, np.int64), np.array(col, np.int32), np.array(val).astype(dtype)


def csr_ladder(d, dtype, T, kmin=5, kmax=40, seed=SEED_CSR, sizes=SIZES):
    rng = np.random.default_rng(seed)
    t = ladder_t(rng, sizes, T)
    g = _direction(rng, d, dtype)
    csr = csr_rows(rng, t, g, dtype, kmin, kmax)
    return EdgeSet(f"csr_ladder_d{d}_k{kmin}-{kmax}_{np.dtype(dtype).name}_T{T}", labels_for(rng, t, True), _offsets(sizes), g, t,
                   dtype, csr=csr, d=d)


SEPARABLE_BANDS = ((4.0, 12.0), (12.0, 16.0), (18.0, 100.0))


def separable(band, layout, dtype=np.float32, seed=2, sizes=SIZES):
    """No flips, |t| uniform in the band: every row is classified with a margin in it, so the
    Logistic loss is the sum of small terms log1p(exp(-|t|)) (about 2e-3, 1.5e-6, 2e-10 per row)."""
    rng = np.random.default_rng(seed + int(band[0]))
    n = int(sum(sizes))
    t = rng.uniform(band[0], band[1], n) * np.where(rng.uniform(size=n) < 0.5, -1.0, 1.0)
    y = labels_for(rng, t, False)
    if layout == "dense":
        g = _direction(rng, 40, dtype)
        return EdgeSet(f"separable_{band[0]:g}-{band[1]:g}_dense", y, _offsets(sizes), g, t, dtype, X=dense_rows(rng, t, g, dtype))
    g = _direction(rng, 3000, dtype)
    return EdgeSet(f"separable_{band[0]:g}-{band[1]:g}_csr", y, _offsets(sizes), g, t, dtype, csr=csr_rows(rng, t, g, dtype, 5, 40),
                   d=3000)


def exact_ties(ulp_exp, P=3, dtype=np.float64):
    """P partitions of 16 rows; row r of partition p has the single entry x = +-1 at coordinate
    16 p + r, and w0 there is 1 - 2^(ulp_exp - 1), 1 or 1 + 2^ulp_exp (ulp_exp = -52: the
    doubles next to 1; -23: the floats). ls * z = w0[coordinate] exactly, whatever the order of
    the dot's sum, and every Gram entry between rows is exactly 0. Hinge is on only below 1.
    Returns the set, the on mask and the exact Hinge loss sum of the first epoch."""
    n, d = 16 * P, 16 * P
    below, above = 1 - np.ldexp(1.0, ulp_exp - 1), 1 + np.ldexp(1.0, ulp_exp)
    pattern = np.array([below, 1.0, above, below, 1.0, below, above, below, 1.0, above, below, above, 1.0, 1.0, above, below])
    w0 = np.concatenate([np.roll(pattern, 3 * p) for p in range(P)])
    y = np.array([(r + p) % 2 for p in range(P) for r in range(16)], np.float64)
    X = np.zeros((n, d), dtype)
    X[np.arange(n), np.arange(n)] = 2 * y - 1          # ls * x = 1: ls * z = w0
    on = w0 < 1.0
    loss_sum = float(np.sum((1 - w0[on]).astype(np.longdouble)))   # exact: multiples of 2^(ulp_exp-1)
    return EdgeSet(f"exact_ties_2^{ulp_exp}", y, _offsets([16] * P), w0, w0 * (2 * y - 1), dtype, X=X), on, loss_sum


def least_squares_control(es):
    """The ladder's rows as a regression: labels 0.5 t (every row starts with the residual 0.5 t, up
    to 400), and the step scaled to the rows, 0.5 / max ||x||^2 -- at the ladder's 0.05 a row of norm
    800 multiplies the residual by 1 - 0.05 * 800^2 and the run overflows."""
    import copy
    ls = copy.copy(es)
    ls.name = es.name + "_ls"
    ls.y = 0.5 * es.t
    if es.X is not None:
        nsq = np.max(np.sum(es.X.astype(np.float64) ** 2, axis=1))
    else:
        rp, _, val = es.csr
        nsq = max(float(np.sum(val[a:b].astype(np.float64) ** 2)) for a, b in zip(rp[:-1], rp[1:]))
    ls.step = 0.5 / nsq
    return ls


def adam_domain(seed=7):
    """Adam leaving its domain: dense d = 40, two partitions of 24 rows. The last row of the first
    partition is 40 e_0 (+ 0.1 elsewhere), misclassified by w0 (z = -8, label 1), so its squared
    gradient average r = 0.001 g^2 = 1.6 > 1 in coordinate 0 and 1 - r^iter < 0: the reference's
    sqrt makes that coordinate NaN ("as pow does"). Every other row is 0 in coordinate 0 and the row
    is its chain's last, so the NaN stays in coordinate 0. One epoch."""
    rng = np.random.default_rng(seed)
    n, d = 48, 40
    X = rng.standard_normal((n, d))
    X[:, 0] = 0.0
    w0 = rng.standard_normal(d) / np.sqrt(d)
    w0[0] = -0.2
    y = ((X @ w0 + rng.logistic(size=n)) > 0).astype(np.float64)
    X[23] = 0.1
    X[23, 0] = 40.0
    X[23, 1:] -= (X[23, 1:] @ w0[1:]) / (w0[1:] @ w0[1:]) * w0[1:]    # z = 40 * w0[0] = -8
    y[23] = 1.0
    return EdgeSet("adam_domain", y, _offsets([24, 24]), w0, X @ w0, np.float64, X=X)


def multinomial_ladder(layout, K=4, seed=5, sizes=SIZES):
    """K = 4 classes, weights (K - 1) x d with rows g, -g, 0: the class margins of a ladder row are
    t, -t, 0, so the largest sweeps past 0 (the maxMargin > 0 shift) and past 709, where exp would
    overflow without the shift. Labels: class 1 for t > 0, 2 for t < 0, 10 % drawn from all four."""
    rng = np.random.default_rng(seed)
    t = ladder_t(rng, sizes, 800.0)
    d = 40 if layout == "dense" else 3000
    g = _direction(rng, d, np.float64)
    y = np.where(t > 0, 1.0, 2.0)
    f = rng.uniform(size=t.size) < 0.1
    y[f] = rng.integers(0, K, size=int(f.sum())).astype(np.float64)
    w0 = np.concatenate([g, -g, np.zeros(d)])
    if layout == "dense":
        es = EdgeSet(f"multinomial_ladder_dense", y, _offsets(sizes), w0, t, np.float64, X=dense_rows(rng, t, g, np.float64))
    else:
        es = EdgeSet(f"multinomial_ladder_csr", y, _offsets(sizes), w0, t, np.float64, csr=csr_rows(rng, t, g, np.float64, 5, 40), d=d)
    es.num_classes = K
    return es


def regimes_populated(t, offs, T):
    """For every partition of more than one row: the count of rows in each |t| regime below T."""
    out = []
    for a, b in zip(offs[:-1], offs[1:]):
        if b - a <= 1:
            continue
        at = np.abs(t[a:b])
        out.append([int(np.sum((at >= lo) & (at < hi))) for lo, hi in REGIMES if lo < T])
    return out
