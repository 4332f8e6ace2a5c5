"""Binary classification metrics on the device (psgd_binary_counts_device / _model_device through
BinaryClassificationMetrics, HipEngine.binary_counts and the host-pointer C form) against a
restatement of the definitions in numpy and Python integers: a stable argsort of the order-preserving
keys, run lengths for the table, rocNumerator in Python ints, areaUnderROC = num / (2 P N), the PR
terms in fp64 added with math.fsum.

Bars: G, P, N, rocNumerator, thresholds (as uint64), cumPos and cumNeg are equal; areaUnderROC is
bit-equal (each case asserts rocNumerator < 2^53 and 2 P N < 2^53: both conversions are exact and
the one division is correctly rounded); areaUnderPR is within (G + 8) 2^-52 relative of the fsum
reference (each term is a few roundings from exact, and a sum of G non-negative terms in any order
errs by at most (G - 1) 2^-53 of the sum); two calls give the same bits in every output."""
import functools
import json
import math
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, has_gpu

pytestmark = pytest.mark.gpu

FAMILIES = ("wide", "seven", "equal", "special", "ascending", "descending", "lowbyte", "highbyte")


def need_gpu():
    if not has_gpu():
        pytest.skip("no GPU")


def tile():
    import __graft_entry__ as g
    return int(g.load_package().evaluation.SORT_TILE)


def sizes():
    T = tile()
    # empty, tiny, around a wave, around a tile, several tiles with a ragged tail, and more than 256
    # tiles: the sort's table scan takes a second sweep
    return (0, 1, 2, 63, 64, 65, T - 1, T, T + 1, 3 * T + 37, 257 * T + 5)


# ---- the reference -----------------------------------------------------------------------------
def key(s):
    """Ascending uint64 keys in java.lang.Double.compare order."""
    b = np.ascontiguousarray(s, dtype=np.float64).view(np.uint64).copy()
    neg = (b >> np.uint64(63)) == 1
    b[neg] = ~b[neg]
    b[~neg] |= np.uint64(1) << np.uint64(63)
    return b


class Ref:
    def __init__(self, s, y):
        s = np.ascontiguousarray(s, dtype=np.float64)
        y = np.ascontiguousarray(y, dtype=np.float64)
        k = key(s)
        order = np.argsort(k, kind="stable")[::-1]
        ks, pos = k[order], y[order] > 0.5
        if len(s):
            start = np.r_[True, ks[1:] != ks[:-1]]
            gid = np.cumsum(start) - 1
            self.thr = s[order][start]
            self.cp = np.cumsum(np.bincount(gid, pos.astype(np.int64)).astype(np.int64))
            self.cn = np.cumsum(np.bincount(gid, (~pos).astype(np.int64)).astype(np.int64))
        else:
            self.thr, self.cp, self.cn = np.zeros(0), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
        self.G = len(self.thr)
        self.P, self.N = (int(self.cp[-1]), int(self.cn[-1])) if self.G else (0, 0)
        cp, cn = [0] + self.cp.tolist(), [0] + self.cn.tolist()
        self.num = sum((cn[g] - cn[g - 1]) * (cp[g] + cp[g - 1]) for g in range(1, self.G + 1))
        P, N = self.P, self.N
        self.exact = self.num < 2 ** 53 and 2 * P * N < 2 ** 53
        self.roc = float("nan") if P + N == 0 else 0.0 if P == 0 else 1.0 if N == 0 else self.num / (2.0 * P * N)
        cpf, cnf = self.cp.astype(np.float64), self.cn.astype(np.float64)
        rec = np.r_[0.0, cpf / float(P) if P else np.zeros(self.G)]
        prec = np.r_[1.0, cpf / (cpf + cnf)]
        self.pr = math.fsum(((rec[1:] - rec[:-1]) * (prec[1:] + prec[:-1]) / 2.0).tolist())


def scores_of(family, n, seed):
    rng = np.random.default_rng(seed)
    if family == "wide":       # every digit pass is live
        return rng.standard_normal(n) * 10.0 ** rng.integers(-300, 301, size=n)
    if family == "seven":      # heavy ties, constant digits
        return rng.integers(-3, 4, size=n).astype(np.float64)
    if family == "equal":
        return np.full(n, 0.75)
    if family == "special":
        vals = np.array([0.0, -0.0, 5e-324, -5e-324, 1.1e-308, -1.1e-308, np.inf, -np.inf, 1.0, -1.0])
        return vals[rng.integers(0, len(vals), size=n)]
    if family == "ascending":
        return np.sort(rng.standard_normal(n))
    if family == "descending":
        return np.sort(rng.standard_normal(n))[::-1].copy()
    if family == "lowbyte":    # keys that differ only in their lowest byte
        bits = np.uint64(0x3FF0000000000000) | rng.integers(0, 256, size=n).astype(np.uint64)
        return bits.view(np.float64)
    if family == "highbyte":   # keys that differ only in their highest byte (sign and 7 exponent bits)
        bits = (rng.integers(0, 256, size=n).astype(np.uint64) << np.uint64(56)) | np.uint64(0x000123456789ABCD)
        return bits.view(np.float64)
    raise KeyError(family)


def labels_of(kind, s, seed):
    rng = np.random.default_rng(seed + 1)
    n = len(s)
    if kind == "odds":         # score-dependent odds
        return (rng.random(n) < 1.0 / (1.0 + np.exp(-np.clip(s, -5.0, 5.0)))).astype(np.float64)
    if kind == "positive":
        return np.ones(n)
    if kind == "negative":
        return np.zeros(n)
    if kind == "edges":        # positive means label > 0.5
        return np.array([0.5, 0.5000001, 2.0, -1.0])[rng.integers(0, 4, size=n)]
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def case(family, n, kind="odds"):
    s = scores_of(family, n, 1000 + 17 * FAMILIES.index(family) + n % 9973)
    y = labels_of(kind, s, n % 7919)
    assert not np.isnan(s).any()
    return s, y, Ref(s, y)


def outputs(m):
    thr, cp, cn = m.cumulativeCounts()
    return (m.numThresholds, m.numPositives, m.numNegatives, m.rocNumerator, thr.view(np.uint64).tolist(),
            cp.tolist(), cn.tolist(), np.float64(m.areaUnderROC()).view(np.uint64), np.float64(m.areaUnderPR()).view(np.uint64))


def check(m, ref, what):
    assert (m.numThresholds, m.numPositives, m.numNegatives, m.rocNumerator) == (ref.G, ref.P, ref.N, ref.num), what
    thr, cp, cn = m.cumulativeCounts()
    assert np.array_equal(thr.view(np.uint64), ref.thr.view(np.uint64)), what
    assert np.array_equal(cp, ref.cp) and np.array_equal(cn, ref.cn), what
    assert ref.exact, (what, ref.num, ref.P, ref.N)
    got = m.areaUnderROC()
    print(what, "G", ref.G, "roc", got, ref.roc, "pr", m.areaUnderPR(), ref.pr)
    assert np.float64(got).view(np.uint64) == np.float64(ref.roc).view(np.uint64), (what, got, ref.roc)
    assert abs(m.areaUnderPR() - ref.pr) <= (ref.G + 8) * 2.0 ** -52 * abs(ref.pr), (what, m.areaUnderPR(), ref.pr)


@pytest.mark.parametrize("n_index", range(11))
@pytest.mark.parametrize("family", FAMILIES)
def test_array_form(pkg, family, n_index):
    need_gpu()
    n = sizes()[n_index]
    s, y, ref = case(family, n)
    m = pkg.BinaryClassificationMetrics(s, y)
    check(m, ref, (family, n))
    again = pkg.BinaryClassificationMetrics(s, y)
    assert outputs(again) == outputs(m), (family, n)


@pytest.mark.parametrize("kind", ("positive", "negative", "edges"))
def test_label_kinds(pkg, kind):
    need_gpu()
    n = 3 * tile() + 37
    s, y, ref = case("seven" if kind == "edges" else "wide", n, kind)
    if kind == "positive":
        assert ref.N == 0 and ref.roc == 1.0
    if kind == "negative":
        assert ref.P == 0 and ref.roc == 0.0 and ref.pr == 0.0
    check(pkg.BinaryClassificationMetrics(s, y), ref, (kind, n))


def test_host_pointer_form_and_areas_alone(pkg):
    """psgd_binary_counts from host arrays (no partition registered), with the table and without;
    device tensors in; the partial-table and null-pointer refusals that need a context."""
    need_gpu()
    import ctypes as C
    import torch
    from spark_parallelized_sgd_amd.optimization import get_context
    N = pkg._native
    ctx = get_context(torch.cuda.current_device())
    for n in (0, 65, tile() + 1):
        s, y, ref = case("wide", n)
        thr, cp, cn, summary, areas = ctx.binary_counts(s, y)
        assert summary.tolist() == [ref.G, ref.P, ref.N, ref.num]
        assert np.array_equal(thr.view(np.uint64), ref.thr.view(np.uint64))
        assert np.array_equal(cp, ref.cp) and np.array_equal(cn, ref.cn)
        none = ctx.binary_counts(s, y, table=False)
        assert none[0] is None and none[3].tolist() == summary.tolist()
        assert none[4].view(np.uint64).tolist() == areas.view(np.uint64).tolist()
        assert math.isnan(areas[0]) if n == 0 else areas[0] == ref.roc
        if n:
            m = pkg.BinaryClassificationMetrics(torch.from_numpy(s).cuda(), torch.from_numpy(y).cuda())
            check(m, ref, ("tensors", n))
    s, y, _ = case("wide", 65)
    L, out4, out2, one = N.lib(), (C.c_int64 * 4)(), (C.c_double * 2)(), np.zeros(65)
    p = lambda a: C.c_void_p(a.ctypes.data)
    assert L.psgd_binary_counts(ctx.handle, p(s), p(y), 65, p(one), None, None, out4, out2) == N.PSGD_EINVAL
    assert L.psgd_binary_counts(ctx.handle, None, p(y), 65, None, None, None, out4, out2) == N.PSGD_EINVAL
    assert L.psgd_binary_counts(ctx.handle, p(s), p(y), 65, None, None, None, None, out2) == N.PSGD_EINVAL
    assert L.psgd_binary_counts(ctx.handle, p(s), p(y), -1, None, None, None, out4, out2) == N.PSGD_EINVAL
    assert L.psgd_binary_counts(ctx.handle, p(s), p(y), 2 ** 31, None, None, None, out4, out2) == N.PSGD_EUNSUPPORTED


# ---- the model form -----------------------------------------------------------------------------
MODEL_SIZES = (700, 0, 1500)   # three partitions, one of them empty


def model_data(pkg, layout):
    """(data, X as f64 [n, d], y, w): the seed is picked so that the margins' order is safe (below)."""
    rng = np.random.default_rng({"dense32": 11, "dense64": 12, "csr": 13}[layout])
    n, d = sum(MODEL_SIZES), 40
    X = rng.standard_normal((n, d))
    if layout == "csr":
        X = X * (rng.random((n, d)) < 0.25)
    if layout == "dense32":
        X = X.astype(np.float32).astype(np.float64)
    w = rng.standard_normal(d)
    y = (rng.random(n) < 1.0 / (1.0 + np.exp(-(X @ w)))).astype(np.float64)
    offs = np.r_[0, np.cumsum(MODEL_SIZES)]
    parts = []
    for a, b in zip(offs[:-1], offs[1:]):
        if layout == "csr":
            rp, cols, vals = [0], [], []
            for r in range(a, b):
                nz = np.nonzero(X[r])[0]
                cols.extend(nz.tolist())
                vals.extend(X[r, nz].tolist())
                rp.append(len(cols))
            parts.append(pkg.CsrPartition(y[a:b], np.array(rp, dtype=np.int64), np.array(cols, dtype=np.int32),
                                          np.array(vals, dtype=np.float64), d))
        else:
            parts.append(pkg.DensePartition(y[a:b], np.ascontiguousarray(
                X[a:b], dtype=np.float32 if layout == "dense32" else np.float64)))
    return pkg.PartitionedData(parts), X, y, w


@pytest.mark.parametrize("layout", ("dense32", "dense64", "csr"))
def test_model_form(pkg, layout):
    need_gpu()
    import torch
    B = pkg.BinaryClassificationMetrics
    data, X, y, w = model_data(pkg, layout)
    engine = pkg.HipEngine(data)
    m = B.fromModel(data, w, engine=engine)
    # the array form on engine.predict's own margins: exactly the same
    margins = torch.cat([engine.predict(p, w) for p in range(3)])
    assert margins.shape[0] == len(y)
    arr = B(margins, y)
    assert outputs(m) == outputs(arr)
    check(m, Ref(margins.cpu().numpy(), y), (layout, "device margins"))
    # numpy's fp64 margins: where no two adjacent margins of opposite labels are closer than the
    # dots' error bound, the order of positives against negatives is the device's, and so is the area
    z = X @ w
    bound = 1e-9 * (1.0 + np.abs(X) @ np.abs(w))
    order = np.argsort(z)
    zs, ys, bs = z[order], y[order], bound[order]
    mixed = ys[1:] != ys[:-1]
    assert np.all((zs[1:] - zs[:-1])[mixed] > np.maximum(bs[1:], bs[:-1])[mixed])
    ref = Ref(z, y)
    assert ref.exact and ref.G == len(y)
    assert (m.numPositives, m.numNegatives, m.rocNumerator) == (ref.P, ref.N, ref.num)
    assert np.float64(m.areaUnderROC()).view(np.uint64) == np.float64(ref.roc).view(np.uint64)
    # probabilities: the reference on the same torch.sigmoid values
    prob = B.fromModel(data, w, score="probability", engine=engine)
    check(prob, Ref(torch.sigmoid(margins).cpu().numpy(), y), (layout, "probability"))
    # the C form from host weights: every registered row, the registry's own labels
    ctx = engine.ctx
    import ctypes as C
    n = len(y)
    thr, cp, cn = np.zeros(n), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    summary, areas = np.zeros(4, dtype=np.int64), np.zeros(2)
    wh = np.ascontiguousarray(w)
    p = lambda a: C.c_void_p(a.ctypes.data)
    rc = pkg._native.lib().psgd_binary_counts_model(ctx.handle, p(wh), p(thr), p(cp), p(cn), p(summary), p(areas))
    assert rc == 0, pkg._native.lib().psgd_last_error()
    G = int(summary[0])
    assert outputs(m)[:4] == tuple(summary.tolist()) and outputs(m)[4:7] == (
        thr[:G].view(np.uint64).tolist(), cp[:G].tolist(), cn[:G].tolist())
    assert areas.view(np.uint64).tolist() == [outputs(m)[7], outputs(m)[8]]


def test_model_form_leaves_the_epoch_state_alone(pkg):
    need_gpu()
    data, X, y, w = model_data(pkg, "dense64")
    engine = pkg.HipEngine(data)
    pkg.runParallelizedSGD(data, pkg.LogisticGradient(), pkg.SimpleSGDUpdater(), 1.0, 1, 0.0, 1.0, np.zeros(40), 0.0)
    before = (engine.ctx.last_kernel(), engine.ctx.chain_launches())
    pkg.BinaryClassificationMetrics.fromModel(data, w, engine=engine)
    assert (engine.ctx.last_kernel(), engine.ctx.chain_launches()) == before


def test_model_form_without_rows_and_without_partitions(pkg):
    """A registry of empty partitions is n = 0 (zeros, NaN, no kernel); no registry is PSGD_ESTATE."""
    need_gpu()
    import ctypes as C
    import torch
    N = pkg._native
    parts = [pkg.DensePartition(np.zeros(0), np.zeros((0, 6))) for _ in range(2)]
    m = pkg.BinaryClassificationMetrics.fromModel(pkg.PartitionedData(parts), np.ones(6))
    assert (m.numThresholds, m.numPositives, m.numNegatives, m.rocNumerator) == (0, 0, 0, 0)
    assert math.isnan(m.areaUnderROC()) and m.areaUnderPR() == 0.0 and m.thresholds().shape == (0,)
    ctx = N.Context(torch.cuda.current_device())
    try:
        w, out4, out2 = (C.c_double * 6)(), (C.c_int64 * 4)(), (C.c_double * 2)()
        assert N.lib().psgd_binary_counts_model(ctx.handle, w, None, None, None, out4, out2) == N.PSGD_ESTATE
        assert b"no partitions registered" in N.lib().psgd_last_error()
        assert N.lib().psgd_binary_counts_model(ctx.handle, None, None, None, None, out4, out2) == N.PSGD_EINVAL
    finally:
        ctx.close()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_ranks(tmp_path, pkg):
    """Two ranks sharing cuda:0 over gloo, each a fresh child process (tests/two_rank_metrics.py):
    both hold the one-rank result bit for bit."""
    need_gpu()
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import two_rank_metrics as T
    out = str(tmp_path / "res.json")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "two_rank_metrics.py"), out], env=env,
                       capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    with open(out) as f:
        res = json.load(f)
    X, y, w = T.make_data()
    data = pkg.PartitionedData.parallelize(y, X, T.PARTS)
    one = T.summarize(pkg.BinaryClassificationMetrics.fromModel(data, w))
    assert len(res) == 2 and one["G"] > 0
    for rank in ("0", "1"):
        assert res[rank] == one, rank
