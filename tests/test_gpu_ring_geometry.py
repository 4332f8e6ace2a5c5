"""The dense chain kernels at every LDS ring geometry, against the CPU oracle.

chain_dense, chain_split, chain_block and chain_block64 stream their rows through an LDS ring
(ring_loader, psgd_device.h) whose size follows from the number of chains: 160 KiB /
ceil(P / CUs) per workgroup. Here they run (a) with more chains than the device has CUs, from the
chain count at which a wide row's ring no longer fits its even share of the LDS and the launch
takes the minimum ring, and (b) at a few chains with PSGD_LDS_BUDGET set to the budgets of
test_ring_geometry.sweep_budgets: the minimum ring, the largest ring on the loader's drain-and-
publish path (R < D + 2 PUB + 2 GB), the smallest one past it, and the default. The partitions are
ragged around the ring's sizes (R - 1, R, R + 1, 2R, D, D + 1, a meta block's 16 rows +- 1, ...),
with and without per-sample breaks before and after the ring has wrapped, and one sampled epoch.
psgd_ctx_last_ring confirms the geometry that ran. The ring moves rows and does no arithmetic:
results at the minimum ring equal the default ring's bit for bit.

Bars: fp64 compute 1e-9 (1e-12 floor) and exact chain counts; fp32 compute FP32_REL /
FP32_LOSS_REL, counts at tol > 0 by fp32_break_counts_agree (test_gpu_parity)."""
import numpy as np
import pytest

import test_ring_geometry as RG
from conftest import has_gpu
from test_gpu_parity import FP32_LOSS_REL, FP32_REL, G, U, assert_close, fp32_break_counts_agree
from test_ring_geometry import BLOCK, BLOCK64, DENSE, F32, F64, SPLIT

pytestmark = pytest.mark.gpu

GRADS = ("logistic", "least_squares", "hinge")


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not has_gpu():
        pytest.skip("no GPU")


def num_cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def variant(family, nv, tol):
    if family == DENSE:
        return 100 + nv
    if family == SPLIT:
        return 800 + 10 * min(nv, 4) + nv
    if family == BLOCK:
        return 300 + (40 if tol > 0 else 0) + nv
    return 700 + (40 if tol > 0 else 0) + (10 if nv >= 2 else 0) + nv   # two chain waves from NV 2


def width(nv, storage, ragged):
    """Features of rows of nv 16-byte vectors per lane; ragged: the last vector is partly past d."""
    top = nv * 64 * (16 // np.dtype(storage).itemsize)
    return top - 5 if ragged else top


def setup(family, nv, storage, k):
    """Gradient, updater, compute mode and step of case k of a family: the three gradients and the
    family's updaters rotate over the cases. chain_dense takes Simple / SquaredL2 / L1 under
    PSGD_PER_SAMPLE=1 (without it only its NV = 1 instances run); chain_split AdaGrad / Adam / L1;
    the blocked kernels Simple / SquaredL2 in their compute mode."""
    grad = GRADS[k % 3]
    f32_rows = np.dtype(storage) == np.float32
    if family == DENSE:
        upd, compute = ("simple", "squared_l2", "l1")[k % 3], ("f64", "f32")[(k // 2) % 2]
    elif family == SPLIT:
        upd = ("adagrad", "adam", "l1")[k % 3]
        compute = "f32" if f32_rows else "f64"
    else:
        upd, compute = ("simple", "squared_l2")[k % 2], "f32" if family == BLOCK else "f64"
    d = width(nv, storage, ragged=f32_rows)
    if upd in ("adagrad", "adam"):   # steps per coordinate: a row moves its dot by ~ step * sum |x_i|
        step = 0.5 / d if grad == "least_squares" else 0.01 if compute == "f32" else 0.05
    else:   # non-chaotic trajectories (||x||^2 ~ d)
        step = {"least_squares": 0.5, "logistic": 4.0, "hinge": 2.0}[grad] / d
    reg = {"simple": 0.0, "squared_l2": 0.05, "l1": 0.001, "adagrad": 0.0, "adam": 0.0}[upd]
    return dict(family=family, nv=nv, storage=storage, grad=grad, upd=upd, compute=compute, d=d,
                step=step, reg=reg, env={"PSGD_PER_SAMPLE": "1"} if family == DENSE else {})


def synth(rng, n, d, grad, storage):
    X = rng.standard_normal((n, d), dtype=np.float32).astype(storage)
    wt = rng.standard_normal(d) / np.sqrt(d)
    z = X.astype(np.float64) @ wt
    if grad == "least_squares":
        y = z + 0.1 * rng.standard_normal(n)
    else:
        y = ((z + rng.logistic(size=n)) > 0).astype(np.float64)
    return X, y


def ragged_lengths(R, D):
    """Chain lengths around the ring's sizes: empty, one row, a block +- 1, the ring +- 1, twice the
    ring (+ 1), the loader's depth (+ 1), a meta block's multiple +- 1 past two rings, and two
    chains of several rings."""
    m = 16 * ((2 * R + 2) // 16 + 1)
    return [0, 1, 7, 8, 9, R - 1, R, R + 1, 2 * R, 2 * R + 1, D, D + 1, m - 1, m + 1, 3 * R + 5, 4 * R + 3]


def pick_tol(oracle, mat, offs, c, w0, iters, R, fp32):
    """A tol at which, by the oracle, some chain breaks before the ring has wrapped (count <= R)
    and some chain after (R < count < its length). From the oracle's traces r_k = diff_k /
    max(norm_k, 1) of the chains longer than R (sample k passes isConverged iff r_k < tol): chain
    a breaks within R samples iff tol > min r_a[:R]; chain b after them and before its end iff
    min r_b[:len - 1] < tol <= min r_b[:R]. The pair with the widest such interval, tol in its
    (geometric) middle: every decision that matters is far from flipping. The counts of the
    oracle's run at that tol are then checked for both kinds of break (fp64 margins by
    CheckedOracle.run when the kernel's result is compared; fp32 compute hands the margins to
    fp32_break_counts_agree)."""
    sizes = np.diff(offs)
    long_chains = [p for p in range(len(sizes)) if sizes[p] >= R + 2]
    low = {p: np.minimum.accumulate(oracle.ratio_trace(mat, offs, p, c["grad"], c["upd"], c["step"], c["reg"], w0))
           for p in long_chains}
    best, tol = 0.0, None
    for a in long_chains:
        for b in long_chains:
            lo, hi = max(low[a][R - 1], low[b][sizes[b] - 2]), low[b][R - 1]
            if a != b and hi > lo and (lo == 0.0 or hi / lo > best):
                best = float("inf") if lo == 0.0 else hi / lo
                tol = hi / 2 if lo == 0.0 else float(np.sqrt(lo * hi))
    assert tol is not None and best > 1.01, f"no tol breaks chains on both sides of R = {R}: {c}"
    _, _, cr, mg = oracle.run_with_margins(mat, offs, c["grad"], c["upd"], c["step"], iters, c["reg"], w0, tol=tol)
    first = [(int(n), int(s)) for n, s in zip(cr[0], sizes)]
    assert any(0 < n <= R and n < s for n, s in first), ("no break before the ring wraps", R, tol, first)
    assert any(R < n < s for n, s in first), ("no break after the ring has wrapped", R, tol, first)
    return tol


def run_and_check(pkg, oracle, c, parts, X, y, offs, tol, iters=2, fraction=1.0, tag=""):
    d = c["d"]
    w0 = np.zeros(d)
    data = pkg.PartitionedData(parts)
    w, h, counts = pkg.runParallelizedSGD(data, getattr(pkg, G[c["grad"]])(), getattr(pkg, U[c["upd"]])(),
                                          c["step"], iters, c["reg"], fraction, w0, tol,
                                          compute_dtype=c["compute"], return_chain_counts=True)
    ctx = pkg.optimization.get_context(0)
    got = (ctx.last_kernel(), ctx.last_ring())
    mat = oracle.Matrix(y, X.astype(np.float64))
    kw = dict(fraction=fraction) if fraction < 1.0 else {}
    if c["compute"] == "f64":
        wr, hr, cr = oracle.run(mat, offs, c["grad"], c["upd"], c["step"], iters, c["reg"], w0, tol=tol, **kw)
        assert [list(map(int, x)) for x in counts] == [list(map(int, x)) for x in cr[: len(counts)]], tag
        assert len(h) == len(hr), tag
        assert_close(w, wr, what=tag + " weights")
        assert_close(h, hr, what=tag + " loss")
    else:
        if tol > 0:
            wr, hr, cr, mg = oracle.run_with_margins(mat, offs, c["grad"], c["upd"], c["step"], iters,
                                                     c["reg"], w0, tol=tol, **kw)
            same = fp32_break_counts_agree(counts, cr, mg, tag) and len(h) == len(hr)
        else:
            wr, hr, cr = oracle.run(mat, offs, c["grad"], c["upd"], c["step"], iters, c["reg"], w0, tol=tol, **kw)
            assert [list(map(int, x)) for x in counts] == [list(map(int, x)) for x in cr], tag
            same = True
        if same:
            err = np.max(np.abs(w - wr)) / max(np.max(np.abs(wr)), 1e-30)
            assert err <= FP32_REL, f"{tag}: weights max err {err:.3g} x max|w|"
            assert_close(h, hr, rel=FP32_LOSS_REL, what=tag + " loss")
    return got, (w, h, counts)


def partitions(pkg, X, y, offs):
    return [pkg.DensePartition(y[a:b], X[a:b]) for a, b in zip(offs[:-1], offs[1:])]


# ---- more chains than CUs ----------------------------------------------------------------------
# (family, nv, storage, chains per CU before the extra one, case index of setup()): the first chain
# count at which the even share of the LDS is below the family's minimum ring -- 160 KiB / 2 for
# the blocked kernels' 8 KiB rows (d 1,024 f64 / 2,048 f32), / 3 for 4 KiB, / 5 for 2 KiB, / 9 for
# 1 KiB; / 4 and / 7 for chain_split's and chain_dense's 8 and 4 KiB rows.
MANY = [
    (BLOCK64, 8, np.float64, 1, 0), (BLOCK64, 8, np.float32, 1, 1), (BLOCK, 8, np.float32, 1, 2),
    (BLOCK, 8, np.float64, 1, 3),
    (BLOCK64, 4, np.float32, 2, 4), (BLOCK, 4, np.float32, 2, 5),
    (BLOCK64, 2, np.float32, 4, 6), (BLOCK, 2, np.float32, 4, 7),
    (BLOCK64, 1, np.float64, 8, 8), (BLOCK, 1, np.float32, 8, 9), (DENSE, 1, np.float64, 8, 10),
    (SPLIT, 8, np.float64, 3, 11), (DENSE, 8, np.float64, 3, 12),
    (SPLIT, 4, np.float32, 6, 13), (DENSE, 4, np.float32, 6, 14),
]


@pytest.mark.parametrize("family,nv,storage,per_cu,k", MANY,
                         ids=[f"{RG.NAMES[f]}-nv{nv}-{np.dtype(s).name}-{p}xCUs+1" for f, nv, s, p, _ in MANY])
def test_more_chains_than_cus(pkg, oracle, monkeypatch, family, nv, storage, per_cu, k):
    """P = per_cu x CUs + 1 chains of 8-24 rows, tol 0: the kernel the shape gets at two chains, at
    the family's minimum ring (chain_dense's 1 KiB rows at 8 x CUs + 1 still fit their share)."""
    c = setup(family, nv, storage, k)
    if family == BLOCK64 and k == 0:
        c.update(grad="logistic", upd="simple")      # d 1,024 f64 rows, Simple, fp64: c3's parity run
        c["step"] = 4.0 / c["d"]
        c["reg"] = 0.0
    for name, v in c["env"].items():
        monkeypatch.setenv(name, v)
    P = per_cu * num_cus() + 1
    rng = np.random.default_rng(1000 + k)
    lens = rng.integers(8, 25, size=P)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(int).tolist()
    X, y = synth(rng, offs[-1], c["d"], c["grad"], storage)
    parts = partitions(pkg, X, y, offs)
    tag = f"{RG.NAMES[family]} nv={nv} P={P}"
    (kern2, _), _ = run_and_check(pkg, oracle, c, parts[:2], X[: offs[2]], y[: offs[2]], offs[:3], 0.0,
                                  tag=tag + " two chains")
    assert kern2 == variant(family, nv, 0.0), tag
    (kern, ring), _ = run_and_check(pkg, oracle, c, parts, X, y, offs, 0.0, tag=tag)
    assert kern == kern2, tag
    compute = F32 if c["compute"] == "f32" else F64
    want = RG.ring_geometry(pkg, family, nv, compute, False, RG.spread_budget(P, num_cus()))
    assert ring == want[:4], (tag, ring, want)
    if not (family == DENSE and nv == 1):
        assert ring[0] == RG.MIN_ROWS[family], (tag, ring)
        assert RG.old_geometry(family, nv, compute, False, RG.spread_budget(P, num_cus())) is None
    else:
        assert ring[0] >= RG.MIN_ROWS[family]


# ---- the geometry sweep at a few chains --------------------------------------------------------
SWEEP = [(fam, nv, st) for fam, nvs in ((DENSE, (1, 2, 4, 8)), (SPLIT, (2, 4, 8)), (BLOCK, (1, 2, 4, 8)),
                                        (BLOCK64, (1, 2, 4, 8)))
         for nv in nvs for st in (np.float32, np.float64)]
SWEEP_IDS = [f"{RG.NAMES[f]}-nv{nv}-{np.dtype(s).name}" for f, nv, s in SWEEP]


def sweep_case(pkg, oracle, monkeypatch, family, nv, storage, k, tol_on, only=None, fraction=1.0):
    c = setup(family, nv, storage, k)
    for name, v in c["env"].items():
        monkeypatch.setenv(name, v)
    compute = F32 if c["compute"] == "f32" else F64
    out = {}
    for name, (budget, R) in RG.sweep_budgets(pkg, family, nv, compute, tol_on).items():
        if only and name not in only:
            continue
        if budget is None:
            monkeypatch.delenv("PSGD_LDS_BUDGET", raising=False)
        else:
            monkeypatch.setenv("PSGD_LDS_BUDGET", str(budget))
        D = RG.DEPTH[nv]
        lens = ragged_lengths(R, D)
        if fraction < 1.0:   # the sampled chains are about as long as the unsampled sweep's
            lens = [int(np.ceil(n / fraction)) for n in lens]
        offs = np.concatenate([[0], np.cumsum(lens)]).astype(int).tolist()
        rng = np.random.default_rng(family * 1000 + nv * 100 + R)
        X, y = synth(rng, offs[-1], c["d"], c["grad"], storage)
        tag = f"{RG.NAMES[family]} nv={nv} {np.dtype(storage).name} {c['grad']} {c['upd']} {c['compute']} {name} R={R}"
        tol = 0.0
        if tol_on:
            tol = pick_tol(oracle, oracle.Matrix(y, X.astype(np.float64)), offs, c, np.zeros(c["d"]), 2, R,
                           c["compute"] == "f32")
        (kern, ring), res = run_and_check(pkg, oracle, c, partitions(pkg, X, y, offs), X, y, offs, tol,
                                          fraction=fraction, tag=f"{tag} tol={tol}")
        assert kern == variant(family, nv, tol), (tag, kern)
        want = RG.ring_geometry(pkg, family, nv, compute, tol_on, budget if budget else RG.spread_budget(1))
        assert ring == want[:4] and ring[0] == R, (tag, ring, want)
        out[name] = res
    return out


@pytest.mark.parametrize("tol_on", [False, True], ids=["tol0", "breaks"])
@pytest.mark.parametrize("family,nv,storage", SWEEP, ids=SWEEP_IDS)
def test_ring_sweep(pkg, oracle, monkeypatch, family, nv, storage, tol_on):
    k = SWEEP.index((family, nv, storage))
    ran = sweep_case(pkg, oracle, monkeypatch, family, nv, storage, k, tol_on)
    assert "min" in ran


BY_FAMILY = [(DENSE, 2, np.float64), (SPLIT, 4, np.float32), (BLOCK, 2, np.float32), (BLOCK64, 1, np.float64),
             (BLOCK64, 4, np.float64)]
BY_FAMILY_IDS = ["chain_dense", "chain_split", "chain_block", "chain_block64-H1", "chain_block64-H2"]


@pytest.mark.parametrize("family,nv,storage", BY_FAMILY, ids=BY_FAMILY_IDS)
def test_sampled_epoch_at_the_minimum_ring(pkg, oracle, monkeypatch, family, nv, storage):
    """miniBatchFraction 0.3: the loader reads the sampled row indices instead of counting rows."""
    k = 3 + BY_FAMILY.index((family, nv, storage))
    sweep_case(pkg, oracle, monkeypatch, family, nv, storage, k, False, only=("min",), fraction=0.3)


@pytest.mark.parametrize("tol_on", [False, True], ids=["tol0", "breaks"])
@pytest.mark.parametrize("family,nv,storage", BY_FAMILY, ids=BY_FAMILY_IDS)
def test_bits_do_not_depend_on_the_ring(pkg, oracle, monkeypatch, family, nv, storage, tol_on):
    """The same data at the minimum ring and at the default one: weights, loss history and counts
    equal bit for bit (the blocks are the chain's rows 8 by 8 from its start whatever R is)."""
    c = setup(family, nv, storage, 1 + BY_FAMILY.index((family, nv, storage)))
    for name, v in c["env"].items():
        monkeypatch.setenv(name, v)
    compute = F32 if c["compute"] == "f32" else F64
    r_def = RG.ring_geometry(pkg, family, nv, compute, tol_on, RG.spread_budget(1))[0]
    offs = np.concatenate([[0], np.cumsum(ragged_lengths(r_def, RG.DEPTH[nv]))]).astype(int).tolist()
    rng = np.random.default_rng(77 + family * 10 + nv)
    X, y = synth(rng, offs[-1], c["d"], c["grad"], storage)
    tol = 0.0
    if tol_on:
        tol = pick_tol(oracle, oracle.Matrix(y, X.astype(np.float64)), offs, c, np.zeros(c["d"]), 2,
                       16, c["compute"] == "f32")   # before / after the 16th row: both rings have wrapped or not
    parts = partitions(pkg, X, y, offs)
    res = {}
    for name, budget in (("min", "256"), ("default", None)):
        if budget is None:
            monkeypatch.delenv("PSGD_LDS_BUDGET", raising=False)
        else:
            monkeypatch.setenv("PSGD_LDS_BUDGET", budget)
        (_, ring), res[name] = run_and_check(pkg, oracle, c, parts, X, y, offs, tol,
                                             tag=f"{RG.NAMES[family]} nv={nv} {name} tol={tol}")
        assert ring[0] == (RG.MIN_ROWS[family] if name == "min" else r_def)
    (w0, h0, c0), (w1, h1, c1) = res["min"], res["default"]
    assert np.array_equal(w0, w1) and np.array_equal(h0, h1)
    assert [list(map(int, x)) for x in c0] == [list(map(int, x)) for x in c1]


def test_last_ring_is_zero_after_a_kernel_without_a_ring(pkg):
    """chain_general (d past the register-resident range) has no LDS ring: zeros, also right after
    a ring kernel's launch on the same context."""
    rng = np.random.default_rng(5)
    ctx = pkg.optimization.get_context(0)
    for d, want_ring in ((100, True), (3000, False)):
        X, y = synth(rng, 64, d, "logistic", np.float64)
        pkg.runParallelizedSGD(pkg.PartitionedData.parallelize(y, X, 2), pkg.LogisticGradient(),
                               pkg.SimpleSGDUpdater(), 1.0 / d, 1, 0.0, 1.0, np.zeros(d), 0.0)
        if want_ring:
            assert ctx.last_kernel() == 701 and ctx.last_ring() == RG.ring_geometry(
                pkg, BLOCK64, 1, F64, False, RG.spread_budget(2, num_cus()))[:4]
        else:
            assert ctx.last_kernel() == 200 and ctx.last_ring() == (0, 0, 0, 0)
