"""The chain kernels on saturated margins and exact ties (tests/edge_data.py; its conditions are
checked on the CPU by tests/test_edge_data.py) against the fp64 oracle.

The other parity tests draw N(0,1) rows and start from zero weights: margins within a few units
of 0. Here the first margins run from 0 to +-800 (fp64: past exp's overflow and the clamps of
recip_one_plus_exp) or +-120 (fp32: past expf's), some rows are misclassified at |margin| up to
30, and the separable sets have every row classified with a margin of 4-12, 12-16 or 18-100, so
that the Logistic loss is a sum of terms down to 1e-44.

Bars: the existing ones. fp64: weights within 1e-9 of the UPDATE max|w_ref - w0| (w0 is a unit
vector here and would hide a wrong multiplier behind max|w|), loss history 1e-9 relative, chain
counts exact. fp32 compute: FP32_REL x max|w_ref| and FP32_LOSS_REL relative on the loss history,
as test_gpu_sparse.py / test_gpu_block.py -- on the separable sets too, where until the
cancellation-free form (psgd_device.h softplus_fast) the CSR kernels and chain_dense returned a
loss of exactly 0 for margins past 17 and 4 % off for margins of 12-16.

Kernel families are selected with the existing environment knobs and checked by the hundreds
digit of last_kernel() (1xx chain_dense, 2xx chain_general, 3xx chain_block, 4xx
chain_sparse / _spec / chain_sparse64, 5xx chain_multinomial, 6xx chain_sparse_lds, 7xx chain_block64,
8xx chain_split).
"""
import numpy as np
import pytest

import edge_data as ED
from conftest import has_gpu

pytestmark = pytest.mark.gpu

FP32_REL = 2e-4
FP32_LOSS_REL = 1e-4
F64_REL = 1e-9
ITERS = 3

G = {"logistic": "LogisticGradient", "least_squares": "LeastSquaresGradient", "hinge": "HingeGradient"}
U = {"simple": "SimpleSGDUpdater", "squared_l2": "SquaredL2SGDUpdater", "l1": "L1SGDUpdater",
     "adagrad": "AdaGradSGDUpdater", "adam": "AdamSGDUpdater"}
KNOBS = ("PSGD_SPARSE_KERNEL", "PSGD_SPARSE_LDS_HEAD", "PSGD_SPARSE_SK", "PSGD_PER_SAMPLE")


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not has_gpu():
        pytest.skip("no GPU")


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


_sets = {}


def cached(key, make):
    if key not in _sets:
        _sets[key] = make()
    return _sets[key]


_refs = {}


def reference(oracle, es, grad, upd, reg, iters, tol=0.0):
    """The oracle's run of a set, computed once and shared (at tol > 0 with its break margins
    checked, conftest.CheckedOracle)."""
    key = (es.name, grad, upd, reg, iters, tol)
    if key not in _refs:
        kw = {"num_classes": es.num_classes} if hasattr(es, "num_classes") else {}
        _refs[key] = oracle.run(es.oracle_matrix(oracle), es.offs, grad, upd, es.step, iters, reg, es.w0, tol=tol, **kw)
    return _refs[key]


def run(pkg, es, grad, upd, reg, iters, compute, tol=0.0):
    kw = {"compute_dtype": "f32"} if compute == "f32" else {}
    g = getattr(pkg, G[grad])(*([es.num_classes] if hasattr(es, "num_classes") else []))
    w, h, counts = pkg.runParallelizedSGD(es.partitions(pkg), g, getattr(pkg, U[upd])(), es.step,
                                          iters, reg, 1.0, es.w0.copy(), tol, return_chain_counts=True, **kw)
    return w, h, counts, pkg.optimization.get_context(0).last_kernel()


def check(pkg, oracle, es, grad, upd, compute, family, reg=0.0, iters=ITERS, tol=0.0):
    wr, hr, cr = reference(oracle, es, grad, upd, reg, iters, tol)
    w, h, counts, variant = run(pkg, es, grad, upd, reg, iters, compute, tol)
    tag = f"{es.name} {grad} {upd} {compute} tol {tol} variant {variant}"
    assert len(h) == len(hr), tag
    assert variant // 100 == family, tag
    assert [list(c) for c in counts] == [list(c) for c in cr[: len(counts)]], tag
    herr = float(np.max(np.abs(h - hr) / np.maximum(np.abs(hr), 1e-300)))
    if compute == "f64":
        werr = float(np.max(np.abs(w - wr)) / np.max(np.abs(wr - es.w0)))
        print(f"{tag}: weights {werr:.3g} x max|w_ref - w0|, loss {herr:.3g} relative, history {h}")
        assert werr <= F64_REL and herr <= F64_REL, tag
    else:
        werr = float(np.max(np.abs(w - wr)) / np.max(np.abs(wr)))
        print(f"{tag}: weights {werr:.3g} x max|w_ref|, loss {herr:.3g} relative, history {h}")
        assert werr <= FP32_REL, tag
        assert herr <= FP32_LOSS_REL, f"{tag}: loss history {h} against {hr}"


# ------------------------------------------------------------------------------------------------
# fp64
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grad", ["logistic", "hinge"])
@pytest.mark.parametrize("d,upd,family,env", [
    (40, "simple", 7, {}),                          # chain_block64, one chain wave
    (700, "simple", 7, {}),                         # chain_block64, two chain waves
    (700, "squared_l2", 7, {}),
    (700, "l1", 8, {}),                             # chain_split
    (700, "adagrad", 8, {}),
    (700, "adam", 8, {}),
    (1100, "simple", 2, {}),                        # chain_general: f64 rows past chain_block64's 1,024
    (40, "adagrad", 1, {}),                         # chain_dense
    (40, "simple", 1, {"PSGD_PER_SAMPLE": "1"}),    # chain_dense with Simple (the per-sample form)
])
def test_dense_ladder_f64(pkg, oracle, monkeypatch, d, upd, family, env, grad):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    es = cached(("dl", d, 64), lambda: ED.dense_ladder(d, np.float64, 800.0))
    check(pkg, oracle, es, grad, upd, "f64", family, reg=0.01 if upd in ("squared_l2", "l1") else 0.0)


@pytest.mark.parametrize("grad", ["logistic", "hinge"])
@pytest.mark.parametrize("family,env", [
    (6, {}),                                        # chain_sparse_lds<double>
    (4, {"PSGD_SPARSE_KERNEL": "hbm64"}),           # chain_sparse64
    (2, {"PSGD_PER_SAMPLE": "1"}),                  # chain_general
])
def test_csr_ladder_f64(pkg, oracle, monkeypatch, family, env, grad):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    es = cached(("cl", 64), lambda: ED.csr_ladder(3000, np.float64, 800.0))
    check(pkg, oracle, es, grad, "simple", "f64", family)


@pytest.mark.parametrize("grad", ["logistic", "hinge"])
@pytest.mark.parametrize("d", [40, 700])
def test_dense_ladder_f64_break(pkg, oracle, d, grad):
    """chain_block64 with the per-sample break (variant 74x): a saturated row moves the weights by
    nothing, so isConverged passes within the first rows of every chain; counts exact."""
    es = cached(("dl", d, 64), lambda: ED.dense_ladder(d, np.float64, 800.0))
    check(pkg, oracle, es, grad, "simple", "f64", 7, tol=1e-3)
    assert (pkg.optimization.get_context(0).last_kernel() // 10) % 10 >= 4


@pytest.mark.parametrize("grad", ["logistic", "hinge"])
@pytest.mark.parametrize("kmin,kmax,d", [(130, 300, 3000), (5, 40, 200000)])
def test_csr_wide_and_past_lds_f64(pkg, oracle, kmin, kmax, d, grad):
    """Rows of 130-300 entries (past chain_sparse_lds's 128) and d = 200,000 (past its LDS range):
    chain_sparse64."""
    es = cached(("cl", d, kmin, 64), lambda: ED.csr_ladder(d, np.float64, 800.0, kmin, kmax))
    check(pkg, oracle, es, grad, "simple", "f64", 4)


@pytest.mark.parametrize("grad", ["logistic", "hinge"])
def test_csr_wide_f32(pkg, oracle, grad):
    es = cached(("cl", 3000, 130, 32), lambda: ED.csr_ladder(3000, np.float32, 120.0, 130, 300))
    check(pkg, oracle, es, grad, "simple", "f32", 4)


@pytest.mark.parametrize("layout", ["dense", "csr"])
def test_multinomial_ladder(pkg, oracle, layout):
    """chain_multinomial: the largest class margin sweeps past 0 (the maxMargin > 0 shift) and 709."""
    es = cached(("mn", layout), lambda: ED.multinomial_ladder(layout))
    check(pkg, oracle, es, "logistic", "simple", "f64", 5)


def test_adam_leaves_its_domain(pkg, oracle):
    """r = 0.001 g^2 > 1 in one coordinate: 1 - r^iter < 0 and the reference's weight there is NaN.
    The NaN mask equals the oracle's and is not empty; the finite coordinates at 1e-9."""
    es = ED.adam_domain()
    wr, hr, cr = oracle.run(es.oracle_matrix(oracle), es.offs, "logistic", "adam", es.step, 1, 0.0, es.w0, tol=0.0)
    w, h, counts, variant = run(pkg, es, "logistic", "adam", 0.0, 1, "f64")
    assert variant // 100 == 1, variant
    assert np.isnan(wr).sum() == 1 and np.isnan(wr[0])
    assert np.array_equal(np.isnan(w), np.isnan(wr))
    fin = ~np.isnan(wr)
    assert np.max(np.abs(w - wr)[fin]) <= F64_REL * np.max(np.abs(wr - es.w0)[fin])
    assert [list(c) for c in counts] == [list(c) for c in cr]
    assert abs(h[0] - hr[0]) <= F64_REL * abs(hr[0])


# LeastSquares as the control, once per family (edge_data.least_squares_control: the ladder's rows
# with labels 0.5 t and the step scaled to them)
@pytest.mark.parametrize("d,upd,family,env", [
    (40, "simple", 7, {}), (700, "l1", 8, {}), (40, "l1", 1, {}), (1100, "simple", 2, {})])
def test_least_squares_control_dense_f64(pkg, oracle, monkeypatch, d, upd, family, env):
    es = cached(("ls", d, 64), lambda: ED.least_squares_control(ED.dense_ladder(d, np.float64, 800.0)))
    check(pkg, oracle, es, "least_squares", upd, "f64", family)


@pytest.mark.parametrize("kmin,kmax,family", [(5, 40, 6), (130, 300, 4)])
def test_least_squares_control_csr_f64(pkg, oracle, kmin, kmax, family):
    es = cached(("ls", "csr", kmin, 64), lambda: ED.least_squares_control(ED.csr_ladder(3000, np.float64, 800.0, kmin, kmax)))
    check(pkg, oracle, es, "least_squares", "simple", "f64", family)


@pytest.mark.parametrize("layout,family", [("dense", 3), ("csr", 6)])
def test_least_squares_control_f32(pkg, oracle, layout, family):
    es = cached(("ls", layout, 32), lambda: ED.least_squares_control(
        ED.dense_ladder(40, np.float32, 120.0) if layout == "dense" else ED.csr_ladder(3000, np.float32, 120.0)))
    check(pkg, oracle, es, "least_squares", "simple", "f32", family)


# ------------------------------------------------------------------------------------------------
# the streaming passes on the ladder: evaluate / predict (score_dense, score_csr) and gradient_sum
# (grad_dense, grad_csr) at w0, where the margins are the ladder itself (to +-800)
# ------------------------------------------------------------------------------------------------
def streaming_truth(es, grad):
    """Per-row dots (longdouble), sum |x_j w_j|, the reference's fp64 multipliers and losses, and
    their longdouble sums."""
    LD = np.longdouble
    w = es.w0.astype(LD)
    n = len(es.y)
    if es.X is not None:
        rows = [(np.arange(es.d), es.X[i].astype(LD)) for i in range(n)]
    else:
        rp, col, val = es.csr
        rows = [(col[rp[i]:rp[i + 1]], val[rp[i]:rp[i + 1]].astype(LD)) for i in range(n)]
    z = np.array([x @ w[idx] for idx, x in rows], LD)
    absum = np.array([float(np.sum(np.abs(x * w[idx]))) for idx, x in rows])
    nnz = np.array([len(idx) for idx, _ in rows])
    # the reference's own fp64 arithmetic per row (MLlib LogisticGradient / HingeGradient) on the
    # correctly rounded dot; only the sums are longdouble
    y, z64 = es.y, np.asarray(z, np.float64)
    if grad == "logistic":
        margin = -z64
        with np.errstate(over="ignore"):
            mult = 1.0 / (1.0 + np.exp(margin)) - y
            l1pe = np.where(margin > 0, margin + np.log1p(np.exp(-np.abs(margin))), np.log1p(np.exp(-np.abs(margin))))
        loss = np.where(y > 0, l1pe, l1pe - margin)
    else:
        ls = 2 * y - 1
        on = 1.0 > ls * z64
        mult, loss = np.where(on, -ls, 0.0), np.where(on, 1.0 - ls * z64, 0.0)
    mult, loss = mult.astype(LD), loss.astype(LD)
    Gs, A = np.zeros(es.d, LD), np.zeros(es.d, LD)
    for (idx, x), m in zip(rows, mult):
        Gs[idx] += m * x
        A[idx] += np.abs(m * x)
    return z, absum, nnz, mult, loss, np.asarray(Gs, np.float64), np.asarray(A, np.float64)


@pytest.mark.parametrize("grad", ["logistic", "hinge"])
@pytest.mark.parametrize("layout", ["dense", "csr"])
def test_streaming_passes_on_the_ladder(pkg, layout, grad):
    es = cached(("dl", 40, 64), lambda: ED.dense_ladder(40, np.float64, 800.0)) if layout == "dense" else \
        cached(("cl", 64), lambda: ED.csr_ladder(3000, np.float64, 800.0))
    z, absum, nnz, mult, loss, Gs, A = streaming_truth(es, grad)
    zb = nnz * 2.0 ** -52 * absum                      # the existing margin bound (test_gpu_evaluate.py)
    z64 = np.asarray(z, np.float64)
    if grad == "hinge":                                 # no row within the dots' error of the hinge
        assert np.all(np.abs(1 - (2 * es.y - 1) * z64) > 4 * zb)
    eng = pkg.HipEngine(es.partitions(pkg))
    g = getattr(pkg, G[grad])()
    got = eng.evaluate(g, es.w0)
    total = float(np.sum(loss))
    assert got.count == len(es.y)
    assert abs(got.lossSum - total) <= 1e-9 * abs(total), (got.lossSum, total)
    # accuracy: exact but for the rows whose dot is within its error of 0 (the ladder's t = 0 rows)
    sure = np.abs(z64) > zb
    right = ((z64 > 0).astype(np.float64) == es.y)
    assert np.sum(right & sure) <= got.nCorrect <= np.sum(right & sure) + np.sum(~sure)
    assert np.sum(~sure) <= 4
    for p, (a, b) in enumerate(zip(es.offs[:-1], es.offs[1:])):
        m = eng.predict(p, es.w0).cpu().numpy()
        assert m.shape == (b - a,) and np.all(np.abs(m - z64[a:b]) <= zb[a:b])
    gs = eng.gradient_sum(g, es.w0).cpu().numpy()
    assert gs.shape == (es.d + 2,) and gs[es.d + 1] == len(es.y)
    err = np.abs(gs[:es.d] - Gs)
    print(f"{es.name} {grad}: lossSum rel {abs(got.lossSum - total) / abs(total):.3g}, gradient worst |G - ref| / A "
          f"{float(np.max(err / np.where(A > 0, A, 1.0))):.3g}, loss rel {abs(gs[es.d] - total) / abs(total):.3g}")
    assert np.all(err <= 1e-9 * A)
    assert abs(gs[es.d] - total) <= 1e-9 * abs(total)


# ------------------------------------------------------------------------------------------------
# fp32 compute
# ------------------------------------------------------------------------------------------------
# (L1 at regParam 0 is Simple's arithmetic through the per-sample kernels: chain_dense at one row
# vector, chain_split from two on; the sets' run_f32 condition is checked with Simple)
DENSE32 = [(40, "simple", 3), (700, "simple", 3), (40, "l1", 1), (700, "l1", 8)]
CSR32 = {"lds": ({"PSGD_SPARSE_KERNEL": "lds"}, 6), "lds_tail": ({"PSGD_SPARSE_KERNEL": "lds", "PSGD_SPARSE_LDS_HEAD": "1000"}, 6),
         "spec": ({"PSGD_SPARSE_KERNEL": "spec"}, 4), "plain": ({"PSGD_SPARSE_KERNEL": "plain"}, 4)}


@pytest.mark.parametrize("grad", ["logistic", "hinge"])
@pytest.mark.parametrize("d,upd,family", DENSE32)
def test_dense_ladder_f32(pkg, oracle, d, upd, family, grad):
    es = cached(("dl", d, 32), lambda: ED.dense_ladder(d, np.float32, 120.0))
    check(pkg, oracle, es, grad, upd, "f32", family)


@pytest.mark.parametrize("grad", ["logistic", "hinge"])
@pytest.mark.parametrize("kernel", sorted(CSR32))
def test_csr_ladder_f32(pkg, oracle, monkeypatch, kernel, grad):
    env, family = CSR32[kernel]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    es = cached(("cl", 32), lambda: ED.csr_ladder(3000, np.float32, 120.0))
    check(pkg, oracle, es, grad, "simple", "f32", family)


@pytest.mark.parametrize("band", ED.SEPARABLE_BANDS)
@pytest.mark.parametrize("upd,family", [("simple", 3), ("l1", 1)])
def test_separable_dense_f32(pkg, oracle, band, upd, family):
    """Loss histories of ~2e-3, 1.5e-6 and 2e-10 at the fp32 mode's 1e-4 relative. (The Simple
    cases run chain_block, which takes Logistic's loss in f64 from the stored margins
    (margin_loss_kernel): they passed before the loss fix too, and no chain kernel calls
    row_loss<G_LOGISTIC> on a Logistic run -- only the probe tests that specialisation. The L1
    cases run chain_dense, whose gradient_scalar<float> loss was wrong.)"""
    es = cached(("sep", band, "dense"), lambda: ED.separable(band, "dense"))
    check(pkg, oracle, es, "logistic", upd, "f32", family)


@pytest.mark.parametrize("band", ED.SEPARABLE_BANDS)
@pytest.mark.parametrize("kernel", sorted(CSR32))
def test_separable_csr_f32(pkg, oracle, monkeypatch, band, kernel):
    env, family = CSR32[kernel]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    es = cached(("sep", band, "csr"), lambda: ED.separable(band, "csr"))
    check(pkg, oracle, es, "logistic", "simple", "f32", family)


# ------------------------------------------------------------------------------------------------
# exact ties
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("compute,ulp_exp,env,family", [
    ("f64", -52, {}, 7), ("f64", -52, {"PSGD_PER_SAMPLE": "1"}, 1), ("f64", -23, {}, 7), ("f32", -23, {}, 3)])
def test_hinge_exact_ties(pkg, oracle, monkeypatch, compute, ulp_exp, env, family):
    """ls * z is exactly 1 - ulp/2, 1 or 1 + ulp: Hinge is on (1.0 > ls * z) only for the first.
    The loss sum and the set of updated coordinates are known in closed form."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    dtype = np.float32 if compute == "f32" else np.float64
    es, on, loss_sum = ED.exact_ties(ulp_exp, dtype=dtype)
    n = len(es.y)
    wr, hr, cr = oracle.run(es.oracle_matrix(oracle), es.offs, "hinge", "simple", ED.STEP, 1, 0.0, es.w0, tol=0.0)
    w, h, counts, variant = run(pkg, es, "hinge", "simple", 0.0, 1, compute)
    assert variant // 100 == family, variant
    assert [list(c) for c in counts] == [list(c) for c in cr]
    assert h[0] == loss_sum / n == hr[0], (h, hr, loss_sum / n)
    # an updated coordinate moved by step / P; the others not at all
    assert np.array_equal(np.abs(w - es.w0) > 1e-3, on)
    assert np.max(np.abs(w - wr)) <= (F64_REL if compute == "f64" else FP32_REL) * np.max(np.abs(wr - es.w0))


@pytest.mark.parametrize("compute,family", [("f64", 7), ("f32", 3)])
def test_logistic_zero_margin(pkg, oracle, compute, family):
    """z exactly 0 in every row: multiplier 1/2 - y, loss ln 2."""
    dtype = np.float32 if compute == "f32" else np.float64
    es, _, _ = ED.exact_ties(-23, dtype=dtype)
    es.w0 = np.zeros_like(es.w0)
    es.name += "_zero"
    wr, hr, cr = oracle.run(es.oracle_matrix(oracle), es.offs, "logistic", "simple", ED.STEP, 1, 0.0, es.w0, tol=0.0)
    w, h, counts, variant = run(pkg, es, "logistic", "simple", 0.0, 1, compute)
    assert variant // 100 == family, variant
    assert abs(hr[0] - np.log(2.0)) < 1e-15
    rel = F64_REL if compute == "f64" else FP32_LOSS_REL
    assert abs(h[0] - hr[0]) <= rel * hr[0]
    assert np.max(np.abs(w - wr)) <= (F64_REL if compute == "f64" else FP32_REL) * np.max(np.abs(wr))
