"""The conditions on the data sets of tests/edge_data.py (CPU; the fp64 oracle and its
single-precision restatement run_f32). They keep the GPU bars of test_gpu_saturation.py honest:

* well conditioned: the oracle run from w0 and from w0 (1 + 1e-13) ends within
  1e-11 max|w - w0| of each other, so a kernel's 1e-9 (of the update) cannot be rounding noise
  amplified by the data;
* fp32-representable: all three orders of run_f32 (left-fold dots, strided partials + tree, only
  the weights in float) stay within half the fp32 bars -- 1e-4 max|w| on the weights, 5e-5
  relative on the loss history -- so an fp32 kernel that misses the full bar is wrong, not unlucky;
* every |margin| regime (< 1, 1-20, 20-88, 88-709, > 709 in fp64) is populated in every partition.
A set that fails a condition is changed, not exempted.
"""
import numpy as np
import pytest

import edge_data as ED

ITERS = 3


def conditioning(oracle, es, grad, upd="simple", reg=0.0, scale="update"):
    mat = es.oracle_matrix(oracle)
    kw = {"num_classes": es.num_classes} if hasattr(es, "num_classes") else {}
    w, h, _ = oracle.run(mat, es.offs, grad, upd, es.step, ITERS, reg, es.w0, tol=0.0, **kw)
    w2, h2, _ = oracle.run(mat, es.offs, grad, upd, es.step, ITERS, reg, es.w0 * (1 + 1e-13), tol=0.0, **kw)
    assert np.all(np.isfinite(w)) and np.all(np.isfinite(h))
    # fp64 bars are taken on the update max|w - w0|; the separable sets (fp32 only: their rows
    # barely move the weights) on max|w|, as the fp32 weight bar is
    den = np.max(np.abs(w - es.w0)) if scale == "update" else np.max(np.abs(w))
    return float(np.max(np.abs(w - w2)) / den), w, h


def f32_distance(oracle, es, grad, w, h, upd="simple", reg=0.0):
    mat = es.oracle_matrix(oracle, dense=True)
    worst_w = worst_h = 0.0
    for order in (0, 1, 2):
        wf, hf, _ = oracle.run_f32(mat, es.offs, grad, upd, es.step, ITERS, reg, es.w0, order=order, tol=0.0)
        worst_w = max(worst_w, float(np.max(np.abs(wf - w)) / np.max(np.abs(w))))
        worst_h = max(worst_h, float(np.max(np.abs(hf - h) / np.maximum(np.abs(h), 1e-30))))
    return worst_w, worst_h


# (layout, d, updater, regParam): every combination test_gpu_saturation.py runs in fp64
LADDERS64 = [("dense", 40, "simple", 0.0), ("dense", 700, "simple", 0.0), ("dense", 700, "squared_l2", 0.01),
             ("dense", 700, "l1", 0.01), ("dense", 700, "adagrad", 0.0), ("dense", 40, "adagrad", 0.0),
             ("csr", 3000, "simple", 0.0), ("dense", 700, "adam", 0.0), ("dense", 1100, "simple", 0.0),
             ("csr_wide", 3000, "simple", 0.0), ("csr", 200000, "simple", 0.0)]
LADDERS32 = [("dense", 40), ("dense", 700), ("csr", 3000), ("csr_wide", 3000)]


def make_ladder(layout, d, dtype, T):
    if layout == "dense":
        return ED.dense_ladder(d, dtype, T)
    return ED.csr_ladder(d, dtype, T, 130, 300) if layout == "csr_wide" else ED.csr_ladder(d, dtype, T)


# the LeastSquares controls of test_gpu_saturation.py: (layout, d, updater, fp32 too)
# (AdaGrad normalises the step away: at the scaled step its update is ~1e-6 of w0 and the condition
# fails at 3e-9, so chain_split and chain_dense take the control through L1 at regParam 0)
LS_CONTROLS = [("dense", 40, "simple", True), ("dense", 700, "l1", False), ("dense", 40, "l1", False),
               ("dense", 1100, "simple", False), ("csr", 3000, "simple", True), ("csr_wide", 3000, "simple", False)]


@pytest.mark.parametrize("layout,d,upd,f32", LS_CONTROLS)
def test_least_squares_control(oracle, layout, d, upd, f32):
    es = ED.least_squares_control(make_ladder(layout, d, np.float64, 800.0))
    c, _, h = conditioning(oracle, es, "least_squares", upd)
    print(f"{es.name} {upd}: step {es.step:.3g}, conditioning {c:.3g}, loss history {h}")
    assert c < 1e-11 and h[-1] < h[0]
    if f32:
        es = ED.least_squares_control(make_ladder(layout, d, np.float32, 120.0))
        c, w, h = conditioning(oracle, es, "least_squares", upd)
        ew, eh = f32_distance(oracle, es, "least_squares", w, h)
        print(f"{es.name}: conditioning {c:.3g}, run_f32 weights {ew:.3g} x max|w|, loss {eh:.3g} relative")
        assert c < 1e-11 and ew <= 1e-4 and eh <= 5e-5


@pytest.mark.parametrize("grad", ["logistic", "hinge"])
@pytest.mark.parametrize("d", [40, 700])
def test_ladder_break_margins(oracle, d, grad):
    """At tol = 1e-3 (chain_block64 with the break) every isConverged decision of the oracle sits
    further from flipping than the kernels' norm error: CheckedOracle.run asserts it."""
    es = ED.dense_ladder(d, np.float64, 800.0)
    w, h, counts = oracle.run(es.oracle_matrix(oracle), es.offs, grad, "simple", es.step, ITERS, 0.0, es.w0, tol=1e-3)
    print(f"{es.name} {grad} tol 1e-3: counts {counts.tolist()}, smallest break margin {oracle.last_margin:.3g}")
    assert counts.sum() > 0


@pytest.mark.parametrize("layout", ["dense", "csr"])
def test_multinomial_ladder(oracle, layout):
    es = ED.multinomial_ladder(layout)
    t = es.first_margins() if False else es.t
    assert np.max(np.abs(t)) > 709 and np.min(np.abs(t)) == 0
    assert set(np.unique(es.y)) == {0.0, 1.0, 2.0, 3.0}
    c, _, h = conditioning(oracle, es, "logistic")
    print(f"{es.name}: conditioning {c:.3g}, loss history {h}")
    assert c < 1e-11


def test_adam_domain(oracle):
    es = ED.adam_domain()
    assert abs(es.X[23] @ es.w0 + 8.0) < 1e-12 and np.all(es.X[np.arange(48) != 23, 0] == 0)
    mat = es.oracle_matrix(oracle)
    w, h, _ = oracle.run(mat, es.offs, "logistic", "adam", es.step, 1, 0.0, es.w0, tol=0.0)
    w2, _, _ = oracle.run(mat, es.offs, "logistic", "adam", es.step, 1, 0.0, es.w0 * (1 + 1e-13), tol=0.0)
    assert np.isnan(w).tolist() == [True] + [False] * 39 and np.array_equal(np.isnan(w), np.isnan(w2))
    c = np.max(np.abs(w - w2)[1:]) / np.max(np.abs(w - es.w0)[1:])
    print(f"adam_domain: conditioning of the finite coordinates {c:.3g}, loss {h}")
    assert c < 1e-11


@pytest.mark.parametrize("grad", ["logistic", "hinge"])
@pytest.mark.parametrize("layout,d,upd,reg", LADDERS64)
def test_ladder_f64(oracle, layout, d, upd, reg, grad):
    es = make_ladder(layout, d, np.float64, 800.0)
    t = es.first_margins()
    assert np.max(np.abs(t - es.t)) <= 1e-9 * 800
    pop = ED.regimes_populated(t, es.offs, np.inf)
    assert len(pop) == 2 and all(len(p) == 5 and min(p) >= 2 for p in pop), pop   # both signs past 709
    c, _, h = conditioning(oracle, es, grad, upd, reg)
    print(f"{es.name} {grad} {upd}: conditioning {c:.3g}, loss history {h}")
    assert c < 1e-11


@pytest.mark.parametrize("grad", ["logistic", "hinge"])
@pytest.mark.parametrize("layout,d", LADDERS32)
def test_ladder_f32(oracle, layout, d, grad):
    es = make_ladder(layout, d, np.float32, 120.0)
    t = es.first_margins()
    assert np.max(np.abs(t - es.t)) <= 1e-6 * 120
    pop = ED.regimes_populated(t, es.offs, 120.0)
    assert len(pop) == 2 and all(len(p) == 4 and min(p) >= 5 for p in pop), pop
    c, w, h = conditioning(oracle, es, grad)
    ew, eh = f32_distance(oracle, es, grad, w, h)
    print(f"{es.name} {grad}: conditioning {c:.3g}, run_f32 weights {ew:.3g} x max|w|, loss {eh:.3g} relative, loss history {h}")
    assert c < 1e-11
    assert ew <= 1e-4 and eh <= 5e-5


@pytest.mark.parametrize("band", ED.SEPARABLE_BANDS)
@pytest.mark.parametrize("layout", ["dense", "csr"])
def test_separable(oracle, layout, band):
    es = ED.separable(band, layout)
    t = es.first_margins()
    assert np.all(np.abs(t) >= band[0] * (1 - 1e-5)) and np.all(np.abs(t) <= band[1] * (1 + 1e-5))
    assert np.array_equal(es.y, (t > 0).astype(np.float64))
    c, w, h = conditioning(oracle, es, "logistic", scale="weights")
    ew, eh = f32_distance(oracle, es, "logistic", w, h)
    print(f"{es.name}: conditioning {c:.3g}, run_f32 weights {ew:.3g} x max|w|, loss {eh:.3g} relative, loss history {h}")
    assert c < 1e-11
    assert ew <= 1e-4 and eh <= 5e-5


@pytest.mark.parametrize("ulp_exp", [-52, -23])
def test_exact_ties(oracle, ulp_exp):
    es, on, loss_sum = ED.exact_ties(ulp_exp)
    n = len(es.y)
    ls = 2 * es.y - 1
    z = es.X.astype(np.float64) @ es.w0
    assert np.array_equal(ls * z, es.w0)                       # exactly 1 or 1 -+ ulp
    G = es.X.astype(np.float64) @ es.X.astype(np.float64).T
    assert np.array_equal(G, np.eye(n))
    assert on.sum() == np.sum(es.w0 < 1) and 0 < on.sum() < n
    w, h, counts = oracle.run(es.oracle_matrix(oracle), es.offs, "hinge", "simple", ED.STEP, 1, 0.0, es.w0, tol=0.0)
    assert h[0] == loss_sum / n
    assert np.array_equal(w != es.w0, on)
