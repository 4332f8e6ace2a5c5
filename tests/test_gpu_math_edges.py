"""The per-sample scalar functions of psgd_device.h at the ends of their ranges, through the
device probe (psgd_mathprobe.hip: the functions the chain kernels call) against longdouble truths
(tests/math_truth.py, themselves checked against mpmath on the CPU).

The other GPU tests feed these functions the margins N(0,1) rows produce: a few units around 0.
Here: every binade, the clamps of recip_one_plus_exp, the overflow / underflow edges of exp, the
half-way points of its range reduction, saturated fp32 margins, non-finite values.

The bars are the claims in the functions' comments, at 4x (the claims are maxima over sampled,
narrower sets; a Newton step squares the estimate's error, so 4x lets the hardware estimate be 2x
worse somewhere in the wider range and no more):
  recip_newton 2.2e-15, rsqrt_newton / sqrt_newton 4.3e-15, recip_one_plus_exp 1e-14 relative;
  fp32 multipliers 2^-21 absolute (three <= 1-ulp hardware operations on a value <= 1, 8x room);
  fp32 row losses 1e-7 max(1, loss) (the claim read "1e-7 absolute": an fp32 loss of 100 has an
  ulp of 7.6e-6, so above 1 the claim can only be relative), and, relative to a small loss,
  softplus_fast's own bound 2^-24 (1.5 |t| + 24);
  one_minus_pow_iter: the bits of the device's own 1.0 - pow(r, iter) at every point (and that
  pow within the 16 ulp the device library is built to).
Measured worst errors go to the JSON file PSGD_MATH_EDGES_OUT names (profiles/math_edges.json is
one such recording).
"""
import ctypes
import json
import os

import numpy as np
import pytest

import math_truth as MT
from conftest import has_gpu

pytestmark = pytest.mark.gpu

LD = np.longdouble
OP = {"recip_one_plus_exp": 0, "recip_newton": 1, "rsqrt_newton": 2, "sqrt_newton": 3, "one_minus_pow_iter": 4,
      "log1p_exp64": 5, "one_minus_pow64": 6, "coef64": 10, "gradient64": 20, "coef32": 30, "row_loss32": 40, "sparse_coef": 50,
      "split_sigmoid": 60, "gradient32": 70, "pow_fast": 80}
LOGISTIC, LEAST_SQUARES, HINGE = 0, 1, 2
RECORD = {}


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not has_gpu():
        pytest.skip("no GPU")
    yield
    out = os.environ.get("PSGD_MATH_EDGES_OUT")
    if out and RECORD:
        with open(out, "w") as f:
            json.dump(RECORD, f, indent=1, sort_keys=True)


@pytest.fixture(scope="module")
def probe(pkg):
    import torch
    lib = ctypes.CDLL(pkg._native.LIB_PATH)
    fn = lib._ZN4psgd10math_probeEilPKvS1_PvS2_P12ihipStream_t
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_int, ctypes.c_int64] + [ctypes.c_void_p] * 5

    def run(op, a, b=None):
        dt = np.float64 if op < OP["coef32"] else np.float32
        a = np.ascontiguousarray(a, dt)
        b = np.zeros_like(a) if b is None else np.ascontiguousarray(np.broadcast_to(np.asarray(b, dt), a.shape))
        dev = torch.device("cuda", 0)
        ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
        o0, o1 = torch.empty_like(ta), torch.empty_like(ta)
        torch.cuda.synchronize()
        rc = fn(op, a.size, ta.data_ptr(), tb.data_ptr(), o0.data_ptr(), o1.data_ptr(), None)
        assert rc == 0, f"math_probe({op}) returned {rc}"
        torch.cuda.synchronize()
        return o0.cpu().numpy(), o1.cpu().numpy()
    return run


def record(name, err, x, bar, note=None):
    """err: error in units of the bar's quantity (array); keeps the worst and its input."""
    err = np.asarray(err, np.float64)
    i = int(np.nanargmax(err)) if err.size else 0
    RECORD[name] = {"worst": float(err[i]) if err.size else 0.0, "input": repr(np.asarray(x)[i].tolist()),
                    "bar": bar, "points": int(err.size)}
    if note:
        RECORD[name]["note"] = note
    print(f"{name}: worst {RECORD[name]['worst']:.3g} at {RECORD[name]['input']} ({err.size} points; {bar})")
    return RECORD[name]["worst"]


def rel_err(got, truth):
    truth = np.asarray(truth, LD)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.asarray(np.abs(np.asarray(got, LD) - truth) / np.abs(truth), np.float64)


TINY64 = np.ldexp(1.0, -1022)


# ------------------------------------------------------------------------------------------------
# fp64
# ------------------------------------------------------------------------------------------------
def test_recip_one_plus_exp(probe):
    m = MT.margin_inputs(np.float64)
    assert m.size >= 200000
    out, _ = probe(OP["recip_one_plus_exp"], m)
    truth = MT.sigmoid_neg(m)
    inside = (m >= -746.0) & (m <= 709.0)
    # 1e-14 relative at 4x; a result below the normal range (m > 708.4) is a multiple of 2^-1074
    # (below the normal range, m > 708.4, a relative bar means nothing: the multiplier's callers
    # need the absolute error far below a weight's ulp, as for recip_newton's quotients there)
    err = np.abs(out.astype(LD) - truth)
    bar = np.where(truth >= TINY64, 4e-14 * truth, LD(TINY64))
    ratio = np.asarray(err / bar, np.float64)
    sub = inside & (truth < TINY64)
    record("recip_one_plus_exp_subnormal_result", np.asarray(err, np.float64)[sub] / TINY64, m[sub],
           "absolute / 2^-1022, bar 1")
    worst = record("recip_one_plus_exp", rel_err(out, truth)[inside & (truth >= TINY64)],
                   m[inside & (truth >= TINY64)], "relative, claim 1e-14, bar 4e-14")
    assert worst <= 4e-14
    assert np.all(ratio[inside] <= 1.0), m[inside][np.argmax(ratio[inside])]
    # the clamps: 1.0 exactly below -746, the value at 709 (~1.2e-308, not 0) above 709
    assert np.all(out[m < -746.0] == 1.0)
    at709 = probe(OP["recip_one_plus_exp"], np.array([709.0]))[0][0]
    assert 0.0 < at709 < 1.3e-308
    assert np.all(out[m > 709.0] == at709)
    nf, _ = probe(OP["recip_one_plus_exp"], np.array(MT.NONFINITE))
    assert nf[0] == at709 and nf[1] == 1.0 and np.isnan(nf[2])
    # monotone over the dense range (a wrong rint / ldexp step shows as a jump)
    ms = np.sort(m[inside])
    os_, _ = probe(OP["recip_one_plus_exp"], ms)
    ts = MT.sigmoid_neg(ms)
    assert np.all(np.diff(os_) <= 8e-14 * np.asarray(ts[:-1], np.float64))


def newton_inputs():
    x = MT.normal_binades(np.float64, -1022, 1023, per=48)
    return np.concatenate([x, -x])


def test_recip_newton(probe):
    x = newton_inputs()
    assert x.size >= 200000
    out, _ = probe(OP["recip_newton"], x)
    truth = 1 / x.astype(LD)
    normal = np.abs(truth) >= TINY64
    worst = record("recip_newton", rel_err(out, truth)[normal], x[normal], "relative, claim 2.2e-15, bar 8.8e-15")
    assert worst <= 8.8e-15
    # |x| > 2^1022: the quotient is below the normal range. recip_one_plus_exp feeds it
    # 1 + 2^1023 e^r at the top of its clamp and uses the result as a multiplier next to 1: it
    # needs the absolute error far below any weight's ulp, which a flush to zero still gives.
    sub = ~normal
    aerr = np.asarray(np.abs(out.astype(LD) - truth), np.float64)[sub]
    record("recip_newton_subnormal_result", aerr / TINY64, x[sub], "absolute / 2^-1022, bar 1",
           note="flushed" if np.all(out[sub] == 0) else "denormal results kept")
    assert np.all(aerr <= TINY64)
    # measured: the quotients are kept as denormals, not flushed. Three operations (the estimate,
    # the two fmas) each round to a multiple of 2^-1074 there: within 4 of them
    assert np.all(aerr <= 4 * 2.0 ** -1074) and np.all(out[sub] != 0)
    assert np.isnan(probe(OP["recip_newton"], np.array([np.nan]))[0][0])
    # the documented range of newton_check, [1, 1e6): the claim itself
    lo = (np.abs(x) >= 1) & (np.abs(x) < 1e6)
    assert np.max(rel_err(out, truth)[lo]) <= 8.8e-15


def test_rsqrt_newton(probe):
    x = np.concatenate([MT.normal_binades(np.float64, 0, 1023, per=200), [1.0, np.finfo(np.float64).max]])
    assert x.size >= 200000
    out, _ = probe(OP["rsqrt_newton"], x)
    truth = 1 / np.sqrt(x.astype(LD))
    worst = record("rsqrt_newton", rel_err(out, truth), x, "relative, claim 4.3e-15, bar 1.72e-14")
    assert worst <= 1.72e-14
    sp, _ = probe(OP["rsqrt_newton"], np.array([1.0, np.inf, np.nan]))
    assert abs(sp[0] - 1.0) <= 1.72e-14 and sp[1] == 0.0 and np.isnan(sp[2])


def test_sqrt_newton(probe):
    x = MT.normal_binades(np.float64, -1022, 1023, per=100)
    assert x.size >= 200000
    out, _ = probe(OP["sqrt_newton"], x)
    truth = np.sqrt(x.astype(LD))
    worst = record("sqrt_newton", rel_err(out, truth), x, "relative, claim 4.3e-15, bar 1.72e-14")
    assert worst <= 1.72e-14
    sp, _ = probe(OP["sqrt_newton"], np.array([0.0, 1.0, np.inf, np.nan, -1.0, -1e-300, -np.inf, 4.0]))
    assert sp[0] == 0.0 and abs(sp[1] - 1.0) <= 1.72e-14 and sp[2] == np.inf
    assert np.all(np.isnan(sp[3:7])) and abs(sp[7] - 2.0) <= 4e-14


def test_one_minus_pow_iter(probe):
    rng = np.random.default_rng(11)
    rs = np.concatenate([[0.0, 1e-40, 1e-30, 1e-20, 1e-10, 1e-5, 1e-3, 0.1, 0.5, 0.9, 0.99, 0.999, 1 - 2.0 ** -20,
                          1 - 2.0 ** -24, 1 - 2.0 ** -25, 1 - 2.0 ** -40, 1 - 2.0 ** -53, 1.0, 1 + 2.0 ** -52, 1.001, 2.0,
                          np.inf, np.nan], rng.uniform(0, 1, 400), 1 - np.ldexp(rng.uniform(1, 2, 400), -rng.integers(1, 53, 400))])
    its = np.array([1, 2, 3, 10, 59, 60, 61, 62, 100, 1e3, 1e6])
    R, I = [a.ravel() for a in np.meshgrid(rs, its)]
    # iter * log2(r) within +-1e-4 of -60 (the fp32 log2 decides there), and of -54 (where the
    # rounding of 1 - p itself flips), for iter from 1 to 1e6
    it2 = np.round(np.exp(rng.uniform(0, np.log(1e6), 100000)))
    for centre in (-60.0, -54.0):
        l2 = (centre + rng.uniform(-1e-4, 1e-4, it2.size)) / it2
        R = np.concatenate([R, np.exp2(l2)])
        I = np.concatenate([I, it2])
    # and the iterations around the boundary for fixed r: iter = ceil(-60 / log2 r) +- 2
    rb = np.concatenate([rng.uniform(1e-3, 0.999, 2000), 1 - np.ldexp(1.0, -rng.integers(3, 24, 2000))])
    for dk in (-2, -1, 0, 1, 2):
        R = np.concatenate([R, rb])
        I = np.concatenate([I, np.maximum(np.ceil(-60.0 / np.log2(rb)) + dk, 1)])
    assert R.size >= 200000
    out, _ = probe(OP["one_minus_pow_iter"], R, I)
    p = MT.pow_ld(R, I)
    truth = 1 - p
    fin = np.isfinite(np.asarray(p, np.float64)) & ~np.isnan(R)
    # where 1.0 - pow(r, iter) is 1.0 in IEEE double for any pow within 16 ulp: exactly 1.0
    one = fin & (p <= LD(2.0) ** -54 * (1 - LD(1e-14)))
    assert np.all(out[one] == 1.0), (R[one][out[one] != 1.0][:4], I[one][out[one] != 1.0][:4])
    # a result of exactly 1.0 is right only there (or where p is 0): the shortcut never fires early
    assert np.all(np.asarray(p, np.float64)[fin & (out == 1.0)] <= 2.0 ** -54 * (1 + 1e-14))
    # everywhere: the bits of the device's own 1.0 - pow(r, iter) (the comment's claim; NaN for NaN)
    dev, _ = probe(OP["one_minus_pow64"], R, I)
    same = (out.view(np.int64) == dev.view(np.int64)) | (np.isnan(out) & np.isnan(dev))
    took_pow = int(np.sum(fin & (out != 1.0)))
    record("one_minus_pow_iter", (~same).astype(np.float64), np.stack([R, I], 1),
           "points whose bits differ from the device's 1.0 - pow(r, iter), bar 0", note=f"{took_pow} points off the shortcut")
    assert np.all(same), (R[~same][:4], I[~same][:4], out[~same][:4], dev[~same][:4])
    assert took_pow >= 20000
    # and that device pow against the truth: 16 ulp of p (the OpenCL bound) and the subtraction's rounding
    with np.errstate(invalid="ignore", over="ignore"):
        err = np.asarray(np.abs(dev.astype(LD) - truth), np.float64)
        bar = np.asarray(16 * 2.0 ** -52 * np.abs(p) + 2.0 ** -53 * np.abs(truth), np.float64)
    chk = fin & np.isfinite(bar)
    record("one_minus_pow64_device_pow", err[chk] / bar[chk], np.stack([R, I], 1)[chk], "error / (16 ulp of pow + 1/2 ulp), bar 1")
    assert np.all(err[chk] <= bar[chk])
    # the boundary points took both sides of the shortcut and agree bit for bit with the direct form
    with np.errstate(invalid="ignore", over="ignore"):
        direct = 1.0 - np.power(R, I)
    near = fin & (np.abs(I * np.log2(np.where(R > 0, R, 1.0)) + 60.0) < 1e-3)
    assert near.sum() >= 90000 and np.all(out[near] == direct[near]) and np.all(direct[near] == 1.0)
    # non-finite and out-of-domain arguments: as pow
    sp, _ = probe(OP["one_minus_pow_iter"], np.array([np.inf, np.nan, 2.0, 1.0, 0.0]), np.array([3.0, 3.0, 2000.0, 7.0, 5.0]))
    assert sp[0] == -np.inf and np.isnan(sp[1]) and sp[2] == -np.inf and sp[3] == 0.0 and sp[4] == 1.0


@pytest.mark.parametrize("y", [0.0, 1.0])
def test_logistic_f64_multiplier_and_loss(probe, y):
    z = MT.margin_inputs(np.float64)
    tm = MT.logistic_mult(z, y)
    sig = MT.sigmoid_neg(-z)
    # coef64 (recip_one_plus_exp): 4e-14 of the sigmoid, then the subtraction of y rounds once
    c, _ = probe(OP["coef64"] + LOGISTIC, z, y)
    # (past its clamp at 709 recip_one_plus_exp returns ~1.2e-308 where the sigmoid is smaller
    # still: an absolute 2^-1022, as for its results below the normal range)
    bar = 4e-14 * sig + LD(2.0) ** -53 * np.abs(tm) + LD(TINY64)
    e = np.asarray(np.abs(c.astype(LD) - tm) / bar, np.float64)
    record(f"coef64_logistic_y{int(y)}", e, z, "error / (4e-14 sigmoid + 1/2 ulp), bar 1")
    assert np.all(e <= 1.0)
    # gradient_scalar<double>: the library exp (<= 3 ulp) and an IEEE division
    g, l = probe(OP["gradient64"] + LOGISTIC, z, y)
    # (past exp's overflow at 709.78 the reference's own 1 / (1 + inf) is 0 where the sigmoid is
    # ~5e-309: absolute below the normal range, as above)
    barg = 4 * 2.0 ** -52 * sig + LD(2.0) ** -53 * np.abs(tm) + LD(TINY64)
    eg = np.asarray(np.abs(g.astype(LD) - tm) / barg, np.float64)
    record(f"gradient64_logistic_mult_y{int(y)}", eg, z, "error / (4 ulp sigmoid + 1/2 ulp), bar 1")
    assert np.all(eg <= 1.0)
    # the loss in the reference's form (label 0: log1pExp(m) - m, which cancels at ulp(|m|))
    tl = MT.logistic_loss(z, y)
    barl = 8 * 2.0 ** -52 * np.maximum(np.maximum(np.abs(z), 1.0), np.asarray(tl, np.float64)) if y == 0.0 \
        else 8 * 2.0 ** -52 * tl + LD(2.0) ** -1072
    el = np.asarray(np.abs(l.astype(LD) - tl) / barl, np.float64)
    record(f"gradient64_logistic_loss_y{int(y)}", el, z, "error / 8 ulp of max(|m|, 1, loss) (y=0) or of the loss (y=1), bar 1")
    assert np.all(el <= 1.0)
    nf, nl = probe(OP["gradient64"] + LOGISTIC, np.array(MT.NONFINITE), y)
    assert nf[0] == 1.0 - y and nf[1] == 0.0 - y and np.isnan(nf[2]) and np.isnan(nl[2])
    nc, _ = probe(OP["coef64"] + LOGISTIC, np.array(MT.NONFINITE), y)
    assert nc[0] == 1.0 - y and abs(nc[1] - (0.0 - y)) <= 1.3e-308 and np.isnan(nc[2])


def test_log1p_exp_f64(probe):
    x = MT.margin_inputs(np.float64)
    out, _ = probe(OP["log1p_exp64"], x)
    t = MT.softplus(x)
    e = np.asarray(np.abs(out.astype(LD) - t) / (8 * 2.0 ** -52 * t + LD(2.0) ** -1072), np.float64)
    record("log1p_exp64", e, x, "error / 8 ulp (exp <= 3 ulp, log1p <= 2 ulp, the sum), bar 1")
    assert np.all(e <= 1.0)


def test_least_squares_and_hinge_f64_exact(probe):
    """LeastSquares and Hinge are plain arithmetic: bit for bit, ties at lz = 1 -+ ulp included."""
    rng = np.random.default_rng(3)
    z = np.concatenate([rng.standard_normal(5000) * 10, [1.0, np.nextafter(1.0, 0), np.nextafter(1.0, 2), -1.0,
                        np.nextafter(-1.0, 0), np.nextafter(-1.0, -2), 0.0]])
    for y in (0.0, 1.0):
        c, _ = probe(OP["coef64"] + HINGE, z, y)
        g, l = probe(OP["gradient64"] + HINGE, z, y)
        ls = 2 * y - 1
        on = 1.0 > ls * z
        assert np.array_equal(c, np.where(on, -ls, 0.0)) and np.array_equal(g, np.where(on, -ls, 0.0))
        assert np.array_equal(l, np.where(on, 1.0 - ls * z, 0.0))
    yv = rng.standard_normal(z.size)
    c, _ = probe(OP["coef64"] + LEAST_SQUARES, z, yv)
    g, l = probe(OP["gradient64"] + LEAST_SQUARES, z, yv)
    assert np.array_equal(c, z - yv) and np.array_equal(g, z - yv) and np.array_equal(l, (z - yv) * (z - yv) / 2.0)


# ------------------------------------------------------------------------------------------------
# fp32
# ------------------------------------------------------------------------------------------------
MULT_BAR32 = 2.0 ** -21


@pytest.mark.parametrize("y", [0.0, 1.0])
def test_logistic_f32_multipliers(probe, y):
    z = MT.margin_inputs(np.float32)
    assert z.size >= 200000
    tm = np.asarray(MT.logistic_mult(z, y), np.float64)
    for name, op, sign in (("sparse_coef", OP["sparse_coef"], -1.0), ("split_sigmoid", OP["split_sigmoid"], 1.0),
                           ("gradient32", OP["gradient32"], 1.0)):
        m, _ = probe(op + LOGISTIC if name != "split_sigmoid" else op, z, y)
        e = np.abs(sign * m.astype(np.float64) - tm)
        assert record(f"{name}_logistic_mult_y{int(y)}", e, z, "absolute, bar 2^-21") <= MULT_BAR32
        nf, _ = probe(op + LOGISTIC if name != "split_sigmoid" else op, np.array(MT.NONFINITE, np.float32), y)
        assert sign * nf[0] == 1.0 - y and sign * nf[1] == 0.0 - y and np.isnan(nf[2])
    # chain_block's coef takes u = -log2(e) * dot
    u = (-z.astype(np.float64) * 1.4426950408889634).astype(np.float32)
    c, _ = probe(OP["coef32"] + LOGISTIC, u, y)
    with np.errstate(over="ignore"):
        sig = 1 / (1 + np.exp2(u.astype(LD)))
    tu = np.asarray(LD(y) - sig, np.float64)          # c = -s * (sig - y), s = 1
    e = np.abs(c.astype(np.float64) - tu)
    assert record(f"coef32_logistic_y{int(y)}", e, u, "absolute, bar 2^-21") <= MULT_BAR32
    nf, _ = probe(OP["coef32"] + LOGISTIC, np.array(MT.NONFINITE, np.float32), y)
    assert nf[0] == y - 0.0 and nf[1] == y - 1.0 and np.isnan(nf[2])


@pytest.mark.parametrize("y", [0.0, 1.0])
def test_logistic_f32_row_losses(probe, y):
    z = MT.margin_inputs(np.float32)
    tl = MT.logistic_loss(z, y)
    tl64 = np.asarray(tl, np.float64)
    t = np.abs(z.astype(np.float64))
    small = (tl64 >= 2.0 ** -100) & (tl64 < 0.7)
    outs = {"row_loss32": probe(OP["row_loss32"] + LOGISTIC, z, y)[0],
            "sparse_coef": probe(OP["sparse_coef"] + LOGISTIC, z, y)[1],
            "gradient32": probe(OP["gradient32"] + LOGISTIC, z, y)[1]}
    failures = []
    for name, l in outs.items():
        a = np.asarray(np.abs(l.astype(LD) - tl), np.float64) / np.maximum(1.0, tl64)
        wa = record(f"{name}_logistic_loss_abs_y{int(y)}", a, z, "absolute / max(1, loss), claim 1e-7, bar 4e-7")
        # relative to a small loss: softplus_fast's bound (psgd_device.h), which the library
        # log1pf(expf) form of gradient_scalar<float> meets too
        r = rel_err(l, tl)[small] / (2.0 ** -24 * (1.5 * t[small] + 24))
        wr = record(f"{name}_logistic_loss_rel_y{int(y)}", r, z[small], "relative / (2^-24 (1.5|t| + 24)), bar 1")
        if not (wa <= 4e-7 and wr <= 1.0):
            failures.append((name, wa, wr))
    assert not failures, failures
    for name, op, idx in (("row_loss32", OP["row_loss32"], 0), ("sparse_coef", OP["sparse_coef"], 1), ("gradient32", OP["gradient32"], 1)):
        nf = probe(op + LOGISTIC, np.array(MT.NONFINITE, np.float32), y)[idx]
        # z = +inf: margin -inf; label 1 loses nothing, label 0 everything
        assert nf[0] == (0.0 if y > 0 else np.inf) and nf[1] == (np.inf if y > 0 else 0.0) and np.isnan(nf[2]), name


def test_least_squares_and_hinge_f32_exact(probe):
    rng = np.random.default_rng(4)
    one = np.float32(1)
    z = np.concatenate([(rng.standard_normal(5000) * 10).astype(np.float32),
                        np.array([1, np.nextafter(one, np.float32(0)), np.nextafter(one, np.float32(2)), -1,
                                  np.nextafter(-one, np.float32(0)), np.nextafter(-one, np.float32(-2)), 0], np.float32)])
    for y in (np.float32(0), np.float32(1)):
        ls = np.float32(2) * y - one
        on = one > ls * z
        want_c = np.where(on, ls, np.float32(0))            # c = -s * mult = s * ls
        want_l = np.where(on, one - ls * z, np.float32(0))
        c, _ = probe(OP["coef32"] + HINGE, z, y)
        sc, sl = probe(OP["sparse_coef"] + HINGE, z, y)
        g, gl = probe(OP["gradient32"] + HINGE, z, y)
        rl, _ = probe(OP["row_loss32"] + HINGE, z, y)
        assert np.array_equal(c, want_c) and np.array_equal(sc, want_c) and np.array_equal(g, -want_c)
        assert np.array_equal(sl, want_l) and np.array_equal(gl, want_l) and np.array_equal(rl, want_l)
    yv = rng.standard_normal(z.size).astype(np.float32)
    d = z - yv
    c, _ = probe(OP["coef32"] + LEAST_SQUARES, z, yv)
    sc, sl = probe(OP["sparse_coef"] + LEAST_SQUARES, z, yv)
    g, gl = probe(OP["gradient32"] + LEAST_SQUARES, z, yv)
    rl, _ = probe(OP["row_loss32"] + LEAST_SQUARES, z, yv)
    assert np.array_equal(c, yv - z) and np.array_equal(sc, -d) and np.array_equal(g, d)
    assert np.array_equal(sl, d * d) and np.array_equal(rl, d * d) and np.array_equal(gl, d * d / np.float32(2))


def test_pow_fast(probe):
    """exp2(b log2 a) with the hardware log2 / exp2 (1 ulp each): the exponent b log2 a carries
    1 ulp of the log and half an ulp of the product, so the relative error of the power is
    2^-23 (1 + 1.5 ln2 |b log2 a|) -- "a few ulp" only while |b log2 a| is a few."""
    rng = np.random.default_rng(8)
    a = np.concatenate([MT.normal_binades(np.float32, -126, 0, per=40), rng.uniform(0.5, 1.0, 50000), [0.9, 0.999, 1.0]]).astype(np.float32)
    b = np.round(np.exp(rng.uniform(0, np.log(1e6), a.size))).astype(np.float32)
    b[rng.integers(0, a.size, 20000)] = 1.0
    # keep the power a normal float: |b log2 a| <= 120
    l2 = np.log2(a.astype(np.float64))
    b = np.where(np.abs(b * l2) > 120, np.maximum(np.floor(120 / np.maximum(np.abs(l2), 1e-30)), 1), b).astype(np.float32)
    keep = np.abs(b * l2) <= 120
    a, b, l2 = a[keep], b[keep], l2[keep]
    out, _ = probe(OP["pow_fast"], a, b)
    p = MT.pow_ld(a, b)
    bar = 2.0 ** -23 * (2 + 1.5 * np.log(2) * np.abs(b * l2))
    e = rel_err(out, p) / bar
    assert record("pow_fast", e, np.stack([a, b], 1), "relative / (2^-23 (2 + 1.04 |b log2 a|)), bar 1") <= 1.0
    sp, _ = probe(OP["pow_fast"], np.array([0.0, 1.0, 0.5], np.float32), np.array([3.0, 1e6, 200.0], np.float32))
    assert sp[0] == 0.0 and sp[1] == 1.0 and sp[2] == 0.0
