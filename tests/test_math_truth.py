"""The longdouble truths of tests/math_truth.py against mpmath at 50 digits (CPU). The GPU bars of
test_gpu_math_edges.py start at 1e-16 relative, so the truths have to be good to ~1e-18."""
import numpy as np
import pytest

import math_truth as MT

LD = np.longdouble


def test_longdouble_is_extended():
    # the truths need more than a double: x86 extended (or better)
    assert np.finfo(LD).eps < 2e-19


def _points():
    rng = np.random.default_rng(5)
    x = np.concatenate([rng.uniform(-760, 760, 150), rng.uniform(-40, 40, 100),
                        np.ldexp(1.0, np.arange(-1074, 10, 37)), -np.ldexp(1.0, np.arange(-1070, 10, 41)),
                        [-746.0, -745.13, -708.4, 0.0, 709.0, 709.78, 710.0, 87.3, -88.7, 103.9]])
    return x


def test_truths_against_mpmath():
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    x = _points()
    assert x.size >= 300
    worst = {}

    def rel(got, want):
        want_ld = LD(mp.nstr(want, 30))
        if want_ld == 0:
            return float(abs(got))
        return float(abs(got - want_ld) / abs(want_ld))

    for v in x:
        m = mp.mpf(float(v))
        cases = {
            "sigmoid_neg": (MT.sigmoid_neg(v), 1 / (1 + mp.exp(m))),
            "mult_y1": (MT.logistic_mult(v, 1.0), -1 / (1 + mp.exp(m))),
            "mult_y0": (MT.logistic_mult(v, 0.0), 1 / (1 + mp.exp(-m))),
            "softplus": (MT.softplus(v), mp.log1p(mp.exp(m))),
            "loss_y1": (MT.logistic_loss(v, 1.0), mp.log1p(mp.exp(-m))),
            "loss_y0": (MT.logistic_loss(v, 0.0), mp.log1p(mp.exp(m))),
        }
        for name, (got, want) in cases.items():
            if abs(want) < mp.mpf(2) ** -16000:
                continue
            worst[name] = max(worst.get(name, 0.0), rel(LD(got), want))
    print("longdouble truths vs mpmath, worst relative error:", worst)
    # a handful of extended-precision roundings each
    assert max(worst.values()) < 2e-18, worst


def test_pow_truth_against_mpmath():
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    rng = np.random.default_rng(6)
    r = np.concatenate([rng.uniform(0.0, 1.0, 100), 1 - np.ldexp(1.0, -rng.integers(1, 53, 50)), [1e-30, 0.5, 2.0]])
    it = rng.choice([1.0, 2.0, 3.0, 10.0, 60.0, 1e3, 1e6], size=r.size)
    worst = 0.0
    for a, b in zip(r, it):
        want = mp.mpf(float(a)) ** mp.mpf(float(b))
        if want < mp.mpf(2) ** -16000:
            continue
        got = MT.pow_ld(a, b)
        worst = max(worst, float(abs(got - LD(mp.nstr(want, 30))) / LD(mp.nstr(want, 30))))
    print("pow truth vs mpmath, worst relative error:", worst)
    # powl at iter = 1e6 carries ~iter * eps / 2^10 in the exponent: far inside the 16-ulp bar
    assert worst < 1e-16
