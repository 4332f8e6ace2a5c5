"""The scoring calls' surface that needs no device: the C ABI's argument errors and exported
symbols, the Python-side refusal of the multinomial gradient, Evaluation's arithmetic on an empty
data set, and psgd_run's --evaluate flag."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

BIN = os.path.join(ROOT, "spark-parallelized-sgd_amd", "psgd_run")
SYMBOLS = ("psgd_evaluate", "psgd_evaluate_device", "psgd_predict", "psgd_predict_device")


def native(pkg):
    import spark_parallelized_sgd_amd._native as N
    if not os.path.exists(N.LIB_PATH):
        pytest.skip("libpsgd.so not built (__graft_entry__.build())")
    return N


def test_library_exports_the_scoring_symbols(pkg):
    N = native(pkg)
    raw = C.CDLL(N.LIB_PATH)
    for name in SYMBOLS:
        assert hasattr(raw, name), name
        assert name in N.EXPORTED


def test_null_context_is_einval(pkg):
    N = native(pkg)
    L = N.lib()
    w = (C.c_double * 4)()
    out = (C.c_double * 3)()
    assert L.psgd_evaluate(None, 0, w, out, None) == N.PSGD_EINVAL
    assert b"ctx is null" in L.psgd_last_error()
    assert L.psgd_evaluate_device(None, 0, None, None, None, None) == N.PSGD_EINVAL
    assert L.psgd_predict(None, 0, w, out) == N.PSGD_EINVAL
    assert L.psgd_predict_device(None, 0, None, None, None) == N.PSGD_EINVAL


def test_multinomial_gradient_is_refused(pkg):
    data = pkg.PartitionedData.parallelize(np.zeros(4), np.ones((4, 2)), 2)
    g = pkg.LogisticGradient(numClasses=3)
    with pytest.raises(pkg.UnsupportedOperationException):
        pkg.evaluate(data, g, pkg.SimpleSGDUpdater(), 0.0, np.zeros(4))
    with pytest.raises(pkg.UnsupportedOperationException):
        pkg.ParallelizedSGD(g, pkg.SimpleSGDUpdater()).evaluate(data, np.zeros(4))


def test_evaluation_of_no_rows(pkg):
    ev = pkg.Evaluation(0.0, 0, 0, 0.25, [0.0, 0.0], [0, 0])
    assert math.isnan(ev.meanLoss) and math.isnan(ev.objective)
    assert ev.accuracy is None and ev.count == 0 and ev.regVal == 0.25
    some = pkg.Evaluation(3.0, 4, 3, 0.5, [1.0, 2.0], [1, 2])
    assert some.meanLoss == 0.75 and some.objective == 1.25 and some.accuracy == 0.75
    assert pkg.Evaluation(3.0, 4, None, 0.0).accuracy is None   # LeastSquaresGradient
    # a data set without partitions needs no device either
    none = pkg.evaluate(pkg.PartitionedData([]), pkg.HingeGradient(), pkg.SimpleSGDUpdater(), 0.0, np.zeros(3))
    assert none.count == 0 and math.isnan(none.objective) and none.accuracy is None


def run(*args):
    return subprocess.run([BIN, *args], capture_output=True, text=True, timeout=120)


def test_psgd_run_evaluate_flag(tmp_path):
    """--evaluate is a flag (no value): the option after it is parsed as an option, an unknown one
    is refused before any device is touched; without the flag the output is what it was."""
    if not os.path.exists(BIN):
        pytest.skip("psgd_run not built (__graft_entry__.build())")
    r = run("x.libsvm", "--evaluate", "--bogus", "1")
    assert r.returncode == 2 and "unknown option --bogus" in r.stderr and r.stdout == ""
    r = run("x.libsvm", "--evaluate", "--gradient", "softmax")
    assert r.returncode == 2 and "unknown gradient" in r.stderr
    r = run(str(tmp_path / "missing.libsvm"), "--evaluate")
    assert r.returncode != 0 and r.stdout == "" and r.stderr != ""
    # the same small run with and without the flag: with a device, the first line is the same but
    # for the wall time and the flag adds one line; without one, both fail alike before any output
    f = tmp_path / "t.libsvm"
    f.write_text("".join(f"{k % 2} 1:{0.5 + k} 3:{-1.0 + 0.25 * k}\n" for k in range(8)))
    opts = [str(f), "--partitions", "2", "--iterations", "2", "--tol", "0"]
    plain, flagged = run(*opts), run(*opts, "--evaluate")
    assert plain.returncode == flagged.returncode
    if plain.returncode != 0:
        assert plain.stdout == flagged.stdout == "" and plain.stderr == flagged.stderr
        return
    strip = lambda s: re.sub(r'"epoch_seconds": [0-9.eE+-]+', "", s)
    a, b = plain.stdout.splitlines(), flagged.stdout.splitlines()
    assert len(a) == 1 and len(b) == 2 and strip(a[0]) == strip(b[0])
    assert b[1].startswith('{"evaluate": {"lossSum": ') and '"objective": ' in b[1]
