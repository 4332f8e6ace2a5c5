"""psgd_tsqr on the GPU: the R of Z = [X, y] from the blocked Householder kernel, against LAPACK's R of
the same Z (numpy.linalg.qr, tests/tsqr_truth.py), and what is built on it in stat.py.

Bars, on data of cond(Z) < 4 (whole numbers in -3 .. 3, standard-normal rows):
  colres(R) = max |R^T R - Z^T Z|_jk / (||z_j|| ||z_k||) <= 8 x LAPACK's own on the same Z (another blocking,
    tile order and merge tree change the rounding, not its order of magnitude);
  max |R - R_lapack| <= 64 a eps ||R||_F, the forward bound cond x gamma_a.
Shapes: a = d + 1 = 4, 16, 17, 33, 128: one partial block, exactly one, a second block of one column, three
blocks, the full 128. Partitions of (37, 0, 63, 5) rows -- an empty one, one with fewer rows than columns,
panels that end mid-tile -- repeated until Z has at least 4 a rows (the bars assume a tall Z)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, has_gpu
from test_gpu_gram import _free_port
from test_gpu_project import dense_data, offsets
from tsqr_truth import colres, lapack_r

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not has_gpu():
        pytest.skip("no GPU")


def make_case(d, storage, kind="whole", sizes=None):
    sizes = sizes or (37, 0, 63, 5) * -(-4 * (d + 1) // 105)
    n = sum(sizes)
    rng = np.random.default_rng(4100 + d + (7 if storage == "f32" else 0))
    dt = np.float32 if storage == "f32" else np.float64
    if kind == "whole":
        X, y = rng.integers(-3, 4, size=(n, d)).astype(dt), rng.integers(-3, 4, size=n).astype(np.float64)
    else:
        X, y = rng.standard_normal((n, d)).astype(dt), rng.standard_normal(n)
    return {"X": X, "y": y, "Z": np.c_[X.astype(np.float64), y]}, sizes


def r_of(pkg, data, d):
    return pkg.HipEngine(data).tsqr().cpu().numpy().reshape(d + 1, d + 1)


def check_bars(R, Z, what):
    a = Z.shape[1]
    L = lapack_r(Z)
    res, ref = colres(R, Z), colres(L, Z)
    fwd, bar = np.abs(R - L).max(), 64 * a * EPS * np.linalg.norm(L)
    print(f"tsqr {what}: colres {res:.3g} / lapack {ref:.3g} = {res / ref:.3g}; forward {fwd:.3g} / bar {bar:.3g} = {fwd / bar:.3g}")
    assert np.isfinite(R).all() and (np.tril(R, -1) == 0.0).all() and (np.diag(R) >= 0.0).all()
    assert res <= 8 * ref
    assert fwd <= bar


@pytest.mark.parametrize("storage", ["f32", "f64"])
@pytest.mark.parametrize("d", [3, 15, 16, 32, 127])
def test_whole_numbers(pkg, d, storage):
    c, sizes = make_case(d, storage)
    engine = pkg.HipEngine(dense_data(pkg, c, sizes))
    R = engine.tsqr().cpu().numpy().reshape(d + 1, d + 1)
    check_bars(R, c["Z"], f"whole d={d} {storage}")
    assert engine.tsqr().cpu().numpy().tobytes() == R.tobytes()     # the same bits from call to call
    assert engine.ctx.tsqr(d).tobytes() == R.tobytes()              # and from the host-pointer form


@pytest.mark.parametrize("storage", ["f32", "f64"])
def test_real_rows(pkg, storage):
    c, sizes = make_case(32, storage, "normal")
    check_bars(r_of(pkg, dense_data(pkg, c, sizes), 32), c["Z"], f"normal d=32 {storage}")


def test_merge_tree_of_three_levels(pkg):
    """Sized from the plan: at least two merge levels, the first level's last node short of children."""
    d, sizes = 3, (200 * 1024 + 5, 92 * 1024 - 2)
    plan = pkg._native.tsqr_plan("f32", d, sum(-(-s // 1024) for s in sizes))
    assert plan["tile_rows"] == 1024 and plan["levels"] >= 2 and plan["items"] % plan["fan_in"] != 0
    c, _ = make_case(d, "f32", sizes=sizes)
    check_bars(r_of(pkg, dense_data(pkg, c, sizes), d), c["Z"], f"tree of {plan['levels']} levels, {plan['items']} items")


def test_degenerate_columns(pkg):
    """A zero column and a duplicated one: finite, an exact 0.0 on the zero column's diagonal."""
    c, sizes = make_case(5, "f64", "normal", sizes=(37, 0, 58, 5))
    c["X"][:, 2] = 0.0
    c["X"][:, 4] = c["X"][:, 1]
    Z = np.c_[c["X"], c["y"]]
    R = r_of(pkg, dense_data(pkg, c, sizes), 5)
    assert np.isfinite(R).all() and R[2, 2] == 0.0 and (np.diag(R) >= 0.0).all()
    res, ref = colres(R, Z), colres(lapack_r(Z), Z)
    print(f"tsqr degenerate: colres {res:.3g} / lapack {ref:.3g}")
    assert res <= 8 * ref


def test_ill_conditioned_least_squares(pkg):
    """The reason for the feature: cond(X) = 1e9, where the normal equations give up. (svd's default
    rCond = 1e-9 is sigma_min / sigma_0 itself and would keep or drop the last value by its last bit.)"""
    rng = np.random.default_rng(12)
    U, V = np.linalg.qr(rng.standard_normal((300, 12)))[0], np.linalg.qr(rng.standard_normal((12, 12)))[0]
    X = (U * np.logspace(0, -9, 12)) @ V.T
    w = rng.standard_normal(12)
    y = X @ w
    data = dense_data(pkg, {"X": X, "y": y}, (300,))
    with pytest.raises(pkg.IllegalArgumentException):
        pkg.normal_equations(data)
    err = np.linalg.norm(pkg.least_squares(data) - w) / np.linalg.norm(w)
    ref = np.linalg.norm(np.linalg.lstsq(X, y, rcond=None)[0] - w) / np.linalg.norm(w)
    s = pkg.qr_factor(data).svd(12, rCond=1e-12)[0]
    assert len(s) == 12
    smin = s[-1]
    print(f"tsqr cond 1e9: least_squares error {err:.3g} / lstsq {ref:.3g} = {err / ref:.3g}; sigma_min {smin:.9g}")
    assert err <= 64 * ref
    assert abs(smin - 1e-9) <= 1e-6 * 1e-9


def test_tall_skinny_qr_with_q(pkg):
    d = 15
    c, sizes = make_case(d, "f64", "normal")
    X = c["X"]
    data = dense_data(pkg, c, sizes)
    Q, R = pkg.tallSkinnyQR(data, computeQ=True)
    assert pkg.tallSkinnyQR(data).Q is None and R.shape == (d, d)
    Qh = np.concatenate([p.x.cpu().numpy()[:, :d] for p in Q.partitions])
    assert np.abs(Qh.T @ Qh - np.eye(d)).max() <= 64 * d * EPS * np.linalg.cond(X) ** 2
    assert np.abs(Qh @ R - X).max() <= 64 * d * EPS * np.linalg.norm(X)


def test_refusals(pkg):
    U = pkg.UnsupportedOperationException
    csr = pkg.CsrPartition(np.ones(2), np.array([0, 1, 2], dtype=np.int64), np.zeros(2, dtype=np.int32), np.ones(2), 5)
    with pytest.raises(U):
        pkg.qr_factor(pkg.PartitionedData([csr]))
    with pytest.raises(U):
        pkg.HipEngine(pkg.PartitionedData([csr])).tsqr()
    wide = pkg.PartitionedData([pkg.DensePartition(np.ones(3), np.ones((3, 128), dtype=np.float32))])
    with pytest.raises(U):
        pkg.qr_factor(wide)
    with pytest.raises(U):
        pkg.HipEngine(wide).tsqr()
    with pytest.raises(pkg.IllegalArgumentException):
        pkg.qr_factor(pkg.PartitionedData([pkg.DensePartition(np.zeros(0), np.zeros((0, 5), dtype=np.float32))]))


def test_two_ranks(tmp_path, pkg):
    """Two ranks sharing cuda:0 over gloo (tests/two_rank_tsqr.py): identical bits, the bar against all rows."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import two_rank_tsqr as T
    out = str(tmp_path / "res.json")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "two_rank_tsqr.py"), out], env=env,
                       capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    with open(out) as f:
        res = json.load(f)
    assert len(res) == 2 and res["0"] == res["1"]
    X, y = T.make_data()
    Z = np.c_[X.astype(np.float64), y]
    R = np.array(res["0"]["matrix"]).reshape(Z.shape[1], Z.shape[1])
    assert (np.diag(R) >= 0.0).all() and colres(R, Z) <= 8 * colres(lapack_r(Z), Z)
