"""psgd_project on the GPU: new rows Y = X B from the fp64 MFMA kernel over dense rows and the lane-group
kernel over CSR rows, against numpy's long-double product (tests/project_truth.py), and what is built
on it: stat.multiply, PCA, computeSVD.

Bars: |Y - truth| <= 1e-9 A elementwise for f64 output (A = |X| |B|, the project's fp64 bar on the sum
of magnitudes); f32 output adds its one rounding, 2^-24 |truth|. Whole-number data (X and B in -3 .. 3)
makes every sum exact in either output dtype (at most 9 x 4,096 < 2^24), so there Y equals the int64
truth bit for bit: a row, a column or a feature chunk taken twice or not at all cannot hide behind a
relative bar. A second call returns the same bytes, the host form the bytes of the f64 device form, the
labels are copied exactly and the pad columns [k, ld) are zero.

Shapes (project_truth.DENSE_DK): d around the 4-, 8- and 16-feature steps and the stage of four steps,
k around one, two and three component blocks, (256, 256) for four chunks of four blocks read through
L2, and one shape the plan sends off LDS. Partitions of 1, 3, 0, 15, 16, 17, 65 and 3 x rows-a-wave + 5
rows: every remainder of the 16-row MFMA, the empty partition in the middle."""
import functools
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, has_gpu

import project_truth as PT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not has_gpu():
        pytest.skip("no GPU")


def np_dtype(storage):
    return np.float32 if storage == "f32" else np.float64


def sizes_of(pkg, layout, storage, d, k):
    rw = pkg._native.project_plan(layout, storage, d, k)["rows_wave"]
    return (1, 3, 0, 15, 16, 17, 65, 3 * rw + 5)


@functools.lru_cache(maxsize=None)
def dense_case(n, d, k, storage, whole):
    rng = np.random.default_rng(9100 + 7 * d + k + (3 if storage == "f32" else 0) + (100000 if whole else 0))
    if whole:
        X = rng.integers(-3, 4, size=(n, d)).astype(np_dtype(storage))
        B = rng.integers(-3, 4, size=(d, k)).astype(np.float64)
        T, A = PT.project_truth_int(X, B), None
    else:
        X = (rng.standard_normal((n, d)) * rng.uniform(0.5, 2.0, size=d) + rng.uniform(-1.0, 1.0, size=d)).astype(np_dtype(storage))
        X[rng.random((n, d)) < 0.05] = 0.0
        B = rng.standard_normal((d, k))
        T, A = PT.project_truth(X, B)
    y = rng.standard_normal(n) + 0.5
    return {"X": X, "B": B, "y": y, "T": T, "A": A}


def offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(int)


def dense_data(pkg, c, sizes):
    o = offsets(sizes)
    return pkg.PartitionedData([pkg.DensePartition(np.ascontiguousarray(c["y"][a:b]), np.ascontiguousarray(c["X"][a:b]))
                                for a, b in zip(o[:-1], o[1:])])


def rows_of(res, k):
    """(Y [n, k], labels [n], pad [n, ld - k]) of a projection's partitions, in partition order."""
    xs = [p.x.cpu().numpy() for p in res.partitions]
    ys = [p.labels.cpu().numpy() for p in res.partitions]
    X = np.concatenate(xs, axis=0)
    assert all(p.d == k for p in res.partitions)
    assert all(p.x.data_ptr() % 16 == 0 and (p.x.stride(0) * p.x.element_size()) % 16 == 0 for p in res.partitions)
    return X[:, :k], np.concatenate(ys), X[:, k:]


def check_all(pkg, data, c, sizes, k, out, what, host_form=True):
    """Everything a projection promises, on one engine."""
    engine = pkg.HipEngine(data)
    res = engine.project(c["B"], out)
    assert [p.n_rows for p in res.partitions] == list(sizes)
    assert (res.partition_counts == np.array(sizes)).all()
    Y, lab, pad = rows_of(res, k)
    assert Y.dtype == np_dtype(out)
    if c["A"] is None:
        assert (Y == c["T"]).all(), f"{what}: {int((Y != c['T']).sum())} entries differ, first at {tuple(np.argwhere(Y != c['T'])[0])}"
    else:
        print(f"{what}: worst error / bar = {PT.check_projection(Y, c['T'], c['A'], out, what):.3g}")
    assert lab.tobytes() == c["y"].tobytes()
    assert (pad == 0.0).all() and not np.signbit(pad).any()
    again, _, _ = rows_of(engine.project(c["B"], out), k)
    assert again.tobytes() == Y.tobytes()               # no atomics: the same bits from call to call
    if host_form:
        Y64 = Y if out == "f64" else rows_of(engine.project(c["B"], "f64"), k)[0]
        o = offsets(sizes)
        for p, (a, b) in enumerate(zip(o[:-1], o[1:])):
            assert engine.ctx.project(p, b - a, c["B"]).tobytes() == np.ascontiguousarray(Y64[a:b]).tobytes()
    return engine


def dense_params():
    for d, k in PT.DENSE_DK:
        for storage, out in PT.combo_of(d, k):
            yield pytest.param(d, k, storage, out, id=f"d{d}-k{k}-{storage}-{out}")


@pytest.mark.parametrize("d,k,storage,out", list(dense_params()))
def test_dense(pkg, d, k, storage, out):
    sizes = sizes_of(pkg, "dense", storage, d, k)
    c = dense_case(sum(sizes), d, k, storage, False)
    check_all(pkg, dense_data(pkg, c, sizes), c, sizes, k, out, f"dense d={d} k={k} {storage}->{out}")


@pytest.mark.parametrize("d,k,storage,out", list(dense_params()))
def test_dense_whole_numbers_are_exact(pkg, d, k, storage, out):
    sizes = sizes_of(pkg, "dense", storage, d, k)
    c = dense_case(sum(sizes), d, k, storage, True)
    check_all(pkg, dense_data(pkg, c, sizes), c, sizes, k, out, f"dense whole d={d} k={k} {storage}->{out}", host_form=False)


@pytest.mark.parametrize("storage,out", [("f32", "f32"), ("f64", "f64")])
def test_dense_off_lds(pkg, storage, out):
    """B too large for LDS (asserted from the plan): the MFMA operands come through L2."""
    d, k = PT.DENSE_OFF_LDS
    plan = pkg._native.project_plan("dense", storage, d, k)
    assert plan["path"] == "dense_l2" and plan["lds_bytes"] == 0
    sizes = (37, 0, 63)
    for whole in (False, True):
        c = dense_case(sum(sizes), d, k, storage, whole)
        check_all(pkg, dense_data(pkg, c, sizes), c, sizes, k, out, f"off-LDS {storage}->{out} whole={whole}", host_form=not whole)


@pytest.mark.parametrize("d,storage,ld", [(13, "f32", 16), (30, "f64", 32), (101, "f32", 104)])
def test_dense_zero_copy_pitch(pkg, d, storage, ld):
    """psgd_register_dense_device rows with ld > d: the pad belongs to the caller (NaN here) and must not
    reach an MFMA, not even against B's zeros."""
    import torch
    k = min(d, 17)
    sizes = sizes_of(pkg, "dense", storage, d, k)
    c = dense_case(sum(sizes), d, k, storage, False)
    dev = torch.device("cuda", 0)
    tdt = torch.float32 if storage == "f32" else torch.float64
    o = offsets(sizes)
    parts = []
    for a, b in zip(o[:-1], o[1:]):
        X = torch.full((b - a, ld), float("nan"), dtype=tdt, device=dev)
        X[:, :d] = torch.from_numpy(np.array(c["X"][a:b])).to(dev)
        parts.append(pkg.DevicePartition(torch.from_numpy(np.array(c["y"][a:b])).to(dev), X, d))
    for out in ("f32", "f64"):
        res = pkg.HipEngine(pkg.PartitionedData(parts)).project(c["B"], out)
        Y, lab, pad = rows_of(res, k)
        assert not np.isnan(Y).any()
        PT.check_projection(Y, c["T"], c["A"], out, f"zero-copy d={d} ld={ld} ->{out}")
        assert lab.tobytes() == c["y"].tobytes() and (pad == 0.0).all()


@pytest.mark.parametrize("storage,out,k,ld", [("f32", "f32", 2, 44), ("f64", "f64", 17, 18), ("f32", "f64", 33, 70)])
def test_wide_output_pitch(pkg, storage, out, k, ld):
    """psgd_project_device at a pitch past B's last block: every column [k, ld) is written as zero."""
    import torch
    d = 65
    sizes = sizes_of(pkg, "dense", storage, d, k)
    c = dense_case(sum(sizes), d, k, storage, False)
    engine = pkg.HipEngine(dense_data(pkg, c, sizes))
    dev, n = engine.dev, sum(sizes)
    odt = torch.float32 if out == "f32" else torch.float64
    o = offsets(sizes)
    with torch.cuda.stream(engine.stream):
        B = torch.from_numpy(c["B"]).to(dev)
        Y = torch.full((n, ld), float("nan"), dtype=odt, device=dev)
        lab = torch.full((n,), float("nan"), dtype=torch.float64, device=dev)
        ptr = lambda t: [t[a:b].data_ptr() if b > a else 0 for a, b in zip(o[:-1], o[1:])]
        engine.ctx.project_device(k, B.data_ptr(), pkg._native.F32 if out == "f32" else pkg._native.F64, ld, ptr(Y), ptr(lab),
                                  engine.stream.cuda_stream)
        engine.stream.synchronize()
    Yh = Y.cpu().numpy()
    PT.check_projection(Yh[:, :k], c["T"], c["A"], out, f"ld={ld}")
    assert (Yh[:, k:] == 0.0).all() and lab.cpu().numpy().tobytes() == c["y"].tobytes()


# ---- CSR ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def csr_case(n, d, k, storage, whole):
    """Ragged rows of 0, 1, 2, 17, d and 70 entries (capped at d), one explicitly stored 0.0 per six rows."""
    dt = np_dtype(storage)
    rng = np.random.default_rng(9900 + d + k + (3 if storage == "f32" else 0) + (100000 if whole else 0))
    lengths = (0, 1, 2, 17, d, 70)
    rows = []
    for r in range(n):
        m = min(lengths[r % len(lengths)], d)
        idx = np.sort(rng.choice(d, size=m, replace=False)).astype(np.int64)
        val = rng.integers(-3, 4, size=m).astype(dt) if whole else (rng.standard_normal(m) + 0.25).astype(dt)
        if r % len(lengths) == 2 and m:
            val[0] = 0.0                         # stored, and zero
        rows.append((idx.tolist(), val))
    X = PT.csr_to_dense(rows, d, dt)
    if whole:
        B = rng.integers(-3, 4, size=(d, k)).astype(np.float64)
        T, A = PT.project_truth_int(X, B), None
    else:
        B = rng.standard_normal((d, k))
        T, A = PT.project_truth(X, B)
    return {"rows": rows, "X": X, "B": B, "y": rng.standard_normal(n) + 0.5, "T": T, "A": A, "dtype": dt, "d": d}


def csr_parts(c, sizes):
    o = offsets(sizes)
    for a, b in zip(o[:-1], o[1:]):
        rows = c["rows"][a:b]
        ptr = np.zeros(b - a + 1, dtype=np.int64)
        for i, r in enumerate(rows):
            ptr[i + 1] = ptr[i] + len(r[0])
        col = np.array([i for r in rows for i in r[0]], dtype=np.int32)
        val = np.array([v for r in rows for v in r[1]], dtype=c["dtype"])
        yield np.ascontiguousarray(c["y"][a:b]), ptr, col, val


def csr_data(pkg, c, sizes, device=False):
    parts = []
    for y, ptr, col, val in csr_parts(c, sizes):
        if not device:
            parts.append(pkg.CsrPartition(y, ptr, col, val, c["d"]))
            continue
        import torch
        dev = torch.device("cuda", 0)
        # row_ptr holds absolute offsets: this partition's entries start at 5, not at 0
        colp = np.concatenate([np.full(5, 0, dtype=np.int32), col])
        valp = np.concatenate([np.full(5, np.nan, dtype=val.dtype), val])
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        parts.append(pkg.DeviceCsrPartition(t(y), t(ptr + 5), t(colp), t(valp), c["d"]))
    return pkg.PartitionedData(parts)


def csr_params():
    """Host partitions run the four (storage, output) pairs, device partitions the two straight ones."""
    for d in PT.CSR_D:
        for k in PT.CSR_K:
            for storage, out in PT.COMBOS:
                yield pytest.param(d, k, storage, out, False, id=f"d{d}-k{k}-{storage}-{out}-host")
            for storage in ("f32", "f64"):
                yield pytest.param(d, k, storage, storage, True, id=f"d{d}-k{k}-{storage}-{storage}-device")


@pytest.mark.parametrize("d,k,storage,out,device", list(csr_params()))
def test_csr(pkg, d, k, storage, out, device):
    plan = pkg._native.project_plan("csr", storage, d, k)
    assert plan["path"] == ("csr_lds" if d == PT.CSR_D[0] else "csr_l2")
    sizes = sizes_of(pkg, "csr", storage, d, k)
    for whole in (False, True):
        c = csr_case(sum(sizes), d, k, storage, whole)
        assert max(len(r[0]) for r in c["rows"]) == d > 64     # a row of all d entries, longer than a wave
        check_all(pkg, csr_data(pkg, c, sizes, device), c, sizes, k, out,
                  f"csr d={d} k={k} {storage}->{out} device={device} whole={whole}", host_form=not whole)


@pytest.mark.parametrize("layout", ["dense", "csr"])
def test_registry_of_empty_partitions(pkg, layout):
    if layout == "dense":
        part = pkg.DensePartition(np.zeros(0), np.zeros((0, 5), dtype=np.float32))
    else:
        part = pkg.CsrPartition(np.zeros(0), np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0), 5)
    engine = pkg.HipEngine(pkg.PartitionedData([part, part]))
    res = engine.project(np.ones((5, 3)))
    assert [p.n_rows for p in res.partitions] == [0, 0] and res.num_features == 3
    assert engine.ctx.project(0, 0, np.ones((5, 3))).shape == (0, 3)


def test_errors(pkg):
    import ctypes
    import torch
    N = pkg._native
    sizes = (5, 7)
    c = dense_case(12, 13, 2, "f32", False)
    engine = pkg.HipEngine(dense_data(pkg, c, sizes))
    engine.project(c["B"])
    L, h = N.lib(), engine.ctx.handle
    B = torch.from_numpy(c["B"]).to(engine.dev)
    Y = torch.zeros((12, 4), dtype=torch.float32, device=engine.dev)
    lab = torch.zeros(12, dtype=torch.float64, device=engine.dev)
    xs = np.array([Y[:5].data_ptr(), Y[5:].data_ptr()], dtype=np.uint64)
    ls = np.array([lab[:5].data_ptr(), lab[5:].data_ptr()], dtype=np.uint64)
    call = lambda k, b, st, ld, x, l: L.psgd_project_device(h, k, b, st, ld, x, l, None)
    assert call(2, B.data_ptr(), N.F32, 4, xs.ctypes.data, ls.ctypes.data) == 0
    torch.cuda.synchronize()
    assert call(2, None, N.F32, 4, xs.ctypes.data, ls.ctypes.data) == N.PSGD_EINVAL
    assert call(2, B.data_ptr(), N.F32, 4, None, ls.ctypes.data) == N.PSGD_EINVAL
    assert call(2, B.data_ptr(), N.F32, 4, xs.ctypes.data, None) == N.PSGD_EINVAL
    assert call(0, B.data_ptr(), N.F32, 4, xs.ctypes.data, ls.ctypes.data) == N.PSGD_EINVAL
    assert call(257, B.data_ptr(), N.F32, 260, xs.ctypes.data, ls.ctypes.data) == N.PSGD_EUNSUPPORTED
    assert call(2, B.data_ptr(), 7, 4, xs.ctypes.data, ls.ctypes.data) == N.PSGD_EINVAL
    assert call(2, B.data_ptr(), N.F32, 1, xs.ctypes.data, ls.ctypes.data) == N.PSGD_EINVAL     # ld_out < k
    assert call(2, B.data_ptr(), N.F32, 3, xs.ctypes.data, ls.ctypes.data) == N.PSGD_EINVAL     # 12-byte rows
    null = np.array([0, Y[5:].data_ptr()], dtype=np.uint64)
    assert call(2, B.data_ptr(), N.F32, 4, null.ctypes.data, ls.ctypes.data) == N.PSGD_EINVAL   # a non-empty partition
    out = np.zeros((5, 2))
    assert L.psgd_project(h, 0, 2, c["B"].ctypes.data, None) == N.PSGD_EINVAL
    assert L.psgd_project(h, 0, 2, None, out.ctypes.data) == N.PSGD_EINVAL
    assert L.psgd_project(h, 9, 2, c["B"].ctypes.data, out.ctypes.data) == N.PSGD_ESTATE
    fresh = ctypes.c_void_p()
    assert L.psgd_ctx_create(0, ctypes.byref(fresh)) == 0
    try:
        assert L.psgd_project(fresh, 0, 2, c["B"].ctypes.data, out.ctypes.data) == N.PSGD_ESTATE
        assert L.psgd_project_device(fresh, 2, B.data_ptr(), N.F32, 4, xs.ctypes.data, ls.ctypes.data, None) == N.PSGD_ESTATE
    finally:
        L.psgd_ctx_destroy(fresh)


# ---- end to end -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pca_case(n=2000, d=12):
    X = PT.scaled_rows(n, d, 41)
    rng = np.random.default_rng(5)
    w = rng.standard_normal(d)
    y = (X @ w + 0.1 * rng.standard_normal(n) > np.median(X @ w)).astype(np.float64)
    return X, y


@pytest.mark.parametrize("storage", ["f32", "f64"])
def test_pca_fit_transform_covariance(pkg, storage):
    """PCA(k).fit, transform (f64 output), covariance of the result: diagonal = the top k eigenvalues, the
    off-diagonals 0, both to 1e-9 of the largest eigenvalue (the bar tests/test_pca_api.py shows to hold)."""
    X, y = pca_case()
    k = 5
    data = pkg.PartitionedData.parallelize(y, X, 3, dtype=np_dtype(storage))
    model = pkg.PCA(k).fit(data)
    ev, V = PT.pca_truth(X)
    assert model.pc.shape == (X.shape[1], k)
    assert (np.abs(np.sum(model.pc * V[:, :k], axis=0)) >= 1.0 - 1e-9).all()
    res = model.transform(data, "f64")
    assert res.num_features == k and res.count() == X.shape[0] and res.column_transform is None
    cov = pkg.covariance(res)
    err = np.abs(cov - np.diag(ev[:k]))
    print(f"PCA end to end {storage}: worst |cov - diag(ev)| / ev0 = {err.max() / ev[0]:.3g}")
    assert (err <= 1e-9 * ev[0]).all()
    np.testing.assert_allclose(model.explainedVariance, ev[:k] / ev.sum(), rtol=1e-8)


def test_transformed_rows_register_and_train(pkg):
    X, y = pca_case()
    data = pkg.PartitionedData.parallelize(y, X, 4, dtype=np.float32)
    res = pkg.PCA(4).fit(data).transform(data)
    assert res.partitions[0].x.dtype.is_floating_point and res.partitions[0].x.element_size() == 4
    w, hist = pkg.GradientDescent.runMiniBatchSGD(res, pkg.LogisticGradient(), pkg.SquaredL2SGDUpdater(), 1.0, 2, 0.01,
                                                  1.0, np.zeros(4))
    assert len(hist) == 2 and np.isfinite(hist).all() and np.isfinite(w).all()


def test_standard_scaler_then_multiply(pkg):
    X, y = pca_case()
    Xf = X.astype(np.float32)
    data = pkg.PartitionedData.parallelize(y, Xf, 3, dtype=np.float32)
    scaler = pkg.StandardScaler(withMean=True, withStd=True).fit(data)
    scaled = scaler.transform(data)
    B = np.random.default_rng(3).standard_normal((X.shape[1], 3))
    res = pkg.multiply(scaled, B, "f64")
    assert res.column_transform is None
    # the registered rows: ((double)x - shift) * factor rounded to the storage
    Xs = ((Xf.astype(np.float64) - scaler.shift) * scaler.factor).astype(np.float32)
    T, A = PT.project_truth(Xs, B)
    Y, lab, _ = rows_of(res, 3)
    PT.check_projection(Y, T, A, "f64", "scaled rows")
    assert lab.tobytes() == y.tobytes()


def test_compute_svd_u_is_orthonormal(pkg):
    X, y = pca_case()
    data = pkg.PartitionedData.parallelize(y, X, 3)
    k = 6
    U, s, V = pkg.computeSVD(data, k, computeU=True)
    assert len(s) == k and V.shape == (X.shape[1], k) and U.num_features == k
    np.testing.assert_allclose(s, np.linalg.svd(X, compute_uv=False)[:k], rtol=1e-9)
    G = pkg.gramian(U).gram
    err = np.abs(G - np.eye(k)).max()
    print(f"computeSVD: worst |U^T U - I| = {err:.3g}")
    assert err <= 1e-9
    assert pkg.computeSVD(data, k)[0] is None


# ---- world size 2 -------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.parametrize("P", [5, 1])
def test_two_ranks(tmp_path, pkg, P):
    """Two ranks sharing cuda:0 over gloo, each a fresh child process (tests/two_rank_project.py): each
    rank's block meets both bars, the other rank's partitions are empty placeholders, partition_counts
    lists every partition on both ranks, and PCA.fit gives the same pc bytes on both."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import two_rank_project as T
    out = str(tmp_path / "res.json")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), PSGD_TEST_P=str(P))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "two_rank_project.py"), out], env=env,
                       capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    with open(out) as f:
        res = json.load(f)
    X, y, B = T.make_data()
    n = X.shape[0]
    bounds = [((i * n) // P, ((i + 1) * n) // P) for i in range(P)]
    counts = [b - a for a, b in bounds]
    T64, A = PT.project_truth(X, B)
    assert res["0"]["pc"] == res["1"]["pc"]                 # floats survive JSON exactly: identical bits
    seen = 0
    for rank in ("0", "1"):
        got = res[rank]
        assert got["counts"] == counts
        lo, hi = got["block"]
        assert got["rows"] == [counts[p] if lo <= p < hi else 0 for p in range(P)]
        for out_storage in ("f32", "f64"):
            Y = np.array(got[out_storage], dtype=np_dtype(out_storage)).reshape(-1, B.shape[1])
            a, b = (bounds[lo][0], bounds[hi - 1][1]) if hi > lo else (0, 0)
            assert Y.shape[0] == b - a
            PT.check_projection(Y, T64[a:b], A[a:b], out_storage, f"rank {rank} {out_storage}")
        assert got["labels"] == y[a:b].tolist()
        seen += hi - lo
    assert seen == P
