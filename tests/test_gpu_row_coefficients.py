"""Every chain kernel's per-row coefficient, read out through tagged rows (tests/tagged_rows.py).

The other fp32 tests compare the folded weights with the fp64 oracle within FP32_REL x max|w|: 100
to 300 times the honest fp32 error, so an error confined to one row (a swapped pair, one row's
step index, one margin from stale weights) passes them. Here chosen rows own a
feature column of their own, whose weight after the epoch is that row's -step x multiplier x
value and nothing else; it is compared with the oracle per coordinate, in units of tag_scale (the
rounding of that one coordinate), against BAR = 4 S_ref from the CPU restatements
(tests/test_tagged_rows.py, profiles/row_coefficients.json) -- BAR64 with the 2^-53 scale for the
fp64 kernels. Tags of rows the oracle did not apply (unsampled, after a per-sample break, inactive
Hinge rows outside the guard band) must be exactly 0.0, all others non-zero. The kernel variant is
confirmed by last_kernel(), the ring by last_ring(), and the FP32_REL / loss bars (1e-9 in fp64)
are checked on the same run.

The observed statistic of every case goes to the JSON file PSGD_ROW_COEFFICIENTS_OUT names
(profiles/row_coefficients.json's "device" section is one such recording).
"""
import json
import os

import numpy as np
import pytest

import tagged_rows as T
from conftest import has_gpu
from test_gpu_parity import FP32_LOSS_REL, FP32_REL, G, U, assert_close, fp32_break_counts_agree
from test_gpu_sparse import KERNELS

pytestmark = pytest.mark.gpu

RECORD = {}
SPARSE_ENV = ("PSGD_SPARSE_KERNEL", "PSGD_SPARSE_LDS_HEAD", "PSGD_SPARSE_SK")


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not has_gpu():
        pytest.skip("no GPU")
    yield
    out = os.environ.get("PSGD_ROW_COEFFICIENTS_OUT")
    if out and RECORD:
        prof = T.load_profile()
        prof["device"] = RECORD
        with open(out, "w") as f:
            json.dump(prof, f, indent=1, sort_keys=True)


@pytest.fixture(params=sorted(KERNELS))
def kernel(request, monkeypatch):
    """As test_gpu_sparse's fixture of the same name (fixtures do not import across modules)."""
    env, base = KERNELS[request.param]
    for k in SPARSE_ENV:
        monkeypatch.delenv(k, raising=False)

    def apply(d):
        for k, v in env.items():
            monkeypatch.setenv(k, str(max(d // 3, 0)) if v == "third" else v)
        return base
    apply.name = request.param
    return apply


def partitions(pkg, c, data):
    offs = data["offs"]
    if T.is_csr(data):
        rp, col, y = data["rp"], data["col"], data["y"]
        val = data["val"].astype(np.float32 if c["compute"] == "f32" else np.float64)
        return [pkg.CsrPartition(y[a:b], rp[a:b + 1] - rp[a], col[rp[a]:rp[b]], val[rp[a]:rp[b]], c["d"])
                for a, b in zip(offs[:-1], offs[1:])]
    X = data["X"].astype(c["storage"])
    return [pkg.DensePartition(data["y"][a:b], X[a:b]) for a, b in zip(offs[:-1], offs[1:])]


def describe(c, ref, q):
    i = ref["info"][ref["which"][q]]
    vec = 16 // np.dtype(c["storage"]).itemsize
    where = f"row {i['row']} = chain {i['chain']} position {i['pos']} (block position {i['pos'] % 8}, iter {i['iter']})"
    if not T.is_csr(ref["data"]):
        where += f", column {i['col']} = lane {(i['col'] // vec) % 64} slot {i['col'] // vec // 64}"
    else:
        where += f", column {i['col']} of {c['d']}"
    return where


def run_case(pkg, monkeypatch, c, want, name, describe=describe, record=RECORD):
    """describe, record: another module's failure text and recorder (tests/test_gpu_sparse_reuse.py)."""
    ref = T.build(pkg, c)
    data = ref["data"]
    for k, v in c["env"].items():
        monkeypatch.setenv(k, v)
    if c["budget"]:
        monkeypatch.setenv("PSGD_LDS_BUDGET", str(c["budget"]))
    else:
        monkeypatch.delenv("PSGD_LDS_BUDGET", raising=False)
    grad = pkg.LogisticGradient(c["K"]) if c["K"] > 2 else getattr(pkg, G[c["grad"]])()
    w, h, counts = pkg.runParallelizedSGD(pkg.PartitionedData(partitions(pkg, c, data)), grad,
                                          getattr(pkg, U[c["upd"]])(), c["step"], c["iters"], c["reg"], c["fraction"],
                                          data["w0"], c["tol"], compute_dtype=c["compute"], return_chain_counts=True)
    ctx = pkg.optimization.get_context(0)
    assert ctx.last_kernel() == want, (name, ctx.last_kernel(), want)
    if ref["R"]:
        assert ctx.last_ring()[0] == ref["R"], (name, ctx.last_ring(), ref["R"])
    wr, hr, cr = ref["wr"], ref["hr"], ref["cr"]
    got = [[int(v) for v in it] for it in counts]
    exp = [[int(v) for v in it] for it in cr[: len(counts)]]
    if c["tol"] > 0 and c["compute"] == "f32":
        same = fp32_break_counts_agree(counts, cr, ref["margins"], name) and len(h) == len(hr)
    else:
        assert got == exp, name
        same = True

    # the tag coordinates
    fp32 = c["compute"] == "f32"
    bar = T.bars()[0 if fp32 else 1]
    idx, which, keep, zero = ref["idx"], ref["which"], ref["keep"].copy(), ref["zero"].copy()
    scale = T.folded_scale(c, ref)
    expect = wr[idx].copy()
    if got[0] != exp[0]:
        # a break one row off (within fp32_break_counts_agree's margin): the shares n_p / N follow
        # the device's counts, and in such a chain only the tags before the earlier break compare
        offs = data["offs"]
        share_dev = np.array(got[0], float) / sum(got[0])
        for q, t in enumerate(which):
            i = ref["info"][t]
            p = i["chain"]
            f = share_dev[p] / ref["share"][p]
            expect[q] *= f
            scale[q] *= f
            if got[0][p] != exp[0][p] and i["row"] - offs[p] >= min(got[0][p], exp[0][p]):
                keep[q] = False
    assert np.all(w[idx][zero & keep] == 0.0), (
        f"{name}: a row the oracle did not apply left its tag non-zero: "
        f"{describe(c, ref, int(np.argmax((w[idx] != 0.0) & zero & keep)))}")
    assert np.all(w[idx][~zero & keep] != 0.0), (
        f"{name}: an applied row left its tag at zero: "
        f"{describe(c, ref, int(np.argmax((w[idx] == 0.0) & ~zero & keep)))}")
    S, q = T.statistic(w, _with(wr, idx, expect), scale, idx, keep)
    record[name] = S
    print(f"{name}: S = {S:.4g} (bar {bar:.4g}) at {describe(c, ref, q)}")
    assert S <= bar, (f"{name}: tag coordinate off by {S:.4g} x its scale (bar {bar:.4g}) at {describe(c, ref, q)}: "
                      f"{w[idx][q]!r} vs {expect[q]!r}")

    # the bars the suite had before, on the same run
    if same:
        if fp32:
            err = np.max(np.abs(w - wr)) / max(np.max(np.abs(wr)), 1e-30)
            assert err <= FP32_REL, f"{name}: weights max err {err:.3g} x max|w|"
            assert_close(h, hr, rel=FP32_LOSS_REL, what=name + " loss")
        else:
            assert_close(w, wr, what=name + " weights")
            assert_close(h, hr, what=name + " loss")


def _with(w, idx, values):
    out = np.array(w, np.float64)
    out[idx] = values
    return out


def cases(*families):
    sel = [c for c in T.CASES if c["family"] in families]
    return dict(argnames="c", argvalues=sel, ids=[c["id"] for c in sel])


@pytest.mark.parametrize(**cases("block", "split", "dense", "block64", "general", "multinomial"))
def test_dense_rows(pkg, monkeypatch, c):
    run_case(pkg, monkeypatch, c, c["variant"], c["id"])


@pytest.mark.parametrize(**cases("csr"))
def test_csr_rows_fp32(pkg, monkeypatch, kernel, c):
    base = kernel(c["d"])
    run_case(pkg, monkeypatch, c, base + 1, f"{c['id']}-{kernel.name}")


@pytest.mark.parametrize(**cases("csr-plain", "csr64"))
def test_csr_rows_default_dispatch(pkg, monkeypatch, c):
    """Rows of more than 128 non-zeros (chain_sparse whatever is asked for) and the fp64 CSR kernels."""
    for k in SPARSE_ENV:
        monkeypatch.delenv(k, raising=False)
    run_case(pkg, monkeypatch, c, c["variant"], c["id"])
