"""plan_chains (psgd_kernels.hip): which chain kernel runs an epoch and what it needs, decided on
the host. Asked through psgd_plan_chains, which needs no device.

The expected variants restate the selection table of DESIGN.md §3. NV is the smallest power of two
with NV * 64 * VEC >= max_ld (VEC = 16 / sizeof(storage)); FULL is min_ld >= NV * 64 * VEC.
PSGD_B64_WAVES and PSGD_SPLIT are read once per process and left to the GPU tests that use them."""
import ctypes

import pytest

from test_ring_geometry import ring_geometry

DENSE, CSR = 0, 1
F64, F32 = 0, 1
LOGISTIC, LEAST_SQUARES, HINGE = 0, 1, 2
SIMPLE, L2, L1, ADAGRAD, ADAM = 0, 1, 2, 3, 4
OUT, WF32, WF64 = 0, 1, 2                      # WeightsIn
FAMILY = ["dense", "general", "block", "block64", "split", "sparse", "sparse_spec", "sparse64",
          "sparse_lds", "multinomial"]
RING_FAMILY = {"dense": 0, "split": 1, "block": 2, "block64": 3}   # ring_geometry's kRing*
NONE, MARGIN_LOSS, LOGISTIC_LOSS64 = 0, 1, 2  # ChainAfter
SETUP_NONE, SETUP_WF32, SETUP_W64 = 0, 1, 2   # ChainSetup
WNSQ0_NONE, WNSQ0_ROUNDED, WNSQ0_EXACT = 0, 1, 2
BUF_NONE, BUF_F32, BUF_F64 = 0, 1, 2
PLAN_FIELDS = ["family", "variant", "nv", "h", "full", "conv", "sk", "lds_k", "tail", "lds_bytes", "R", "MB",
               "D", "GS", "weights_in", "after", "setup", "wnsq0", "zbuf", "vec", "vec_stride", "walpha",
               "wnsq0_buf", "reroll_head"]
SWITCHES = ["PSGD_PER_SAMPLE", "PSGD_SPARSE_KERNEL", "PSGD_B64_CONV", "PSGD_SPARSE_SK", "PSGD_SPARSE_LDS_HEAD"]
RCV1_D = 47236
BIG = 2**31 - 1

_fn = None


def chain_plan(pkg, layout=DENSE, storage=F32, compute=F32, gradient=LEAST_SQUARES, updater=SIMPLE, tol=False,
               d=None, nc=0, min_ld=None, max_ld=512, max_nnz=0, n_max=1000, alpha_ok=True, budget=0,
               no_f64_vectors=False):
    """The plan as a dict of PLAN_FIELDS (family by name). d defaults to max_ld, min_ld to max_ld."""
    global _fn
    if _fn is None:
        _fn = ctypes.CDLL(pkg._native.LIB_PATH).psgd_plan_chains
        _fn.restype = ctypes.c_int32
        _fn.argtypes = [ctypes.POINTER(ctypes.c_int64), ctypes.c_int32, ctypes.POINTER(ctypes.c_int64), ctypes.c_int32]
    d = max_ld if d is None else d
    min_ld = max_ld if min_ld is None else min_ld
    spec = (ctypes.c_int64 * 15)(layout, storage, compute, gradient, updater, int(tol), d, nc, min_ld, max_ld,
                                 max_nnz, n_max, int(alpha_ok), budget, int(no_f64_vectors))
    out = (ctypes.c_int64 * len(PLAN_FIELDS))()
    assert _fn(spec, 15, out, len(PLAN_FIELDS)) == 0
    p = dict(zip(PLAN_FIELDS, (int(v) for v in out)))
    p["family"] = FAMILY[p["family"]]
    return p


@pytest.fixture(autouse=True)
def no_switches(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)


def rcv1(pkg, **kw):
    kw.setdefault("storage", F32)
    kw.setdefault("d", RCV1_D)
    kw.setdefault("max_nnz", 94)
    return chain_plan(pkg, layout=CSR, max_ld=kw.pop("d"), **kw)


def test_short_arrays_are_refused(pkg):
    chain_plan(pkg)
    spec = (ctypes.c_int64 * 15)()
    out = (ctypes.c_int64 * 24)()
    assert _fn(spec, 14, out, 24) == -1 and _fn(spec, 15, out, 23) == -1
    assert _fn(None, 15, out, 24) == -1 and _fn(spec, 15, None, 24) == -1


# (storage, compute, updater, tol, switches, max_ld, variant)
DENSE_CASES = [
    (F32, F32, SIMPLE, False, {}, 512, 302), (F32, F32, SIMPLE, True, {}, 512, 342),
    (F32, F32, SIMPLE, False, {}, 2048, 308), (F32, F32, SIMPLE, False, {}, 2052, 200),
    (F32, F64, L2, False, {}, 256, 701), (F32, F64, L2, False, {}, 512, 712), (F32, F64, L2, True, {}, 512, 752),
    (F64, F64, L2, False, {}, 1024, 718), (F64, F64, L2, False, {}, 1026, 200),
    (F32, F32, ADAGRAD, False, {}, 256, 101), (F32, F32, ADAGRAD, False, {}, 512, 822),
    (F32, F32, ADAGRAD, False, {}, 1024, 844), (F32, F32, ADAGRAD, False, {}, 2048, 848),
    (F32, F64, ADAGRAD, False, {}, 256, 101), (F32, F64, ADAGRAD, False, {}, 512, 822),
    (F32, F64, ADAGRAD, False, {}, 1024, 844), (F32, F64, ADAGRAD, False, {}, 2048, 848),
    (F64, F32, ADAM, False, {}, 1024, 848), (F64, F64, ADAM, False, {}, 1024, 848),
    (F32, F32, SIMPLE, True, {"PSGD_B64_CONV": "0"}, 512, 822), (F32, F64, SIMPLE, True, {"PSGD_B64_CONV": "0"}, 512, 822),
    (F32, F32, SIMPLE, True, {"PSGD_B64_CONV": "0"}, 256, 101), (F32, F64, SIMPLE, True, {"PSGD_B64_CONV": "0"}, 256, 101),
    (F32, F32, SIMPLE, False, {"PSGD_PER_SAMPLE": "1"}, 512, 102),
]


def family_of(variant):
    return {1: "dense", 2: "general", 3: "block", 4: None, 5: "multinomial", 6: "sparse_lds", 7: "block64",
            8: "split"}[variant // 100]


@pytest.mark.parametrize("storage,compute,updater,tol,env,max_ld,variant", DENSE_CASES)
def test_dense_selection_table(pkg, monkeypatch, storage, compute, updater, tol, env, max_ld, variant):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    vec = 4 if storage == F32 else 2
    nv = 1
    while nv * 64 * vec < max_ld:
        nv *= 2
    for gradient in (LOGISTIC, LEAST_SQUARES, HINGE):
        for budget in (0, 40 * 1024):
            p = chain_plan(pkg, storage=storage, compute=compute, gradient=gradient, updater=updater, tol=tol,
                           max_ld=max_ld, budget=budget)
            fam = family_of(variant)
            assert (p["variant"], p["family"], p["weights_in"], p["conv"]) == (variant, fam, OUT, int(tol))
            if fam == "general":
                assert (p["nv"], p["h"], p["full"], p["lds_bytes"]) == (0, 0, 0, 0)
                assert (p["R"], p["MB"], p["D"], p["GS"]) == (0, 0, 0, 0)
            else:
                assert (p["nv"], p["full"]) == (nv, 1)
                h = {"dense": 0, "block": 0, "block64": 1 + (variant - 700) % 40 // 10, "split": variant % 100 // 10}[fam]
                assert p["h"] == h
                # the ring is ring_geometry's for the same family, NV, CONV and budget
                ring = ring_geometry(pkg, RING_FAMILY[fam], nv, compute, tol, budget)
                assert (p["R"], p["MB"], p["D"], p["GS"], p["lds_bytes"]) == ring
                # FULL flips when the shortest row pitch drops below NV * 64 * VEC
                q = chain_plan(pkg, storage=storage, compute=compute, gradient=gradient, updater=updater, tol=tol,
                               max_ld=max_ld, min_ld=nv * 64 * vec - vec, budget=budget)
                assert (q["variant"], q["nv"], q["full"]) == (variant, nv, 0)
            # a dense binary Logistic epoch gets the per-row margins (fp32) / dots (fp64); the loss is
            # summed after the chain by the blocked kernels, chain_split, and chain_dense in fp64
            logistic = gradient == LOGISTIC
            assert p["zbuf"] == ((BUF_F32 if compute == F32 else BUF_F64) if logistic else BUF_NONE)
            after = {"general": NONE, "dense": NONE if compute == F32 else LOGISTIC_LOSS64, "block": MARGIN_LOSS,
                     "block64": LOGISTIC_LOSS64, "split": MARGIN_LOSS if compute == F32 else LOGISTIC_LOSS64}[fam]
            assert p["after"] == (after if logistic else NONE)
            assert (p["vec"], p["vec_stride"], p["walpha"], p["wnsq0_buf"], p["setup"], p["wnsq0"]) == (0,) * 6


@pytest.mark.parametrize("layout", [DENSE, CSR])
@pytest.mark.parametrize("storage", [F64, F32])
def test_multinomial_takes_every_layout(pkg, layout, storage):
    p = chain_plan(pkg, layout=layout, storage=storage, compute=F64, gradient=LOGISTIC, nc=3, max_nnz=10)
    assert (p["family"], p["variant"], p["weights_in"]) == ("multinomial", 500 + layout, OUT)
    assert p["lds_bytes"] == 2 * 3 * 8          # the K - 1 margins and multipliers
    assert (p["zbuf"], p["vec"], p["walpha"], p["wnsq0_buf"]) == (BUF_NONE, BUF_NONE, 0, 0)


def vec_stride(d):
    return (d + 128 + 1024 + 63) // 64 * 64


# (storage, switches, kwargs, tol, variant, family)
CSR32_CASES = [
    (F32, {}, {}, False, 601, "sparse_lds"), (F64, {}, {}, False, 600, "sparse_lds"),
    (F32, {}, {}, True, 641, "sparse_lds"),
    (F32, {"PSGD_SPARSE_SK": "8"}, {}, False, 611, "sparse_lds"), (F32, {"PSGD_SPARSE_SK": "8"}, {}, True, 641, "sparse_lds"),
    (F32, {"PSGD_SPARSE_KERNEL": "spec"}, {}, False, 411, "sparse_spec"),
    (F32, {"PSGD_SPARSE_KERNEL": "plain"}, {}, False, 401, "sparse"),
    (F32, {"PSGD_SPARSE_KERNEL": "plain"}, {}, True, 441, "sparse"),
    (F32, {"PSGD_SPARSE_KERNEL": "hbm64"}, {}, False, 401, "sparse"),     # any other value is `plain` in fp32
    (F32, {"PSGD_SPARSE_KERNEL": "lds"}, {}, False, 601, "sparse_lds"),
    (F32, {"PSGD_SPARSE_KERNEL": "lds"}, {"max_nnz": 129}, False, 401, "sparse"),
    (F32, {}, {"max_nnz": 129}, False, 401, "sparse"),
    (F32, {}, {"n_max": BIG + 1}, False, 411, "sparse_spec"),
    (F32, {}, {"n_max": BIG + 1}, True, 441, "sparse"),                    # chain_sparse_spec has no break
    (F32, {}, {"d": 2**22}, False, 401, "sparse"),
    (F32, {}, {"updater": L1}, False, 201, "general"), (F32, {}, {"updater": ADAGRAD}, False, 201, "general"),
    (F32, {"PSGD_PER_SAMPLE": "1"}, {}, False, 201, "general"),
]


@pytest.mark.parametrize("storage,env,kw,tol,variant,family", CSR32_CASES)
def test_csr_fp32_selection_table(pkg, monkeypatch, storage, env, kw, tol, variant, family):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    for updater in ((SIMPLE, L2) if "updater" not in kw else (kw["updater"],)):
        p = rcv1(pkg, **dict(kw, storage=storage, compute=F32, updater=updater, tol=tol))
        assert (p["variant"], p["family"]) == (variant, family)
        assert (p["nv"], p["h"], p["full"], p["R"], p["MB"], p["D"], p["GS"]) == (0,) * 7
        # every fp32-compute CSR epoch gets its fp32 vectors, chain_general's included
        d = kw.get("d", RCV1_D)
        assert (p["vec"], p["vec_stride"], p["walpha"], p["wnsq0_buf"], p["zbuf"]) == (BUF_F32, vec_stride(d), 1, 1, BUF_NONE)
        if family == "general":
            assert (p["weights_in"], p["setup"], p["wnsq0"]) == (OUT, SETUP_NONE, WNSQ0_NONE)
        else:
            # weights start as float(w_in) and end in the vectors; ||float(w_in)||^2 for SquaredL2 and the break
            assert (p["weights_in"], p["setup"]) == (WF32, SETUP_WF32)
            assert p["wnsq0"] == (WNSQ0_ROUNDED if updater == L2 or tol else WNSQ0_NONE)


def test_sparse_lds_head_and_reroll(pkg, monkeypatch):
    """chain_sparse_lds keeps features [0, K) in LDS: of a CU's 160 KiB its fixed area (32 B header, the
    128-row meta ring, SR = 16 (SK 4) or 32 (SK 8) slots of 128 entries) leaves sizeof(T) K + 2 (d - K)
    bytes (the tail's u16 tags), K a multiple of 4. The placement re-roll probes past the fp32 head
    for both vector widths."""
    def head(T, sk):
        meta = 128 * (2 * T + 8 + 4)
        fixed = 32 + meta + (16 if sk == 4 else 32) * 128 * (4 + T + 4)
        K = ((160 * 1024 - fixed - 2 * (RCV1_D + 4)) // (T - 2)) & ~3
        return K, fixed + T * K + 2 * ((RCV1_D - K + 3) & ~3)
    p = rcv1(pkg, compute=F32)
    assert (p["sk"], p["lds_k"], p["tail"], p["lds_bytes"]) == (4, *head(4, 4)[:1], 1, head(4, 4)[1])
    assert p["lds_k"] == 21096 and p["lds_bytes"] <= 160 * 1024 and p["reroll_head"] == p["lds_k"]
    q = rcv1(pkg, compute=F64)
    assert (q["sk"], q["lds_k"], q["tail"], q["lds_bytes"]) == (4, head(8, 4)[0], 1, head(8, 4)[1])
    assert q["lds_k"] == 5496 and q["lds_bytes"] <= 160 * 1024 and q["reroll_head"] == p["lds_k"]
    small = rcv1(pkg, compute=F32, d=1000)       # every feature in LDS: no tail
    assert (small["variant"], small["lds_k"], small["tail"], small["reroll_head"]) == (601, 1000, 0, 1000)
    monkeypatch.setenv("PSGD_SPARSE_LDS_HEAD", "202")   # the tests' cap, rounded down to a multiple of 4
    capped = rcv1(pkg, compute=F32, d=1000)
    assert (capped["variant"], capped["lds_k"], capped["tail"], capped["reroll_head"]) == (601, 200, 1, 1000)
    monkeypatch.delenv("PSGD_SPARSE_LDS_HEAD")
    monkeypatch.setenv("PSGD_SPARSE_SK", "8")
    p8 = rcv1(pkg, compute=F32)
    assert (p8["variant"], p8["sk"], p8["lds_k"], p8["lds_bytes"]) == (611, 8, *head(4, 8))
    assert p8["reroll_head"] == p8["lds_k"]
    p8c = rcv1(pkg, compute=F32, tol=True)       # the break has instances at SK = 4 only
    assert (p8c["variant"], p8c["sk"], p8c["lds_k"], p8c["reroll_head"]) == (641, 4, head(4, 4)[0], p8["lds_k"])
    assert (rcv1(pkg, compute=F64)["variant"], rcv1(pkg, compute=F64, tol=True)["variant"]) == (631, 661)


# (switches, kwargs, variant, family, weights_in)
CSR64_CASES = [
    ({}, {}, 621, "sparse_lds", OUT), ({}, {"tol": True}, 661, "sparse_lds", OUT),
    ({}, {"storage": F64}, 620, "sparse_lds", OUT),
    ({"PSGD_SPARSE_KERNEL": "hbm64"}, {}, 421, "sparse64", WF64), ({"PSGD_SPARSE_KERNEL": "hbm64"}, {"tol": True}, 461, "sparse64", WF64),
    ({}, {"d": 2**22}, 421, "sparse64", WF64), ({}, {"d": 2**22, "tol": True}, 461, "sparse64", WF64),
    ({}, {"d": 2**22, "storage": F64}, 420, "sparse64", WF64),
    ({}, {"max_nnz": 129}, 421, "sparse64", WF64), ({}, {"n_max": BIG + 1}, 421, "sparse64", WF64),
    ({"PSGD_SPARSE_KERNEL": "plain"}, {}, 621, "sparse_lds", OUT),        # fp64 knows hbm64 only
    ({}, {"updater": L2, "alpha_ok": False}, 201, "general", OUT),
    ({"PSGD_SPARSE_KERNEL": "hbm64"}, {"updater": L2, "alpha_ok": False}, 201, "general", OUT),
    ({}, {"updater": L1}, 201, "general", OUT), ({}, {"updater": ADAM}, 201, "general", OUT),
    ({}, {"no_f64_vectors": True}, 201, "general", OUT), ({}, {"d": 2**22, "no_f64_vectors": True}, 201, "general", OUT),
    ({"PSGD_PER_SAMPLE": "1"}, {}, 201, "general", OUT),
]


@pytest.mark.parametrize("env,kw,variant,family,weights_in", CSR64_CASES)
def test_csr_fp64_selection_table(pkg, monkeypatch, env, kw, variant, family, weights_in):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    for updater in ((SIMPLE, L2) if "updater" not in kw else (kw["updater"],)):
        p = rcv1(pkg, **dict(kw, compute=F64, updater=updater))
        assert (p["variant"], p["family"], p["weights_in"]) == (variant, family, weights_in)
        d, tol = kw.get("d", RCV1_D), kw.get("tol", False)
        if family == "general":
            # chain_general keeps its weights in w_out: no vectors (tens of GB at d = 2^22)
            assert (p["vec"], p["vec_stride"], p["walpha"], p["wnsq0_buf"], p["setup"], p["wnsq0"]) == (0,) * 6
        else:
            # the chain's f64 vector in L.wf32's memory: twice the fp32 stride, in floats; ||w_in||^2
            # only for the per-sample break
            assert (p["vec"], p["vec_stride"], p["walpha"]) == (BUF_F64, 2 * vec_stride(d), 1)
            assert p["wnsq0"] == (WNSQ0_EXACT if tol else WNSQ0_NONE) and p["wnsq0_buf"] >= (p["wnsq0"] != 0)
            assert p["setup"] == (SETUP_W64 if family == "sparse64" else SETUP_NONE)
        assert (p["zbuf"], p["after"]) == (BUF_NONE, NONE)
