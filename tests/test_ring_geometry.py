"""The LDS ring geometry of the dense chain kernels, on the host (no device needed).

Every dense chain kernel streams its rows through an LDS ring whose geometry {R row slots, MB meta
blocks, D loader depth, GS Gram slots} its launcher takes from psgd::ring_geometry (one function for
chain_dense, chain_split, chain_block and chain_block64). The per-workgroup LDS budget comes from
the number of chains P (psgd_capi.cpp lds_spread_bytes, restated in spread_budget below), so with
many chains per CU it drops below what a wide row's minimum ring needs; the launch then takes the
minimum ring instead of failing. Checked here for every family x NV x CONV instance and every
budget the spread can produce: a geometry comes back, it respects the kernels' invariants and the
160 KiB of a CU, and wherever the budget was enough before the minimum-ring rule existed it is
exactly what the launchers computed then (their arithmetic is restated in old_geometry)."""
import ctypes

import pytest

DENSE, SPLIT, BLOCK, BLOCK64 = 0, 1, 2, 3
NAMES = {DENSE: "chain_dense", SPLIT: "chain_split", BLOCK: "chain_block", BLOCK64: "chain_block64"}
F64, F32 = 0, 1            # compute
LDS_CU = 160 * 1024
DEPTH = {1: 56, 2: 28, 4: 14, 8: 7}      # loader_depth(NV): <= 56 DMA instructions in flight
MIN_ROWS = {DENSE: 6, SPLIT: 6, BLOCK: 16, BLOCK64: 16}
PUB = {DENSE: 4, SPLIT: 4, BLOCK: 8, BLOCK64: 8}     # rows per publish
GB = {DENSE: 0, SPLIT: 0, BLOCK: 8, BLOCK64: 8}      # rows per helper-wave block
META = 256                 # bytes of a meta block (16 rows)


def instances():
    """(family, nv, compute, conv) of every launcher instance whose geometry differs."""
    out = [(DENSE, nv, F64, False) for nv in (1, 2, 4, 8)]
    out += [(SPLIT, nv, c, conv) for nv in (2, 4, 8) for c in (F64, F32) for conv in (False, True)]
    out += [(fam, nv, F32 if fam == BLOCK else F64, conv)
            for fam in (BLOCK, BLOCK64) for nv in (1, 2, 4, 8) for conv in (False, True)]
    return out


def shallow_threshold(family, nv):
    """ring_loader drains its DMA and publishes before it blocks on a full ring when
    R < D + 2 PUB + 2 GB (psgd_device.h)."""
    return DEPTH[nv] + 2 * PUB[family] + 2 * GB[family]


def spread_budget(P, cus=256):
    """lds_spread_bytes: an even share of a CU's 160 KiB for ceil(P / CUs) chains, less 512 bytes,
    rounded down to a multiple of 256."""
    per_cu = max((P + cus - 1) // cus, 1)
    return (LDS_CU // per_cu - 512) & ~255


_fn = None


def ring_geometry(pkg, family, nv, compute, conv, budget):
    """psgd::ring_geometry through its mangled name: (R, MB, D, GS, bytes), or None when it
    returns non-zero."""
    global _fn
    if _fn is None:
        lib = ctypes.CDLL(pkg._native.LIB_PATH)
        _fn = lib._ZN4psgd13ring_geometryEiiiblPi
        _fn.restype = ctypes.c_int
        _fn.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_bool, ctypes.c_int64,
                        ctypes.POINTER(ctypes.c_int32)]
    out = (ctypes.c_int32 * 5)()
    if _fn(family, nv, compute, conv, budget, out) != 0:
        return None
    return tuple(int(v) for v in out)


def fixed_bytes(family, nv, compute, conv):
    if family == DENSE:
        return 16                                  # RingHeader
    if family == SPLIT:                            # + the compute waves' exchange and SIMD ids
        h = min(nv, 4)
        pc = (1 if compute == F32 else 2) * (3 if conv else 1)
        return (16 + 2 * h * pc * 8 + (h + 1) * 4 + 15) // 16 * 16
    if family == BLOCK:
        return 16 + 16                             # RingHeader, GramHeader
    return 16 + 16 + 32 + 36 * 8                   # + XchgHeader64 and the exchange doubles


def gram_slot_bytes(family, nv, conv):
    if family == BLOCK:
        return (64 + (8 if conv else 0)) * 4
    if family == BLOCK64:
        return (64 + (8 if conv else 0)) * 8 * (2 if nv >= 8 else 1)   # two sub-slots: feature-split Gram
    return 0


def old_geometry(family, nv, compute, conv, budget):
    """What launch_reg / launch_split / launch_block / launch_block64 computed before they shared
    one function, step by step as they did; None where they returned hipErrorInvalidValue."""
    budget = budget if budget > 0 else 64 * 1024
    fix, row = fixed_bytes(family, nv, compute, conv), nv * 1024
    mb = lambda r: (r + 15) // 16 + 2
    if family in (DENSE, SPLIT):
        if budget < fix + 3 * META:
            return None
        r = (budget - fix - 3 * META) // row
        while r > 0 and fix + mb(r) * META + r * row > budget:
            r -= 1
        if r < 6:
            return None
        return (r, mb(r), DEPTH[nv], 0, fix + mb(r) * META + r * row)
    gs = gram_slot_bytes(family, nv, conv)
    bytes_for = lambda r: fix + mb(r) * META + (r // 8 + 1) * gs + r * row
    if budget < fix:
        return None
    r = (budget - fix) // row // 8 * 8
    while r > 0 and bytes_for(r) > budget:
        r -= 8
    if r < 16:
        return None
    return (r, mb(r), DEPTH[nv], r // 8 + 1, bytes_for(r))


def check_invariants(family, nv, conv, g):
    r, mb, d, gs, nbytes = g
    assert r >= MIN_ROWS[family]
    assert mb >= (r + 15) // 16 + 2
    assert d == DEPTH[nv]
    if family in (BLOCK, BLOCK64):
        assert r % 8 == 0 and gs == r // 8 + 1
    else:
        assert gs == 0
    assert nbytes <= LDS_CU
    assert nbytes >= mb * META + r * nv * 1024     # the rings themselves


@pytest.mark.parametrize("family,nv,compute,conv", instances())
def test_every_spread_budget_gets_a_ring(pkg, family, nv, compute, conv):
    budgets = [0] + [spread_budget(k * 256) for k in range(1, 65)] + [spread_budget(P) for P in (257, 100_000, 10**7)]
    assert spread_budget(256) == 163328 and spread_budget(257) == 81408 and spread_budget(16384) == 2048
    for b in budgets:
        g = ring_geometry(pkg, family, nv, compute, conv, b)
        assert g is not None, (NAMES[family], nv, b)
        check_invariants(family, nv, conv, g)
        old = old_geometry(family, nv, compute, conv, b)
        if old is not None:                        # the budget was enough: nothing moves
            assert g == old, (NAMES[family], nv, b)
            assert g[4] <= (b if b > 0 else 64 * 1024)
        else:                                      # it was not: the family's minimum ring
            assert g[0] == MIN_ROWS[family], (NAMES[family], nv, b, g)


@pytest.mark.parametrize("family,nv,compute,conv", instances())
def test_geometry_unchanged_wherever_the_budget_was_enough(pkg, family, nv, compute, conv):
    """Every budget PSGD_LDS_BUDGET can name, byte-granular around each multiple of 256 up to the
    CU's LDS: identical to the launchers' former arithmetic, the minimum ring below it."""
    first_fit = None
    for base in range(0, LDS_CU + 1, 256):
        for b in (base - 1, base, base + 1):
            if b < 1 or b > LDS_CU:
                continue
            g = ring_geometry(pkg, family, nv, compute, conv, b)
            old = old_geometry(family, nv, compute, conv, b)
            if old is None:
                assert first_fit is None, "a budget stops fitting above one that fits"
                assert g is not None and g[0] == MIN_ROWS[family], (b, g)
                check_invariants(family, nv, conv, g)
            else:
                first_fit = first_fit or b
                assert g == old, (NAMES[family], nv, b, g, old)
                assert g[4] <= b
    # the minimum ring's request is exactly the first budget that was enough
    need = ring_geometry(pkg, family, nv, compute, conv, 1)[4]
    assert old_geometry(family, nv, compute, conv, need - 1) is None
    assert old_geometry(family, nv, compute, conv, need) == ring_geometry(pkg, family, nv, compute, conv, need)
    assert first_fit is not None and need <= first_fit < need + 257


# R at one chain per CU (budget 163,328 bytes), per family and NV: the geometry the benchmark's
# configurations run (c2 d 512 f32: NV 2; c3 d 1,024: NV 4 f32 / NV 8 f64). From the launchers'
# former arithmetic (old_geometry).
R_ONE_PER_CU = {
    DENSE: {1: 156, 2: 78, 4: 39, 8: 19},
    SPLIT: {2: 78, 4: 39, 8: 19},
    BLOCK: {1: 144, 2: 72, 4: 32, 8: 16},
    BLOCK64: {1: 144, 2: 72, 4: 32, 8: 16},
}


@pytest.mark.parametrize("family,nv,compute,conv", instances())
def test_rows_at_one_chain_per_cu_are_pinned(pkg, family, nv, compute, conv):
    b = spread_budget(256)
    want = R_ONE_PER_CU[family][nv]
    assert old_geometry(family, nv, compute, conv, b)[0] == want
    assert ring_geometry(pkg, family, nv, compute, conv, b)[0] == want
    # only chain_dense / chain_split at every NV, and the blocked kernels at NV 1 and 2, are deep there
    assert (want >= shallow_threshold(family, nv)) == (family in (DENSE, SPLIT) or nv <= 2)


def test_first_failing_chain_counts_of_the_old_launchers():
    """Where the spread budget first fell below the minimum ring (256 CUs): rows of 8 KiB from one
    chain more than there are CUs on the blocked kernels."""
    def first_fail(family, nv, conv=False):
        compute = F32 if family == BLOCK else F64
        k = 1
        while old_geometry(family, nv, compute, conv, spread_budget(k * 256)) is not None:
            k += 1
        return (k - 1) * 256 + 1
    for fam in (BLOCK, BLOCK64):
        assert [first_fail(fam, nv) for nv in (8, 4, 2, 1)] == [257, 513, 1025, 2049]
    for fam in (DENSE, SPLIT):
        assert [first_fail(fam, nv) for nv in (8, 4)] == [769, 1537]
        assert first_fail(fam, 2) > 2049


def test_unknown_family_or_nv(pkg):
    assert ring_geometry(pkg, 4, 1, F64, False, 65536) is None
    assert ring_geometry(pkg, DENSE, 3, F64, False, 65536) is None
    assert ring_geometry(pkg, SPLIT, 1, F64, False, 65536) is None   # chain_split starts at two row vectors


def sweep_budgets(pkg, family, nv, compute, conv):
    """The budgets the GPU sweep runs one instance at, from ring_geometry itself (so the test and
    the launcher cannot drift): {name: (PSGD_LDS_BUDGET or None for the default, R)} for the
    minimum ring (a budget below its request), the largest shallow ring the CU's LDS reaches
    (R < D + 2 PUB + 2 GB), the smallest deep one where it reaches one, and the default (one
    chain per CU). Budgets that give an R already listed are left out."""
    top = spread_budget(1)
    by_r = {}
    for b in range(256, top + 1, 256):
        by_r.setdefault(ring_geometry(pkg, family, nv, compute, conv, b)[0], b)
    thr = shallow_threshold(family, nv)
    out = {"min": (256, MIN_ROWS[family])}
    assert ring_geometry(pkg, family, nv, compute, conv, 256)[0] == MIN_ROWS[family]
    shallow = max(r for r in by_r if r < thr)
    deep = min((r for r in by_r if r >= thr), default=None)
    for name, r in (("shallow", shallow), ("deep", deep)):
        if r is not None and r not in [v[1] for v in out.values()]:
            out[name] = (by_r[r], r)
    r_def = ring_geometry(pkg, family, nv, compute, conv, top)[0]
    if r_def not in [v[1] for v in out.values()]:
        out["default"] = (None, r_def)
    return out


@pytest.mark.parametrize("family,nv,compute,conv", instances())
def test_sweep_budgets_reach_both_loader_paths(pkg, family, nv, compute, conv):
    s = sweep_budgets(pkg, family, nv, compute, conv)
    thr = shallow_threshold(family, nv)
    assert s["min"][1] == MIN_ROWS[family] < thr
    rs = [r for _, r in s.values()]
    assert len(set(rs)) == len(rs)
    # a deep ring is out of reach only for the blocked kernels' 4 and 8 KiB rows
    assert any(r >= thr for r in rs) == (family in (DENSE, SPLIT) or nv <= 2)
    if "shallow" in s:
        assert s["min"][1] < s["shallow"][1] < thr
    if "deep" in s:
        assert thr <= s["deep"][1] < thr + (8 if family in (BLOCK, BLOCK64) else 1)
