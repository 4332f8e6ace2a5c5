"""The tagged-row construction on the CPU (tests/tagged_rows.py): what fixes the bar that
tests/test_gpu_row_coefficients.py holds the kernels to, and the evidence that the bar can see one
wrong row.

- The float64 restatement equals the C oracle on every tag coordinate to 1e-12 relative: the
  helper is pinned to the oracle, not to itself.
- S = max over tags of |dw[tag]| / tag_scale of the float32 restatement (both dot orders) and of
  oracle.run_f32 (orders 0 and 1, where it applies) against the fp64 oracle, on every data set
  the GPU module uses; S_ref is the largest, BAR = 4 S_ref (the room test_gpu_math_edges.py takes
  for a kernel's other summation tree). profiles/row_coefficients.json records them; recomputed
  here and compared (the hosts' float32 exp may differ in the last place: 10 % room on S_ref).
- Power: on every case each of the five one-row mutations, applied at a tagged active row, gives
  a statistic above 4 BAR: the first tagged row that has a predecessor, and for the stale margin
  the tagged row that shares most with the row before it. (Hinge's multiplier is +-1, so a stale
  margin shows only where it flips the decision: tagged_rows.hinge_pivot puts one tagged row of
  every Hinge data set there.)
- Hinge: at most 2 % of a case's tagged rows sit inside the guard band and are left out.
- Every case's tags cover the kernels' geometry: Gram block positions, tails, ring wraps, lanes
  and vector slots, the partly filled last vector, LDS head and HBM tail.
"""
import numpy as np
import pytest

import tagged_rows as T


@pytest.fixture(scope="module")
def stats(pkg):
    return {c["id"]: T.cpu_statistics(pkg, c) for c in T.CASES}


@pytest.mark.parametrize("c", T.CASES, ids=T.CASE_IDS)
def test_float64_restatement_equals_the_oracle(pkg, oracle, c):
    ref = T.build(pkg, c)
    data, idx = ref["data"], ref["idx"]
    w, ws, _ = T.run(data, c["grad"], c["upd"], c["step"], c["reg"], c["iters"], c["fraction"], ref["limits"])
    assert np.all(np.abs(w[idx] - ref["wr"][idx]) <= 1e-12 * np.abs(ref["wr"][idx])), c["id"]
    if c["fraction"] >= 1.0 and c["iters"] == 1:
        wc, _, _, cnt = oracle.run_chains(T.matrix(data), data["offs"], c["grad"], c["upd"], c["step"], c["reg"],
                                          data["w0"], tol=c["tol"], **ref["kw"])
        assert [int(v) for v in cnt] == ref["limits"]
        for p in range(len(ws)):
            assert np.all(np.abs(ws[p][idx] - wc[p][idx]) <= 1e-12 * np.abs(wc[p][idx])), (c["id"], p)
    # exact zeros where the oracle applied nothing, non-zero elsewhere
    assert np.all(ref["wr"][idx][ref["zero"]] == 0.0)
    assert np.all(ref["wr"][idx][~ref["zero"]] != 0.0)


def test_bars_are_the_recorded_ones(stats):
    cpu = T.load_profile()["cpu"]
    for compute, key in (("f32", "S_ref"), ("f64", "S_ref64")):
        s = max(max(stats[c["id"]].values()) for c in T.CASES if c["compute"] == compute)
        print(f"{key}: recomputed {s:.4g}, recorded {cpu[key]:.4g}")
        assert abs(s - cpu[key]) <= 0.1 * cpu[key], (key, s, cpu[key])
    assert cpu["BAR"] == 4 * cpu["S_ref"] and cpu["BAR64"] == 4 * cpu["S_ref64"]
    assert sorted(cpu["cases"]) == sorted(T.CASE_IDS)


def _candidates(ref):
    """Tagged, applied, active rows outside the guard band that have a predecessor and a
    successor, in processing order, the longest chain first, as (tag, chain, position)."""
    out = []
    for t, i in enumerate(ref["info"]):
        n_p = ref["limits"][i["chain"]]
        if i["pos"] >= 1 and i["active"] and not ref["guard"][t] and i["pos"] + 1 < n_p:
            out.append((-n_p, i["pos"], t, i["chain"], i["pos"]))
    return [(t, p, k) for _, _, t, p, k in sorted(out)]


def _mutated(c, ref, mutation, at):
    dtype = np.float32 if c["compute"] == "f32" else np.float64
    w, _, traces = T.run(ref["data"], c["grad"], c["upd"], c["step"], c["reg"], c["iters"], c["fraction"],
                         ref["limits"], dtype=dtype, mutate=mutation, at=at)
    return T.statistic(w, ref["wr"], T.folded_scale(c, ref), ref["idx"], ref["keep"])[0], traces


@pytest.mark.parametrize("c", T.CASES, ids=T.CASE_IDS)
def test_every_mutation_is_far_above_the_bar(pkg, c):
    ref = T.build(pkg, c)
    bar = T.bars()[0 if c["compute"] == "f32" else 1]
    cand = _candidates(ref)
    assert cand, c["id"]
    for mutation in T.MUTATIONS:
        if mutation == "stale" and c["grad"] == "hinge":
            # the row the generator put between its current and its stale margin (hinge_pivot)
            t, p, k = next(x for x in cand if ref["info"][x[0]]["row"] == ref["data"]["pivot_row"])
        elif mutation == "stale" and c["K"] == 2:
            # a stale margin is an error only as far as the row shares features with the one before it:
            # the tagged row where the multiplier's change, in units of the tag's scale, is largest
            scale = T.folded_scale(c, ref)

            def effect(x):
                i = ref["info"][x[0]]
                f = (lambda z: 1.0 / (1.0 + np.exp(-z))) if c["grad"] == "logistic" else (lambda z: z)
                return (abs(f(i["z"]) - f(i["z_stale"])) * c["step"] / np.sqrt(i["iter"]) * abs(i["xtag"])
                        * ref["share"][i["chain"]] / scale[x[0]])
            t, p, k = max(cand, key=effect)
        elif mutation == "dup" and c["grad"] == "hinge":
            # a row applied twice recomputes its margin: the first tagged row that its own update
            # (+ s ||x||^2 on its margin) leaves active
            t, p, k = next(x for x in cand if (2 * ref["info"][x[0]]["y"] - 1) * ref["info"][x[0]]["z"]
                           + c["step"] / np.sqrt(ref["info"][x[0]]["iter"]) * ref["info"][x[0]]["xnorm"] ** 2 < 0.9)
        else:
            t, p, k = cand[0]   # the first tagged row with a predecessor
        s, _ = _mutated(c, ref, mutation, (p, k))
        print(f"{c['id']} {mutation}: {s:.4g} (4 BAR = {4 * bar:.4g})")
        assert s > 4 * bar, (c["id"], mutation, s, 4 * bar)


@pytest.mark.parametrize("c", [c for c in T.CASES if c["grad"] == "hinge"],
                         ids=[c["id"] for c in T.CASES if c["grad"] == "hinge"])
def test_hinge_guard_band_leaves_out_at_most_two_percent(pkg, c):
    ref = T.build(pkg, c)
    applied = np.array([i["pos"] >= 0 for i in ref["info"]])
    active = np.array([i["active"] for i in ref["info"]])
    assert ref["guard"].sum() <= 0.02 * len(ref["info"]), (c["id"], int(ref["guard"].sum()), len(ref["info"]))
    keep = applied & ~ref["guard"]
    assert (keep & active).any() and (keep & ~active).any(), c["id"]   # both decisions are compared


@pytest.mark.parametrize("c", T.CASES, ids=T.CASE_IDS)
def test_tags_cover_the_kernel_geometry(pkg, c):
    ref = T.build(pkg, c)
    data = ref["data"]
    rows, cols = data["tags"]
    offs = data["offs"]
    assert len(set(cols.tolist())) == len(cols) and len(set(rows.tolist())) == len(rows)
    assert np.all(data["w0"].reshape(max(c["K"] - 1, 1), -1)[:, cols] == 0.0)
    if T.is_csr(data):
        for r, col in zip(rows, cols):   # the tag column appears in its row only
            assert (data["col"] == col).sum() == 1 and col in data["col"][data["rp"][r]:data["rp"][r + 1]]
        assert (cols < c["d"] // 3).any() and (cols >= c["d"] // 3).any()     # LDS head and HBM tail
        assert offs[-1] <= 4000
    else:
        X = data["X"]
        assert np.count_nonzero(X[:, cols]) == len(cols) and np.all(X[rows, cols] != 0.0)
        assert np.all((np.abs(X[rows, cols]) >= 0.5) & (np.abs(X[rows, cols]) <= 2.0))
        assert offs[-1] <= 2000
        if c["nv"] > 0:
            vec = 16 // np.dtype(c["storage"]).itemsize
            nvec = (c["d"] + vec - 1) // vec
            assert set((cols // vec).tolist()) == set(range(nvec))   # every lane x slot, the ragged last one too
    tagged = set(rows.tolist())
    thread = 64 if 0.0 < c["fraction"] <= 0.4 else None
    for p, seq in enumerate(T.sampled_rows(offs, c["fraction"])):
        for k in T.required_positions(len(seq), ref["R"], thread):
            assert int(seq[k]) in tagged, (c["id"], p, k)
    if c["fraction"] < 1.0:
        assert ref["zero"].any()             # tags on rows the epoch skips
    if c["tol"] > 0:
        sizes = np.diff(offs)
        cut = [int(n) for n, s in zip(ref["limits"], sizes) if n < s]
        assert any(n % 8 for n in cut), (c["id"], ref["limits"])    # breaks inside a Gram block
        assert ref["zero"].any()


def test_ring_wraps_are_tagged_at_the_minimum_ring(pkg):
    c = next(c for c in T.CASES if c["id"] == "block-min-ring")
    ref = T.build(pkg, c)
    assert ref["R"] == 16 and max(c["sizes"]) > 5 * ref["R"]
