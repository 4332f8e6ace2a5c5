"""The reuse schedules on the CPU (tests/reuse_schedule.py): that the data tests/test_gpu_sparse_reuse.py
runs really place features at the distances, entries, chunks and chain ends the CSR kernels'
look-ahead bookkeeping can get wrong, and that one wrong read there is far above the bar.

- The audit: every case covers what reuse_schedule.required asks of it at each of its depths, and
  the LeastSquares cases (the multiplier is linear in the margin) cover it with hazards whose
  mutations are above 4 x the bar alone.
- A numpy model of the two tag mechanisms, written from DESIGN.md §3 (chain_sparse_lds: window
  1..SK, sweep of chunk u & 127 in steps of 4 rows keeping rows u0 - SK .. u0 - 1; chain_sparse_spec:
  a row's tags cleared when its slot of 32 is reused), names for every tail entry of every row
  exactly the latest earlier row within SK that holds the feature -- and with the sweep or the
  clearing switched off it names a wrong row at every hazard of 256 + k or 512 + k rows: the schedule
  depends on the mechanism under test.
- The float64 restatement equals the C oracle on the tag coordinates to 1e-12 relative.
- S of the restatements in the case's precision against the fp64 oracle (as tests/test_tagged_rows.py
  computes it) is within the recorded S_ref / S_ref64 on every case, so the GPU module uses
  profiles/row_coefficients.json's BAR / BAR64 unchanged.
- Power: the stale mutation (row b's margin takes w[f] from before row a's update: a missed
  correction, or at distance SK + 1 a store not yet visible) and the alias mutation (256 + j and
  512 + j rows: row b takes what entry e_a of row b - j left in its slot) move row b's tag by more
  than 4 x the bar at every counted hazard; the one-pass figure equals a whole mutated run.
- profiles/reuse_schedule.json's CPU section is reproduced (10 % room, as for the other profile).
"""
import numpy as np
import pytest

import reuse_schedule as R
import tagged_rows as T

ROOM = 0.1


def bar_of(c):
    return T.bars()[0 if c["compute"] == "f32" else 1]


@pytest.fixture(scope="module")
def counted(pkg):
    return {c["id"]: R.counted(c, R.build(pkg, c), bar_of(c)) for c in R.CASES}


@pytest.mark.parametrize("c", R.CASES, ids=R.CASE_IDS)
def test_audit_is_complete(pkg, counted, c):
    ref = R.build(pkg, c)
    data = ref["data"]
    got = R.audit(c, data)
    ok, weakest, pw = counted[c["id"]]
    print(f"{c['id']}: {len(pw)} hazards, {len(ok)} counted, weakest {weakest}, "
          f"{sum(len(g) for g in got.values())} items covered")
    if c["required"]:
        R.audit(c, data, counted=ok)      # by the hazards that pass the power check alone
        assert len(ok) == len(pw), (c["id"], len(ok), len(pw))
    assert len(ok) > 0
    # wide rows exist and the entry halves are real: second entries of a lane on both sides
    tail = [h for h in data["hazards"] if h["zone"] == "tail"]
    assert any(h["ea"] >= 64 for h in tail) and any(h["eb"] >= 64 for h in tail)
    assert max(np.diff(data["rp"])) <= 128 and (np.diff(data["rp"]) > 64).any()
    assert data["head"] % 4 == 0 and data["offs"][-1] <= 1000


@pytest.mark.parametrize("c", R.CASES, ids=R.CASE_IDS)
def test_tag_model_names_the_latest_earlier_row(pkg, c):
    data = R.build(pkg, c)["data"]
    for rows in R.chain_rows(data):
        for SK in c["sks"]:
            assert R.model_lds(rows, data["d"], data["head"], SK) == R.truth(rows, data["head"], SK), (c["id"], SK)
        assert R.model_spec(rows, data["d"]) == R.truth(rows, 0, 8), c["id"]


@pytest.mark.parametrize("c", [c for c in R.CASES if c["kind"] != "small"],
                         ids=[c["id"] for c in R.CASES if c["kind"] != "small"])
def test_without_sweep_or_clearing_every_alias_hazard_names_a_wrong_row(pkg, c):
    data = R.build(pkg, c)["data"]
    rows = R.chain_rows(data)
    seen = 0
    for SK in c["sks"]:
        for p, rr in enumerate(rows):
            lds = R.model_lds(rr, data["d"], data["head"], SK, sweep=False)
            spec = R.model_spec(rr, data["d"], SK, clear=False)
            want = R.truth(rr, data["head"], SK)
            for h in data["hazards"]:
                if h["chain"] == p and h["zone"] == "tail" and R.aliases(h["k"], SK):
                    key = (h["b"], h["eb"])
                    wrong = (h["b"] - h["k"] % 256, h["ea"])     # a row that does not hold the feature
                    assert key not in want
                    assert lds.get(key) == wrong and spec.get(key) == wrong, (c["id"], SK, h)
                    seen += 1
    assert seen >= 4 * 8


@pytest.mark.parametrize("c", R.CASES, ids=R.CASE_IDS)
def test_float64_restatement_equals_the_oracle(pkg, oracle, c):
    ref = R.build(pkg, c)
    data, idx = ref["data"], ref["idx"]
    w, ws, _ = T.run(data, c["grad"], c["upd"], c["step"], c["reg"], 1, c["fraction"], ref["limits"])
    assert np.all(np.abs(w[idx] - ref["wr"][idx]) <= 1e-12 * np.abs(ref["wr"][idx])), c["id"]
    assert np.all(ref["wr"][idx][ref["zero"]] == 0.0)
    assert np.all(ref["wr"][idx][~ref["zero"]] != 0.0)
    if c["fraction"] < 1.0 or c.get("brk"):
        assert ref["zero"].any()
    if c.get("brk"):
        # the chain breaks at the row whose label is its margin, and nowhere near any other row
        p, k = c["brk"]
        sizes = np.diff(data["offs"])
        assert ref["limits"] == [k + 1 if q == p else int(sizes[q]) for q in range(len(sizes))]
        assert (k + 1) % 5 and float(ref["margins"].min()) > 100 * oracle.BREAK_MARGIN_F64
        t = int(np.flatnonzero(data["tags"][0] == data["brk_row"])[0])
        assert ref["zero"][t] and ref["wr"][idx][t] == 0.0
        after = [h for h in data["hazards"] if h["chain"] == p and h["a"] < k < h["b"]]
        assert len(after) >= 9 and all(ref["zero"][h["tag"]] for h in after)


@pytest.mark.parametrize("c", R.CASES, ids=R.CASE_IDS)
def test_statistic_is_within_the_recorded_reference(pkg, c):
    cpu = T.load_profile()["cpu"]
    s_ref = cpu["S_ref"] if c["compute"] == "f32" else cpu["S_ref64"]
    stats = T.cpu_statistics(pkg, c)
    rec = R.load_profile()["cpu"]["cases"][c["id"]]["S"]
    print(f"{c['id']}: S = {stats} (recorded reference {s_ref:.4g})")
    assert max(stats.values()) <= s_ref, (c["id"], stats, s_ref)
    assert sorted(rec) == sorted(stats)
    # (10 % of the case's own figure, and of the smallest figure that matters, S_ref / 100)
    assert abs(max(stats.values()) - max(rec.values())) <= ROOM * max(max(rec.values()), 0.01 * s_ref), (stats, rec)


@pytest.mark.parametrize("c", R.CASES, ids=R.CASE_IDS)
def test_counted_mutations_are_far_above_the_bar(pkg, counted, c):
    ref = R.build(pkg, c)
    bar = bar_of(c)
    ok, weakest, pw = counted[c["id"]]
    live = [q for q in sorted(ok) if pw[q]["stale"] is not None]
    assert live and weakest["stale"] > 4 * bar
    for q in live:
        assert pw[q]["stale"] > 4 * bar and (pw[q]["alias"] is None or pw[q]["alias"] > 4 * bar)
    if c["kind"] != "small":
        assert weakest["alias"] is not None and weakest["alias"] > 4 * bar
    # the one-pass figure is a whole mutated run's: the weakest hazards and a few others
    pick = sorted(live, key=lambda q: pw[q]["stale"])[:3] + live[:: max(len(live) // 3, 1)][:3]
    pick += sorted([q for q in live if pw[q]["alias"] is not None], key=lambda q: pw[q]["alias"])[:2]
    for q in pick:
        for m in ("stale", "alias"):
            if pw[q][m] is not None:
                full = R.mutated(c, ref, q, m)
                print(f"{c['id']} hazard {q} {m}: {pw[q][m]:.4g} one pass, {full:.4g} mutated run (4 BAR = {4 * bar:.4g})")
                assert abs(full - pw[q][m]) <= 1e-6 * pw[q][m] + 1e-3, (c["id"], q, m, full, pw[q][m])
                assert full > 4 * bar


def test_recorded_profile_is_reproduced(counted):
    rec = R.load_profile()["cpu"]["cases"]
    assert sorted(rec) == sorted(R.CASE_IDS)
    for c in R.CASES:
        ok, weakest, pw = counted[c["id"]]
        r = rec[c["id"]]
        assert (r["hazards"], r["counted"]) == (len(pw), len(ok)), c["id"]
        for m in ("stale", "alias"):
            assert (weakest[m] is None) == (r["weakest"][m] is None), (c["id"], m)
            if weakest[m] is not None:
                assert abs(weakest[m] - r["weakest"][m]) <= ROOM * r["weakest"][m], (c["id"], m, weakest[m], r["weakest"][m])


def test_geometry_restated(pkg):
    """The kernels' head and sweep chunk as the cases assume them (psgd_sparse_lds.hip)."""
    assert R.lds_head(2000, 4, "f32") == 2000 and R.lds_head(47_236, 4, "f64") == 5496
    assert R.sweep_chunk(2000, 400) == 256 and R.n_chunks(2000, 400) == 7     # the last one partial
    for c in R.CASES:
        if c["kind"] == "long":
            assert R.tag_entries(c["d"], c["head"]) > 32768 and R.sweep_chunk(c["d"], c["head"]) == 512
            assert c["head"] <= R.lds_head(c["d"], 4, c["compute"])
