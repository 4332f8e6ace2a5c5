"""Reuse schedules: CSR chains in which chosen features come back at chosen distances (helper, no tests).

chain_sparse_lds (its HBM tail, fp32 and fp64, SK = 4 or 8) and chain_sparse_spec (SK = 8) gather a
row's weights SK samples ahead and repair them from an LDS tag table: a per-feature
tag (row & 255) << 8 | entry names the latest earlier row with the feature, a lookup accepts it when
the row delta modulo 256 is in 1..SK, the earlier row's new weight is read from its ring slot, and
stale tags are removed before the 8-bit row number wraps (chain_sparse_lds: a sweep of chunk u & 127
of the table at row u, in tagger steps of TB = 4 rows; chain_sparse_spec: a row's tags are cleared
when its slot is reused). A reuse at distance SK + 1 is repaired by nothing: it relies on the store
being in L2 before the sc1 gather issued one sample later. chain_sparse / chain_sparse64 keep the
next row's loads in flight: distance 1 is their edge.

Here the data are built from a list of hazards (feature f, earlier position a, later position
b = a + k of one chain's processing order): f is a probe feature that occurs in that chain at a and
b and nowhere between, row b owns a tag column (tests/tagged_rows.py), so one stale or aliased read
of w[f] at row b moves one coordinate that is compared at its own rounding scale. Contents: the
kernels' geometry restated (lds_head, sweep_chunk), the planner (Plan, plan_long, plan_small,
plan_short), the generator (generate), the ground truth and a numpy model of the two tag mechanisms
with their sweep / clearing switchable (truth, model_lds, model_spec), the audit of what a case
covers (audit), the two one-read mutations stale and alias and their effect on row b's tag (power,
mutated), the case table both test modules share (CASES, gpu_cases) and the profile recorder.

`python tests/reuse_schedule.py` recomputes the CPU section of profiles/reuse_schedule.json.
"""
import json
import os
import sys

import numpy as np

import tagged_rows as T

PROFILE = os.path.join(T.ROOT, "profiles", "reuse_schedule.json")

SKS = (4, 8)          # the speculation depths of the kernels (chain_sparse_spec: 8)
SK_MAX = 8            # one schedule serves both: it is laid out for 8 and audited for each
TB = 4                # rows per tagger step (PSGD_LDS_TB)
SWEEP_ROWS = 128      # the tag table is swept once per this many rows (kSweepRows)
SPEC_SR = 32          # chain_sparse_spec's ring
SPEC_GROUP = 8        # rows chain_sparse_spec's helper stages per step
FAR = (513, 516)      # the two 512 + k distances (k = 1 and 4: inside the window at either depth)
LONG = 803            # rows of the long chain: 512 + SK + 2 past the first use, no multiple of 4, 5 or 9
SHORT = (0, 1, 4, 5, 6, 8, 9, 10, 18, 45)   # 0, 1, SK, SK + 1, SK + 2 and multiples of SK + 1, SK = 4 and 8
CAP = 6               # probes per row at most
WIDE_FILL = 72        # filler entries of a wide row, all below the probes of its upper half
PROBE_VALUES = (2.0, 4.0)   # a probe's value before the row is normalised (fillers: 0.1 .. 1, as synth_csr)
W0_SCALE = 0.5        # of w0 on every feature but the tags (a tenth of that on the wide rows' pool)
LABEL_GAP = {"f32": 4.0, "f64": 0.125}   # LeastSquares: |y - z| of every processed row (see labels())


# ------------------------------------------------------------------------------------------------
# The kernels' geometry (psgd_sparse_lds.hip: lds_fixed_bytes, lds_head, tag_entries, the tagger's chunk)
# ------------------------------------------------------------------------------------------------
def lds_head(d, SK, compute):
    """Features [0, K) chain_sparse_lds<., T> keeps in LDS at depth SK when nothing caps K."""
    size = 4 if compute == "f32" else 8
    SR = 16 if 2 * SK + 8 <= 16 else 32
    fixed = 32 + 128 * (2 * size + 8 + 4) + SR * 128 * (4 + size + 4)
    budget = 160 * 1024 - fixed
    if size * d <= budget:
        return d
    K = (budget - 2 * (d + 4)) // (size - 2)
    assert K >= 0
    return K & ~3


def tag_entries(d, K):
    return (d - K + 3) & ~3


def sweep_chunk(d, K):
    """Tags per sweep chunk: 1/128 of the table, rounded up to 256 (one 4-tag word per lane)."""
    return ((tag_entries(d, K) + SWEEP_ROWS - 1) // SWEEP_ROWS + 255) & ~255


def n_chunks(d, K):
    return (tag_entries(d, K) + sweep_chunk(d, K) - 1) // sweep_chunk(d, K)


def distances(SK):
    return sorted(set(range(1, SK + 3)) | {15, 16, 17, 31, 32, 33, 127, 128, 129, 255, 256}
                  | set(range(257, 256 + SK + 2)) | set(FAR))


def aliases(k, SK=SK_MAX):
    """A reuse at k rows whose tag, left alone, is taken for one of k mod 256 rows ago."""
    return k > 256 and 1 <= k % 256 <= SK


def region(a):
    """Where a hazard's earlier row lies in a long chain: in the first sweep cycle, in the middle,
    or past row 512 (two wraps of the 8-bit row number)."""
    return "first" if a < 128 else "late" if a >= 512 else "middle" if a >= 256 else "other"


# ------------------------------------------------------------------------------------------------
# The planner: positions of one chain's hazards
# ------------------------------------------------------------------------------------------------
class Plan:
    """Hazards of one chain of n processed rows. A hazard: dict(a, b, k, kind, zone "tail" / "head",
    half = (probe's entry >= 64 in row a, in row b) or None, chunk = the sweep chunk its feature must
    lie in or None, group = hazards that share one feature or None). wide[position]: whether the row
    has 65-128 entries, once a hazard depends on it."""

    def __init__(self, rng, n, blocked=()):
        self.rng, self.n = rng, n
        self.haz, self.wide, self.blocked = [], {}, set(blocked)
        self.later = np.zeros(max(n, 1), int)
        self.load = np.zeros(max(n, 1), int)
        self.tagged = set()
        self.groups = 0

    def _fits(self, a, b, half):
        k = b - a
        if a in self.blocked or b in self.blocked or self.load[a] >= CAP or self.load[b] >= CAP:
            return None
        want = {}
        if half:
            want[a], want[b] = half
        if aliases(k):
            # the alias mutation reads entry e_a of row b - k % 256: that row has to have it
            r = b - k % 256
            if r in self.blocked:
                return None
            wa = want.get(a, self.wide.get(a, False))
            want[a] = wa
            if wa:
                if want.get(r, True) is not True:
                    return None
                want[r] = True
        for pos, w in want.items():
            if self.wide.get(pos, w) != w:
                return None
        return want

    def add(self, a, b, kind, zone="tail", half=None, chunk=None, group=None, want=None):
        assert 0 <= a < b < self.n
        self.wide.update(want or {})
        self.haz.append(dict(a=a, b=b, k=b - a, kind=kind, zone=zone, half=half, chunk=chunk, group=group))
        self.later[b] += 1
        self.load[a] += 1
        self.load[b] += 1
        self.tagged.add(b)

    def pick(self, k, kind, ok=None, **kw):
        """Place a hazard of distance k where `ok(a, b)` holds: at a later row no other hazard
        ends at, if there is one, and in the emptiest rows."""
        best = None
        for b in range(k, self.n):
            a = b - k
            if ok and not ok(a, b):
                continue
            want = self._fits(a, b, kw.get("half"))
            if want is None:
                continue
            key = (self.later[b], self.load[a] + self.load[b], self.rng.random())
            if best is None or key < best[0]:
                best = (key, a, b, want)
        assert best is not None, f"no room for a hazard of distance {k} ({kind}) in a chain of {self.n} rows"
        self.add(best[1], best[2], kind, want=best[3], **kw)

    def run(self, positions, kind):
        """One feature at every one of `positions`."""
        positions = list(positions)
        self.groups += 1
        for a, b in zip(positions[:-1], positions[1:]):
            self.add(a, b, kind, group=(kind, self.groups))


def _common(P, n, sks, kmax_only):
    """Entry halves, distances x residues of b mod TB, head controls: what every plan has."""
    far = [] if kmax_only else list(range(257, 257 + SK_MAX))
    for k in list(range(1, SK_MAX + 1)) + far:
        for ha in (False, True):
            for hb in (False, True):
                P.pick(k, "half", half=(ha, hb))
    for k in (range(1, SK_MAX + 3) if kmax_only else distances(SK_MAX)):
        spans = [(0, 128), (256, 512), (512, n)] if (k < 130 and not kmax_only) else [(0, n)]
        for res in range(TB):
            for lo, hi in spans:
                P.pick(k, "distance", ok=lambda a, b: b % TB == res and lo <= a < hi)
    for k in sorted({1} | set(sks) | {s + 1 for s in sks}):
        P.pick(k, "head", zone="head")


def plan_long(rng, n, chunks):
    """The long chain: every distance at every residue and region, entry halves, runs, ends, head
    controls, and hazards tagged next to their chunk's sweep."""
    P = Plan(rng, n)
    hot = range(400, 400 + 3 * SK_MAX)
    P.run(hot, "hot")
    P.tagged.add(hot[0])
    for SK, at in ((4, 440), (8, 460)):
        P.run([at + i * SK for i in range(4)], "ladder")
        P.run([at + 1 + i * (SK + 1) for i in range(3)], "ladder1")
    P.pick(3, "row0", ok=lambda a, b: a == 0)
    P.pick(2, "last", ok=lambda a, b: b == n - 1)
    _common(P, n, SKS, False)
    pick = sorted({0, chunks // 2, chunks - 1})
    for j in range(1, SK_MAX + 1):
        for off in (-1, 0, 1):
            c = pick[(j + off) % len(pick)]
            P.pick(256 + j, "sweep", ok=lambda a, b: (a & (SWEEP_ROWS - 1)) == (c + off) % SWEEP_ROWS, chunk=c)
    return P


def plan_small(rng, n, blocked=(), straddle=None):
    """A chain of a hundred rows or so: distances up to SK + 2, entry halves, head controls;
    straddle = position of a per-sample break: hazards across it and up to the row before it."""
    P = Plan(rng, n, blocked)
    if straddle is not None:
        for k in (1, 4, 5):
            P.pick(k, "before-break", ok=lambda a, b: b == straddle - 1)
        for k in range(2, SK_MAX + 3):     # (distance 1 has no row between)
            P.pick(k, "straddle", ok=lambda a, b: a < straddle < b and straddle - a <= 4)
    _common(P, n, SKS, True)
    return P


def plan_short(rng, n):
    """A short chain: row 0 to the last row, the last two rows, rows 0 and 1."""
    P = Plan(rng, n)
    if n >= 2:
        P.add(0, n - 1, "ends")
    if n >= 3:
        P.add(n - 2, n - 1, "ends")
        P.add(0, 1, "ends")
    if n == 1:
        P.tagged.add(0)
    for k in (4, 5, 8, 9):
        if n > 2 * k:
            P.pick(k, "ends", ok=lambda a, b: b == n - 1)
            P.pick(k, "ends", ok=lambda a, b: a == 0)
    return P


# ------------------------------------------------------------------------------------------------
# The generator
# ------------------------------------------------------------------------------------------------
def _allocate(rng, d, K, plans):
    """Feature roles. Head [0, K): probes of the head controls (K - 1 first), 40 fillers. Tail:
    a pool of wide rows' fillers in its lower 40 % (never feature K), 60 fillers anywhere, the
    probes of the entry-half hazards in its upper 60 % (d - 1 first), the probes tied to a sweep
    chunk in that chunk, all others round robin over the chunks (K first). Returns the pools and
    the features still free (tags are drawn from them)."""
    chunk, nch = sweep_chunk(d, K), n_chunks(d, K)
    zb0 = K + int(0.4 * (d - K))
    free = np.ones(d, bool)

    def take(cands, n):
        cands = np.asarray(cands)
        got = rng.choice(cands[free[cands]], size=n, replace=False)
        free[got] = False
        return np.sort(got)

    wide_pool = take(np.arange(K + 1, zb0), 160)
    pool = np.concatenate([take(np.arange(0, K - 1), 40), take(np.arange(K + 1, zb0), 30), take(np.arange(zb0, d - 1), 30)])
    forced = {"head": [K - 1], "upper": [d - 1], "chunk0": [K]}
    rr = [0]

    def one(lo, hi, key=None):
        if key and forced[key] and free[forced[key][0]]:
            f = forced[key].pop()
        else:
            cands = np.arange(lo, hi)
            cands = cands[free[cands]]
            assert len(cands), (lo, hi)
            f = int(cands[rng.integers(len(cands))])
        free[f] = False
        return f

    by_group = {}
    for P in plans:
        for h in P.haz:
            if h["group"] is not None and (id(P), h["group"]) in by_group:
                h["f"] = by_group[(id(P), h["group"])]
                continue
            if h["zone"] == "head":
                f = one(0, K, "head")
            elif h["half"] is not None:
                f = one(zb0, d, "upper")
            elif h["chunk"] is not None:
                c = h["chunk"]
                f = one(K + c * chunk, min(K + (c + 1) * chunk, d), "chunk0" if c == 0 else None)
            else:
                for _ in range(nch):
                    c = rr[0] % nch
                    rr[0] += 1
                    lo, hi = K + c * chunk, min(K + (c + 1) * chunk, d)
                    if free[lo:hi].any():
                        break
                f = one(lo, hi, "chunk0" if c == 0 else None)
            h["f"] = f
            if h["group"] is not None:
                by_group[(id(P), h["group"])] = f
    assert not any(forced.values()), forced
    return wide_pool, pool, free


def generate(kind, seed, sizes, d, head, storage=np.float32, fraction=1.0, brk=None):
    """The rows, tags, w0 and hazards of a case, without labels (labels() adds them):
    dict(rp, col, val, w0, tags, offs, d, K = 2, head, hazards, wide, brk_row, fraction).
    Rows: their probes, 2-6 fillers from a pool (wide rows: 72 from a pool below their upper-half
    probes), values as test_gpu_sparse.synth_csr (uniform(0.1, 1), the row normalised, rounded to
    the storage type) but for the probes, which are the row's large entries (PROBE_VALUES before
    the normalisation) so that one wrong weight shows in the margin; columns ascending; a tagged
    row has one more entry of magnitude 0.5-2 in a column of its own. w0: N(0, W0_SCALE^2) on every
    feature but the tags, where it is zero.
    kind: "main" (a long chain and the short ones), "long" (one long chain), "small" (chains of
    about a hundred processed rows each). brk = (chain, position): that row holds one feature
    nobody else has, with value 1 and w0 = 0.5, and a tag (a LeastSquares label of 0.5 makes its
    update exactly zero in every precision: the per-sample break)."""
    rng = np.random.default_rng(seed)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(int)
    seqs = T.sampled_rows(offs, fraction)
    K = head
    plans = []
    for p, seq in enumerate(seqs):
        n = len(seq)
        if kind == "small":
            here = brk is not None and brk[0] == p
            plans.append(plan_small(rng, n, blocked=[brk[1]] if here else (), straddle=brk[1] if here else None))
        elif n >= 600:
            plans.append(plan_long(rng, n, n_chunks(d, K)))
        else:
            plans.append(plan_short(rng, n))
    wide_pool, pool, free = _allocate(rng, d, K, plans)
    f_brk = None
    if brk is not None:
        f_brk = int(rng.choice(np.flatnonzero(free)))
        free[f_brk] = False

    # the rows: probes, fillers, and wide rows' 72 fillers below every upper-half probe
    cols = [set() for _ in range(offs[-1])]
    is_wide = np.zeros(offs[-1], bool)
    tagged = set()
    for p, (seq, P) in enumerate(zip(seqs, plans)):
        for h in P.haz:
            cols[seq[h["a"]]].add(h["f"])
            cols[seq[h["b"]]].add(h["f"])
        for pos, w in P.wide.items():
            is_wide[seq[pos]] = w
        tagged.update(int(seq[pos]) for pos in P.tagged)
        missed = np.setdiff1d(np.arange(offs[p], offs[p + 1]), seq)
        tagged.update(int(r) for r in missed[:: max(len(missed) // 12, 1)])   # rows the epoch skips: exact zeros
    brk_row = None
    for r in range(offs[-1]):
        if is_wide[r]:
            cols[r].update(rng.choice(wide_pool, size=WIDE_FILL, replace=False).tolist())
        elif cols[r] or r in tagged or rng.random() < 0.9:      # one row in ten of those nothing depends on is empty
            cols[r].update(rng.choice(pool, size=int(rng.integers(2, 7)), replace=False).tolist())
    if brk is not None:
        brk_row = int(seqs[brk[0]][brk[1]])
        cols[brk_row] = {f_brk}
        tagged.add(brk_row)
    # the alias mutation's guarantee: row b - k % 256 has an entry e_a (filled up from the row's own pool)
    changed = True
    while changed:
        changed = False
        for seq, P in zip(seqs, plans):
            for h in P.haz:
                if aliases(h["k"]):
                    ea = sorted(cols[seq[h["a"]]]).index(h["f"])
                    r = seq[h["b"] - h["k"] % 256]
                    while len(cols[r]) <= ea + 1:
                        src = wide_pool if is_wide[r] else pool
                        cols[r].add(int(src[rng.integers(len(src))]))
                        changed = True
    # tags: a column of its own per tagged row, from the features nothing else uses, head and tail
    rows = np.array(sorted(tagged), np.int64)
    tcols = rng.choice(np.flatnonzero(free), size=len(rows), replace=False)
    assert (tcols < K).any() and (tcols >= K).any()
    tag_of = dict(zip(rows.tolist(), tcols.tolist()))
    w0 = np.zeros(d)
    used = np.ones(d, bool)
    used[tcols] = False
    w0[used] = W0_SCALE * rng.standard_normal(int(used.sum()))
    w0[wide_pool] *= 0.1
    probe = np.zeros(d, bool)
    probe[[h["f"] for P in plans for h in P.haz]] = True
    if f_brk is not None:
        w0[f_brk] = 0.5
    rp, col, val = [0], [], []
    for r in range(offs[-1]):
        idx = np.array(sorted(cols[r]), np.int64)
        v = rng.uniform(0.1, 1.0, size=len(idx))
        v[probe[idx]] = rng.uniform(*PROBE_VALUES, size=int(probe[idx].sum()))
        v = (v / max(np.linalg.norm(v), 1e-12)).astype(np.float32).astype(storage).astype(np.float64)
        if r == brk_row:
            v[:] = 1.0
        if r in tag_of:
            t = float(rng.uniform(0.5, 2.0) * rng.choice([-1.0, 1.0]))
            idx, v = np.append(idx, tag_of[r]), np.append(v, np.float64(np.dtype(storage).type(t)))
            o = np.argsort(idx)
            idx, v = idx[o], v[o]
        assert len(idx) <= 128
        col += idx.tolist()
        val += v.tolist()
        rp.append(len(col))
    data = dict(rp=np.array(rp, np.int64), col=np.array(col, np.int32), val=np.array(val, np.float64),
                w0=w0, tags=(rows, np.asarray(tcols, np.int64)), offs=offs.tolist(), d=d, K=2, head=K,
                wide=is_wide, brk_row=brk_row, fraction=fraction)
    # the hazards as realised: rows, entry indices, the tag that reads them out
    tag_no = {int(r): t for t, r in enumerate(rows)}
    hz = []
    for p, (seq, P) in enumerate(zip(seqs, plans)):
        for h in P.haz:
            ra, rb = int(seq[h["a"]]), int(seq[h["b"]])
            ca, cb = row_cols(data, ra), row_cols(data, rb)
            hz.append(dict(h, chain=p, n=len(seq), row_a=ra, row_b=rb, ea=int(np.searchsorted(ca, h["f"])),
                           eb=int(np.searchsorted(cb, h["f"])), tag=tag_no[rb]))
    data["hazards"] = hz
    return data


def row_cols(data, r):
    return data["col"][data["rp"][r]:data["rp"][r + 1]]


def row_vals(data, r):
    return data["val"][data["rp"][r]:data["rp"][r + 1]]


def shrinks(n, upd, step, reg):
    """SquaredL2's factor 1 - s_j lambda of every position (ones otherwise): a weight that nothing
    updates from position k to before position m is multiplied by between(A, k, m)."""
    f = [1.0 - step / np.sqrt(float(j)) * reg if upd == "squared_l2" else 1.0 for j in range(1, n + 1)]
    return np.array(f)


def between(A, k, m):
    return float(np.prod(A[k:m]))


def _label_pass(data, grad, upd, step, reg, gap, sign, noise):
    """One run of the chains (float64, sample by sample as tagged_rows.chain) that sets every
    processed row's label from its margin. Returns (y, {alias hazard: (what row b would read
    through an aliased tag minus w[f], the change of that difference if row a's sign flipped)})."""
    offs = data["offs"]
    y = np.zeros(offs[-1])
    for r in range(offs[-1]):
        z = float(row_vals(data, r) @ data["w0"][row_cols(data, r)])
        y[r] = z + 0.1 * noise[r] if grad == "least_squares" else float(z + noise[r] > 0)
    diffs = {}
    for p, seq in enumerate(T.sampled_rows(offs, data["fraction"])):
        A = shrinks(len(seq), upd, step, reg)
        at = {}
        for q, h in enumerate(data["hazards"]):
            if h["chain"] == p and aliases(h["k"]):
                at.setdefault(h["b"] - h["k"] % 256 + 1, []).append((q, "slot"))
                at.setdefault(h["b"], []).append((q, "b"))
        slot = {}
        w = data["w0"].copy()
        for k, r in enumerate(seq):
            s = step / np.sqrt(float(k + 1))
            idx, x = row_cols(data, r), row_vals(data, r)
            for q, what in at.get(k, ()):
                h = data["hazards"][q]
                if what == "slot":
                    slot[q] = w[row_cols(data, seq[k - 1])[h["ea"]]]
                else:
                    ra = seq[h["a"]]
                    sa = step / np.sqrt(float(h["a"] + 1))
                    xa = float(row_vals(data, ra)[h["ea"]])
                    diffs[q] = (slot[q] * between(A, k - h["k"] % 256 + 1, k) - w[h["f"]],
                                2.0 * sa * gap * sign[ra] * xa * between(A, h["a"] + 1, k), ra)
            z = float(x @ w[idx])
            if r == data["brk_row"]:
                y[r] = z
                break
            if grad == "least_squares":
                y[r] = z + gap * sign[r]
                mult = z - y[r]
            elif grad == "logistic":
                y[r] = float(z < 0)
                mult = 1.0 / (1.0 + np.exp(-z)) - y[r]
            else:
                ls = 2 * y[r] - 1
                mult = -ls if 1.0 > ls * z else 0.0
            if upd == "squared_l2":
                w *= 1.0 - s * reg
            w[idx] -= s * mult * x
    return y, diffs


def labels(data, seed, grad, upd, step, reg, gap):
    """Labels, set while the chain runs: a stale read of w[f] at row b is off by row a's update,
    s_a mult_a x_af, so every processed row's multiplier is kept away from zero. LeastSquares:
    y = z +- gap (the multiplier is -+ gap whatever the weights; LABEL_GAP: 4 in fp32, and a
    fraction of that in fp64, where the tag's scale is 2^29 times finer and a multiplier of 4 would
    only carry its own roundings, 4 eps each, past the recorded S_ref64). The signs are random, but
    for the earlier rows of the 256 + j and 512 + j hazards: an aliased tag makes row b read another
    feature's weight, which is a wrong read only as far as the two weights differ, and with the
    multipliers fixed a row's sign moves nothing but its own update, so the sign that leaves the
    larger difference is taken (a second pass). Logistic: the label the margin contradicts
    (|mult| > 1/2). Hinge: the labels of a noisy model, active and inactive rows both. Rows the
    epoch skips: z(w0) + noise. The break row: y = its margin, 0.5."""
    rng = np.random.default_rng(seed + 7919)
    n = data["offs"][-1]
    sign = rng.choice([-1.0, 1.0], size=n)
    noise = rng.standard_normal(n) if grad == "least_squares" else rng.logistic(size=n)
    y, diffs = _label_pass(data, grad, upd, step, reg, gap, sign, noise)
    if grad == "least_squares" and diffs:
        by_row = {}
        for dd, flip, ra in diffs.values():
            by_row.setdefault(ra, []).append((dd, flip))
        for ra, v in by_row.items():
            if min(abs(dd + flip) for dd, flip in v) > min(abs(dd) for dd, flip in v):
                sign[ra] = -sign[ra]
        y, _ = _label_pass(data, grad, upd, step, reg, gap, sign, noise)
    data["y"] = y
    return data


# ------------------------------------------------------------------------------------------------
# The ground truth and the numpy model of the two tag mechanisms
# ------------------------------------------------------------------------------------------------
def chain_rows(data):
    """Per chain, the processed rows' column arrays in processing order."""
    return [[row_cols(data, r) for r in seq] for seq in T.sampled_rows(data["offs"], data["fraction"])]


def truth(rows, K, SK):
    """{(row u, entry e): (earlier row, its entry)}: for every entry of a feature >= K, the latest
    earlier row within SK that holds the feature; absent when there is none."""
    last, out = {}, {}
    for u, cols in enumerate(rows):
        for e, f in enumerate(cols.tolist()):
            if f >= K and f in last and u - last[f][0] <= SK:
                out[(u, e)] = last[f]
        for e, f in enumerate(cols.tolist()):
            last[f] = (u, e)
    return out


def _lookup(tagpos, u, cols, K, SK, out):
    """Row u's lookups and tag writes: what both kernels do per entry of a feature >= K."""
    sel = np.flatnonzero(cols >= K)
    f = cols[sel] - K
    v = tagpos[f].astype(np.int64)
    dl = (u - (v >> 8)) & 255
    hit = (v != 0xFFFF) & (dl >= 1) & (dl <= SK)
    for e, vv, dd in zip(sel[hit], v[hit], dl[hit]):
        out[(u, int(e))] = (u - int(dd), int(vv & 255))
    tagpos[f] = ((u & 255) << 8) | sel


def model_lds(rows, d, K, SK, sweep=True):
    """chain_sparse_lds's tagger: steps of TB rows; a step first sweeps the chunks (u & 127) of its
    rows, keeping only tags of rows u0 - SK .. u0 - 1 (u0 the step's first row), then looks up and
    tags its rows in order. Returns truth()'s mapping as the kernel would build it."""
    nt, chunk = tag_entries(d, K), sweep_chunk(d, K)
    tagpos = np.full(nt, 0xFFFF, np.uint16)
    out = {}
    for u0 in range(0, len(rows), TB):
        if sweep:
            for u in range(u0, u0 + TB):
                lo = (u & (SWEEP_ROWS - 1)) * chunk
                v = tagpos[lo:lo + chunk].astype(np.int64)        # (an empty slice past the table)
                dl = (u0 - (v >> 8)) & 255
                tagpos[lo:lo + chunk] = np.where((v != 0xFFFF) & (dl >= 1) & (dl <= SK), v, 0xFFFF)
        for u in range(u0, min(u0 + TB, len(rows))):
            _lookup(tagpos, u, rows[u], K, SK, out)
    return out


def model_spec(rows, d, SK=8, clear=True):
    """chain_sparse_spec's helper: steps of 8 rows; a step first clears the tags rows
    u - SR + 1 (u its rows) still own, whose slots the next rows reuse, then looks up and tags its
    rows in order. Every feature has a tag."""
    tagpos = np.full(d, 0xFFFF, np.uint16)
    out = {}
    for u0 in range(0, len(rows), SPEC_GROUP):
        last = min(u0 + SPEC_GROUP, len(rows))
        if clear:
            for u in range(u0, last):
                o = u - SPEC_SR + 1
                if o >= 0:
                    own = tagpos[rows[o]] == (((o & 255) << 8) | np.arange(len(rows[o])))
                    tagpos[rows[o][own]] = 0xFFFF
        for u in range(u0, last):
            _lookup(tagpos, u, rows[u], 0, SK, out)
    return out


# ------------------------------------------------------------------------------------------------
# The audit
# ------------------------------------------------------------------------------------------------
def required(c, SK):
    """What a case must cover at depth SK (the items of covered())."""
    kind = c["kind"]
    need = set()
    small = kind == "small"
    for k in (range(1, SK + 3) if small else distances(SK)):
        for res in range(TB):
            for reg in (("first", "middle", "late") if (k < 130 and not small) else ("any",)):
                need.add(("distance", k, res, reg))
    for k in list(range(1, SK + 1)) + ([] if small else list(range(257, 257 + SK))):
        need.update(("half", k, ha, hb) for ha in (False, True) for hb in (False, True))
    need.update(("head", k) for k in (1, SK, SK + 1))
    need.update(("probe", w) for w in ("K-1", "K", "d-1"))
    if c.get("brk"):
        need.update(("straddle", k) for k in range(2, SK + 3))
        need.add(("before-break",))
    if small:
        return need
    need.update({("hot", SK), ("ladder", SK), ("ladder1", SK), ("row0",), ("last-row",)})
    need.update(("chunk", ch) for ch in range(n_chunks(c["d"], c["head"])))
    need.update(("sweep", j, off) for j in range(1, SK + 1) for off in (-1, 0, 1))
    if kind == "main":
        for n in (0, 1, SK, SK + 1, SK + 2):
            need.add(("chain-rows", n))
            if n >= 2:
                need.add(("chain-last-row", n))
        need.update({("chain-multiple", SK), ("chain-multiple-last-row", SK)})
    if kind == "long":
        need.add(("chunk-over-256",))
    return need


def covered(c, data, SK, counted=None):
    """The items the case's hazards cover (those in `counted`, a set of hazard numbers, if given),
    after checking the construction itself: ascending columns, each probe at a and b and nowhere
    between, a tag of its own on row b, w0."""
    K, d = data["head"], data["d"]
    chunk = sweep_chunk(d, K)
    rows = chain_rows(data)
    trows, tcols = data["tags"]
    tag_at = dict(zip(trows.tolist(), tcols.tolist()))
    assert len(set(tcols.tolist())) == len(tcols) and np.all(data["w0"][tcols] == 0.0)
    for t in tcols.tolist():
        assert (data["col"] == t).sum() == 1
    for r in range(data["offs"][-1]):
        cc = row_cols(data, r)
        assert np.all(np.diff(cc) > 0) and len(cc) <= 128, r
        assert np.all(data["w0"][[f for f in cc.tolist() if f != tag_at.get(r)]] != 0.0), r
    got = set()
    hot = {}
    for p, rr in enumerate(rows):
        got.add(("chain-rows", len(rr)))
        if len(rr) and len(rr) % (SK + 1) == 0:
            got.add(("chain-multiple", SK))
    for q, h in enumerate(data["hazards"]):
        rr = rows[h["chain"]]
        a, b, k, f = h["a"], h["b"], h["k"], h["f"]
        assert b - a == k and rr[a][h["ea"]] == f and rr[b][h["eb"]] == f, h
        assert not any(f in rr[u] for u in range(a + 1, b)), h
        assert h["row_b"] in tag_at and trows[h["tag"]] == h["row_b"], h
        assert (f < K) == (h["zone"] == "head"), h
        if counted is not None and q not in counted:
            continue
        if h["kind"] == "hot" and b == a + 1:
            hot.setdefault(h["group"], []).append(a)
        if h["zone"] == "head":
            got.add(("head", k))
            if f == K - 1:
                got.add(("probe", "K-1"))
            continue
        got.update({("distance", k, b % TB, region(a)), ("distance", k, b % TB, "any"),
                    ("half", k, h["ea"] >= 64, h["eb"] >= 64), ("chunk", (f - K) // chunk)})
        if f in (K, d - 1):
            got.add(("probe", "K" if f == K else "d-1"))
        if a == 0:
            got.add(("row0",))
        if b == h["n"] - 1:
            got.update({("last-row",), ("chain-last-row", h["n"])})
            if h["n"] % (SK + 1) == 0:
                got.add(("chain-multiple-last-row", SK))
        if aliases(k, SK):
            for off in (-1, 0, 1):
                if (a & (SWEEP_ROWS - 1)) == ((f - K) // chunk + off) % SWEEP_ROWS:
                    got.add(("sweep", k - 256, off))
        if c.get("brk") and h["chain"] == c["brk"][0]:
            if a < c["brk"][1] < b:
                got.add(("straddle", k))
            if b == c["brk"][1] - 1:
                got.add(("before-break",))
    # runs: a feature in every row of >= 3 SK consecutive rows, all tagged; ladders of SK and SK + 1
    for g, starts in hot.items():
        if len(starts) + 1 >= 3 * SK:
            got.add(("hot", SK))
    by_f = {}
    for q, h in enumerate(data["hazards"]):
        if h["group"] is not None and (counted is None or q in counted):
            by_f.setdefault((h["chain"], h["f"]), []).append(h["k"])
    for ks in by_f.values():
        if ks.count(SK) >= 3:
            got.add(("ladder", SK))
        if ks.count(SK + 1) >= 2:
            got.add(("ladder1", SK))
    if chunk > 256:
        got.add(("chunk-over-256",))
    return got


def audit(c, data=None, counted=None):
    """The items case c covers at each of its depths; fails with the missing ones named."""
    data = data if data is not None else c["make"](c)
    out = {}
    for SK in c["sks"]:
        got = covered(c, data, SK, counted)
        missing = sorted(required(c, SK) - got, key=repr)
        assert not missing, f"{c['id']} at SK = {SK} does not cover {missing[:8]} ({len(missing)} items)"
        out[SK] = got
    return out


# ------------------------------------------------------------------------------------------------
# The two one-read mutations, in the float64 restatement
# ------------------------------------------------------------------------------------------------
class Reads:
    """tagged_rows.chain's `read` for one chain. Records, per hazard of the chain, what its
    mutations substitute (stale: w[f] from before row a's update; alias: what entry e_a of row
    b - k % 256 left in its slot, the new weight of the feature at that entry; SquaredL2: the
    kernels keep v of w = alpha v, so the value read at row b is the old v under row b's alpha, the
    old weight times the factors 1 - s lambda since) and row b's state; with mutate = (hazard
    number, "stale" | "alias") it makes that one read."""

    def __init__(self, data, p, c, mutate=None):
        self.data, self.mutate = data, mutate
        self.rows = chain_rows(data)[p]
        self.A = shrinks(len(self.rows), c["upd"], c["step"], c["reg"])
        self.at = {}
        self.rec = {}
        for q, h in enumerate(data["hazards"]):
            if h["chain"] != p:
                continue
            self.rec[q] = {}
            self.at.setdefault(h["a"], []).append((q, "stale", h["f"]))
            if aliases(h["k"]):
                r = h["b"] - h["k"] % 256
                g = int(self.rows[r][h["ea"]])
                assert g != h["f"]
                self.at.setdefault(r + 1, []).append((q, "alias", g))
            self.at.setdefault(h["b"], []).append((q, "b", h["f"]))

    def __call__(self, k, r, idx, wv, w):
        for q, what, f in self.at.get(k, ()):
            h = self.data["hazards"][q]
            if what != "b":
                self.rec[q][what] = float(w[f]) * between(self.A, k, h["b"])
                continue
            self.rec[q].update(z=float(row_vals(self.data, r).astype(wv.dtype) @ wv), w=float(w[f]), pos=k)
            if self.mutate and self.mutate[0] == q:
                wv = wv.copy()
                wv[h["eb"]] = wv.dtype.type(self.rec[q][self.mutate[1]])
        return wv


def _mult(grad, z, y):
    if grad == "least_squares":
        return z - y
    if grad == "logistic":
        return 1.0 / (1.0 + np.exp(-z)) - y
    ls = 2 * y - 1
    return -ls if 1.0 > ls * z else 0.0


def power(c, ref):
    """Per hazard, by how many units of its tag's scale each mutation moves row b's tag (float64;
    None where the mutation does not apply or the chain broke before row b): one pass of the restatement
    with Reads as observer; row b's margin with the substituted weight, its multiplier, and the
    tag it leaves, -s mult x_tag, times the later samples' SquaredL2 factors and the chain's share."""
    data = ref["data"]
    P = len(data["offs"]) - 1
    reads = {p: Reads(data, p, c) for p in range(P)}
    T.run(data, c["grad"], c["upd"], c["step"], c["reg"], 1, c["fraction"], ref["limits"], read=reads)
    scale = T.folded_scale(c, ref)
    trows, tcols = data["tags"]
    out = []
    for q, h in enumerate(data["hazards"]):
        rec = reads[h["chain"]].rec[q]
        res = dict(stale=None, alias=None)
        if "z" in rec:
            n_p = ref["limits"][h["chain"]]
            j = rec["pos"] + 1
            s = c["step"] / np.sqrt(float(j))
            later = np.prod([1.0 - c["step"] / np.sqrt(float(i)) * c["reg"] for i in range(j + 1, n_p + 1)]) \
                if c["upd"] == "squared_l2" else 1.0
            rb = h["row_b"]
            x = row_vals(data, rb)
            xt = float(x[list(row_cols(data, rb)).index(tcols[h["tag"]])])
            for m in ("stale", "alias"):
                if m in rec:
                    z2 = rec["z"] + float(x[h["eb"]]) * (rec[m] - rec["w"])
                    dm = _mult(c["grad"], z2, data["y"][rb]) - _mult(c["grad"], rec["z"], data["y"][rb])
                    res[m] = abs(s * dm * xt * later) * ref["share"][h["chain"]] / scale[h["tag"]]
        out.append(res)
    return out


def mutated(c, ref, q, mutation):
    """Units by which the tag of hazard q's row b is off the oracle when the float64 restatement
    makes that one wrong read (the whole run, nothing analytic)."""
    data = ref["data"]
    h = data["hazards"][q]
    w, _, _ = T.run(data, c["grad"], c["upd"], c["step"], c["reg"], 1, c["fraction"], ref["limits"],
                    read={h["chain"]: Reads(data, h["chain"], c, (q, mutation))})
    i = ref["idx"][h["tag"]]
    return abs(w[i] - ref["wr"][i]) / T.folded_scale(c, ref)[h["tag"]]


def counted(c, ref, bar):
    """(numbers of the hazards whose mutations all move row b's tag by more than 4 x bar, the
    weakest counted effect per mutation, power()'s list). A hazard whose row b comes after a
    per-sample break has nothing to move: its tag is held to exactly 0.0, and it counts."""
    pw = power(c, ref)
    ok = {q for q, r in enumerate(pw) if r["stale"] is None or
          (r["stale"] > 4 * bar and (r["alias"] is None or r["alias"] > 4 * bar))}
    weakest = {m: min((pw[q][m] for q in ok if pw[q][m] is not None), default=None) for m in ("stale", "alias")}
    return ok, weakest, pw


def describe_hazards(ref, t):
    """The hazards read out by tag number t, for a failure message."""
    hs = [h for h in ref["data"]["hazards"] if h["tag"] == t]
    return "; ".join(f"hazard {h['kind']}: chain {h['chain']} positions {h['a']} -> {h['b']} (distance {h['k']}), "
                     f"feature {h['f']} (head {ref['data']['head']}), entries {h['ea']} -> {h['eb']}" for h in hs) \
        or "no hazard ends at this row"


# ------------------------------------------------------------------------------------------------
# The cases
# ------------------------------------------------------------------------------------------------
_DATA = {}


def _make(c):
    key = (c["kind"], c["seed"], tuple(c["sizes"]), c["d"], c["head"], c["compute"], c["fraction"], c.get("brk"))
    if key not in _DATA:
        _DATA[key] = generate(c["kind"], c["seed"], c["sizes"], c["d"], c["head"],
                              np.float32 if c["compute"] == "f32" else np.float64, c["fraction"], c.get("brk"))
    base = _DATA[key]
    return labels(dict(base), c["seed"], c["grad"], c["upd"], c["step"], c["reg"], LABEL_GAP[c["compute"]])


def _cases():
    C = []

    def add(id, **kw):
        base = dict(id=id, layout="csr", family="reuse", compute="f32", reg=0.0, fraction=1.0, tol=0.0, iters=1,
                    env={}, K=2, storage=np.float32, budget=None, nv=0, make=_make, kind="main", sks=SKS,
                    d=2000, head=400, sizes=[9, LONG] + [n for n in SHORT if n != 9], seed=900, required=True,
                    kernels="all", grad="least_squares", upd="simple", step=0.5)
        base.update(kw)
        C.append(base)

    for compute in ("f32", "f64"):
        f = dict(compute=compute)
        add(f"main-{compute}-least_squares-simple", **f)
        add(f"main-{compute}-least_squares-squared_l2", upd="squared_l2", reg=0.05, **f)
        add(f"main-{compute}-logistic-simple", grad="logistic", step=1.0, required=False, **f)
        # the per-sample break: chain 0 stops at its row 37 (no multiple of SK + 1), chain 1 runs through
        add(f"break-{compute}", kind="small", sizes=[90, 61], brk=(0, 37), tol=1e-4, seed=910,
            kernels="break", sks=(4,), **f)
        add(f"sampled-{compute}", kind="small", sizes=[260, 181], fraction=0.5, seed=920, **f)
    add("main-f32-hinge-simple", grad="hinge", required=False)
    # chain_general on CSR rows: SquaredL2 with 1 - s lambda = 0 at the first sample (as general-csr)
    # (factors 1 - 1 / sqrt(j) shrink the early rows' tags to nothing: only the hazards that pass count)
    add("general-f64", compute="f64", upd="squared_l2", step=1.0, reg=1.0, kernels="general", sks=(4,), required=False)
    # the sweep's path for tables of more than 32,768 tags (chunk 512): fp64 at rcv1's d with its
    # natural head, fp32 with a head of 1,000 features forced on d = 40,000
    add("wide-f64", compute="f64", kind="long", sizes=[LONG], d=47_236, head=lds_head(47_236, 4, "f64"), seed=930,
        kernels="wide", sks=(4,))
    add("wide-f32", kind="long", sizes=[LONG], d=40_000, head=1000, seed=931, kernels="wide", sks=(4,))
    return C


CASES = _cases()
CASE_IDS = [c["id"] for c in CASES]


def build(pkg, c):
    """tagged_rows.build's reference for the case; the break row's tag joins the exact zeros (its
    update is -s * 0 * x)."""
    fresh = c["id"] not in T._BUILT
    ref = T.build(pkg, c)
    if fresh and ref["data"]["brk_row"] is not None:
        t = int(np.flatnonzero(ref["data"]["tags"][0] == ref["data"]["brk_row"])[0])
        ref["zero"] = ref["zero"] | (ref["which"] == t)
    return ref


def gpu_cases():
    """(case with the kernel's environment, expected variant, name) for tests/test_gpu_sparse_reuse.py.
    fp32: every kernel of test_gpu_sparse.KERNELS, fp64: of KERNELS64, the head named by the case."""
    f32 = {"lds": (600, {"PSGD_SPARSE_KERNEL": "lds"}, None),
           "lds_tail": (600, {"PSGD_SPARSE_KERNEL": "lds"}, 4),
           "lds_tail_sk8": (610, {"PSGD_SPARSE_KERNEL": "lds", "PSGD_SPARSE_SK": "8"}, 8),
           "spec": (410, {"PSGD_SPARSE_KERNEL": "spec"}, None),
           "plain": (400, {"PSGD_SPARSE_KERNEL": "plain"}, None)}
    f64 = {"lds64": (620, {}, None), "lds64_tail": (620, {}, 4), "lds64_tail_sk8": (630, {"PSGD_SPARSE_SK": "8"}, 8),
           "hbm64": (420, {"PSGD_SPARSE_KERNEL": "hbm64"}, None)}
    out = []
    for c in CASES:
        table = f32 if c["compute"] == "f32" else f64
        store = 1 if c["compute"] == "f32" else 0
        names = {"all": sorted(table), "wide": ["lds_tail" if store else "lds64_tail"], "general": [None],
                 "break": (["lds", "lds_tail", "plain"] if store else ["lds64", "lds64_tail"])}[c["kernels"]]
        for name in names:
            if name is None:
                out.append((c, 201, c["id"]))
                continue
            base, env, sk = table[name]
            env = dict(env)
            if sk:
                env["PSGD_SPARSE_LDS_HEAD"] = str(c["head"])
            out.append((dict(c, env=env), base + (40 if c["tol"] > 0 else 0) + store, f"{c['id']}-{name}"))
    return out


# ------------------------------------------------------------------------------------------------
# The profile
# ------------------------------------------------------------------------------------------------
def load_profile():
    with open(PROFILE) as f:
        return json.load(f)


def cpu_section(pkg):
    bar, bar64 = T.bars()
    cases = {}
    for c in CASES:
        ref = build(pkg, c)
        ok, weakest, pw = counted(c, ref, bar if c["compute"] == "f32" else bar64)
        cases[c["id"]] = dict(S=T.cpu_statistics(pkg, c), hazards=len(pw), counted=len(ok), weakest=weakest)
    return dict(cases=cases)


def write_cpu_profile(pkg):
    prof = load_profile() if os.path.exists(PROFILE) else {}
    prof["what"] = ("Per case of tests/reuse_schedule.py: S = max over tag coordinates of |w - w_oracle| / tag_scale "
                    "of the numpy restatements in the case's compute precision (both dot orders) against the fp64 "
                    "oracle; the hazards whose stale and alias mutations both move row b's tag by more than 4 x "
                    "the bar of profiles/row_coefficients.json (BAR, fp64: BAR64), and the weakest such effect in "
                    "units of the tag's scale. 'device': what the kernels gave on an MI355X, per test case.")
    prof["cpu"] = cpu_section(pkg)
    prof.setdefault("device", {})
    with open(PROFILE, "w") as f:
        json.dump(prof, f, indent=1, sort_keys=True)
    return prof


if __name__ == "__main__":
    sys.path.insert(0, T.ROOT)
    import __graft_entry__ as g
    p = write_cpu_profile(g.load_package())
    for k, v in p["cpu"]["cases"].items():
        print(k, v)
