#!/usr/bin/env python3
"""Time the decision tree's passes on device-resident data, beside their yardsticks in the same process,
alternating call by call (diagnostic tool). Rows: c2's (10M x 512 f32 in 256 partitions), K = 2, maxBins = 32.

  tree_bin                  psgd_tree_bin_device: f32 rows in, one byte a feature out;
  tree_hist A=1, 16, 64     psgd_tree_histogram_device at the root and over frontiers of 16 and 64 slots (rows spread
    r=1 / r=2               evenly), with one copy of the LDS sub-table / two by row parity (two halve the feature
                            chunk here);
  tree_best_split A=64      psgd_tree_best_split_device over 64 slots;
  score_dense               psgd_evaluate_device, the f32 row stream: the histogram pass reads a quarter of its bytes;
  torch level A=1           torch.bincount over (feature, bin, label) indices made from the binned uint8 tensor,
                            in chunks of 2^20 rows: the library path materialises an int64 index tensor;
  trainClassifier depth 5   the whole call (find_splits, binning, six levels), host clock around a synchronise;
  torch six levels          the torch level at frontiers of 1, 2, 4, 8, 16, 32 slots and nothing else (no splits,
                            no routing): less than a torch restatement of the training would take.

HIP events around each call; a round times every call once, so the calls alternate; median and min of --reps
rounds after --warmup, the torch yardsticks and the training included. One JSON line per measurement.

usage: python tools/tree_bench.py [--rows N] [--reps K] [--no-torch]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def regression(pkg, torch, engine, bins, slots, n, d, MB, a):
    """--regression: the target pass (range and targets over a caller's float64 labels), the moments pass, the
    regression histogram at the root and over a 16-slot frontier, and the classifier's tree_hist at K = 2 on the
    same binned rows and slots (the same table shape: 2 x 64 bits a bin); alternating, one process."""
    from kmeans_bench import alternate
    from project_bench import report
    st, ctx, dev = engine.stream, engine.ctx, engine.dev
    y = torch.randn(n, dtype=torch.float64, device=dev) * 3.0 - 1.0
    t = engine.tree_targets(y)
    rng = torch.zeros(3, dtype=torch.int64, device=dev)
    mom = torch.zeros(16 * 4, dtype=torch.int64, device=dev)
    hist = torch.zeros(1 + 16 * d * MB * 2, dtype=torch.int64, device=dev)

    def targets():
        ctx.tree_label_range_device(y.data_ptr(), rng.data_ptr(), st.cuda_stream)
        ctx.tree_targets_device(y.data_ptr(), t.ymin, t.s, t.q.data_ptr(), st.cuda_stream)

    calls = [("tree_targets (range + targets)", st, targets)]
    for A in (1, 16):
        calls += [(f"tree_moments A={A}", st, lambda A=A: ctx.tree_moments_device(
                      t.q.data_ptr(), slots[A].data_ptr(), 0, A, mom.data_ptr(), st.cuda_stream)),
                  (f"tree_hist_reg A={A}", st, lambda A=A: ctx.tree_histogram_reg_device(
                      bins.bins.data_ptr(), t.q.data_ptr(), slots[A].data_ptr(), MB, 0, A, 0, hist.data_ptr() + 8, st.cuda_stream)),
                  (f"tree_hist K=2 A={A}", st, lambda A=A: ctx.tree_histogram_device(
                      bins.bins.data_ptr(), bins.labels.data_ptr(), slots[A].data_ptr(), 2, MB, 0, A, 0, hist.data_ptr() + 8,
                      hist.data_ptr(), st.cuda_stream))]
    ms = alternate(torch, calls, a.reps, a.warmup)
    med = {name: report("c2", name, ms[name], {"rows": n, "features": d, "maxBins": MB}) for name in ms}
    print(json.dumps({"shape": "c2", **{f"hist_reg_over_hist_K2_A{A}": round(med[f"tree_hist_reg A={A}"] / med[f"tree_hist K=2 A={A}"], 3)
                                        for A in (1, 16)}}), flush=True)


def main():
    from kmeans_bench import alternate
    from project_bench import report
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--regression", action="store_true",
                    help="time the regression passes beside the classifier's tree_hist at K = 2 on the same binned rows")
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20")

    import numpy as np
    import torch
    import __graft_entry__ as g
    import bench as B
    pkg = g.load_package()
    dev = torch.device("cuda", 0)
    n, d, P, K, MB = a.rows, 512, 256, 2, 32
    X, y, offs = B.make_shard(torch, dev, n, d, P, "logistic", "f32", 7)
    offs = [int(v) for v in offs]
    data = pkg.PartitionedData([pkg.DevicePartition(y[s:e], X[s:e], d) for s, e in zip(offs[:-1], offs[1:])])
    engine = pkg.HipEngine(data)
    st, cur, ctx = engine.stream, torch.cuda.current_stream(dev), engine.ctx
    thr, nbins = pkg.find_splits(data, MB, seed=1, engine=engine)
    bins = engine.tree_bin(thr, nbins)
    pitch = bins.bins.shape[1]
    torch.cuda.synchronize()
    print(f"rows ready: {n} x {d}; bins per feature {int(nbins.min())} .. {int(nbins.max())}", file=sys.stderr, flush=True)

    slots = {A: (torch.arange(n, device=dev, dtype=torch.int32) % A).contiguous() for A in (1, 2, 4, 8, 16, 32, 64)}
    if a.regression:
        return regression(pkg, torch, engine, bins, slots, n, d, MB, a)
    hist = torch.zeros(1 + 64 * d * MB * K, dtype=torch.int64, device=dev)
    rec = torch.zeros(64 * (6 + 2 * K), dtype=torch.float64, device=dev)
    w = torch.randn(d, dtype=torch.float64, device=dev) / d ** 0.5
    out3 = torch.zeros(3, dtype=torch.float64, device=dev)

    def hist_call(A, repl):
        return lambda: ctx.tree_histogram_device(bins.bins.data_ptr(), bins.labels.data_ptr(), slots[A].data_ptr(), K, MB, 0, A,
                                                 repl, hist.data_ptr() + 8, hist.data_ptr(), st.cuda_stream)

    calls = [("tree_bin", st, lambda: ctx.tree_bin_device(thr, nbins, MB, bins.thresholds.data_ptr(), bins.nbins.data_ptr(),
                                                          bins.bins.data_ptr(), bins.labels.data_ptr(), st.cuda_stream)),
             *[(f"tree_hist A={A} r={r}", st, hist_call(A, r)) for A in (1, 16, 64) for r in (1, 2)],
             ("tree_best_split A=64", st, lambda: ctx.tree_best_split_device(
                 hist.data_ptr() + 8, bins.thresholds.data_ptr(), bins.nbins.data_ptr(), d, MB, K, 64, 0, 1, 0.0, rec.data_ptr(),
                 st.cuda_stream)),
             ("score_dense (evaluate)", st, lambda: ctx.evaluate_device(1, w.data_ptr(), out3.data_ptr(), None, st.cuda_stream))]
    ms = alternate(torch, calls, a.reps, a.warmup)

    base = (torch.arange(d, device=dev, dtype=torch.int64) * (MB * K))[None, :]
    chunk = 1 << 20

    def torch_level(A):
        H = torch.zeros(A * d * MB * K, dtype=torch.int64, device=dev)
        for s in range(0, n, chunk):
            idx = bins.bins[s:s + chunk, :d].to(torch.int64) * K + base
            idx += (slots[A][s:s + chunk].to(torch.int64) * (d * MB * K) + bins.labels[s:s + chunk].to(torch.int64))[:, None]
            H += torch.bincount(idx.view(-1), minlength=H.numel())
        return H

    if not a.no_torch:
        ctx.tree_histogram_device(bins.bins.data_ptr(), bins.labels.data_ptr(), slots[1].data_ptr(), K, MB, 0, 1, 0,
                                  hist.data_ptr() + 8, hist.data_ptr(), st.cuda_stream)
        st.synchronize()
        assert torch.equal(torch_level(1), hist[1: 1 + d * MB * K]), "the torch level and tree_hist disagree"
        tcalls = [("torch level A=1", cur, lambda: torch_level(1)),
                  ("torch six levels", cur, lambda: [torch_level(A) for A in (1, 2, 4, 8, 16, 32)])]
        ms.update(alternate(torch, tcalls, a.reps, 1))
        calls += tcalls

    train_s = []
    for r in range(a.reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        model = pkg.DecisionTree.trainClassifier(data, K, maxDepth=5, maxBins=MB, seed=1, engine=engine)
        torch.cuda.synchronize()
        if r:
            train_s.append((time.perf_counter() - t0) * 1e3)
    ms["trainClassifier depth 5"] = train_s

    med = {}
    for name in ms:
        m = statistics.median(ms[name])
        extra = {"rows": n, "features": d, "K": K, "maxBins": MB}
        if name.startswith("tree_hist"):
            extra["TBps_binned_rows_median"] = round(n * pitch / m / 1e9, 3)
            extra["G_lds_adds_per_s_median"] = round(n * d / m / 1e6, 1)
        elif name.startswith("score_dense"):
            extra["TBps_rows_median"] = round(n * d * 4 / m / 1e9, 3)
        elif name == "tree_bin":
            extra["TBps_rows_plus_bins_median"] = round(n * (d * 4 + pitch) / m / 1e9, 3)
        elif name.startswith("trainClassifier"):
            extra.update({"nodes": model.numNodes, "depth": model.depth})
        med[name] = report("c2", name, ms[name], extra)
    line = {"shape": "c2", "root_hist_over_score_dense": round(med["tree_hist A=1 r=1"] / med["score_dense (evaluate)"], 3),
            **{f"hist_A{A}_r2_over_r1": round(med[f"tree_hist A={A} r=2"] / med[f"tree_hist A={A} r=1"], 3) for A in (1, 16, 64)}}
    if not a.no_torch:
        line["root_hist_over_torch_level"] = round(min(med["tree_hist A=1 r=1"], med["tree_hist A=1 r=2"]) / med["torch level A=1"], 4)
        line["train_over_torch_six_levels"] = round(med["trainClassifier depth 5"] / med["torch six levels"], 4)
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
