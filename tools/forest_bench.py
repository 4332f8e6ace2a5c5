#!/usr/bin/env python3
"""Time the random forest's histogram pass on device-resident data beside the single tree's only route to the same
node counts, alternating call by call in one process (diagnostic tool). Rows: c2's (10M x 512 f32 in 256
partitions), K = 2, maxBins = 32, 20 trees, "sqrt" (m = 23), Poisson(1) bags.

  forest_hist level 0       psgd_forest_histogram_device over the 20 roots (A = 20);
  forest_hist level 4       ... over 16 open nodes a tree (A = 320), the rows of a tree spread evenly over them;
  20 x tree_hist A=1 / 16   psgd_tree_histogram_device called 20 times at the same depth's frontier: all 512
                            features, no bag weight -- that route cannot bag, it is the yardstick for time alone;
  trainClassifier           RandomForest.trainClassifier, 20 trees of depth 5, host clock around a synchronise.

HIP events around each call; a round times every call once, so the calls alternate; median and min of --reps
rounds after --warmup. One JSON line per measurement, then the ratios.

usage: python tools/forest_bench.py [--rows N] [--reps K] [--train-reps K]
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


def main():
    from kmeans_bench import alternate
    from project_bench import report
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--train-reps", type=int, default=5)
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20")

    import numpy as np
    import torch
    import __graft_entry__ as g
    import bench as B
    pkg = g.load_package()
    dev = torch.device("cuda", 0)
    n, d, P, K, MB, T, seed = a.rows, 512, 256, 2, 32, 20, 7
    X, y, offs = B.make_shard(torch, dev, n, d, P, "logistic", "f32", 7)
    offs = [int(v) for v in offs]
    data = pkg.PartitionedData([pkg.DevicePartition(y[s:e], X[s:e], d) for s, e in zip(offs[:-1], offs[1:])])
    engine = pkg.HipEngine(data)
    st, ctx = engine.stream, engine.ctx
    thr, nbins = pkg.find_splits(data, MB, seed=1, engine=engine)
    bins = engine.tree_bin(thr, nbins)
    m, cut = pkg.forest_subset_size("sqrt", d, T), pkg.forest_cut(T, 1.0)
    torch.cuda.synchronize()
    print(f"rows ready: {n} x {d}; m = {m}", file=sys.stderr, flush=True)

    rows = torch.arange(n, device=dev, dtype=torch.int32)
    level = {}
    for depth, per in ((0, 1), (4, 16)):
        slots = torch.stack([(rows * 7 + t) % per for t in range(T)]).contiguous()
        flat = [(t, per + s) for t in range(T) for s in range(per)]          # MLlib ids of a full level
        sub = np.stack([pkg.forest_subset(seed, t, nid, d, m) for t, nid in flat])
        fr = engine.forest_frontier(np.repeat(np.arange(T), per), np.arange(T + 1) * per, sub)
        level[depth] = (slots, fr, T * per, pkg._native.forest_plan(d, MB, K, m, T * per, T, -(-n // 256), n))
        print(f"level {depth}: plan {level[depth][3]}", file=sys.stderr, flush=True)
    tslots = {A: (rows % A).contiguous() for A in (1, 16)}
    hist = torch.zeros(1 + 320 * d * MB * K, dtype=torch.int64, device=dev)

    def forest_call(depth):
        slots, fr, A, _ = level[depth]
        return lambda: ctx.forest_histogram_device(bins.bins.data_ptr(), bins.labels.data_ptr(), slots.data_ptr(), T,
                                                   fr.node_tree.data_ptr(), fr.tree_base.data_ptr(), fr.sub.data_ptr(), A, m,
                                                   K, MB, 0, A, seed, cut, 0, 0, hist.data_ptr() + 8, hist.data_ptr(),
                                                   st.cuda_stream)

    def tree_calls(A):
        def run():
            for _ in range(T):
                ctx.tree_histogram_device(bins.bins.data_ptr(), bins.labels.data_ptr(), tslots[A].data_ptr(), K, MB, 0, A, 0,
                                          hist.data_ptr() + 8, hist.data_ptr(), st.cuda_stream)
        return run

    calls = [("forest_hist level 0", st, forest_call(0)), ("20 x tree_hist A=1", st, tree_calls(1)),
             ("forest_hist level 4", st, forest_call(4)), ("20 x tree_hist A=16", st, tree_calls(16))]
    ms = alternate(torch, calls, a.reps, a.warmup)

    # the weighted rows a level adds: sum over trees and rows of [w > 0] (one LDS add a subset feature each)
    w = engine.forest_bag(seed, cut, (0, T))
    active = int((w > 0).sum().item())
    del w
    med = {}
    for name in ms:
        mm = statistics.median(ms[name])
        extra = {"rows": n, "features": d, "K": K, "maxBins": MB, "trees": T}
        if name.startswith("forest_hist"):
            depth = int(name[-1])
            plan = level[depth][3]
            subgroups = -(-level[depth][2] // plan["node_subgroup"])
            extra.update({"m": m, "nodes": level[depth][2], "node_subgroup": plan["node_subgroup"], "lds_bytes": plan["lds_bytes"],
                          "G_lds_adds_per_s_median": round(active * m / mm / 1e6, 1),
                          "TBps_binned_rows_median": round(subgroups * n * d / mm / 1e9, 3)})
        else:
            extra.update({"G_lds_adds_per_s_median": round(T * n * d / mm / 1e6, 1),
                          "TBps_binned_rows_median": round(T * n * d / mm / 1e9, 3)})
        med[name] = report("c2", name, ms[name], extra)

    train_s = []
    for r in range(a.train_reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        model = pkg.RandomForest.trainClassifier(data, K, {}, T, "sqrt", maxDepth=5, maxBins=MB, seed=1, engine=engine)
        torch.cuda.synchronize()
        if r:
            train_s.append((time.perf_counter() - t0) * 1e3)
    report("c2", "RandomForest.trainClassifier 20 trees depth 5", train_s, {"rows": n, "nodes": model.totalNumNodes})
    print(json.dumps({"shape": "c2", "note": "the tree_hist route cannot bag and counts all 512 features",
                      "level0_forest_over_20_tree_hist": {"of_medians": round(med["forest_hist level 0"] / med["20 x tree_hist A=1"], 4),
                                                          "of_minima": round(min(ms["forest_hist level 0"]) / min(ms["20 x tree_hist A=1"]), 4)},
                      "level4_forest_over_20_tree_hist": {"of_medians": round(med["forest_hist level 4"] / med["20 x tree_hist A=16"], 4),
                                                          "of_minima": round(min(ms["forest_hist level 4"]) / min(ms["20 x tree_hist A=16"]), 4)}}),
          flush=True)


if __name__ == "__main__":
    main()
