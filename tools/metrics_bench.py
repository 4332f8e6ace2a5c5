#!/usr/bin/env python3
"""Time psgd_binary_counts_device on device-resident scores at c2's row count (diagnostic tool):
10M scores with labels of score-dependent odds, three inputs --

  distinct  standard normals (every score a group of its own; the sort's eight passes are live);
  seven     seven distinct values (heavy ties; most digit passes are skipped on the device);
  equal     one value (every pass is skipped).

In the same session, alternating with it rep by rep: torch.sort of the same scores alone (the tuned
library sort a torch-built pipeline would start from -- values and indices, no labels, no table, no
areas), and psgd_evaluate_device at c2 (10M x 512 f32 rows in 256 partitions: score_dense, the pass
that produces such scores). HIP events around each call after a warm-up; one JSON line per input
with median and min milliseconds, and one for the scoring pass.

usage: python tools/metrics_bench.py [--n N] [--reps K] [--warmup W] [--no-score]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(torch, st, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    fn()
    e1.record(st)
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-score", action="store_true", help="skip the c2 scoring pass (20 GB of rows)")
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20")

    import torch
    import __graft_entry__ as g
    pkg = g.load_package()
    from spark_parallelized_sgd_amd.optimization import get_context
    dev = torch.device("cuda", 0)
    ctx = get_context(0)
    st = torch.cuda.Stream(device=dev)
    n = a.n
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    normals = torch.randn(n, dtype=torch.float64, device=dev, generator=gen)
    inputs = {
        "distinct": normals,
        "seven": torch.randint(-3, 4, (n,), device=dev, generator=gen).to(torch.float64),
        "equal": torch.full((n,), 0.75, dtype=torch.float64, device=dev),
    }
    thr = torch.empty(n, dtype=torch.float64, device=dev)
    cp = torch.empty(n, dtype=torch.int64, device=dev)
    cn = torch.empty(n, dtype=torch.int64, device=dev)
    small = torch.zeros(6, dtype=torch.int64, device=dev)
    for name, s in inputs.items():
        y = (torch.rand(n, dtype=torch.float64, device=dev, generator=gen) < torch.sigmoid(s)).to(torch.float64)
        torch.cuda.synchronize()
        ours, areas_only, lib = [], [], []
        with torch.cuda.stream(st):
            for k in range(a.warmup + a.reps):
                t0 = timed(torch, st, lambda: ctx.binary_counts_device(
                    s.data_ptr(), y.data_ptr(), n, thr.data_ptr(), cp.data_ptr(), cn.data_ptr(), small.data_ptr(),
                    small.data_ptr() + 32, st.cuda_stream))
                t1 = timed(torch, st, lambda: ctx.binary_counts_device(
                    s.data_ptr(), y.data_ptr(), n, None, None, None, small.data_ptr(), small.data_ptr() + 32,
                    st.cuda_stream))
                t2 = timed(torch, st, lambda: torch.sort(s, descending=True))
                if k >= a.warmup:
                    ours.append(t0)
                    areas_only.append(t1)
                    lib.append(t2)
            h = small.cpu().numpy()
        med = statistics.median
        print(json.dumps({"input": name, "n": n, "reps": len(ours),
                          "binary_counts_ms_median": round(med(ours), 4), "binary_counts_ms_min": round(min(ours), 4),
                          "areas_only_ms_median": round(med(areas_only), 4), "areas_only_ms_min": round(min(areas_only), 4),
                          "torch_sort_ms_median": round(med(lib), 4), "torch_sort_ms_min": round(min(lib), 4),
                          "binary_counts_over_torch_sort": round(med(ours) / med(lib), 3),
                          "G": int(h[0]), "P": int(h[1]), "N": int(h[2]),
                          "areaUnderROC": float(h[4:].view("float64")[0]),
                          "areaUnderPR": float(h[4:].view("float64")[1])}), flush=True)
    del inputs, normals, thr, cp, cn
    torch.cuda.empty_cache()
    if a.no_score:
        return

    import bench as B
    rows, d, P = n, 512, 256
    X, y, offs = B.make_shard(torch, dev, rows, d, P, "least_squares", "f32", 7)
    parts = [pkg.DevicePartition(y[s:e], X[s:e], d) for s, e in zip(offs[:-1], offs[1:])]
    engine = pkg.HipEngine(pkg.PartitionedData(parts))
    w = torch.randn(d, dtype=torch.float64, device=dev) / d ** 0.5
    out = torch.zeros(3 + 2 * P, dtype=torch.float64, device=dev)
    est = engine.stream
    torch.cuda.synchronize()
    ms = []
    with torch.cuda.stream(est):
        for k in range(a.warmup + a.reps):
            t = timed(torch, est, lambda: engine.ctx.evaluate_device(1, w.data_ptr(), out.data_ptr(),
                                                                     out.data_ptr() + 24, est.cuda_stream))
            if k >= a.warmup:
                ms.append(t)
    print(json.dumps({"shape": "c2", "kernel": "score_dense", "rows": rows, "features": d, "partitions": P,
                      "reps": len(ms), "ms_median": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4)}),
          flush=True)


if __name__ == "__main__":
    main()
