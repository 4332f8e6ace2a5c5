#!/usr/bin/env python3
"""Time psgd_column_stats_device on device-resident data at the flagship shapes, and
psgd_transform_columns_device at c2 (diagnostic tool):

  c2: 10M x 512 f32 dense rows in 256 partitions;
  c4: 20M rcv1-like CSR rows, 47,236 features, 94 non-zeros, f32 values, 256 partitions.

HIP events around each call after a warm-up; prints one JSON line per shape: median and min
milliseconds, ns per row, and the bytes of the rows (dense: n * ld * sizeof; CSR: col + val +
row_ptr, read once per pass -- the CSR statistics make two passes, and `atomic_GBps_median` is
their atomic traffic: per non-zero 16 bytes in pass 1 (fp64 sum + 64-bit count) and 8 in pass 2)
divided by the time. The yardstick to run in the same session is tools/eval_bench.py: score_dense /
score_csr read the same rows once.

--transform adds the in-place transform at the c2 shape (it reads and writes the rows: 2 x the
row bytes). The transform refuses zero-copy partitions, so these rows are registered from the host:
every partition from one shared zero-filled host block (the values do not matter to the time, and a
factor of 1.0 without and with a zero shift leaves them as they are from repetition to repetition).

usage: python tools/colstats_bench.py [--shape c2|c4|both] [--rows N] [--partitions P] [--reps K] [--transform]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {
    # name: (rows, features, partitions, nnz (0: dense))
    "c2": (10_000_000, 512, 256, 0),
    "c4": (20_000_000, 47_236, 256, 94),
}


def timed(torch, st, reps, warmup, call):
    ms = []
    with torch.cuda.stream(st):
        for k in range(warmup + reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            call()
            e1.record(st)
            e1.synchronize()
            if k >= warmup:
                ms.append(e0.elapsed_time(e1))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="both", choices=["c2", "c4", "both"])
    ap.add_argument("--rows", type=int, default=0, help="rows instead of the shape's own (smaller boxes)")
    ap.add_argument("--partitions", type=int, default=0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--transform", action="store_true", help="also time the transform at the c2 shape")
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20")

    import numpy as np
    import torch
    import __graft_entry__ as g
    import bench as B
    pkg = g.load_package()
    dev = torch.device("cuda", 0)

    for name in (["c2", "c4"] if a.shape == "both" else [a.shape]):
        n, d, P, nnz = SHAPES[name]
        n, P = a.rows or n, a.partitions or P
        if nnz:
            row_ptr, col, val, y, offs = B.make_csr_shard(torch, dev, n, d, P, "logistic", "f32", 7, nnz)
            parts = [pkg.DeviceCsrPartition(y[s:e], row_ptr[s:e + 1], col, val, d) for s, e in zip(offs[:-1], offs[1:])]
            nbytes, passes = n * nnz * 8 + (n + P) * 8, 2
        else:
            X, y, offs = B.make_shard(torch, dev, n, d, P, "least_squares", "f32", 7)
            parts = [pkg.DevicePartition(y[s:e], X[s:e], d) for s, e in zip(offs[:-1], offs[1:])]
            nbytes, passes = n * d * 4, 1
        engine = pkg.HipEngine(pkg.PartitionedData(parts))
        out = torch.zeros(1 + 5 * d, dtype=torch.float64, device=dev)
        st = engine.stream
        torch.cuda.synchronize()
        ms = timed(torch, st, a.reps, a.warmup,
                   lambda: engine.ctx.column_stats_device(out.data_ptr(), st.cuda_stream))
        h = out.cpu().numpy()
        med, lo = statistics.median(ms), min(ms)
        line = {"shape": name, "call": "column_stats", "rows": n, "features": d, "partitions": P, "nnz": nnz,
                "reps": len(ms), "ms_median": round(med, 4), "ms_min": round(lo, 4),
                "ns_per_row_median": round(med * 1e6 / n, 3), "row_bytes": nbytes, "passes": passes,
                "GBps_median": round(passes * nbytes / med / 1e6, 1), "GBps_best": round(passes * nbytes / lo / 1e6, 1),
                "count": int(h[0]), "mean0": float(h[1]), "m2_0": float(h[1 + d])}
        if nnz:
            line["atomic_GBps_median"] = round(n * nnz * 24 / med / 1e6, 1)
        print(json.dumps(line), flush=True)
        del engine, parts
        torch.cuda.empty_cache()

    if a.transform:
        n, d, P, _ = SHAPES["c2"]
        n, P = a.rows or n, a.partitions or P
        rows = -(-n // P)
        block = np.zeros((rows, d), dtype=np.float32)
        labels = np.zeros(rows)
        data = pkg.PartitionedData([pkg.DensePartition(labels, block) for _ in range(P)])
        engine = pkg.HipEngine(data)
        st = engine.stream
        factor = torch.ones(d, dtype=torch.float64, device=dev)
        shift = torch.zeros(d, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        nbytes = rows * P * d * 4
        for what, s_ptr in (("transform factor", None), ("transform shift+factor", shift.data_ptr())):
            ms = timed(torch, st, a.reps, a.warmup,
                       lambda: engine.ctx.transform_columns_device(s_ptr, factor.data_ptr(), st.cuda_stream))
            med, lo = statistics.median(ms), min(ms)
            print(json.dumps({"shape": "c2", "call": what, "rows": rows * P, "features": d, "partitions": P,
                              "reps": len(ms), "ms_median": round(med, 4), "ms_min": round(lo, 4),
                              "row_bytes": nbytes, "GBps_median": round(2 * nbytes / med / 1e6, 1),
                              "GBps_best": round(2 * nbytes / lo / 1e6, 1)}), flush=True)


if __name__ == "__main__":
    main()
