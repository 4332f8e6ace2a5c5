#!/usr/bin/env python3
"""Time psgd_evaluate_device on device-resident data at the flagship shapes (diagnostic tool):

  c2: 10M x 512 f32 dense rows in 256 partitions (LeastSquares), the row stream of chain_block;
  c4: 20M rcv1-like CSR rows, 47,236 features, 94 non-zeros, f32 values, 256 partitions (Logistic).

HIP events around each call after a warm-up; prints one JSON line per shape: median and min
milliseconds, ns per row, and the bytes of the rows (dense: n * ld * sizeof; CSR: col + val +
row_ptr; plus the labels) divided by the time. Yardsticks to run in the same session:
tools/stream_bench plain at the same row bytes and partition count (the read ceiling, no
arithmetic), python bench.py (chain_block's c2 kernel time), tools/gather_bench at the table size.

usage: python tools/eval_bench.py [--shape c2|c4|both] [--rows N] [--partitions P] [--reps K]
                                  [--gradient logistic|least_squares|hinge]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {
    # name: (rows, features, partitions, nnz (0: dense), gradient)
    "c2": (10_000_000, 512, 256, 0, "least_squares"),
    "c4": (20_000_000, 47_236, 256, 94, "logistic"),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="both", choices=["c2", "c4", "both"])
    ap.add_argument("--rows", type=int, default=0, help="rows instead of the shape's own (smaller boxes)")
    ap.add_argument("--partitions", type=int, default=0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--gradient", default="", choices=["", "logistic", "least_squares", "hinge"])
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20")

    import torch
    import __graft_entry__ as g
    import bench as B
    pkg = g.load_package()
    dev = torch.device("cuda", 0)
    kinds = {"logistic": 0, "least_squares": 1, "hinge": 2}

    for name in (["c2", "c4"] if a.shape == "both" else [a.shape]):
        n, d, P, nnz, grad = SHAPES[name]
        n, P, grad = a.rows or n, a.partitions or P, a.gradient or grad
        if nnz:
            row_ptr, col, val, y, offs = B.make_csr_shard(torch, dev, n, d, P, grad, "f32", 7, nnz)
            parts = [pkg.DeviceCsrPartition(y[s:e], row_ptr[s:e + 1], col, val, d) for s, e in zip(offs[:-1], offs[1:])]
            nbytes = n * nnz * 8 + (n + P) * 8 + n * 8
        else:
            X, y, offs = B.make_shard(torch, dev, n, d, P, grad, "f32", 7)
            parts = [pkg.DevicePartition(y[s:e], X[s:e], d) for s, e in zip(offs[:-1], offs[1:])]
            nbytes = n * d * 4 + n * 8
        engine = pkg.HipEngine(pkg.PartitionedData(parts))
        w = torch.randn(d, dtype=torch.float64, device=dev) / d ** 0.5
        out = torch.zeros(3 + 2 * P, dtype=torch.float64, device=dev)
        st = engine.stream
        torch.cuda.synchronize()
        ms = []
        with torch.cuda.stream(st):
            for k in range(a.warmup + a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                engine.ctx.evaluate_device(kinds[grad], w.data_ptr(), out.data_ptr(), out.data_ptr() + 24,
                                           st.cuda_stream)
                e1.record(st)
                e1.synchronize()
                if k >= a.warmup:
                    ms.append(e0.elapsed_time(e1))
        h = out.cpu().numpy()
        med, lo = statistics.median(ms), min(ms)
        print(json.dumps({"shape": name, "rows": n, "features": d, "partitions": P, "nnz": nnz, "gradient": grad,
                          "reps": len(ms), "ms_median": round(med, 4), "ms_min": round(lo, 4),
                          "ns_per_row_median": round(med * 1e6 / n, 3), "bytes": nbytes,
                          "GBps_median": round(nbytes / med / 1e6, 1), "GBps_best": round(nbytes / lo / 1e6, 1),
                          "lossSum": float(h[0]), "count": int(h[1]), "nCorrect": int(h[2])}), flush=True)
        del engine, parts
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
