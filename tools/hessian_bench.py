#!/usr/bin/env python3
"""Time the second-order passes on device-resident data, each beside its yardstick in the same process
with the two calls alternating (diagnostic tool):

  curvature:  psgd_row_curvature_device (curvature_dense) beside psgd_evaluate_device (score_dense +
              eval_reduce) on c2's rows: 10M x 512 f32 dense rows in 256 partitions, Logistic;
  weighted:   psgd_gramian_weighted_device beside psgd_gramian_device (gram_dense + gram_merge) on the
              same rows, the weights the rows' curvature;
  newton:     one Newton iteration end to end on the same rows (runNewton with numIterations = 1: the
              objective at the start, gradient_sum, row_curvature, the weighted Gramian, the 512 x 512
              Cholesky on the host and the line search's evaluate), wall clock;
  csr:        the weighted beside the unweighted Gramian on 20M CSR rows of 32 non-zeros over 4,096
              features (gram_bench's CSR shape).

HIP events around each call after a warm-up; one JSON line per measurement: median and min ms, and per
pair the ratio of the medians and of the minima.

usage: python tools/hessian_bench.py [--shape curvature,weighted,newton,csr | all] [--rows N] [--csr-rows N] [--reps K]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed_pair(torch, st, reps, warmup, first, second):
    """first() and second() alternating on `st`: two lists of ms."""
    ms = ([], [])
    with torch.cuda.stream(st):
        for k in range(warmup + reps):
            for which, call in enumerate((first, second)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                call()
                e1.record(st)
                e1.synchronize()
                if k >= warmup:
                    ms[which].append(e0.elapsed_time(e1))
    return ms


def report(shape, call, ms, extra=None):
    line = {"shape": shape, "call": call, "reps": len(ms), "ms_median": round(statistics.median(ms), 4),
            "ms_min": round(min(ms), 4)}
    line.update(extra or {})
    print(json.dumps(line), flush=True)


def ratio(shape, name, num, den):
    print(json.dumps({"shape": shape, name: {"of_medians": round(statistics.median(num) / statistics.median(den), 3),
                                             "of_minima": round(min(num) / min(den), 3)}}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="all")
    ap.add_argument("--rows", type=int, default=10_000_000, help="dense rows (c2's by default)")
    ap.add_argument("--csr-rows", type=int, default=20_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20")
    shapes = ["curvature", "weighted", "newton", "csr"] if a.shape == "all" else a.shape.split(",")
    for s in shapes:
        if s not in ("curvature", "weighted", "newton", "csr"):
            ap.error(f"unknown shape {s}")

    import numpy as np
    import torch
    import __graft_entry__ as g
    import bench as B
    pkg = g.load_package()
    dev = torch.device("cuda", 0)

    if any(s in shapes for s in ("curvature", "weighted", "newton")):
        n, d, P = a.rows, 512, 256
        X, y, offs = B.make_shard(torch, dev, n, d, P, "logistic", "f32", 7)
        data = pkg.PartitionedData([pkg.DevicePartition(y[s:e], X[s:e], d) for s, e in zip(offs[:-1], offs[1:])])
        engine = pkg.HipEngine(data)
        st, ctx = engine.stream, engine.ctx
        w = torch.randn(d, device=dev, dtype=torch.float64) / d ** 0.5
        h = engine.row_curvature(pkg.LogisticGradient(), w)          # registers; the weights of "weighted"
        out3 = torch.zeros(3 + 2 * P, dtype=torch.float64, device=dev)
        M = torch.zeros((d + 2) * (d + 2), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        row_bytes = n * d * 4
        if "curvature" in shapes:
            cur, score = timed_pair(
                torch, st, a.reps, a.warmup,
                lambda: ctx.row_curvature_device(0, w.data_ptr(), h.data_ptr(), st.cuda_stream),
                lambda: ctx.evaluate_device(0, w.data_ptr(), out3.data_ptr(), out3.data_ptr() + 24, st.cuda_stream))
            report("c2", "row_curvature (curvature_dense)", cur,
                   {"rows": n, "features": d, "row_GBps_median": round(row_bytes / statistics.median(cur) / 1e6, 1)})
            report("c2", "evaluate (score_dense + eval_reduce)", score,
                   {"row_GBps_median": round(row_bytes / statistics.median(score) / 1e6, 1)})
            ratio("c2", "row_curvature_over_evaluate", cur, score)
        if "weighted" in shapes:
            wt, plain = timed_pair(
                torch, st, a.reps, a.warmup,
                lambda: ctx.gramian_weighted_device(h.data_ptr(), M.data_ptr(), st.cuda_stream),
                lambda: ctx.gramian_device(M.data_ptr(), st.cuda_stream))
            report("c2", "gramian_weighted (gram_dense weighted + gram_merge)", wt, {"rows": n, "features": d})
            report("c2", "gramian (gram_dense + gram_merge)", plain)
            ratio("c2", "weighted_over_unweighted", wt, plain)
        if "newton" in shapes:
            w0 = np.zeros(d)
            wall = []
            for k in range(a.warmup + a.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                pkg.runNewton(data, pkg.LogisticGradient(), pkg.SquaredL2SGDUpdater(), 1, 0.01, w0, engine=engine)
                torch.cuda.synchronize()
                if k >= a.warmup:
                    wall.append((time.perf_counter() - t0) * 1e3)
            report("c2", "one Newton iteration (runNewton, numIterations = 1), wall clock", wall, {"rows": n, "features": d})
        del engine, data, X, y, h, M
        torch.cuda.empty_cache()

    if "csr" in shapes:
        n, d, P, nnz = a.csr_rows, 4096, 256, 32
        row_ptr, col, val, y, offs = B.make_csr_shard(torch, dev, n, d, P, "logistic", "f32", 7, nnz)
        parts = [pkg.DeviceCsrPartition(y[s:e], row_ptr[s:e + 1], col, val, d) for s, e in zip(offs[:-1], offs[1:])]
        engine = pkg.HipEngine(pkg.PartitionedData(parts))
        st, ctx = engine.stream, engine.ctx
        w = torch.randn(d, device=dev, dtype=torch.float64) / nnz ** 0.5
        h = engine.row_curvature(pkg.LogisticGradient(), w)
        M = torch.zeros((d + 2) * (d + 2), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        wt, plain = timed_pair(
            torch, st, a.reps, a.warmup,
            lambda: ctx.gramian_weighted_device(h.data_ptr(), M.data_ptr(), st.cuda_stream),
            lambda: ctx.gramian_device(M.data_ptr(), st.cuda_stream))
        report("csr", "gramian_weighted (gram_csr weighted + gram_mirror)", wt, {"rows": n, "features": d, "nnz": nnz})
        report("csr", "gramian (gram_csr + gram_mirror)", plain)
        ratio("csr", "weighted_over_unweighted", wt, plain)


if __name__ == "__main__":
    main()
