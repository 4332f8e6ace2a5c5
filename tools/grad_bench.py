#!/usr/bin/env python3
"""Time psgd_gradient_sum_device on device-resident data at the flagship shapes, beside the two
passes that read the same rows once in fp64 -- psgd_evaluate_device (score_dense / score_csr) and
psgd_column_stats_device (stats_dense / stats_csr) -- in the same process (diagnostic tool):

  c2:     10M x 512 f32 dense rows in 256 partitions, LeastSquares and Logistic;
  c3:     12.5M x 1,024 f32 dense rows in 256 partitions, Logistic (skipped when HBM cannot hold it);
  wide:   the fused kernel's largest d (2,048 f32) beside the two-pass path just past it (2,052);
  c4:     20M rcv1-like CSR rows, 47,236 features, 94 non-zeros, f32 values, 256 partitions, Hinge;
  narrow: CSR rows of 32 non-zeros over 4,096 features, the LDS-accumulator path and the
          global-atomic path (PSGD_GRAD_CSR_GLOBAL=1) on the same rows;
  gd:     one full GradientDescent iteration (gradient_sum + gd_update + the scalars' read-back) at c2
          beside one ParallelizedSGD step (epoch + scalars). Time per outer iteration only: the two do
          different amounts of optimization per pass, and no claim about convergence per second is made.

HIP events around each call after a warm-up; one JSON line per measurement: median and min
milliseconds, ns per row, the bytes of the rows (dense: n * d * sizeof; CSR: col + val + row_ptr) over
the time, and for CSR the atomic bytes (8 per non-zero) over the time.

usage: python tools/grad_bench.py [--shape c2,c3,wide,c4,narrow,gd | all] [--rows N] [--reps K]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KIND = {"logistic": 0, "least_squares": 1, "hinge": 2}


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


def report(shape, call, ms, n, nbytes, extra=None):
    med, lo = statistics.median(ms), min(ms)
    line = {"shape": shape, "call": call, "rows": n, "reps": len(ms), "ms_median": round(med, 4),
            "ms_min": round(lo, 4), "ns_per_row_median": round(med * 1e6 / n, 3), "row_bytes": nbytes,
            "GBps_median": round(nbytes / med / 1e6, 1), "GBps_best": round(nbytes / lo / 1e6, 1)}
    line.update(extra or {})
    print(json.dumps(line), flush=True)
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="all")
    ap.add_argument("--rows", type=int, default=0, help="rows instead of each shape's own (smaller boxes)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20")
    shapes = ["c2", "c3", "wide", "c4", "narrow", "gd"] if a.shape == "all" else a.shape.split(",")

    import numpy as np
    import torch
    import __graft_entry__ as g
    import bench as B
    pkg = g.load_package()
    dev = torch.device("cuda", 0)

    def dense_engine(n, d, P, grad):
        X, y, offs = B.make_shard(torch, dev, n, d, P, grad, "f32", 7)
        parts = [pkg.DevicePartition(y[s:e], X[s:e], d) for s, e in zip(offs[:-1], offs[1:])]
        return pkg.HipEngine(pkg.PartitionedData(parts))

    def csr_engine(n, d, P, nnz):
        row_ptr, col, val, y, offs = B.make_csr_shard(torch, dev, n, d, P, "logistic", "f32", 7, nnz)
        parts = [pkg.DeviceCsrPartition(y[s:e], row_ptr[s:e + 1], col, val, d) for s, e in zip(offs[:-1], offs[1:])]
        return pkg.HipEngine(pkg.PartitionedData(parts))

    def weights(d, scale):
        gen = torch.Generator(device=dev)
        gen.manual_seed(11)
        return torch.randn(d, generator=gen, device=dev, dtype=torch.float64) * scale

    def passes(shape, engine, n, d, nbytes, grads, nnz=0, yardsticks=True):
        """gradient_sum for each gradient, then the two yardsticks, on the engine's stream."""
        st = engine.stream
        w = weights(d, 1.0 / d ** 0.5 if not nnz else 1.0)
        out = torch.zeros(d + 2, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        res = {}
        for grad in grads:
            ms = timed(torch, st, a.reps, a.warmup,
                       lambda: engine.ctx.gradient_sum_device(KIND[grad], w.data_ptr(), 1.0, 0, out.data_ptr(),
                                                              st.cuda_stream))
            h = out.cpu().numpy()
            extra = {"features": d, "gradient": grad, "lossSum": float(h[d]), "count": int(h[d + 1])}
            if nnz:
                extra["atomic_GBps_median"] = round(n * nnz * 8 / statistics.median(ms) / 1e6, 1)
            res[grad] = report(shape, "gradient_sum", ms, n, nbytes, extra)
        if yardsticks:
            o3 = torch.zeros(3, dtype=torch.float64, device=dev)
            for grad in grads:
                ms = timed(torch, st, a.reps, a.warmup,
                           lambda: engine.ctx.evaluate_device(KIND[grad], w.data_ptr(), o3.data_ptr(), None,
                                                              st.cuda_stream))
                med = report(shape, "evaluate", ms, n, nbytes, {"features": d, "gradient": grad})
                print(json.dumps({"shape": shape, "gradient": grad, "gradient_sum_over_evaluate": round(res[grad] / med, 3)}),
                      flush=True)
            so = torch.zeros(1 + 5 * d, dtype=torch.float64, device=dev)
            ms = timed(torch, st, a.reps, a.warmup, lambda: engine.ctx.column_stats_device(so.data_ptr(), st.cuda_stream))
            med = report(shape, "column_stats", ms, n, nbytes * (2 if nnz else 1), {"features": d})
            for grad in grads:
                print(json.dumps({"shape": shape, "gradient": grad, "gradient_sum_over_column_stats": round(res[grad] / med, 3)}),
                      flush=True)
        return res

    for shape in shapes:
        if shape == "c2":
            n, d, P = a.rows or 10_000_000, 512, 256
            engine = dense_engine(n, d, P, "least_squares")
            passes("c2", engine, n, d, n * d * 4, ["least_squares", "logistic"])
        elif shape == "c3":
            n, d, P = a.rows or 12_500_000, 1024, 256
            try:
                engine = dense_engine(n, d, P, "logistic")
            except torch.cuda.OutOfMemoryError:
                print(json.dumps({"shape": "c3", "skipped": "out of memory"}), flush=True)
                continue
            passes("c3", engine, n, d, n * d * 4, ["logistic"])
        elif shape == "wide":
            n, P = a.rows or 1_000_000, 256
            for d in (2048, 2052):
                engine = dense_engine(n, d, P, "logistic")
                passes(f"wide d={d} ({'fused' if d <= 2048 else 'two-pass'})", engine, n, d, n * d * 4, ["logistic"],
                       yardsticks=(d == 2048))
                del engine
                torch.cuda.empty_cache()
            continue
        elif shape == "c4":
            n, d, P, nnz = a.rows or 20_000_000, 47_236, 256, 94
            engine = csr_engine(n, d, P, nnz)
            passes("c4", engine, n, d, n * nnz * 8 + (n + P) * 8, ["hinge", "logistic"], nnz=nnz)
        elif shape == "narrow":
            n, d, P, nnz = a.rows or 20_000_000, 4096, 256, 32
            engine = csr_engine(n, d, P, nnz)
            nbytes = n * nnz * 8 + (n + P) * 8
            os.environ.pop("PSGD_GRAD_CSR_GLOBAL", None)
            passes("narrow d=4096 nnz=32 (LDS accumulators)", engine, n, d, nbytes, ["logistic"], nnz=nnz, yardsticks=False)
            os.environ["PSGD_GRAD_CSR_GLOBAL"] = "1"
            passes("narrow d=4096 nnz=32 (global atomics)", engine, n, d, nbytes, ["logistic"], nnz=nnz, yardsticks=False)
            os.environ.pop("PSGD_GRAD_CSR_GLOBAL", None)
        elif shape == "gd":
            n, d, P = a.rows or 10_000_000, 512, 256
            engine = dense_engine(n, d, P, "least_squares")
            grad, upd = pkg.LeastSquaresGradient(), pkg.SimpleSGDUpdater()
            w = engine.weights(np.zeros(d))
            params = pkg.make_params(grad, upd, 1e-3, 0.0, 1.0, 0.0, "f64")

            def gd_iteration():
                gs = engine.gradient_sum(grad, w, 1.0, 1)
                engine.batch_scalars(gs)
                engine.gd_update(upd, w, gs, 1e-3, 1, 0.0)

            def psgd_step():
                folded, _ = engine.epoch(params, w)
                engine.scalars(folded)

            for name, fn in (("GradientDescent iteration", gd_iteration), ("ParallelizedSGD step (fp64)", psgd_step)):
                wall = []
                for k in range(a.warmup + a.reps):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    if k >= a.warmup:
                        wall.append((time.perf_counter() - t0) * 1e3)
                report("c2", name, wall, n, n * d * 4, {"features": d, "clock": "host wall, synchronised"})
        else:
            ap.error(f"unknown shape {shape}")
        del engine
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
