#!/usr/bin/env python3
"""Time psgd_gradient_sum_multinomial_device on device-resident data (diagnostic tool):

  c2:     10M x 512 f32 dense rows in 256 partitions at K = 3 (the fused kernel) and K = 10 (the general
          two-pass path);
  narrow: 20M x 100 f32 dense rows at K = 10 (the fused kernel with 16 class accumulators a lane);
  wide:   1M x 2,048 f32 dense rows at K = 3 (the fused kernel's widest rows);
  c4:     20M rcv1-like CSR rows, 47,236 features, 94 non-zeros, f32 values, 256 partitions at K = 3;
  sweep:  (not in `all`) f32 dense rows of d = 8 .. 1,024 at K = 3 .. 17, 4M rows or 2 GB: every shape the
          register budget would let run fused (PSGD_GRAD_MN_FUSE_ALL=1), fused beside general -- the
          measurement the fused kernel's range (grad_mn_geometry) was set from.

Each multinomial gradient is timed in turn -- one call of each, alternating, in one session, under the
same clocks and neighbours -- with
  the same shape forced down the general path (PSGD_GRAD_MN_TWO_PASS=1) where it runs fused,
  psgd_evaluate_multinomial_device at the same K (score_dense_mn / score_csr_mn),
  the binary psgd_gradient_sum_device, Logistic (grad_dense / grad_csr).
HIP events around each call after a warm-up; one JSON line per case: median and min milliseconds of
each, the ratios of the medians, the bytes of the rows over the time and, for the dense shapes, the f64
fma count 2 (K - 1) n d (margins and accumulation) over the time beside the vector f64 ceiling of
tools/multiclass_bench.py (39.3 T fma/s).

usage: python tools/grad_mn_bench.py [--what c2,narrow,wide,c4,sweep | all] [--rows N] [--partitions P] [--reps K]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F64_FMA_PER_S = 256 * 4 * 16 * 2.4e9   # vector f64 fma a second at the 2.4 GHz peak clock


def timed(st, torch, calls, warmup, reps):
    """calls: {name: fn}; one call of each per round, in turn. -> {name: [ms]}"""
    ms = {name: [] for name in calls}
    with torch.cuda.stream(st):
        for k in range(warmup + reps):
            for name, fn in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                fn()
                e1.record(st)
                e1.synchronize()
                if k >= warmup:
                    ms[name].append(e0.elapsed_time(e1))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="all")
    ap.add_argument("--rows", type=int, default=0, help="rows instead of the shape's own (smaller boxes)")
    ap.add_argument("--partitions", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20")
    what = ["c2", "narrow", "wide", "c4"] if a.what == "all" else a.what.split(",")

    import torch
    import __graft_entry__ as g
    import bench as B
    pkg = g.load_package()
    dev = torch.device("cuda", 0)
    P = a.partitions

    def case(name, parts, layout, n, d, nbytes, classes, max_nnz=0):
        engine = pkg.HipEngine(pkg.PartitionedData(parts))
        st = engine.stream
        gen = torch.Generator(device=dev)
        gen.manual_seed(11)
        scale = 1.0 / d ** 0.5 if layout == "dense" else 1.0 / max_nnz ** 0.5
        wb = torch.randn(d, dtype=torch.float64, device=dev, generator=gen) * scale
        ob = torch.zeros(d + 2, dtype=torch.float64, device=dev)
        o3 = torch.zeros(3 + 2 * P, dtype=torch.float64, device=dev)
        for K in classes:
            os.environ.pop("PSGD_GRAD_MN_TWO_PASS", None)
            plan = pkg._native.gradient_multinomial_plan(layout, "f32", d, K, max_nnz)
            w = torch.randn((K - 1) * d, dtype=torch.float64, device=dev, generator=gen) * scale
            out = torch.zeros((K - 1) * d + 2, dtype=torch.float64, device=dev)

            def grad_mn(two_pass):
                # (the switch is read at every call)
                if two_pass:
                    os.environ["PSGD_GRAD_MN_TWO_PASS"] = "1"
                else:
                    os.environ.pop("PSGD_GRAD_MN_TWO_PASS", None)
                engine.ctx.gradient_sum_multinomial_device(K, w.data_ptr(), 1.0, 0, out.data_ptr(), st.cuda_stream)

            calls = {"gradient_mn": lambda: grad_mn(False)}
            if plan["path"] == "fused":
                calls["gradient_mn_general"] = lambda: grad_mn(True)
            calls["score_mn"] = lambda: engine.ctx.evaluate_multinomial_device(K, w.data_ptr(), o3.data_ptr(),
                                                                               o3.data_ptr() + 24, st.cuda_stream)
            calls["gradient_binary"] = lambda: engine.ctx.gradient_sum_device(0, wb.data_ptr(), 1.0, 0, ob.data_ptr(),
                                                                              st.cuda_stream)
            torch.cuda.synchronize()
            ms = timed(st, torch, calls, a.warmup, a.reps)
            os.environ.pop("PSGD_GRAD_MN_TWO_PASS", None)
            med = {k: statistics.median(v) for k, v in ms.items()}
            rec = {"case": f"{name} K={K}", "path": plan["path"], "rows": n, "features": d, "partitions": P,
                   "reps": a.reps, "bytes": nbytes}
            for k, v in ms.items():
                rec[k + "_ms_median"] = round(med[k], 4)
                rec[k + "_ms_min"] = round(min(v), 4)
            rec["GBps_median"] = round(nbytes / med["gradient_mn"] / 1e6, 1)
            rec["over_score_mn"] = round(med["gradient_mn"] / med["score_mn"], 3)
            rec["over_gradient_binary"] = round(med["gradient_mn"] / med["gradient_binary"], 3)
            if "gradient_mn_general" in med:
                rec["fused_over_general"] = round(med["gradient_mn"] / med["gradient_mn_general"], 3)
            if layout == "dense":
                fma = 2 * (K - 1) * n * d
                rec["f64_fma"] = fma
                rec["Tfma_per_s_median"] = round(fma / med["gradient_mn"] / 1e9, 2)
                rec["f64_ceiling_ms"] = round(fma / F64_FMA_PER_S * 1e3, 3)
            h = out.cpu().numpy()
            rec["lossSum"], rec["count"] = float(h[-2]), int(h[-1])
            print(json.dumps(rec), flush=True)
        del engine

    dense = {"c2": (10_000_000, 512, (3, 10)), "narrow": (20_000_000, 100, (10,)), "wide": (1_000_000, 2048, (3,))}
    if "sweep" in what:
        what.remove("sweep")
        os.environ["PSGD_GRAD_MN_FUSE_ALL"] = "1"
        for d in (8, 32, 100, 256, 512, 1024):
            n = a.rows or min(4_000_000, 2_000_000_000 // (4 * d))
            classes = tuple(K for K in (3, 4, 5, 6, 9, 10, 17)
                            if pkg._native.gradient_multinomial_plan("dense", "f32", d, K)["path"] == "fused")
            X, _, offs = B.make_shard(torch, dev, n, d, P, "logistic", "f32", 7)
            y = torch.randint(0, 3, (n,), device=dev).to(torch.float64)
            parts = [pkg.DevicePartition(y[s:e], X[s:e], d) for s, e in zip(offs[:-1], offs[1:])]
            case(f"sweep d={d}", parts, "dense", n, d, n * d * 4 + n * 8, classes)
            del parts, X, y
            torch.cuda.empty_cache()
        os.environ.pop("PSGD_GRAD_MN_FUSE_ALL", None)
    for name in what:
        if name in dense:
            n, d, classes = dense[name]
            n = a.rows or n
            X, _, offs = B.make_shard(torch, dev, n, d, P, "logistic", "f32", 7)
            y = torch.randint(0, 3, (n,), device=dev).to(torch.float64)   # classes of K = 3: valid labels for K = 10 too
            parts = [pkg.DevicePartition(y[s:e], X[s:e], d) for s, e in zip(offs[:-1], offs[1:])]
            case(name, parts, "dense", n, d, n * d * 4 + n * 8, classes)
            del parts, X, y
        elif name == "c4":
            n, d, nnz = a.rows or 20_000_000, 47_236, 94
            row_ptr, col, val, _, offs = B.make_csr_shard(torch, dev, n, d, P, "logistic", "f32", 7, nnz)
            y = torch.randint(0, 3, (n,), device=dev).to(torch.float64)
            parts = [pkg.DeviceCsrPartition(y[s:e], row_ptr[s:e + 1], col, val, d) for s, e in zip(offs[:-1], offs[1:])]
            case("c4", parts, "csr", n, d, n * nnz * 8 + (n + P) * 8 + n * 8, (3,), max_nnz=nnz)
            del parts, row_ptr, col, val, y
        else:
            ap.error(f"unknown case {name}")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
