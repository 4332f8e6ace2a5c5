#!/usr/bin/env python3
"""Time psgd_project_device on device-resident data, beside its yardsticks in the same process,
alternating call by call (diagnostic tool):

  dense:  c2's rows (10M x 512 f32 in 256 partitions) for k = 2, 16, 64, f32 and f64 output, beside
            score_dense          psgd_evaluate_device, the row stream;
            evaluate_multinomial psgd_evaluate_multinomial_device at K - 1 = k, the same arithmetic on
                                 lane reductions (score_dense_mn);
            torch.mm(X.double(), B), the library's dgemm on a float64 copy of the rows;
  csr:    c4's rows (20M CSR rows of 94 non-zeros over 47,236 features) at k = 16 beside score_csr.

HIP events around each call; a round times every call of a group once, so the calls alternate; median
and min of --reps rounds after --warmup. One JSON line per measurement with the TB/s of rows read plus
output written and the T fma/s computed as n * d * kpad (CSR: n * nnz * k).

usage: python tools/project_bench.py [--shape dense,csr | all] [--rows N] [--reps K] [--k 2,16,64]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def alternate(torch, calls, reps, warmup):
    """calls: [(name, stream, fn)]; every round runs each once, timed by events on its stream."""
    ms = {name: [] for name, _, _ in calls}
    for r in range(warmup + reps):
        for name, st, fn in calls:
            with torch.cuda.stream(st):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                fn()
                e1.record(st)
                e1.synchronize()
            if r >= warmup:
                ms[name].append(e0.elapsed_time(e1))
    return ms


def report(shape, call, ms, extra=None):
    med, lo = statistics.median(ms), min(ms)
    line = {"shape": shape, "call": call, "reps": len(ms), "ms_median": round(med, 4), "ms_min": round(lo, 4)}
    line.update(extra or {})
    print(json.dumps(line), flush=True)
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="all")
    ap.add_argument("--rows", type=int, default=0, help="rows instead of each shape's own (smaller boxes)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--k", default="2,16,64")
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20")
    shapes = ["dense", "csr"] if a.shape == "all" else a.shape.split(",")
    ks = [int(v) for v in a.k.split(",")]

    import torch
    import __graft_entry__ as g
    import bench as B
    pkg = g.load_package()
    N = pkg._native
    dev = torch.device("cuda", 0)

    def outputs(n, k, odt, offs):
        es = 4 if odt == torch.float32 else 8
        ld = (k * es + 15) // 16 * 16 // es
        Y = torch.empty((n, ld), dtype=odt, device=dev)
        lab = torch.empty(n, dtype=torch.float64, device=dev)
        ptr = lambda t: [t[s:e].data_ptr() if e > s else 0 for s, e in zip(offs[:-1], offs[1:])]
        return Y, lab, ld, ptr(Y), ptr(lab)

    def dense(n, d, P):
        X, y, offs = B.make_shard(torch, dev, n, d, P, "logistic", "f32", 7)
        offs = [int(v) for v in offs]
        parts = [pkg.DevicePartition(y[s:e], X[s:e], d) for s, e in zip(offs[:-1], offs[1:])]
        engine = pkg.HipEngine(pkg.PartitionedData(parts))
        st, cur = engine.stream, torch.cuda.current_stream(dev)
        Xd = X.double()
        out3 = torch.zeros(3, dtype=torch.float64, device=dev)
        w = torch.randn(d, dtype=torch.float64, device=dev) / d ** 0.5
        for k in ks:
            plan = N.project_plan("dense", "f32", d, k)
            Bm = torch.randn((d, k), dtype=torch.float64, device=dev) / d ** 0.5
            wmn = Bm.t().contiguous()          # K - 1 = k class blocks of d
            torch.cuda.synchronize()
            calls = []
            keep = []
            for name, odt in (("f32", torch.float32), ("f64", torch.float64)):
                Y, lab, ld, xs, ls = outputs(n, k, odt, offs)
                keep.append((Y, lab))
                calls.append((f"project k={k} -> {name}", st,
                              lambda ld=ld, xs=xs, ls=ls, o=(N.F32 if odt == torch.float32 else N.F64):
                              engine.ctx.project_device(k, Bm.data_ptr(), o, ld, xs, ls, st.cuda_stream)))
            calls.append(("score_dense (evaluate)", st,
                          lambda: engine.ctx.evaluate_device(1, w.data_ptr(), out3.data_ptr(), None, st.cuda_stream)))
            calls.append((f"evaluate_multinomial K-1={k}", st,
                          lambda: engine.ctx.evaluate_multinomial_device(k + 1, wmn.data_ptr(), out3.data_ptr(), None,
                                                                         st.cuda_stream)))
            calls.append((f"torch.mm(X.double(), B) k={k}", cur, lambda: torch.mm(Xd, Bm)))
            ms = alternate(torch, calls, a.reps, a.warmup)
            med = {}
            for name, _, _ in calls:
                extra = {"rows": n, "features": d, "k": k}
                m = statistics.median(ms[name])
                if name.startswith("project"):
                    es = 4 if name.endswith("f32") else 8
                    ld = (k * es + 15) // 16 * 16 // es
                    extra.update({"plan": plan, "TBps_rows_plus_output_median": round((n * d * 4 + n * ld * es + n * 16) / m / 1e9, 3),
                                  "Tfma_per_s_median": round(n * d * plan["kpad"] / m / 1e9, 2)})
                elif name.startswith("score_dense"):
                    extra["TBps_rows_median"] = round(n * d * 4 / m / 1e9, 3)
                else:
                    extra["Tfma_per_s_median"] = round(n * d * k / m / 1e9, 2)
                med[name] = report("c2", name, ms[name], extra)
            p32 = med[f"project k={k} -> f32"]
            print(json.dumps({"shape": "c2", "k": k,
                              "project_f32_over_score_dense": round(p32 / med["score_dense (evaluate)"], 2),
                              "project_f32_over_evaluate_multinomial": round(p32 / med[f"evaluate_multinomial K-1={k}"], 2),
                              "project_f32_over_torch_mm": round(p32 / med[f"torch.mm(X.double(), B) k={k}"], 3)}), flush=True)
            del keep, calls
        del Xd
        torch.cuda.empty_cache()

    def csr(n, d, P, nnz, k):
        row_ptr, col, val, y, offs = B.make_csr_shard(torch, dev, n, d, P, "hinge", "f32", 7, nnz)
        offs = [int(v) for v in offs]
        parts = [pkg.DeviceCsrPartition(y[s:e], row_ptr[s:e + 1], col, val, d) for s, e in zip(offs[:-1], offs[1:])]
        engine = pkg.HipEngine(pkg.PartitionedData(parts))
        st = engine.stream
        plan = N.project_plan("csr", "f32", d, k, nnz)
        Bm = torch.randn((d, k), dtype=torch.float64, device=dev) / nnz ** 0.5
        w = torch.randn(d, dtype=torch.float64, device=dev)
        out3 = torch.zeros(3, dtype=torch.float64, device=dev)
        Y, lab, ld, xs, ls = outputs(n, k, torch.float32, offs)
        torch.cuda.synchronize()
        calls = [(f"project k={k} -> f32", st,
                  lambda: engine.ctx.project_device(k, Bm.data_ptr(), N.F32, ld, xs, ls, st.cuda_stream)),
                 ("score_csr (evaluate)", st,
                  lambda: engine.ctx.evaluate_device(2, w.data_ptr(), out3.data_ptr(), None, st.cuda_stream))]
        ms = alternate(torch, calls, a.reps, a.warmup)
        row_bytes = n * nnz * 8 + n * 8
        m = statistics.median(ms[calls[0][0]])
        p = report("c4", calls[0][0], ms[calls[0][0]],
                   {"rows": n, "features": d, "nnz": nnz, "k": k, "plan": plan,
                    "TBps_rows_plus_output_median": round((row_bytes + n * ld * 4 + n * 16) / m / 1e9, 3),
                    "Tfma_per_s_median": round(n * nnz * k / m / 1e9, 3),
                    "B_gather_TBps_median": round(n * nnz * k * 8 / m / 1e9, 3)})
        m = statistics.median(ms[calls[1][0]])
        s = report("c4", calls[1][0], ms[calls[1][0]], {"TBps_rows_median": round(row_bytes / m / 1e9, 3)})
        print(json.dumps({"shape": "c4", "k": k, "project_over_score_csr": round(p / s, 2)}), flush=True)

    for shape in shapes:
        if shape == "dense":
            dense(a.rows or 10_000_000, 512, 256)
        elif shape == "csr":
            csr(a.rows or 20_000_000, 47_236, 256, 94, 16)
        else:
            ap.error(f"unknown shape {shape}")


if __name__ == "__main__":
    main()
