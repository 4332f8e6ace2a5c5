#!/usr/bin/env python3
"""Time the k-means passes on device-resident data, beside their yardsticks in the same process,
alternating call by call (diagnostic tool):

  dense:  c2's rows (10M x 512 f32 in 256 partitions) for k = 2, 16, 64, 256:
            kmeans_assign        psgd_kmeans_assign_device (assign and dist2 written);
            kmeans_step          psgd_kmeans_step_device (assign, then the sums and their merge);
            project -> f32       psgd_project_device at the same k: the same loads and MFMAs as the
                                 assignment, 4 k bytes a row written instead of 12;
            score_dense          psgd_evaluate_device, the row stream;
            torch step           one Lloyd step with torch.cdist / argmin / index_add_ on a float64 copy
                                 of the rows made beforehand, --torch-reps rounds of its own after 1;
  csr:    c4's rows (20M CSR rows of 94 non-zeros over 47,236 features) at k = 16: assign and step beside
          project_csr and score_csr.

The sums pass has no entry point of its own: its time is reported as step - assign (medians). HIP events
around each call; a round times every call of a group once, so the calls alternate; median and min of
--reps rounds after --warmup. One JSON line per measurement. T fma/s of the assignment is n * dpad * kpad,
of the dense sums the MFMAs issued (rows / 4 per block pair, 1,024 fma each) -- most of them multiply a
one-hot operand's zeros.

usage: python tools/kmeans_bench.py [--shape dense,csr | all] [--rows N] [--reps K] [--k 2,16,64,256] [--no-torch]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def alternate(torch, calls, reps, warmup):
    """project_bench's alternation: every round runs each call once, timed by events on its stream. The
    warm-up rounds print each call's time to stderr as they go, so that a slow yardstick shows at once."""
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
            else:
                print(f"warm-up {r}: {name}: {e0.elapsed_time(e1):.3f} ms", file=sys.stderr, flush=True)
    return ms


def main():
    from project_bench import report
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="all")
    ap.add_argument("--rows", type=int, default=0, help="rows instead of each shape's own (smaller boxes)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--k", default="2,16,64,256")
    ap.add_argument("--torch-reps", type=int, default=3, help="rounds of the torch yardstick (after 1)")
    ap.add_argument("--no-torch", action="store_true", help="leave the torch yardstick (and its float64 copy) out")
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

    def outputs(n, k, offs):
        ld = (k + 3) // 4 * 4
        Y = torch.empty((n, ld), dtype=torch.float32, device=dev)
        lab = torch.empty(n, dtype=torch.float64, device=dev)
        ptr = lambda t: [t[s:e].data_ptr() if e > s else 0 for s, e in zip(offs[:-1], offs[1:])]
        return Y, lab, ld, ptr(Y), ptr(lab)

    def kmeans_calls(engine, n, d, k, C):
        st = engine.stream
        assign = torch.empty(n, dtype=torch.int32, device=dev)
        dist2 = torch.empty(n, dtype=torch.float64, device=dev)
        step = torch.empty(k * (d + 1) + 2, dtype=torch.float64, device=dev)
        calls = [(f"kmeans_assign k={k}", st, lambda: engine.ctx.kmeans_assign_device(
                      k, C.data_ptr(), assign.data_ptr(), dist2.data_ptr(), st.cuda_stream)),
                 (f"kmeans_step k={k}", st, lambda: engine.ctx.kmeans_step_device(k, C.data_ptr(), step.data_ptr(), st.cuda_stream))]
        return calls, (assign, dist2, step)

    def dense(n, d, P):
        X, y, offs = B.make_shard(torch, dev, n, d, P, "logistic", "f32", 7)
        offs = [int(v) for v in offs]
        parts = [pkg.DevicePartition(y[s:e], X[s:e], d) for s, e in zip(offs[:-1], offs[1:])]
        engine = pkg.HipEngine(pkg.PartitionedData(parts))
        st, cur = engine.stream, torch.cuda.current_stream(dev)
        Xd = None if a.no_torch else X.double()
        print(f"dense rows ready: {n} x {d}", file=sys.stderr, flush=True)
        out3 = torch.zeros(3, dtype=torch.float64, device=dev)
        w = torch.randn(d, dtype=torch.float64, device=dev) / d ** 0.5
        n_tiles = sum(-(-(e - s) // 16) for s, e in zip(offs[:-1], offs[1:]))
        for k in ks:
            plan = N.kmeans_plan("dense", "f32", d, k, n_tiles)
            C = torch.randn((k, d), dtype=torch.float64, device=dev)
            Bm = C.t().contiguous()
            calls, keep = kmeans_calls(engine, n, d, k, C)
            Y, lab, ld, xs, ls = outputs(n, k, offs)
            calls.append((f"project k={k} -> f32", st,
                          lambda: engine.ctx.project_device(k, Bm.data_ptr(), N.F32, ld, xs, ls, st.cuda_stream)))
            calls.append(("score_dense (evaluate)", st,
                          lambda: engine.ctx.evaluate_device(1, w.data_ptr(), out3.data_ptr(), None, st.cuda_stream)))
            if Xd is not None:
                def torch_step():
                    idx = torch.cdist(Xd, C).argmin(dim=1)
                    torch.zeros((k, d), dtype=torch.float64, device=dev).index_add_(0, idx, Xd)
                    torch.bincount(idx, minlength=k)
            torch.cuda.synchronize()
            ms = alternate(torch, calls, a.reps, a.warmup)
            if Xd is not None:
                # (index_add_ into k rows is seconds a call at small k: a few rounds of its own, after the others)
                calls.append((f"torch cdist/argmin/index_add_ step k={k}", cur, torch_step))
                ms.update(alternate(torch, calls[-1:], a.torch_reps, 1))
            med = {}
            for name, _, _ in calls:
                m = statistics.median(ms[name])
                extra = {"rows": n, "features": d, "k": k}
                if name.startswith("kmeans_assign"):
                    extra.update({"plan": plan, "TBps_rows_plus_output_median": round((n * d * 4 + n * 12) / m / 1e9, 3),
                                  "Tfma_per_s_median": round(n * d * plan["kpad"] / m / 1e9, 2)})
                elif name.startswith("score_dense"):
                    extra["TBps_rows_median"] = round(n * d * 4 / m / 1e9, 3)
                med[name] = report("c2", name, ms[name], extra)
            asg, stp = med[f"kmeans_assign k={k}"], med[f"kmeans_step k={k}"]
            sums = stp - asg
            nbf = -(-(d + 1) // 16)
            mfma = (n / 4) * (plan["kpad"] // 16) * nbf
            line = {"shape": "c2", "k": k, "sums_ms_step_minus_assign": round(sums, 4),
                    "sums_Tfma_per_s_issued": round(mfma * 1024 / sums / 1e9, 2),
                    "assign_over_project_f32": round(asg / med[f"project k={k} -> f32"], 3),
                    "assign_over_score_dense": round(asg / med["score_dense (evaluate)"], 2)}
            if Xd is not None:
                line["step_over_torch_step"] = round(stp / med[f"torch cdist/argmin/index_add_ step k={k}"], 3)
            print(json.dumps(line), flush=True)
            del keep, calls
        del Xd
        torch.cuda.empty_cache()

    def csr(n, d, P, nnz, k):
        row_ptr, col, val, y, offs = B.make_csr_shard(torch, dev, n, d, P, "hinge", "f32", 7, nnz)
        offs = [int(v) for v in offs]
        parts = [pkg.DeviceCsrPartition(y[s:e], row_ptr[s:e + 1], col, val, d) for s, e in zip(offs[:-1], offs[1:])]
        engine = pkg.HipEngine(pkg.PartitionedData(parts))
        st = engine.stream
        n_tiles = sum(-(-(e - s) // 256) for s, e in zip(offs[:-1], offs[1:]))
        plan = N.kmeans_plan("csr", "f32", d, k, n_tiles)
        C = torch.randn((k, d), dtype=torch.float64, device=dev) / nnz ** 0.5
        Bm = C.t().contiguous()
        w = torch.randn(d, dtype=torch.float64, device=dev)
        out3 = torch.zeros(3, dtype=torch.float64, device=dev)
        calls, keep = kmeans_calls(engine, n, d, k, C)
        Y, lab, ld, xs, ls = outputs(n, k, offs)
        calls.append((f"project k={k} -> f32", st,
                      lambda: engine.ctx.project_device(k, Bm.data_ptr(), N.F32, ld, xs, ls, st.cuda_stream)))
        calls.append(("score_csr (evaluate)", st,
                      lambda: engine.ctx.evaluate_device(2, w.data_ptr(), out3.data_ptr(), None, st.cuda_stream)))
        torch.cuda.synchronize()
        ms = alternate(torch, calls, a.reps, a.warmup)
        med = {name: report("c4", name, ms[name], {"rows": n, "features": d, "nnz": nnz, "k": k, "plan": plan})
               for name, _, _ in calls}
        asg, stp = med[f"kmeans_assign k={k}"], med[f"kmeans_step k={k}"]
        print(json.dumps({"shape": "c4", "k": k, "sums_ms_step_minus_assign": round(stp - asg, 4),
                          "sums_atomics_G_per_s": round(n * nnz / (stp - asg) / 1e6, 2),
                          "assign_over_project_f32": round(asg / med[f"project k={k} -> f32"], 3),
                          "assign_over_score_csr": round(asg / med["score_csr (evaluate)"], 2)}), flush=True)

    for shape in shapes:
        if shape == "dense":
            dense(a.rows or 10_000_000, 512, 256)
        elif shape == "csr":
            csr(a.rows or 20_000_000, 47_236, 256, 94, 16)
        else:
            ap.error(f"unknown shape {shape}")


if __name__ == "__main__":
    main()
