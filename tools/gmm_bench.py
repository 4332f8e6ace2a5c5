#!/usr/bin/env python3
"""Time the Gaussian mixture's passes on device-resident data, beside their yardsticks in the same process,
alternating call by call (diagnostic tool). Shapes (rows x features f32 in 256 partitions, k components):
10M x 32 k = 8 and 10M x 16 k = 16 (packed operands in LDS), 4M x 128 k = 2 (read through L2). Per shape:

  gmm_responsibilities   psgd_gmm_responsibilities_device (resp and q written, the log-likelihood merged);
  project -> f64         psgd_project_device onto the same k x 16 db columns with f64 output: the same MFMAs
                         as the E-step, 16 db times its output -- bar (a): E-step median <= 1.0 x this;
  gmm_moments            psgd_gmm_moments_device on the responsibilities just computed;
  k x gramian(weights=)  k psgd_gramian_weighted_device calls, weights = column j of the responsibilities
                         (contiguous copies made beforehand) -- bar (b): moments median <= 1.0 x this;
  gmm_step               psgd_gmm_step_device, both passes;
  kmeans_step            psgd_kmeans_step_device at the same (d, k), for scale;
  torch E-step           a float64 E-step with torch matmul / exp / logsumexp on a float64 copy of the rows
                         made beforehand, --torch-reps rounds of its own after 1.

HIP events around each call; a round times every call once, so the calls alternate; median and min of
--reps rounds after --warmup. One JSON line per measurement. T fma/s: the E-step's n x dpad x 16 k db, the
moments' MFMAs issued (rows / 4 per kept block and component, 1,024 fma each), against the bare MFMA rate
of 39.1 T fma/s.

usage: python tools/gmm_bench.py [--shape lds32,lds16,l2 | all] [--rows N] [--reps K] [--no-torch]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

SHAPES = {"lds32": (10_000_000, 32, 8), "lds16": (10_000_000, 16, 16), "l2": (4_000_000, 128, 2)}
MFMA_RATE = 39.1   # T fma/s, tools/gram_bench.py's mfma_rate


def main():
    from kmeans_bench import alternate
    from project_bench import report
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="all")
    ap.add_argument("--rows", type=int, default=0, help="rows instead of each shape's own (smaller boxes)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--torch-reps", type=int, default=3, help="rounds of the torch yardstick (after 1)")
    ap.add_argument("--no-torch", action="store_true", help="leave the torch yardstick (and its float64 copy) out")
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20")
    shapes = list(SHAPES) if a.shape == "all" else a.shape.split(",")

    import torch
    import __graft_entry__ as g
    import bench as B
    pkg = g.load_package()
    N = pkg._native
    dev = torch.device("cuda", 0)

    def run(shape, n, d, k, P=256):
        X, y, offs = B.make_shard(torch, dev, n, d, P, "logistic", "f32", 7)
        offs = [int(v) for v in offs]
        parts = [pkg.DevicePartition(y[s:e], X[s:e], d) for s, e in zip(offs[:-1], offs[1:])]
        engine = pkg.HipEngine(pkg.PartitionedData(parts))
        st, cur = engine.stream, torch.cuda.current_stream(dev)
        n_tiles = sum(-(-(e - s) // 16) for s, e in zip(offs[:-1], offs[1:]))
        plan = N.gmm_plan("dense", "f32", d, k, n_tiles)
        db = plan["component_blocks"]
        cols = 16 * db * k
        gen = torch.Generator(device=dev).manual_seed(11)
        A = torch.randn((k, d, d), dtype=torch.float64, device=dev, generator=gen) / d ** 0.5
        b = torch.randn((k, d), dtype=torch.float64, device=dev, generator=gen)
        c = torch.full((k,), -float(torch.log(torch.tensor(float(k)))), dtype=torch.float64, device=dev)
        resp = torch.empty((n, k), dtype=torch.float64, device=dev)
        q = torch.empty((n, k), dtype=torch.float64, device=dev)
        ll = torch.zeros(1, dtype=torch.float64, device=dev)
        a1 = d + 1
        mom = torch.empty(k * a1 * a1, dtype=torch.float64, device=dev)
        step = torch.empty(k * a1 * a1 + 2, dtype=torch.float64, device=dev)
        engine.column_stats()   # (registers the rows)
        engine.ctx.gmm_responsibilities_device(k, A.data_ptr(), b.data_ptr(), c.data_ptr(), resp.data_ptr(), q.data_ptr(),
                                               ll.data_ptr(), st.cuda_stream)
        st.synchronize()
        omegas = [resp[:, j].contiguous() for j in range(k)]
        gout = torch.empty((d + 2) * (d + 2), dtype=torch.float64, device=dev)
        # the yardstick of (a): the k matrices side by side, each widened to 16 db columns
        Bm = torch.zeros((d, cols), dtype=torch.float64, device=dev)
        for j in range(k):
            Bm[:, 16 * db * j: 16 * db * j + d] = A[j]
        Y = torch.empty((n, cols), dtype=torch.float64, device=dev)
        lab = torch.empty(n, dtype=torch.float64, device=dev)
        ptr = lambda t: [t[s:e].data_ptr() if e > s else 0 for s, e in zip(offs[:-1], offs[1:])]
        ys, ls = ptr(Y), ptr(lab)
        C = torch.randn((k, d), dtype=torch.float64, device=dev, generator=gen)
        kstep = torch.empty(k * (d + 1) + 2, dtype=torch.float64, device=dev)

        def gramians():
            for om in omegas:
                engine.ctx.gramian_weighted_device(om.data_ptr(), gout.data_ptr(), st.cuda_stream)

        calls = [("gmm_responsibilities", st, lambda: engine.ctx.gmm_responsibilities_device(
                      k, A.data_ptr(), b.data_ptr(), c.data_ptr(), resp.data_ptr(), q.data_ptr(), ll.data_ptr(), st.cuda_stream)),
                 (f"project onto {cols} -> f64", st,
                  lambda: engine.ctx.project_device(cols, Bm.data_ptr(), N.F64, cols, ys, ls, st.cuda_stream)),
                 ("gmm_moments", st, lambda: engine.ctx.gmm_moments_device(k, resp.data_ptr(), mom.data_ptr(), st.cuda_stream)),
                 (f"{k} x gramian(weights=)", st, gramians),
                 ("gmm_step", st, lambda: engine.ctx.gmm_step_device(k, A.data_ptr(), b.data_ptr(), c.data_ptr(),
                                                                     step.data_ptr(), st.cuda_stream)),
                 ("kmeans_step", st, lambda: engine.ctx.kmeans_step_device(k, C.data_ptr(), kstep.data_ptr(), st.cuda_stream))]
        torch.cuda.synchronize()
        ms = alternate(torch, calls, a.reps, a.warmup)
        if not a.no_torch:
            Xd = X[:, :d].double()

            def torch_estep():
                t = torch.stack([c[j] - 0.5 * ((Xd @ A[j] - b[j]) ** 2).sum(dim=1) for j in range(k)], dim=1)
                lse = torch.logsumexp(t, dim=1)
                return torch.exp(t - lse[:, None]), lse.sum()
            calls.append(("torch float64 E-step", cur, torch_estep))
            ms.update(alternate(torch, calls[-1:], a.torch_reps, 1))
            del Xd
        extra = {"rows": n, "features": d, "k": k, "plan": plan}
        med = {name: report(shape, name, ms[name], extra if name == "gmm_responsibilities" else None) for name, _, _ in calls}
        nbz = -(-(d + 1) // 16)
        dpad = -(-d // 16) * 16
        es, mo = med["gmm_responsibilities"], med["gmm_moments"]
        line = {"shape": shape, "rows": n, "features": d, "k": k, "path": plan["path"],
                "estep_over_project_f64": round(es / med[f"project onto {cols} -> f64"], 3),
                "moments_over_k_gramians": round(mo / med[f"{k} x gramian(weights=)"], 3),
                "estep_Tfma_per_s": round(n * dpad * cols / es / 1e9, 2),
                "moments_Tfma_per_s_issued": round((n / 4) * k * (nbz * (nbz + 1) // 2) * 1024 / mo / 1e9, 2),
                "mfma_rate_Tfma_per_s": MFMA_RATE,
                "step_over_kmeans_step": round(med["gmm_step"] / med["kmeans_step"], 3)}
        if not a.no_torch:
            line["estep_over_torch_estep"] = round(es / med["torch float64 E-step"], 3)
        print(json.dumps(line), flush=True)
        del calls, omegas, Y, resp, q, X
        torch.cuda.empty_cache()

    for shape in shapes:
        if shape not in SHAPES:
            ap.error(f"unknown shape {shape}")
        n, d, k = SHAPES[shape]
        run(shape, a.rows or n, d, k)


if __name__ == "__main__":
    main()
