"""Time the k-means of caption embeddings at COCO scale (N = 118 287, D = 768) for K = 10 and K = 256 on one GPU and print one JSON line per K:
one Lloyd iteration split into its three parts (the exact-f32 score GEMM, the assignment, accumulate + update), each between stream events
after a warm-up, median of the repeats, with the bytes each part moves over its time; and the whole `kmeans.fit` (wall clock, host loop and
its one synchronisation per iteration included). The embeddings are seeded unit-norm Gaussian rows.

    python tools/bench_kmeans.py [--repeats 20] [--niter 20]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_TBS = 8.0        # MI355X peak HBM3E bandwidth; the step's kernels reach 3.2 - 4.9 TB/s


def timed(fn, repeats, warmup=3):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--niter", type=int, default=20, help="iterations of the timed fit")
    a = ap.parse_args()
    from clip_lite_amd import kmeans
    N, D = 118287, 768
    X = torch.randn(N, D, device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))
    X = X / X.norm(dim=1, keepdim=True)
    for K in (10, 256):
        st = kmeans._State(X, K)
        st.set_centroids(X[kmeans.init_rows(N, K, 1234).cuda()])
        st.assign_step(), st.accumulate(), st.update()
        Kp = st.Kp
        from clip_lite_amd import hip
        gemm = lambda: hip.gemm_nt(hip.F32, st.X, st.C, N, Kp, D, hip.epilogue(st.scores, Kp, out_f32=True), lda=st.ld)
        assign = lambda: hip.kmeans_assign(st.scores, Kp, st.hc, st.xnorm, N, K, st.assign, st.dist, st.stat[K:K + 1])
        accum = lambda: (st.accumulate(), st.update())
        parts = {"gemm": (gemm, 4 * (N * D + Kp * D + N * Kp)), "assign": (assign, 4 * (N * Kp + 3 * N)),
                 "accumulate_update": (accum, 4 * (N * D + 6 * N + 2 * K * D))}
        out = {"N": N, "D": D, "K": K, "hbm_peak_tb_s": HBM_TBS}
        for name, (fn, nbytes) in parts.items():
            med, best = timed(fn, a.repeats)
            out[name] = {"ms_median": round(med, 4), "ms_min": round(best, 4), "mbytes": round(nbytes / 1e6, 1), "tb_s": round(nbytes / med / 1e9, 3)}
        out["gemm"]["tflops"] = round(2.0 * N * Kp * D / out["gemm"]["ms_median"] / 1e9, 2)
        out["iteration_ms"] = round(sum(out[p]["ms_median"] for p in parts), 4)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = kmeans.fit(X, K, niter=a.niter, seed=1234)
        out["fit"] = {"niter": a.niter, "iterations": res["iterations"], "wall_ms": round(1e3 * (time.perf_counter() - t0), 2),
                      "inertia": res["inertia"]}
        out["fit"]["wall_ms_per_iteration"] = round(out["fit"]["wall_ms"] / (res["iterations"] + 1), 3)
        print(json.dumps(out))


if __name__ == "__main__":
    main()
