"""Time the logistic-regression probe's solver (clip-lite_amd/logreg.py) at ImageNet shape (N = 1 281 167 rows, D = 2048 features, C = 1000
classes, P = 4 costs) on one GPU and print one JSON line: the pieces of one Newton iteration between stream events (the softmax / gradient
operand, the Hessian apply and the line-search evaluation with their bytes per second against the 6.3 TB/s an HBM-bound kernel reaches here; the
two exact-f32 GEMMs of a CG iteration with their FLOP/s; the per-problem vector kernels), then a whole logreg.fit on the same seeded features
with its Newton / CG counts and the share of its time that the GEMMs account for (their count x their measured time).

    python tools/bench_logreg.py [--repeats 5] [--rows 1281167] [--features 2048] [--classes 1000] [--cost 1 10 100 1000] [--skip-solve]
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

HBM_TBPS = 6.3                  # what a streaming kernel achieves on the MI355X
CHUNK = 65536


def clustered_rows(n, d, classes, seed):
    """(f32 [n][d] unit rows, int64 [n] labels): seeded Gaussian class clusters, made 65 536 rows at a time on the device."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    centres = torch.randn(classes, d, device="cuda", generator=g)
    y = torch.randint(0, classes, (n,), device="cuda", generator=g)
    y[:classes] = torch.arange(classes, device="cuda")                 # every class present
    out = torch.empty(n, d, device="cuda")
    for r in range(0, n, CHUNK):
        m = min(CHUNK, n - r)
        x = 0.25 * centres[y[r:r + m]] + torch.randn(m, d, device="cuda", generator=g)
        out[r:r + m] = x / x.norm(dim=1, keepdim=True)
    return out, y


def timed(fn, repeats):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return {"ms": statistics.median(ms), "ms_min_max": [min(ms), max(ms)]}


def bench_pieces(hip, logreg, X, y, C, costs, repeats):
    from clip_lite_amd.svm import augment
    N, D = X.shape
    P = len(costs)
    Dp, Cp = logreg._ceil8(D + 1), logreg._ceil8(C)
    ldz, n = P * Cp, Cp * Dp
    dev = X.device
    Xt = augment(X)
    y32 = y.to(torch.int32)
    cd = torch.tensor(costs, device=dev, dtype=torch.float32)
    w = torch.ones(N, P, device=dev)
    g = torch.Generator(device="cuda").manual_seed(7)
    W = torch.zeros(P * Cp, Dp, device=dev)
    W.view(P, Cp, Dp)[:, :C, :D + 1] = 0.5 * torch.randn(P, C, D + 1, device=dev, generator=g)
    G, Xd, R, Dc, HD = (torch.zeros(P * Cp, Dp, device=dev) for _ in range(5))
    Z, Pr, T = (torch.zeros(N, ldz, device=dev) for _ in range(3))
    loss = torch.zeros(P, device=dev)
    work = torch.zeros(2 * hip.logreg_blocks(N) * P, device=dev)
    state = torch.zeros(P, hip.LOGREG_STATE, device=dev)
    state[:, 9] = 1.0
    out = {}
    arr = 4.0 * N * ldz                                                # bytes of one [N][P * Cp] operand
    flop = 2.0 * N * ldz * Dp

    def rate(r, nbytes):
        r["TBps"] = nbytes / r["ms"] / 1e9
        r["share_of_6.3_TBps"] = r["TBps"] / HBM_TBPS
        return r

    out["gemm_nt"] = timed(lambda: logreg._nt(Xt, W, N, ldz, Dp, Z), repeats)
    out["gemm_nt"]["TFLOPs"] = flop / out["gemm_nt"]["ms"] / 1e9
    out["softmax"] = rate(timed(lambda: hip.logreg_softmax(Z, y32, cd, w, N, P, C, ldz, Pr, T, loss, work), repeats), 3 * arr)
    out["gemm_tn"] = timed(lambda: logreg._tn(T, Xt, ldz, Dp, N, G, W), repeats)
    out["gemm_tn"]["TFLOPs"] = flop / out["gemm_tn"]["ms"] / 1e9
    out["newton_begin"] = timed(lambda: hip.logreg_newton_begin(G, n, n, P, Xd, R, Dc, state, 0.0, 1000000, 0.1), repeats)
    logreg._nt(Xt, Dc, N, ldz, Dp, T)
    out["hess_apply"] = rate(timed(lambda: hip.logreg_hess_apply(Pr, cd, w, N, P, C, ldz, T), repeats), 3 * arr)
    logreg._tn(T, Xt, ldz, Dp, N, HD, Dc)
    state[:, 4] = 0.0                                                  # CG tolerance 0: the update below never stops
    out["cg_update"] = timed(lambda: hip.logreg_cg_update(HD, n, n, P, Xd, R, Dc, state), repeats)
    logreg._nt(Xt, Xd, N, ldz, Dp, T)
    L = hip.lib()
    st = hip.stream_ptr(Z)
    out["ray_begin"] = timed(lambda: hip.check(L.clite_logreg_ray_begin(hip.p(G), hip.p(W), hip.p(Xd), n, n, P, hip.p(state), st), "ray_begin"), repeats)
    state[:, 18], state[:, 13] = 0.0, 1.0                              # every search open at t = 1
    out["ray_eval"] = rate(timed(lambda: hip.check(L.clite_logreg_ray_eval(hip.p(Z), hip.p(T), hip.p(y32), hip.p(cd), hip.p(w), N, P, C, ldz,
                                                                           hip.p(state), hip.p(work), st), "ray_eval"), repeats), 2 * arr)

    def step():
        state[:, 18] = 0.0
        hip.check(L.clite_logreg_ray_step(hip.p(work), N, P, hip.p(state), 0, st), "ray_step")

    out["ray_step"] = timed(step, repeats)
    state[:, 18], state[:, 5] = 1.0, 1e-3
    out["ray_finish"] = timed(lambda: hip.check(L.clite_logreg_ray_finish(hip.p(W), hip.p(Xd), n, n, P, hip.p(state), st), "ray_finish"), repeats)
    out["operand_GB"] = arr / 1e9
    out["cg_iteration_ms"] = out["gemm_nt"]["ms"] + out["hess_apply"]["ms"] + out["gemm_tn"]["ms"] + out["cg_update"]["ms"]
    out["gemm_share_of_cg_iteration"] = (out["gemm_nt"]["ms"] + out["gemm_tn"]["ms"]) / out["cg_iteration_ms"]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rows", type=int, default=1281167)
    ap.add_argument("--features", type=int, default=2048)
    ap.add_argument("--classes", type=int, default=1000)
    ap.add_argument("--cost", type=float, nargs="+", default=[1.0, 10.0, 100.0, 1000.0])
    ap.add_argument("--tol", type=float, default=1e-5)
    ap.add_argument("--max-newton", type=int, default=50)
    ap.add_argument("--skip-solve", action="store_true", help="time the pieces only")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_logreg: no GPU visible; nothing here can be measured without one")
    from clip_lite_amd import hip, logreg
    res = {"metric": "logreg", "N": a.rows, "D": a.features, "C": a.classes, "costs": a.cost, "repeats": a.repeats}
    X, y = clustered_rows(a.rows, a.features, a.classes, 0)
    res["pieces"] = p = bench_pieces(hip, logreg, X, y, a.classes, a.cost, a.repeats)
    torch.cuda.empty_cache()
    for k in ("gemm_nt", "softmax", "gemm_tn", "hess_apply", "ray_eval", "newton_begin", "cg_update", "ray_begin", "ray_step", "ray_finish"):
        r = p[k]
        extra = f"{r['TBps']:.2f} TB/s ({100 * r['share_of_6.3_TBps']:.0f} % of {HBM_TBPS})" if "TBps" in r else (f"{r['TFLOPs']:.1f} TFLOP/s" if "TFLOPs" in r else "")
        print(f"{k:>13} {r['ms']:>10.3f} ms  {extra}", flush=True)
    if not a.skip_solve:
        small = min(a.rows, 4096)
        logreg.fit(X[:small].contiguous(), y[:small] % 8, 8, a.cost, max_newton=2)        # warm-up of the solver's host path
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sol = logreg.fit(X, y, a.classes, a.cost, tol=a.tol, max_newton=a.max_newton)
        torch.cuda.synchronize()
        s = time.perf_counter() - t0
        iters = int(sol["newton"].max())
        n_nt, n_tn = 2 * iters + 1 + sol["cg_launched"], iters + 1 + sol["cg_launched"]
        gemm_s = (n_nt * p["gemm_nt"]["ms"] + n_tn * p["gemm_tn"]["ms"]) / 1e3
        res["solve"] = {"s": s, "newton": sol["newton"].tolist(), "cg": sol["cg"].tolist(), "cg_launched": sol["cg_launched"],
                        "rel_grad": sol["rel_grad"].tolist(), "converged": bool((sol["rel_grad"] <= a.tol).all()), "gemm_nt_calls": n_nt,
                        "gemm_tn_calls": n_tn, "gemm_s_from_piece_times": gemm_s, "gemm_share_of_solve": gemm_s / s}
        print(f"solve {s:.1f} s: newton {res['solve']['newton']}, cg {res['solve']['cg']} ({sol['cg_launched']} launched), GEMMs {100 * gemm_s / s:.0f} % of it")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
