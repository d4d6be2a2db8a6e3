"""Time the bias evaluation's streaming pass (clite_debias_rows) on one GPU beside a device-to-device copy of the same bytes, and print a table
and one JSON line.

N = 32 768 rows of D = 2 048 f32 (256 MiB), R = 1 component: the kernel reads N D floats once and writes xn, xd (2 N D) and coef (N R), 768 MiB
in all. The yardstick is a copy on the same card that moves the same bytes: one third of them read, two thirds written is not what a copy does
(it reads as much as it writes), so two copies are shown: 384 MiB -> 384 MiB (the same total) and the plain 256 MiB -> 256 MiB of the input.
Each figure is the median over --repeats windows of --calls back-to-back calls between stream events, after a warm-up window; GB/s = the
bytes the algorithm needs (computed here from the shapes) over that time. The outputs of the first and the last call are compared bit for bit.
Also timed: xd alone (the evaluation's debiased bank when xn exists already) and coef alone (a read-only pass).

    python tools/bench_debias.py [--repeats 9] [--calls 20] [--rows 32768] [--dim 2048] [--components 1]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def timed(fn, repeats, calls):
    window(fn, calls)
    ms = [window(fn, calls) for _ in range(repeats)]
    return {"ms": statistics.median(ms), "ms_min_max": [min(ms), max(ms)]}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rows", type=int, default=32768)
    ap.add_argument("--dim", type=int, default=2048)
    ap.add_argument("--components", type=int, default=1)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_debias: no GPU visible; nothing here can be measured without one")
    from clip_lite_amd import hip
    N, D, R = a.rows, a.dim, a.components
    g = torch.Generator(device="cuda").manual_seed(1)
    x = 3.0 * torch.randn(N, D, device="cuda", generator=g)
    q, _ = torch.linalg.qr(torch.randn(D, R, device="cuda", generator=g))
    comps = q.t().contiguous()
    xn, xd = torch.empty_like(x), torch.empty_like(x)
    coef = torch.empty(N, R, device="cuda")
    hip.debias_rows(x, comps, N, D, R, xn, xd, coef)
    first = (xn.clone(), xd.clone(), coef.clone())
    res = {"metric": "debias_rows", "N": N, "D": D, "R": R, "repeats": a.repeats, "calls": a.calls}
    forms = {"all": (xn, xd, coef, 4 * (3 * N * D + N * R + R * D)), "xd_only": (None, xd, None, 4 * (2 * N * D + R * D)),
             "coef_only": (None, None, coef, 4 * (N * D + N * R + R * D))}
    for name, (o1, o2, o3, nbytes) in forms.items():
        r = timed(lambda: hip.debias_rows(x, comps, N, D, R, o1, o2, o3), a.repeats, a.calls)
        r["bytes"], r["GBps"] = nbytes, nbytes / r["ms"] / 1e6
        res[name] = r
    hip.debias_rows(x, comps, N, D, R, xn, xd, coef)
    res["bitwise_equal_reruns"] = all(bool(torch.equal(p, q_)) for p, q_ in zip(first, (xn, xd, coef)))
    half = 3 * N * D // 2
    src, dst = torch.empty(half, device="cuda").normal_(generator=g), torch.empty(half, device="cuda")
    for name, (s, d) in {"copy_same_total": (src, dst), "copy_of_input": (x.view(-1), xn.view(-1))}.items():
        r = timed(lambda: d.copy_(s), a.repeats, a.calls)
        r["bytes"], r["GBps"] = 8 * s.numel(), 8 * s.numel() / r["ms"] / 1e6
        res[name] = r
    res["rows_over_copy_same_total"] = res["all"]["GBps"] / res["copy_same_total"]["GBps"]
    print(f"{'':>16} {'ms':>8} {'min':>8} {'max':>8} {'MiB':>8} {'GB/s':>8}")
    for name in ("all", "xd_only", "coef_only", "copy_same_total", "copy_of_input"):
        r = res[name]
        print(f"{name:>16} {r['ms']:>8.4f} {r['ms_min_max'][0]:>8.4f} {r['ms_min_max'][1]:>8.4f} {r['bytes'] / 2**20:>8.1f} {r['GBps']:>8.1f}")
    print(f"clite_debias_rows at {res['rows_over_copy_same_total']:.2f} x the copy of the same bytes; reruns bitwise equal: {res['bitwise_equal_reruns']}")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
