"""Time the k-NN evaluation's three kernels on one GPU, each between stream events, and print a table and one JSON line.

ImageNet scale: a bank of 1 281 167 x 2048 seeded unit rows (f32, 10.5 GB), one block of 1 024 queries, k = 200, the bank in chunks of 65 536
rows. A sweep is what knn.topk does for one query block: per chunk one exact-f32 clite_gemm_nt into the score scratch and one
clite_knn_topk_merge; the GEMMs and the merges of a sweep are timed separately (sums over the chunks, and the merge of the first chunk, which
fills the empty lists, apart from the later ones). Then the vote (ks 10, 20, 100, 200; 1 000 classes). After one warm-up sweep the figures are
medians over --repeats sweeps in one process. The merge's bytes are the scratch tiles it reads once (Q x Nc x 4 per chunk).

The same at a bank of 100 000 rows, where the whole 1 024 x 100 000 score matrix fits one tile; there the yardstick is torch.topk(scores, 200)
on the same matrix on the same card, against one merge launch over it (empty lists), and the two selections' scores are compared.

    python tools/bench_knn.py [--repeats 7] [--bank 1281167] [--small-bank 100000]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

Q, D, K, CHUNK, CLASSES = 1024, 2048, 200, 65536, 1000
KS = (10, 20, 100, 200)


def unit_rows(n, seed):
    """f32 [n][D] unit rows from a seeded device generator, made 65 536 rows at a time."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    out = torch.empty(n, D, device="cuda")
    for r in range(0, n, CHUNK):
        x = torch.randn(min(CHUNK, n - r), D, device="cuda", generator=g)
        out[r:r + x.shape[0]] = x / x.norm(dim=1, keepdim=True)
    return out


def sweep(hip, xq, bank, scratch, top_s, top_i):
    """One pass of a query block over the bank; returns (gemm ms per chunk, merge ms per chunk)."""
    N = bank.shape[0]
    ev = []
    for base in range(0, N, CHUNK):
        nc = min(CHUNK, N - base)
        assert nc % 8 == 0 or base + nc == N
        n8 = nc // 8 * 8                     # the benchmark drops the bank's last N % 8 rows instead of copying a padded tail
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        hip.gemm_nt(hip.F32, xq, bank[base:base + n8], Q, n8, D, hip.epilogue(scratch, n8, out_f32=True))
        e[1].record()
        hip.knn_topk_merge(scratch, n8, Q, n8, base, K, min(K, base), top_s, top_i)
        e[2].record()
        ev.append((e, n8))
    torch.cuda.synchronize()
    return [e[0].elapsed_time(e[1]) for e, _ in ev], [e[1].elapsed_time(e[2]) for e, _ in ev], [n for _, n in ev]


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
    return statistics.median(ms), min(ms), max(ms)


def bench_bank(hip, N, repeats):
    bank, xq = unit_rows(N, 1), unit_rows(Q, 2)
    scratch = torch.empty(Q, CHUNK, device="cuda")
    top_s = torch.empty(Q, K, device="cuda")
    top_i = torch.empty(Q, K, device="cuda", dtype=torch.int32)
    sweep(hip, xq, bank, scratch, top_s, top_i)                      # warm-up: first launches, the GEMM's tile selection
    runs = [sweep(hip, xq, bank, scratch, top_s, top_i) for _ in range(repeats)]
    cols = runs[0][2]
    gemm = [sum(r[0]) for r in runs]
    merge = [sum(r[1]) for r in runs]
    first = [r[1][0] for r in runs]
    later = [sum(r[1][1:]) for r in runs]
    med = statistics.median
    out = {"bank": N, "chunks": len(cols), "gemm_ms": med(gemm), "gemm_ms_min_max": [min(gemm), max(gemm)], "merge_ms": med(merge),
           "merge_ms_min_max": [min(merge), max(merge)], "merge_first_chunk_ms": med(first), "merge_later_chunks_ms": med(later),
           "gemm_TFLOPs": 2.0 * Q * sum(cols) * D / med(gemm) / 1e9, "merge_bytes": 4 * Q * sum(cols),
           "merge_TBps": 4.0 * Q * sum(cols) / med(merge) / 1e9}
    if len(cols) > 1:
        out["merge_later_chunks_TBps"] = 4.0 * Q * sum(cols[1:]) / med(later) / 1e9
    out["merge_first_chunk_TBps"] = 4.0 * Q * cols[0] / med(first) / 1e9
    labels = torch.randint(0, CLASSES, (N,), device="cuda", dtype=torch.int32, generator=torch.Generator(device="cuda").manual_seed(3))
    pred = torch.empty(len(KS), Q, hip.KNN_PRED, device="cuda", dtype=torch.int32)
    v = timed(lambda: hip.knn_vote(top_s, top_i, labels, Q, K, N, CLASSES, KS, 1 / 0.07, None, pred), repeats)
    out["vote_ms"], out["vote_ms_min_max"] = v[0], [v[1], v[2]]
    out["merge_share_of_gemm"] = out["merge_ms"] / out["gemm_ms"]
    return out, bank, xq


def bench_against_torch_topk(hip, bank, xq, repeats):
    """One tile over the whole (small) bank: torch.topk on it against one merge launch from empty lists."""
    N = bank.shape[0] // 8 * 8
    scores = torch.empty(Q, N, device="cuda")
    hip.gemm_nt(hip.F32, xq, bank[:N], Q, N, D, hip.epilogue(scores, N, out_f32=True))
    top_s = torch.empty(Q, K, device="cuda")
    top_i = torch.empty(Q, K, device="cuda", dtype=torch.int32)
    ours = timed(lambda: hip.knn_topk_merge(scores, N, Q, N, 0, K, 0, top_s, top_i), repeats)
    ref = timed(lambda: torch.topk(scores, K, dim=1), repeats)
    want = torch.topk(scores, K, dim=1)
    return {"bank": N, "merge_one_tile_ms": ours[0], "merge_one_tile_ms_min_max": [ours[1], ours[2]], "merge_one_tile_TBps": 4.0 * Q * N / ours[0] / 1e9,
            "torch_topk_ms": ref[0], "torch_topk_ms_min_max": [ref[1], ref[2]], "torch_topk_over_merge": ref[0] / ours[0],
            "scores_equal_torch_topk": bool(torch.equal(want.values, top_s)),
            "indices_equal_torch_topk": bool(torch.equal(want.indices.to(torch.int32), top_i))}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--bank", type=int, default=1281167)
    ap.add_argument("--small-bank", type=int, default=100000)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_knn: no GPU visible; nothing here can be measured without one")
    from clip_lite_amd import hip
    res = {"metric": "knn", "Q": Q, "D": D, "K": K, "chunk": CHUNK, "repeats": a.repeats}
    small, bank, xq = bench_bank(hip, a.small_bank, a.repeats)
    res["small"] = small
    res["small_vs_torch_topk"] = bench_against_torch_topk(hip, bank, xq, a.repeats)
    del bank
    torch.cuda.empty_cache()
    res["large"], _, _ = bench_bank(hip, a.bank, a.repeats)
    print(f"{'bank':>9} {'GEMM ms':>9} {'TFLOP/s':>8} {'merge ms':>9} {'TB/s':>6} {'first chunk ms':>15} {'later ms':>9} {'later TB/s':>10} {'vote ms':>8}")
    for r in (res["small"], res["large"]):
        print(f"{r['bank']:>9} {r['gemm_ms']:>9.3f} {r['gemm_TFLOPs']:>8.1f} {r['merge_ms']:>9.3f} {r['merge_TBps']:>6.2f} {r['merge_first_chunk_ms']:>15.3f} "
              f"{r['merge_later_chunks_ms']:>9.3f} {r.get('merge_later_chunks_TBps', float('nan')):>10.2f} {r['vote_ms']:>8.3f}")
    t = res["small_vs_torch_topk"]
    print(f"one tile {Q} x {t['bank']}: merge {t['merge_one_tile_ms']:.3f} ms ({t['merge_one_tile_TBps']:.2f} TB/s), torch.topk {t['torch_topk_ms']:.3f} ms "
          f"({t['torch_topk_over_merge']:.2f} x), scores equal {t['scores_equal_torch_topk']}")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
