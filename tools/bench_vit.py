"""Time the ViT image tower on one GPU: forward + backward of ViT-B/32 at batch 128 and 224 pixels in bf16 beside ResNet-50's in the same process,
and the three streaming kernels of csrc/vit_ops.hip beside a device-to-device copy (hipMemcpy) of the same bytes. Prints a table and one JSON line.

Both towers run through ImageEncoder on eager launches (no hipGraph: the figure includes what the host needs to enqueue a pass, which for a
few hundred small launches is not nothing); a pass is the forward, then the backward from a fixed feature gradient, parameter gradients
accumulated into the arena. Each figure is the median over --repeats windows of --calls back-to-back calls between stream events, after a
warm-up window. GB/s = the bytes the kernel must move (computed here from the shapes: every input read once, every output written once) over
that time; the copy moves the same total, half read and half written. At these sizes (10 - 115 MB) the tensors fit the 256 MB last-level cache,
for the kernels and for the copy alike.

With --patch-dropout R (FLIP patch dropout, MODEL.VISUAL.PATCH_DROPOUT) the same process also times the tower's forward + backward with each image
keeping kept_patches(P, R) patches, beside the ratio-0 figure and the ratio of the row counts B L' / B L, and the three streaming keep-kernels
at those shapes beside a copy of the bytes they move (the index kernel, latency-bound, is timed without a copy beside it).

    python tools/bench_vit.py [--repeats 7] [--calls 10] [--batch 128] [--size 224] [--skip-resnet] [--patch-dropout R]
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


class _Holder(torch.nn.Module):
    def __init__(self, enc):
        super().__init__()
        self.image_encoder = enc


def tower(name, size, patch_dropout=0.0):
    from clip_lite_amd.encoder import ImageEncoder
    from clip_lite_amd.model import attach_runtime
    holder = _Holder(ImageEncoder(name, image_size=size, patch_dropout=patch_dropout)).to("cuda").train()
    holder.rt = attach_runtime(holder, torch.device("cuda", torch.cuda.current_device()), True)
    return holder


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--skip-resnet", action="store_true")
    ap.add_argument("--patch-dropout", type=float, default=0.0, help="also time the tower and the keep-kernels at this ratio")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_vit: no GPU visible; nothing here can be measured without one")
    from clip_lite_amd import hip
    B, S, p, C = a.batch, a.size, 32, 768
    g = torch.Generator(device="cuda").manual_seed(1)
    image = torch.randn(B, 3, S, S, device="cuda", generator=g)
    res = {"metric": "vit_b_32_fwd_bwd", "batch": B, "size": S, "dtype": "bf16", "repeats": a.repeats, "calls": a.calls}

    R = a.patch_dropout
    towers = [("vit_b_32", "vit_b_32", 0.0)] + ([("vit_b_32_keep", "vit_b_32", R)] if R > 0 else []) + ([] if a.skip_resnet else [("resnet50", "resnet50", 0.0)])
    for name, net, ratio in towers:
        holder = tower(net, S, ratio)
        dfeat = torch.randn(B, holder.image_encoder.out_dim, device="cuda", generator=g).to(torch.bfloat16)

        def fwd_bwd():
            holder.image_encoder(image).backward(dfeat)

        def fwd():
            with torch.no_grad():
                holder.image_encoder(image)
        res[name] = {"fwd_bwd": timed(fwd_bwd, a.repeats, a.calls), "fwd": timed(fwd, a.repeats, a.calls),
                     "parameters": sum(q.numel() for q in holder.parameters())}
        res[name]["images_per_s"] = B / res[name]["fwd_bwd"]["ms"] * 1e3
        del holder
        torch.cuda.empty_cache()

    # the three kernels at the tower's shapes
    P, K = (S // p) ** 2, 3 * p * p
    L = P + 1
    bf = torch.bfloat16
    patches = torch.empty(B * P, K, device="cuda", dtype=bf)
    e = torch.randn(B * P, C, device="cuda", generator=g).to(bf)
    cls, pos = torch.randn(C, device="cuda", generator=g).to(bf), torch.randn(L, C, device="cuda", generator=g).to(bf)
    s0, ds0, de = torch.empty(B * L, C, device="cuda", dtype=bf), torch.randn(B * L, C, device="cuda", generator=g).to(bf), torch.empty(B * P, C, device="cuda", dtype=bf)
    dpos, dcls = torch.zeros(L, C, device="cuda"), torch.zeros(C, device="cuda")
    kernels = {
        "patchify": (lambda: hip.vit_patchify(hip.BF16, image, patches, B, S, S, p), 4 * image.numel() + 2 * patches.numel()),
        "tokens_fwd": (lambda: hip.vit_tokens_fwd(hip.BF16, e, cls, pos, s0, B, P, C), 2 * (e.numel() + cls.numel() + pos.numel() + s0.numel())),
        "tokens_bwd": (lambda: hip.vit_tokens_bwd(hip.BF16, ds0, de, dpos, dcls, B, P, C), 2 * (ds0.numel() + de.numel()) + 8 * (dpos.numel() + dcls.numel())),
    }
    res["kernels"] = {}
    for name, (fn, nbytes) in kernels.items():
        r = timed(fn, a.repeats, a.calls)
        half = nbytes // 2 // 16 * 16
        src, dst = torch.empty(half, device="cuda", dtype=torch.uint8), torch.empty(half, device="cuda", dtype=torch.uint8)
        c = timed(lambda: dst.copy_(src), a.repeats, a.calls)
        r["bytes"], r["GBps"] = nbytes, nbytes / r["ms"] / 1e6
        r["copy_ms"], r["copy_GBps"] = c["ms"], 2 * half / c["ms"] / 1e6
        res["kernels"][name] = r
    if R > 0:
        from clip_lite_amd.vit import kept_patches
        Kk = kept_patches(P, R)
        Lk = Kk + 1
        res["patch_dropout"] = {"ratio": R, "patches": P, "kept": Kk, "rows": B * Lk, "rows_full": B * L, "row_ratio": Lk / L,
                                "time_ratio": res["vit_b_32_keep"]["fwd_bwd"]["ms"] / res["vit_b_32"]["fwd_bwd"]["ms"]}
        idx, inv = torch.empty(B, Kk, device="cuda", dtype=torch.int32), torch.empty(B, P, device="cuda", dtype=torch.int32)
        hip.vit_keep_indices(idx, inv, B, P, Kk, 1234, 1)
        pk, ek = torch.empty(B * Kk, K, device="cuda", dtype=bf), torch.randn(B * Kk, C, device="cuda", generator=g).to(bf)
        sk, dsk, dek = torch.empty(B * Lk, C, device="cuda", dtype=bf), torch.randn(B * Lk, C, device="cuda", generator=g).to(bf), torch.empty(B * Kk, C, device="cuda", dtype=bf)
        keep = {
            "keep_indices": (lambda: hip.vit_keep_indices(idx, inv, B, P, Kk, 1234, 1), 4 * (idx.numel() + inv.numel())),
            "patchify_keep": (lambda: hip.vit_patchify_keep(hip.BF16, image, idx, pk, B, S, S, p, Kk), 6 * pk.numel() + 4 * idx.numel()),
            "tokens_keep_fwd": (lambda: hip.vit_tokens_keep_fwd(hip.BF16, ek, cls, pos, idx, sk, B, P, Kk, C),
                                2 * (ek.numel() + cls.numel() + pos.numel() + sk.numel()) + 4 * idx.numel()),
            "tokens_keep_bwd": (lambda: hip.vit_tokens_keep_bwd(hip.BF16, dsk, inv, dek, dpos, dcls, B, P, Kk, C),
                                2 * (dsk.numel() + dek.numel()) + 8 * (dpos.numel() + dcls.numel()) + 4 * inv.numel()),
        }
        for name, (fn, nbytes) in keep.items():
            r = timed(fn, a.repeats, a.calls)
            r["bytes"], r["GBps"] = nbytes, nbytes / r["ms"] / 1e6
            if name != "keep_indices":
                half = nbytes // 2 // 16 * 16
                src, dst = torch.empty(half, device="cuda", dtype=torch.uint8), torch.empty(half, device="cuda", dtype=torch.uint8)
                c = timed(lambda: dst.copy_(src), a.repeats, a.calls)
                r["copy_ms"], r["copy_GBps"] = c["ms"], 2 * half / c["ms"] / 1e6
            else:
                r["copy_ms"], r["copy_GBps"] = float("nan"), float("nan")
            res["kernels"][name] = r
    first = dpos.clone()
    dpos.zero_(), dcls.zero_()
    hip.vit_tokens_bwd(hip.BF16, ds0, de, dpos, dcls, B, P, C)
    one = dpos.clone()
    dpos.zero_(), dcls.zero_()
    hip.vit_tokens_bwd(hip.BF16, ds0, de, dpos, dcls, B, P, C)
    res["tokens_bwd_bitwise_equal_reruns"] = bool(torch.equal(one, dpos)) and bool(torch.isfinite(first).all())

    print(f"{'':>12} {'fwd+bwd ms':>11} {'min':>8} {'max':>8} {'fwd ms':>8} {'img/s':>9} {'params':>12}")
    for name in ("vit_b_32", "vit_b_32_keep", "resnet50"):
        if name in res:
            r = res[name]
            fb = r["fwd_bwd"]
            print(f"{name:>12} {fb['ms']:>11.3f} {fb['ms_min_max'][0]:>8.3f} {fb['ms_min_max'][1]:>8.3f} {r['fwd']['ms']:>8.3f} {r['images_per_s']:>9.0f} {r['parameters']:>12}")
    print(f"{'':>12} {'us':>8} {'min':>8} {'max':>8} {'MB':>8} {'GB/s':>8} {'copy us':>8} {'copy GB/s':>9}")
    for name, r in res["kernels"].items():
        print(f"{name:>12} {1e3 * r['ms']:>8.1f} {1e3 * r['ms_min_max'][0]:>8.1f} {1e3 * r['ms_min_max'][1]:>8.1f} {r['bytes'] / 1e6:>8.1f} {r['GBps']:>8.0f} "
              f"{1e3 * r['copy_ms']:>8.1f} {r['copy_GBps']:>9.0f}")
    if R > 0:
        d = res["patch_dropout"]
        print(f"patch dropout {R}: {d['kept']} of {d['patches']} patches, rows {d['rows']} / {d['rows_full']} = {d['row_ratio']:.3f}, "
              f"fwd+bwd time ratio {d['time_ratio']:.3f}")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
