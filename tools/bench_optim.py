"""Update-path timing of an optimizer and its layer-wise form on one item table (bf16 copy on), in one process, between stream events:

    --pair sgd-lars     clite_sgd_step against clite_lars_norms + clite_lars_step on the benchmark model (ResNet-50 + BERT-base)
    --pair adamw-lamb   clite_adamw_step against clite_lamb_moments + clite_lamb_step on the transformer pair (ViT-B/32 + BERT-base)

The model is laid out on meta tensors (shapes only); the flat buffers hold random values. Every timed call is preceded by a refill of the gradient
buffer (the updates zero it) and of the optimizer state, outside the timed region, for both optimizers alike; the two are timed alternately,
repeat by repeat, and the medians are reported. Prints one JSON line.

Bytes per element on a non-sync step. SGD reads p, g, v (12 B) and writes p, v, g, bf16 (14 B); the norms read p and g once more (+8 B), so the
expectation for LARS is (26 + 8) / 26 = 1.31 x the SGD update. AdamW reads p, g, m, v2 (16 B) and writes p, m, v2, g, bf16 (18 B); LAMB's moments
pass reads the same 16 B and writes m, v2 (8 B), its step pass reads p, m, v2 (12 B) and writes p, g, bf16 (10 B): 46 / 34 = 1.35 x the AdamW update.

    python tools/bench_optim.py [--pair sgd-lars|adamw-lamb] [--repeats 30] [--warmup 5]
"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def item_table(hip, chunk, pair):
    """(device bytes of the table, items, norm slots, arena elements, elements inside items, elements of adapted tensors)"""
    from clip_lite_amd.encoder import ImageEncoder, TextEncoder
    from clip_lite_amd.loss import JSDInfoMaxLoss
    from clip_lite_amd.model import VLInfoModel
    from clip_lite_amd.runtime import Arena
    image, width = ("resnet50", 2048) if pair == "sgd-lars" else ("vit_b_32", 768)
    with torch.device("meta"):
        M = VLInfoModel(TextEncoder(mode="train_sbert", num_hidden_layers=12), ImageEncoder(image), JSDInfoMaxLoss(width, 768, "dot", 0.1, True, True),
                        "train_sbert", is_amp=True)
    named = list(M.named_parameters())
    _, index, total = Arena.layout(named, M.text_encoder.strans.contiguous_groups("text_encoder.strans."))
    rows, slots, adapted = [], 0, 0
    for n, p in named:
        o, numel = index[n]
        tag = 0
        if p.dim() >= 2:
            slots += 1
            tag = slots
            adapted += numel
        lr, wd = ((0.2 if "image_encoder" in n else 1e-3), 1e-4) if pair == "sgd-lars" else (1e-3, 1e-2)
        n4 = (numel + 3) // 4 * 4
        for s in range(0, n4, chunk):
            rows.append((o + s, min(chunk, n4 - s), lr, wd, tag))
    rows.sort()
    arr = (hip.OptimItem * len(rows))(*[hip.OptimItem(*r) for r in rows])
    dev = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()
    return dev, len(rows), slots, total, sum(r[1] for r in rows), adapted


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--pair", choices=["sgd-lars", "adamw-lamb"], default="sgd-lars")
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    from clip_lite_amd import hip
    from clip_lite_amd.optim.fused_sgd import CHUNK
    items, n_items, slots, total, covered, adapted = item_table(hip, CHUNK, a.pair)
    ip = C.c_void_p(items.data_ptr())
    gen = torch.Generator(device="cuda").manual_seed(0)
    p = torch.randn(total, device="cuda", generator=gen) * 0.05
    g0 = torch.randn(total, device="cuda", generator=gen) * 1e-3
    g, slow, lp = g0.clone(), p.clone(), p.to(torch.bfloat16)
    norms, partials = torch.zeros(slots, 2, device="cuda"), torch.zeros(2 * n_items, device="cuda")
    ss = (g0.double() ** 2).sum().float().reshape(1)
    # hp: lr multiplier 0 (the parameters stay put over the repeats; the kernels do the same work), momentum / beta1, clip at half the norm, no sync,
    # alpha, pre-scale; then eta, eps | beta2, eps, the bias corrections of step 1000, 1 - beta1, 1 - beta2, TRUST_CLIP off
    common = [0.0, 0.9, float(ss.sqrt()) / 2, 0.0, 0.5, 1.0]
    if a.pair == "sgd-lars":
        base, layer, first, second = "sgd", "lars", "norms", "step"
        hp = torch.tensor(common + [1e-3, 1e-8], device="cuda")
        v = torch.zeros_like(p)
        state = [(v, None)]          # (buffer, its value before every call; None: zeros)
        calls = {"base": lambda h: hip.sgd_step(p, g, v, slow, lp, ip, n_items, h, ss),
                 "first": lambda h: hip.lars_norms(p, g, ip, n_items, partials, norms),
                 "second": lambda h: hip.lars_step(p, g, v, slow, lp, ip, n_items, h, ss, norms)}
    else:
        base, layer, first, second = "adamw", "lamb", "moments", "step"
        hp = torch.tensor(common + [0.999, 1e-6, 1 - 0.9 ** 1000, 1 - 0.999 ** 1000, 1 - 0.9, 1 - 0.999, 0.0, 0.0, 0.0, 0.0], device="cuda")
        m0 = torch.randn(total, device="cuda", generator=gen) * 1e-3
        v0 = m0 * m0 * 1.5
        m, v2 = m0.clone(), v0.clone()
        state = [(m, m0), (v2, v0)]
        calls = {"base": lambda h: hip.adamw_step(p, g, m, v2, slow, lp, ip, n_items, h, ss),
                 "first": lambda h: hip.lamb_moments(p, g, m, v2, ip, n_items, h, ss, partials, norms),
                 "second": lambda h: hip.lamb_step(p, g, m, v2, slow, lp, ip, n_items, h, ss, norms)}
    hp_sync = hp.clone()
    hp_sync[3] = 1.0

    def both(h):
        calls["first"](h)
        calls["second"](h)

    k_base, k_first, k_second, k_both = f"{base}_step", f"{layer}_{first}", f"{layer}_{second}", f"{layer}_{first}_and_{second}"
    cases = [(k_base, calls["base"], hp), (k_first, calls["first"], hp), (k_second, calls["second"], hp), (k_both, both, hp),
             (k_base + "_sync", calls["base"], hp_sync), (k_both + "_sync", both, hp_sync)]
    times = {name: [] for name, _, _ in cases}
    for r in range(a.warmup + a.repeats):
        for name, fn, h in cases:          # alternately, repeat by repeat: drift of the clocks hits every case alike
            g.copy_(g0)
            for buf, init in state:
                buf.zero_() if init is None else buf.copy_(init)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(h)
            e1.record()
            torch.cuda.synchronize()
            if r >= a.warmup:
                times[name].append(e0.elapsed_time(e1) * 1e3)
    assert int((g != 0).sum()) <= total - covered and torch.isfinite(p).all() and norms.min().item() > 0          # g is zero inside items
    med = {k: sorted(t)[len(t) // 2] for k, t in times.items()}
    out = {"device": torch.cuda.get_device_name(0), "arena_elements": total, "elements_in_items": covered, "adapted_elements": adapted, "items": n_items,
           "norm_slots": slots, "repeats": a.repeats, "unit": "us (median)", **{k: round(x, 1) for k, x in med.items()},
           "min_us": {k: round(min(t), 1) for k, t in times.items()},
           f"{layer}_over_{base}": round(med[k_both] / med[k_base], 3),
           f"{layer}_over_{base}_sync": round(med[k_both + "_sync"] / med[k_base + "_sync"], 3)}
    if a.pair == "sgd-lars":
        out.update({"expected_from_bytes": round(34 / 26, 3), "sgd_TBps": round(covered * 26 / med[k_base] / 1e6, 2),
                    "lars_norms_TBps": round(adapted * 8 / med[k_first] / 1e6, 2)})
    else:
        out.update({"expected_from_bytes": round(46 / 34, 3), "adamw_TBps": round(covered * 34 / med[k_base] / 1e6, 2),
                    "lamb_moments_TBps": round(covered * 24 / med[k_first] / 1e6, 2), "lamb_step_TBps": round(covered * 22 / med[k_second] / 1e6, 2)})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
