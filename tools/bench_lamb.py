"""Update-path timing on the item table of the transformer pair (ViT-B/32 + BERT-base, bf16 copy on): clite_adamw_step alone against
clite_lamb_moments + clite_lamb_step, in one process, between stream events. The model is laid out on meta tensors (shapes only); the flat buffers
hold random values. Every timed call is preceded by a refill of the gradient buffer (both updates zero it) and of the moments, outside the timed
region, for both optimizers alike; the two are timed alternately, repeat by repeat, and the medians are reported. Prints one JSON line.

Bytes per element on a non-sync step: AdamW reads p, g, m, v2 (16 B) and writes p, m, v2, g, bf16 (18 B); LAMB's moments pass reads the same 16 B
and writes m, v2 (8 B), its step pass reads p, m, v2 (12 B) and writes p, g, bf16 (10 B): the expectation is 46 / 34 = 1.35 x the AdamW update.

    python tools/bench_lamb.py [--repeats 30] [--warmup 5]
"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def item_table(hip, chunk):
    """(device bytes of the table, items, norm slots, arena elements, elements inside items, elements of adapted tensors)"""
    from clip_lite_amd.encoder import ImageEncoder, TextEncoder
    from clip_lite_amd.loss import JSDInfoMaxLoss
    from clip_lite_amd.model import VLInfoModel
    from clip_lite_amd.runtime import Arena
    with torch.device("meta"):
        M = VLInfoModel(TextEncoder(mode="train_sbert", num_hidden_layers=12), ImageEncoder("vit_b_32"), JSDInfoMaxLoss(768, 768, "dot", 0.1, True, True),
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
        n4 = (numel + 3) // 4 * 4
        for s in range(0, n4, chunk):
            rows.append((o + s, min(chunk, n4 - s), 1e-3, 1e-2, tag))
    rows.sort()
    arr = (hip.OptimItem * len(rows))(*[hip.OptimItem(*r) for r in rows])
    dev = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()
    return dev, len(rows), slots, total, sum(r[1] for r in rows), adapted


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    from clip_lite_amd import hip
    from clip_lite_amd.optim.fused_sgd import CHUNK
    items, n_items, slots, total, covered, adapted = item_table(hip, CHUNK)
    ip = C.c_void_p(items.data_ptr())
    gen = torch.Generator(device="cuda").manual_seed(0)
    p = torch.randn(total, device="cuda", generator=gen) * 0.05
    g0 = torch.randn(total, device="cuda", generator=gen) * 1e-3
    m0 = torch.randn(total, device="cuda", generator=gen) * 1e-3
    v0 = m0 * m0 * 1.5
    g, m, v2, slow = g0.clone(), m0.clone(), v0.clone(), p.clone()
    lp = p.to(torch.bfloat16)
    norms, partials = torch.zeros(slots, 2, device="cuda"), torch.zeros(2 * n_items, device="cuda")
    ss = (g0.double() ** 2).sum().float().reshape(1)
    # lr multiplier 0 (the parameters stay put over the repeats; the kernels do the same work), beta1, clip at half the norm, no sync, alpha, pre-scale,
    # beta2, eps, the bias corrections of step 1000, 1 - beta1, 1 - beta2, TRUST_CLIP off
    hp = torch.tensor([0.0, 0.9, float(ss.sqrt()) / 2, 0.0, 0.5, 1.0, 0.999, 1e-6, 1 - 0.9 ** 1000, 1 - 0.999 ** 1000, 1 - 0.9, 1 - 0.999, 0.0, 0.0, 0.0, 0.0],
                      device="cuda")
    hp_sync = hp.clone()
    hp_sync[3] = 1.0

    def adamw(h):
        hip.adamw_step(p, g, m, v2, slow, lp, ip, n_items, h, ss)

    def lamb_moments(h):
        hip.lamb_moments(p, g, m, v2, ip, n_items, h, ss, partials, norms)

    def lamb_step(h):
        hip.lamb_step(p, g, m, v2, slow, lp, ip, n_items, h, ss, norms)

    def lamb(h):
        lamb_moments(h)
        lamb_step(h)

    cases = [("adamw_step", adamw, hp), ("lamb_moments", lamb_moments, hp), ("lamb_step", lamb_step, hp), ("lamb_moments_and_step", lamb, hp),
             ("adamw_step_sync", adamw, hp_sync), ("lamb_moments_and_step_sync", lamb, hp_sync)]
    times = {name: [] for name, _, _ in cases}
    for r in range(a.warmup + a.repeats):
        for name, fn, h in cases:          # alternately, repeat by repeat: drift of the clocks hits every case alike
            g.copy_(g0)
            m.copy_(m0)
            v2.copy_(v0)
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
           "lamb_over_adamw": round(med["lamb_moments_and_step"] / med["adamw_step"], 3),
           "lamb_over_adamw_sync": round(med["lamb_moments_and_step_sync"] / med["adamw_step_sync"], 3),
           "expected_from_bytes": round(46 / 34, 3),
           "adamw_TBps": round(covered * 34 / med["adamw_step"] / 1e6, 2), "lamb_moments_TBps": round(covered * 24 / med["lamb_moments"] / 1e6, 2),
           "lamb_step_TBps": round(covered * 22 / med["lamb_step"] / 1e6, 2)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
