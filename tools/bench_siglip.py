"""Loss-head timing: siglip_fwd + siglip_bwd beside infonce_fwd + infonce_bwd on the same cosine matrix C [B][B], bf16 gradients, at
B = 128, 1024 and 4096. Prints one JSON line. The yardstick is the InfoNCE pair of the same commit, measured twice so that the run shows its own
spread. Back-to-back launches per timed call and the median of repeated calls, as tools/bench_text.py.

Bytes per pair of calls: SigLIP reads C twice (4 B^2 each) and writes dC once (2 B^2); InfoNCE reads C five times (row max + row sum, column max
+ column sum, backward) and writes dC once.

    python tools/bench_siglip.py [--sizes 128 1024 4096] [--repeats 20]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from tools.bench_text import timeit  # noqa: E402


def pair(B, repeats):
    from clip_lite_amd import hip
    g = torch.Generator(device="cuda").manual_seed(B)
    a = torch.nn.functional.normalize(torch.randn(B, 256, device="cuda", generator=g), dim=-1)
    b = torch.nn.functional.normalize(torch.randn(B, 256, device="cuda", generator=g) + 0.7 * a, dim=-1)
    Cm = (a @ b.T).contiguous()
    f32 = lambda *shape: torch.zeros(*shape, device="cuda", dtype=torch.float32)
    temp_i, temp_s, bias = f32(1).fill_(2.6593), f32(1).fill_(2.302585), f32(1).fill_(-10.0)
    lse, part, acc, gout, dtemp, dbias = f32(2, B), f32(2 * B), f32(8), f32(1).fill_(1.0), f32(1), f32(1)
    dC = torch.empty(B, B, device="cuda", dtype=torch.bfloat16)
    inner = 50 if B <= 1024 else 10          # back-to-back launches per timed call: at B = 128 a pair takes ~10 us, an event pair resolves no better

    def per_call(fn):
        def many():
            for _ in range(inner):
                fn()
        return timeit(many, repeats) / inner

    def infonce():
        hip.infonce_fwd(Cm, B, B, temp_i, lse[0], lse[1], acc)
        hip.infonce_bwd(hip.BF16, Cm, B, B, temp_i, lse[0], lse[1], gout, 0.9, dC, B, dtemp)

    def siglip():
        hip.siglip_fwd(Cm, B, B, temp_s, bias, part, acc)
        hip.siglip_bwd(hip.BF16, Cm, B, B, temp_s, bias, gout, 0.9, dC, B, part, dtemp, dbias)

    r = {"infonce_fwd_bwd": per_call(infonce), "siglip_fwd_bwd": per_call(siglip), "infonce_fwd_bwd_again": per_call(infonce),
         "siglip_fwd": per_call(lambda: hip.siglip_fwd(Cm, B, B, temp_s, bias, part, acc)),
         "siglip_bwd": per_call(lambda: hip.siglip_bwd(hip.BF16, Cm, B, B, temp_s, bias, gout, 0.9, dC, B, part, dtemp, dbias)),
         "infonce_fwd": per_call(lambda: hip.infonce_fwd(Cm, B, B, temp_i, lse[0], lse[1], acc)),
         "infonce_bwd": per_call(lambda: hip.infonce_bwd(hip.BF16, Cm, B, B, temp_i, lse[0], lse[1], gout, 0.9, dC, B, dtemp))}
    assert torch.isfinite(dC.float()).all() and torch.isfinite(acc).all()
    r["siglip_over_infonce"] = r["siglip_fwd_bwd"] / r["infonce_fwd_bwd"]
    r["infonce_spread"] = abs(r["infonce_fwd_bwd_again"] - r["infonce_fwd_bwd"]) / r["infonce_fwd_bwd"]
    r["siglip_GBps"] = (2 * 4 + 2) * B * B / r["siglip_fwd_bwd"] / 1e3          # bytes / us = MB/s
    r["infonce_GBps"] = (5 * 4 + 2) * B * B / r["infonce_fwd_bwd"] / 1e3
    return {k: round(v, 3) for k, v in r.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 1024, 4096])
    ap.add_argument("--repeats", type=int, default=20)
    a = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "dtype": "bf16", "unit": "us (median) per fwd + bwd pair"}
    for B in a.sizes:
        out[str(B)] = pair(B, a.repeats)
        print(json.dumps({str(B): out[str(B)]}), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
