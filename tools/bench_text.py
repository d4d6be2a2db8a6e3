"""Text-tower timing: forward + backward of the BERT and of the MPNet tower in the same process (B = 128, L = 30, 12 layers, bf16), and the attention
kernels alone with and without the relative-position bias. Prints one JSON line. The yardstick is the BERT tower of the same commit.
With --length above 32 (up to 128) only the BERT side runs (MPNet stays at 32 tokens), and the attention section adds the kernels with dropout off
beside torch.nn.functional.scaled_dot_product_attention forward + backward at the same shape and mask in the same process.

With --causal it times instead the causal attention kernels of the CLIP text tower beside the non-causal ones at L = 77 and 128 (B = 128, 8 heads, bf16,
dropout off; the non-causal pair measured twice, so that the run shows its own spread) and the clip_text_b tower's forward + backward.

    python tools/bench_text.py [--batch 128] [--length 30] [--layers 12] [--repeats 20] [--causal]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

MPNET = "sentence-transformers/paraphrase-mpnet-base-v2"


def timeit(fn, repeats, warmup=5):
    """median of `repeats` event-timed calls, in microseconds"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    ts.sort()
    return ts[len(ts) // 2]


class Holder(torch.nn.Module):
    def __init__(self, te):
        super().__init__()
        self.text_encoder = te


def tower(name, layers, B, L, repeats):
    """forward + backward of one tower, recorded once into a hipGraph the way train_loop.TrainStep records its text phases (launch cost off the
    measurement) and replayed; dropout on as in training, weight gradients as one grouped launch"""
    from clip_lite_amd import hip
    from clip_lite_amd.bert import bert_backward, bert_forward
    from clip_lite_amd.encoder import TextEncoder
    from clip_lite_amd.model import attach_runtime
    te = TextEncoder(mode="train_sbert", model_name=name, num_hidden_layers=layers)
    holder = Holder(te).to("cuda").train()
    rt = attach_runtime(holder, torch.device("cuda", torch.cuda.current_device()), True)
    lo = 1000 if "bert" in name else 4
    ids = torch.randint(lo, 30000, (B, L), device="cuda")
    mask = torch.ones(B, L, dtype=torch.long, device="cuda")
    mask[::3, L - 5:] = 0
    ids[mask == 0] = 0 if "bert" in name else 1
    dy = torch.randn(B, 768, device="cuda").to(rt.tdtype)
    ws = hip.WgradGroup.alloc_workspace(rt.device)          # pinned staging: cannot be allocated inside a capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    rt.begin_capture()
    try:
        with torch.no_grad(), torch.cuda.graph(graph, capture_error_mode="thread_local"):
            rt.arena.ensure_transposed(force=True, capturing=True)
            out, ctx = bert_forward(rt, te.strans, ids, mask, rt.next_step(True))
            group = hip.WgradGroup(rt.dt, ws)
            bert_backward(rt, te.strans, ctx, dy, defer=group)
            group.launch()
            rt.arena.flat_g.zero_()
            rt.end_capture()
    except BaseException:
        rt.abort_capture()
        raise

    def step():
        rt.sync_graph_seeds()
        graph.replay()

    us = timeit(step, repeats)
    assert torch.isfinite(out.float()).all()
    return us


def attention(B, L, H, repeats):
    from clip_lite_amd import hip
    qkv = (torch.randn(B * L, 3 * H * 64, device="cuda") * 0.7).bfloat16()
    dctx = torch.randn(B * L, H * 64, device="cuda").bfloat16()
    mask = torch.ones(B, L, dtype=torch.long, device="cuda")
    bias = torch.randn(H, 32, 32, device="cuda")
    table = torch.tensor(hip.relative_position_buckets(), dtype=torch.int32, device="cuda")
    ctx, dqkv = torch.empty_like(dctx), torch.empty_like(qkv)
    partials, drel, rel = torch.empty(B * H, 32, device="cuda"), torch.zeros(32, H, device="cuda"), torch.randn(32, H, device="cuda")
    drop = (0.1, 12345, 3)
    partials12 = partials.repeat(12, 1)
    INNER = 50          # back-to-back launches per timed call: the kernels take ~10 us, an event pair alone resolves no better

    def per_launch(fn):
        def many():
            for _ in range(INNER):
                fn()
        return timeit(many, repeats) / INNER

    if L > 32:
        return attention_long(B, L, H, per_launch, qkv, dctx, ctx, dqkv, drop)
    return {
        "fwd": per_launch(lambda: hip.attention_fwd(hip.BF16, qkv, mask, ctx, B, L, H, drop)),
        "fwd_bias": per_launch(lambda: hip.attention_bias_fwd(hip.BF16, qkv, mask, bias, ctx, B, L, H, drop)),
        "bwd": per_launch(lambda: hip.attention_bwd(hip.BF16, qkv, mask, dctx, dqkv, B, L, H, drop)),
        "bwd_bias": per_launch(lambda: hip.attention_bias_bwd(hip.BF16, qkv, mask, bias, table, dctx, dqkv, partials, B, L, H, drop)),
        "bias_build": per_launch(lambda: hip.attention_bias_build(rel, table, bias, H, L)),
        "bias_grad_reduce_12_layers": per_launch(lambda: hip.attention_bias_grad_reduce(partials12, drel, 12 * B, H)),
    }


def attention_long(B, L, H, per_launch, qkv, dctx, ctx, dqkv, drop):
    """33..128 tokens: the kernels with dropout on (as trained) and off, and torch's fused attention with the same ragged mask, dropout off"""
    import torch.nn.functional as F
    from clip_lite_amd import hip
    mask = torch.ones(B, L, dtype=torch.long, device="cuda")
    mask[::3, L - 5:] = 0
    x = qkv.view(B, L, 3, H, 64)
    q, k, v = (x[:, :, i].permute(0, 2, 1, 3).contiguous().requires_grad_(True) for i in range(3))      # [B][H][L][64], as SDPA wants them
    amask = (mask != 0)[:, None, None, :].expand(B, 1, L, L)
    dO = dctx.view(B, L, H, 64).permute(0, 2, 1, 3).contiguous()

    def sdpa():
        o = F.scaled_dot_product_attention(q, k, v, attn_mask=amask)
        torch.autograd.grad(o, (q, k, v), dO)

    def ours(d):
        hip.attention_fwd(hip.BF16, qkv, mask, ctx, B, L, H, d)
        hip.attention_bwd(hip.BF16, qkv, mask, dctx, dqkv, B, L, H, d)

    return {
        "fwd": per_launch(lambda: hip.attention_fwd(hip.BF16, qkv, mask, ctx, B, L, H, drop)),
        "bwd": per_launch(lambda: hip.attention_bwd(hip.BF16, qkv, mask, dctx, dqkv, B, L, H, drop)),
        "fwd_bwd_no_dropout": per_launch(lambda: ours(hip.NO_DROP)),
        "torch_sdpa_fwd_bwd_no_dropout": per_launch(sdpa),
    }


def causal(B, H, repeats):
    """causal against non-causal attention, same shapes, same ragged mask, dropout off: {L: times in us and the causal / non-causal ratio}"""
    from clip_lite_amd import hip
    INNER = 50
    out = {}
    for L in (77, 128):
        qkv = (torch.randn(B * L, 3 * H * 64, device="cuda") * 0.7).bfloat16()
        dctx = torch.randn(B * L, H * 64, device="cuda").bfloat16()
        ctx, dqkv = torch.empty_like(dctx), torch.empty_like(qkv)
        mask = torch.ones(B, L, dtype=torch.long, device="cuda")
        mask[::3, L - 5:] = 0

        def per_launch(fn):
            def many():
                for _ in range(INNER):
                    fn()
            return timeit(many, repeats) / INNER

        def plain():
            hip.attention_fwd(hip.BF16, qkv, mask, ctx, B, L, H)
            hip.attention_bwd(hip.BF16, qkv, mask, dctx, dqkv, B, L, H)

        def tri():
            hip.attention_causal_fwd(hip.BF16, qkv, mask, ctx, B, L, H)
            hip.attention_causal_bwd(hip.BF16, qkv, mask, dctx, dqkv, B, L, H)

        r = {"non_causal_fwd": per_launch(lambda: hip.attention_fwd(hip.BF16, qkv, mask, ctx, B, L, H)),
             "causal_fwd": per_launch(lambda: hip.attention_causal_fwd(hip.BF16, qkv, mask, ctx, B, L, H)),
             "non_causal_bwd": per_launch(lambda: hip.attention_bwd(hip.BF16, qkv, mask, dctx, dqkv, B, L, H)),
             "causal_bwd": per_launch(lambda: hip.attention_causal_bwd(hip.BF16, qkv, mask, dctx, dqkv, B, L, H)),
             "non_causal_fwd_bwd": per_launch(plain), "causal_fwd_bwd": per_launch(tri), "non_causal_fwd_bwd_again": per_launch(plain)}
        r["causal_over_non_causal"] = r["causal_fwd_bwd"] / r["non_causal_fwd_bwd"]
        r["non_causal_spread"] = abs(r["non_causal_fwd_bwd_again"] - r["non_causal_fwd_bwd"]) / r["non_causal_fwd_bwd"]
        nt = (L + 31) // 32
        r["tile_ratio_expected"] = (nt * (nt + 1) // 2) / (nt * nt)
        out[str(L)] = r
    return out


def clip_tower(layers, B, L, repeats):
    """forward + backward of the clip_text_b tower, captured once and replayed as `tower` does"""
    from clip_lite_amd import hip
    from clip_lite_amd.cliptext import cliptext_backward, cliptext_forward
    from clip_lite_amd.encoder import TextEncoder
    from clip_lite_amd.model import attach_runtime
    te = TextEncoder(mode="train_sbert", model_name="clip_text_b", num_hidden_layers=layers, txt_enc_dim=512, context_length=max(L, 77))
    holder = Holder(te).to("cuda").train()
    rt = attach_runtime(holder, torch.device("cuda", torch.cuda.current_device()), True)
    ids = torch.randint(1000, 30000, (B, L), device="cuda")
    mask = torch.ones(B, L, dtype=torch.long, device="cuda")
    mask[::3, L - 5:] = 0
    ids[mask == 0] = 0
    dy = torch.randn(B, 512, device="cuda").to(rt.tdtype)
    ws = hip.WgradGroup.alloc_workspace(rt.device)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    rt.begin_capture()
    try:
        with torch.no_grad(), torch.cuda.graph(graph, capture_error_mode="thread_local"):
            rt.arena.ensure_transposed(force=True, capturing=True)
            out, ctx = cliptext_forward(rt, te.strans, ids, mask)
            group = hip.WgradGroup(rt.dt, ws)
            cliptext_backward(rt, te.strans, ctx, dy, defer=group)
            group.launch()
            rt.arena.flat_g.zero_()
            rt.end_capture()
    except BaseException:
        rt.abort_capture()
        raise
    us = timeit(graph.replay, repeats)
    assert torch.isfinite(out.float()).all()
    return us


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--length", type=int, default=30)
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--causal", action="store_true", help="the causal attention kernels beside the non-causal ones at L = 77 and 128 (8 heads), and the clip_text_b tower")
    a = ap.parse_args()
    if a.causal:
        out = {"device": torch.cuda.get_device_name(0), "batch": a.batch, "heads": 8, "layers": a.layers, "dtype": "bf16", "unit": "us (median)"}
        out["attention_kernels"] = causal(a.batch, 8, a.repeats)
        print(json.dumps(out["attention_kernels"]), file=sys.stderr, flush=True)
        out["tower_fwd_bwd"] = {"clip_text_b_77_tokens": clip_tower(a.layers, a.batch, 77, a.repeats)}
        print(json.dumps(out))
        return
    out = {"device": torch.cuda.get_device_name(0), "batch": a.batch, "length": a.length, "layers": a.layers, "dtype": "bf16", "unit": "us (median)"}
    out["attention_kernels"] = attention(a.batch, a.length, 12, a.repeats)
    print(json.dumps(out["attention_kernels"]), file=sys.stderr, flush=True)
    out["tower_fwd_bwd"] = {"bert": tower("bert-base-uncased", a.layers, a.batch, a.length, a.repeats)}
    if a.length <= 32:
        out["tower_fwd_bwd"]["mpnet"] = tower(MPNET, a.layers, a.batch, a.length, a.repeats)
        out["tower_fwd_bwd"]["mpnet_over_bert"] = out["tower_fwd_bwd"]["mpnet"] / out["tower_fwd_bwd"]["bert"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
