"""The checks of the CLIP text tower's kernels (csrc/bert_ops.hip: clite_attention_causal_fwd / _bwd, clite_embed_clip_fwd, clite_last_token_gather /
_scatter), written once against tests/cliptext_ref.py and run by tests/test_wavesim_cliptext.py (wave simulator, numpy buffers) and
tests/test_gpu_cliptext.py (MI355X, torch tensors) through the backends of tests/loss_backends.py.

Bounds of the attention kernels are the project's existing ones for the non-causal kernels (tests/test_gpu_ops.py, test_gpu_attention_long.py):
1e-5 of max |ref| in f32; in bf16 1e-2 forward and 2e-2 backward."""
import ctypes as C

import numpy as np
import torch

import cliptext_ref as R
from loss_backends import BF16, F32, HipBackend, SimBackend

_V, _I, _F, _U64, _U32 = C.c_void_p, C.c_int, C.c_float, C.c_uint64, C.c_uint32
SIGNATURES = {
    "attention_causal_fwd": [_I, _V, _V, _V, _I, _I, _I],
    "attention_causal_bwd": [_I, _V, _V, _V, _V, _I, _I, _I],
    "embed_clip_fwd": [_I, _V, _V, _V, _V, _I, _I, _I, _I],
    "last_token_gather": [_I, _V, _V, _V, _V, _I, _I, _I],
    "last_token_scatter": [_I, _V, _V, _V, _I, _I, _I],
    "attention_fwd": [_I, _V, _V, _V, _I, _I, _I, _F, _U64, _U32],
    "attention_bwd": [_I, _V, _V, _V, _V, _I, _I, _I, _F, _U64, _U32],
}
TOL = {BF16: (1e-2, 2e-2), F32: (1e-5, 1e-5)}
# one partial tile; a full tile; the second tile of one row; three tiles, CLIP's shape; four tiles
SHAPES = [(3, 7, 2), (2, 32, 4), (3, 33, 2), (2, 77, 8), (2, 128, 4)]


class Sim(SimBackend):
    def __init__(self):
        super().__init__()
        for n, sig in SIGNATURES.items():
            getattr(self.L, "clite_" + n).argtypes = sig + [_V]


class Hip(HipBackend):
    def set_deterministic(self, on):
        self.hip.set_deterministic(on)


def problem(B, L, H, seed):
    """bf16-representable inputs (both dtypes see the same values): qkv and dctx as float32 tensors, and the ragged right-padded mask"""
    g = torch.Generator().manual_seed(seed)
    qkv = (torch.randn(B * L, 3 * H * 64, generator=g) * 0.7).bfloat16().float()
    dctx = torch.randn(B * L, H * 64, generator=g).bfloat16().float()
    return qkv, dctx, R.ragged_mask(B, L, seed)


def run(be, dtype, qkv, mask, dctx, B, L, H):
    """(ctx, dqkv) of the causal entry points as float32 tensors; dctx None: forward only"""
    dq, dm = be.dev(qkv.numpy(), dtype), None if mask is None else be.dev(mask.numpy(), "i64")
    ctx = be.dev(np.full((B * L, H * 64), np.nan, np.float32), dtype)
    assert be.call("attention_causal_fwd", dtype, dq, dm, ctx, B, L, H) == 0
    dqkv = None
    if dctx is not None:
        dqkv = be.dev(np.full((B * L, 3 * H * 64), np.nan, np.float32), dtype)
        assert be.call("attention_causal_bwd", dtype, dq, dm, be.dev(dctx.numpy(), dtype), dqkv, B, L, H) == 0
        dqkv = torch.from_numpy(be.host(dqkv))
    return torch.from_numpy(be.host(ctx)), dqkv


def check_against_float64(be, dtype, B, L, H):
    qkv, dctx, mask = problem(B, L, H, 1000 + L)
    ref_ctx, ref_dqkv = R.causal_attention(qkv, mask, B, L, H), R.causal_attention_bwd(qkv, mask, dctx, B, L, H)
    ctx, dqkv = run(be, dtype, qkv, mask, dctx, B, L, H)
    ef, eb = R.rel_err(ctx, ref_ctx), R.rel_err(dqkv, ref_dqkv)
    print(f"causal attention, dtype {dtype} (B, L, H) = {(B, L, H)}: forward {ef:.3e}, backward {eb:.3e}")
    assert torch.isfinite(ctx).all() and torch.isfinite(dqkv).all()
    assert ef < TOL[dtype][0]
    assert eb < TOL[dtype][1]
    # a sample of length 1 (the last one): its first row is v[0] - the probability is exactly 1, so only the store rounds (and v is bf16 already)
    if B > 1:
        r = (B - 1) * L
        v0 = qkv[r].reshape(3, H * 64)[2]
        assert torch.equal(ctx[r], v0)
    # the same bits again, in both settings of the deterministic switch
    for on in (True, False):
        be.set_deterministic(on)
        try:
            ctx2, dqkv2 = run(be, dtype, qkv, mask, dctx, B, L, H)
        finally:
            be.set_deterministic(False)
        assert torch.equal(ctx2.view(torch.int32), ctx.view(torch.int32)) and torch.equal(dqkv2.view(torch.int32), dqkv.view(torch.int32))


def check_causality(be, dtype, L, i0, B=2, H=2):
    """Other q, k, v rows behind token i0 leave the ctx rows up to i0 bit-identical; with dctx zero behind i0, dK and dV behind i0 are exactly zero."""
    qkv, dctx, _ = problem(B, L, H, 7 * L + i0)
    mask = torch.ones(B, L, dtype=torch.long)
    mask[B - 1, L - 5:] = 0
    other = qkv.clone().reshape(B, L, -1)
    g = torch.Generator().manual_seed(99)
    other[:, i0 + 1:] = (torch.randn(B, L - i0 - 1, 3 * H * 64, generator=g) * 3.0).bfloat16().float()
    other = other.reshape(B * L, -1)
    assert not torch.equal(other, qkv)
    d0 = dctx.clone().reshape(B, L, -1)
    d0[:, i0 + 1:] = 0
    d0 = d0.reshape(B * L, -1)
    ctx_a, dqkv_a = run(be, dtype, qkv, mask, d0, B, L, H)
    ctx_b, _ = run(be, dtype, other, mask, None, B, L, H)
    a, b = ctx_a.reshape(B, L, -1), ctx_b.reshape(B, L, -1)
    assert torch.equal(a[:, :i0 + 1].contiguous().view(torch.int32), b[:, :i0 + 1].contiguous().view(torch.int32))
    assert not torch.equal(a[:, i0 + 1:], b[:, i0 + 1:])
    d = dqkv_a.reshape(B, L, 3, H * 64)
    assert (d[:, i0 + 1:, 1] == 0).all() and (d[:, i0 + 1:, 2] == 0).all()
    assert d[:, :i0 + 1, 1].abs().max() > 0 and d[:, :i0 + 1, 2].abs().max() > 0 and d[:, :i0 + 1, 0].abs().max() > 0


def check_null_mask(be, dtype, L, B=2, H=2):
    """mask == NULL is the all-ones mask, bit for bit"""
    qkv, dctx, _ = problem(B, L, H, 31 * L)
    ones = torch.ones(B, L, dtype=torch.long)
    ctx_a, dqkv_a = run(be, dtype, qkv, None, dctx, B, L, H)
    ctx_b, dqkv_b = run(be, dtype, qkv, ones, dctx, B, L, H)
    assert torch.equal(ctx_a.view(torch.int32), ctx_b.view(torch.int32)) and torch.equal(dqkv_a.view(torch.int32), dqkv_b.view(torch.int32))
    assert torch.isfinite(ctx_a).all() and torch.isfinite(dqkv_a).all()


def _cast(x, dtype):
    x = np.ascontiguousarray(x, np.float32)
    return torch.from_numpy(x).to(torch.bfloat16).float().numpy() if dtype == BF16 else x


def check_gather_scatter(be, dtype, Cc=24, raw=False):
    """exact copies; idx = mask.sum(1) - 1 with a full-length and a length-1 sample. raw: the backend reaches the C entry without a wrapper
    that checks the shapes itself, so the entry's own refusals can be seen"""
    B, L = 4, 9
    lens = np.array([9, 1, 4, 6])
    mask = (np.arange(L)[None, :] < lens[:, None]).astype(np.int64)
    rng = np.random.default_rng(Cc)
    x = _cast(rng.standard_normal((B, L, Cc), dtype=np.float32), dtype)
    out, idx = be.dev(np.full((B, Cc), np.nan), dtype), be.dev(np.full(B, -7), "i32")
    assert be.call("last_token_gather", dtype, be.dev(x.reshape(B * L, Cc), dtype), be.dev(mask, "i64"), out, idx, B, L, Cc) == 0
    got_idx = be.host(idx)
    assert np.array_equal(got_idx, mask.sum(1) - 1) and np.array_equal(got_idx, lens - 1)
    assert np.array_equal(be.host(out), x[np.arange(B), lens - 1])
    d = _cast(rng.standard_normal((B, Cc), dtype=np.float32), dtype)
    dx = be.dev(np.zeros((B * L, Cc)), dtype)
    assert be.call("last_token_scatter", dtype, be.dev(d, dtype), idx, dx, B, L, Cc) == 0
    want = np.zeros((B, L, Cc), np.float32)
    want[np.arange(B), lens - 1] = d
    assert np.array_equal(be.host(dx).reshape(B, L, Cc), want)
    if not raw:
        return
    assert be.call("last_token_gather", dtype, be.dev(x.reshape(B * L, Cc), dtype), be.dev(mask, "i64"), out, idx, B, L, Cc - 4) == -1          # C % 8
    assert be.call("last_token_scatter", dtype, be.dev(d, dtype), idx, dx, B, 0, Cc) == -1


def check_embed(be, dtype, Cc=24):
    """token_embedding[ids] + positional_embedding[l], exact to one rounding of the two-term sum"""
    B, L, vocab, ctxlen = 3, 5, 50, 8
    rng = np.random.default_rng(5 + Cc)
    word, pos = _cast(rng.standard_normal((vocab, Cc), dtype=np.float32), dtype), _cast(rng.standard_normal((ctxlen, Cc), dtype=np.float32), dtype)
    ids = rng.integers(0, vocab, (B, L))
    ids[0, 0], ids[1, 2], ids[2, 4] = 0, vocab - 1, 0
    out = be.dev(np.full((B * L, Cc), np.nan), dtype)
    assert be.call("embed_clip_fwd", dtype, be.dev(ids, "i64"), be.dev(word, dtype), be.dev(pos, dtype), out, B * L, L, Cc, vocab) == 0
    # the float64 sum of two f32 / bf16 values rounded to f32 is their f32 sum, then the store's rounding
    want = (word[ids].astype(np.float64) + pos[None, :L].astype(np.float64)).astype(np.float32).reshape(B * L, Cc)
    assert np.array_equal(be.host(out), _cast(want, dtype))


def check_refusals(be):
    """129 tokens, no tokens: -1 from both causal entries in both dtypes"""
    B, H = 1, 1
    big = np.zeros((B * 129, 3 * H * 64), np.float32)
    for dtype in (BF16, F32):
        a, c = be.dev(big, dtype), be.dev(big[:, :64], dtype)
        assert be.call("attention_causal_fwd", dtype, a, None, c, B, 129, H) == -1
        assert be.call("attention_causal_bwd", dtype, a, None, c, a, B, 129, H) == -1
        assert be.call("attention_causal_fwd", dtype, a, None, c, B, 0, H) == -1
        assert be.call("attention_causal_bwd", dtype, a, None, c, a, B, 0, H) == -1


# ------------------------------------------------------------------------------------------------ the tower
class Holder(torch.nn.Module):
    """Gives a lone TextEncoder the `text_encoder` slot the runtime looks for."""

    def __init__(self, enc):
        super().__init__()
        self.text_encoder = enc


def build_tower(layers, device, lowp, salt="clite", round_bf16=False, small=None, context_length=None):
    """(holder with .rt, the tower's state dict as filled) of a TextEncoder("clip_text_b") on `device` ("cpu": the simulator build must be
    injected). small = (vocab, width, heads): the same module tree at another size, for the simulator."""
    from detfill import det_fill
    from clip_lite_amd.cliptext import ClipTextModel
    from clip_lite_amd.encoder import TextEncoder
    from clip_lite_amd.model import attach_runtime
    enc = TextEncoder(model_name="clip_text_b", num_hidden_layers=0 if small else layers, txt_enc_dim=512, context_length=context_length)
    if small:
        vocab, width, heads = small
        enc.strans = ClipTextModel(vocab=vocab, context_length=context_length or 77, width=width, heads=heads, num_hidden_layers=layers, embed_dim=width)
    det_fill(enc, salt)
    if round_bf16:
        with torch.no_grad():
            for q in enc.parameters():
                q.copy_(q.to(torch.bfloat16).float())
    sd = {k: v.clone() for k, v in enc.strans.state_dict().items()}
    assert all(v.abs().max() > 0 for v in sd.values())
    holder = Holder(enc).to(device)
    dev = torch.device(device, torch.cuda.current_device()) if device == "cuda" else torch.device("cpu")
    holder.rt = attach_runtime(holder, dev, lowp)
    return holder.train(), sd


def captions(lens, L, vocab=30522, seed=0):
    """(ids, mask) int64 [B][L]: [CLS] words [SEP] of the given lengths (a length-1 caption is [CLS] alone), right-padded with id 0"""
    g = torch.Generator().manual_seed(seed)
    B = len(lens)
    ids, mask = torch.zeros(B, L, dtype=torch.long), torch.zeros(B, L, dtype=torch.long)
    for b, n in enumerate(lens):
        row = torch.randint(min(1000, vocab // 2), vocab, (n,), generator=g)
        row[0] = min(101, vocab - 2)
        if n > 1:
            row[n - 1] = min(102, vocab - 1)
        ids[b, :n], mask[b, :n] = row, 1
    return ids, mask


def tower_pass(holder, ids, mask, dfeat):
    """one training pass: (features, {name: gradient}) on the host"""
    rt, net = holder.rt, holder.text_encoder.strans
    rt.arena.flat_g.zero_()
    dev = rt.device
    feat = holder.text_encoder({"input_ids": ids.to(dev), "attention_mask": mask.to(dev)})
    feat.backward(dfeat.to(dev).to(feat.dtype))
    if dev.type == "cuda":
        torch.cuda.synchronize()
    return feat.detach().cpu(), {k: q.grad.detach().cpu().clone() for k, q in net.named_parameters()}


def check_tower_f32(holder, sd, layers, heads, ids, mask, dfeat):
    """exact-f32 mode against float64: the bars of tests/test_gpu_model.py - pooled output within 1e-4 of max |ref|, every parameter's gradient
    norm within 2e-3 of the float64 one relative to max(norm, 1e-3 of the largest) - and, as tests/test_gpu_vit.py adds, every gradient
    element-wise within 2e-3 of its max. The pad id's embedding row gets no gradient at all."""
    feat, grads = tower_pass(holder, ids, mask, dfeat)
    want, ref = R.features_and_grads(sd, ids, mask, layers, heads, dfeat)
    err = ((feat.double() - want).abs().max() / want.abs().max()).item()
    print(f"features max |err| / max |ref| = {err:.3e}")
    assert err <= 1e-4
    assert sorted(grads) == sorted(ref)
    gmax = max(g.norm().item() for g in ref.values())
    for k, got in grads.items():
        got, g = got.double(), ref[k]
        assert got.shape == g.shape and g.abs().max() > 0, k
        assert (got - g).abs().max() <= 2e-3 * g.abs().max(), (k, ((got - g).abs().max() / g.abs().max()).item())
        assert abs(got.norm().item() - g.norm().item()) <= 2e-3 * max(g.norm().item(), 1e-3 * gmax), k
    assert (mask == 0).any() and grads["token_embedding.weight"][0].abs().max() == 0
    return feat, grads
