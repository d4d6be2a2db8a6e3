"""float64 references of the CLIP text tower (clip_lite_amd/cliptext.py) and of its causal attention kernels (csrc/bert_ops.hip,
attention_causal_*): the definitions written out in torch float64, forward AND backward for the attention, forward for the tower (its gradients
come from autograd on this forward). tests/test_cliptext_host.py pins both against torch's own modules (nn.MultiheadAttention with a boolean
upper-triangular attn_mask and a key_padding_mask, nn.LayerNorm, nn.GELU, nn.Embedding). Needs torch only; shared by the CPU and the GPU tests.

Layouts are the kernels': qkv [B*L][3*H*64] (q | k | v, head h at columns h*64..), ctx [B*L][H*64], mask int64 [B][L] (1 = attend) or None.
Query i sees key j iff j <= i and mask[b][j] == 1; a masked key in front of the diagonal gets finfo(float32).min added to its score (the
kernels' arithmetic), a key behind the diagonal -inf."""
import torch

NEG = float(torch.finfo(torch.float32).min)
LN_EPS = 1e-5


def ragged_mask(B, L, seed=0):
    """[B][L] int64, right-padded: sample 0 is full, the last sample (B >= 2) has length 1, the others a random length in 2 .. L - 1."""
    lens = torch.randint(2, max(L, 3), (B,), generator=torch.Generator().manual_seed(seed)).clamp(max=L)
    lens[0] = L
    if B > 1:
        lens[B - 1] = 1
    return (torch.arange(L)[None, :] < lens[:, None]).long()


def _split(qkv, B, L, H):
    x = qkv.double().reshape(B, L, 3, H, 64)
    return tuple(x[:, :, i].permute(0, 2, 1, 3) for i in range(3))          # [B][H][L][64]


def _rows(x, B, L, H):
    return x.permute(0, 2, 1, 3).reshape(B * L, H * 64)


def causal_probs(q, k, mask):
    L = q.shape[-2]
    s = q @ k.transpose(-1, -2) / 8.0
    if mask is not None:
        s = s + (mask == 0).double()[:, None, None, :] * NEG
    s = s.masked_fill(torch.ones(L, L, dtype=torch.bool).triu(1), float("-inf"))
    return torch.softmax(s, dim=-1)


def causal_attention(qkv, mask, B, L, H):
    """ctx [B*L][H*64] in float64; differentiable (the tower below runs through it)."""
    q, k, v = _split(qkv, B, L, H)
    return _rows(causal_probs(q, k, mask) @ v, B, L, H)


def causal_attention_bwd(qkv, mask, dctx, B, L, H):
    """dqkv [B*L][3*H*64] in float64 from the formulas the kernels implement: dV = P^T dO, dP = dO V^T, dS = P (dP - rowsum(dP P)),
    dQ = dS K / 8, dK = dS^T Q / 8."""
    q, k, v = _split(qkv, B, L, H)
    dO = dctx.double().reshape(B, L, H, 64).permute(0, 2, 1, 3)
    p = causal_probs(q, k, mask)
    dv = p.transpose(-1, -2) @ dO
    dp = dO @ v.transpose(-1, -2)
    ds = p * (dp - (dp * p).sum(-1, keepdim=True))
    dq, dk = ds @ k / 8.0, ds.transpose(-1, -2) @ q / 8.0
    return torch.stack([dq, dk, dv], 2).permute(0, 3, 2, 1, 4).reshape(B * L, 3 * H * 64)          # [B][H][3][L][64] -> [B][L][3][H][64]


def rel_err(got, ref):
    return ((got.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-6)).item()


def bf16_round(x):
    return x.float().bfloat16().double()


def emulate_bf16(qkv, mask, dctx, B, L, H):
    """The MFMA kernels' roundings on exact arithmetic (tests/attention_long_ref.emulate_bf16 with the causal probabilities): P and dS enter the
    second products in bf16, the outputs are stored in bf16; scores, softmax, dP and the row sum stay in f32 in the kernels (float64 here)."""
    q, k, v = _split(qkv, B, L, H)
    dO = dctx.double().reshape(B, L, H, 64).permute(0, 2, 1, 3)
    p = causal_probs(q, k, mask)
    ctx = bf16_round(bf16_round(p) @ v)
    dp = dO @ v.transpose(-1, -2)
    dsr = bf16_round(p * (dp - (dp * p).sum(-1, keepdim=True)))
    dv = bf16_round(p).transpose(-1, -2) @ dO
    dq, dk = dsr @ k / 8.0, dsr.transpose(-1, -2) @ q / 8.0
    return _rows(ctx, B, L, H), bf16_round(torch.stack([dq, dk, dv], 2).permute(0, 3, 2, 1, 4).reshape(B * L, 3 * H * 64))


# ------------------------------------------------------------------------------------------------ the tower
def _ln(x, w, b):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + LN_EPS) * w + b


def _gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / 2.0 ** 0.5))


def tower(sd, ids, mask, layers, heads):
    """features [B][embed_dim] in float64 of the tower whose state dict (open_clip TextTransformer names) is `sd`; differentiable in sd's tensors."""
    B, L = ids.shape
    x = sd["token_embedding.weight"][ids] + sd["positional_embedding"][:L]
    for i in range(layers):
        g = lambda n: sd[f"transformer.resblocks.{i}.{n}"]
        y = _ln(x, g("ln_1.weight"), g("ln_1.bias"))
        qkv = y @ g("attn.in_proj_weight").T + g("attn.in_proj_bias")
        ctx = causal_attention(qkv.reshape(B * L, -1), mask, B, L, heads).reshape(B, L, -1)
        x = x + ctx @ g("attn.out_proj.weight").T + g("attn.out_proj.bias")
        z = _ln(x, g("ln_2.weight"), g("ln_2.bias"))
        x = x + _gelu(z @ g("mlp.c_fc.weight").T + g("mlp.c_fc.bias")) @ g("mlp.c_proj.weight").T + g("mlp.c_proj.bias")
    idx = mask.sum(1) - 1
    xe = x[torch.arange(B), idx]
    return _ln(xe, sd["ln_final.weight"], sd["ln_final.bias"]) @ sd["text_projection"]


def features_and_grads(sd, ids, mask, layers, heads, dfeat):
    """(features, {name: gradient}) in float64 by autograd through `tower`."""
    leaf = {k: v.detach().double().clone().requires_grad_(True) for k, v in sd.items()}
    feat = tower(leaf, ids, mask, layers, heads)
    feat.backward(dfeat.double())
    return feat.detach(), {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaf.items()}
