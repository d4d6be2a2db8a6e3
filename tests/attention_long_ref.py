"""References for the attention kernels of 33..128 tokens (csrc/bert_ops.hip, attention_long_*): the definition in float64, and the same math
with the probabilities and dS rounded to bf16 at the points where the MFMA kernels round them. Needs torch only; shared by the wave-simulator
tests and the GPU tests.

softmax(q k^T / 8 + (mask == 0) * finfo(f32).min) [* keep] v per (batch, head); qkv [B*L][3*H*64] (q | k | v), ctx [B*L][H*64]."""
import torch

import mpnet_ref

NEG = mpnet_ref.NEG


def masks(B, L, seed=0):
    """[B][L] int64, ragged: sample 0 is full, the last sample (B >= 2) has length 1, the others a random length in 2 .. L - 1."""
    lens = torch.randint(2, L, (B,), generator=torch.Generator().manual_seed(seed))
    lens[0] = L
    if B > 1:
        lens[B - 1] = 1
    return (torch.arange(L)[None, :] < lens[:, None]).long()


def _heads(x, B, L, H):
    return x.reshape(B, L, H, 64).permute(0, 2, 1, 3)


def _rows(x, B, L, H):
    return x.permute(0, 2, 1, 3).reshape(B * L, H * 64)


def reference(qkv, mask, dctx, B, L, H, keep=None):
    """float64 (ctx [B*L][H*64], dqkv [B*L][3*H*64]) by autograd through mpnet_ref.attention without a bias; keep: multiplier [B][H][L][L]."""
    q = qkv.double().reshape(B, L, 3 * H * 64).clone().requires_grad_(True)
    ctx = mpnet_ref.attention(q, mask, None, H, keep=None if keep is None else keep.double())
    ctx.backward(dctx.double().reshape(B, L, H * 64))
    return ctx.detach().reshape(B * L, H * 64), q.grad.reshape(B * L, 3 * H * 64)


def bf16_round(x):
    return x.float().bfloat16().double()


def emulate_bf16(qkv, mask, dctx, B, L, H, keep=None):
    """The MFMA kernels' roundings on exact arithmetic: the inputs are bf16 values already; forward feeds the dropped, normalised P to the second
    product in bf16 and stores ctx in bf16; backward feeds the dropped P (dV) and dS (dK, dQ) in bf16 and stores the three gradients in bf16.
    Scores, the softmax, dP and the row sum stay in f32 in the kernels (float64 here)."""
    x = qkv.double().reshape(B, L, 3, H, 64)
    q, k, v = (x[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    dO = _heads(dctx.double(), B, L, H)
    s = q @ k.transpose(-1, -2) / 8.0 + (mask == 0).double()[:, None, None, :] * NEG
    p = torch.softmax(s, dim=-1)
    m = torch.ones_like(p) if keep is None else keep.double()
    pd = p * m
    ctx = bf16_round(bf16_round(pd) @ v)
    dp = (dO @ v.transpose(-1, -2)) * m
    ds = p * (dp - (dp * p).sum(-1, keepdim=True))
    dsr = bf16_round(ds)
    dv = bf16_round(pd).transpose(-1, -2) @ dO
    dq = dsr @ k / 8.0
    dk = dsr.transpose(-1, -2) @ q / 8.0
    dqkv = bf16_round(torch.stack([dq, dk, dv], 2).permute(0, 3, 2, 1, 4).reshape(B * L, 3 * H * 64))      # [B][H][3][L][64] -> [B][L][3][H][64]
    return _rows(ctx, B, L, H), dqkv


def rel_err(got, ref):
    return ((got.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-6)).item()


def one_hot_probe(qkv, B, L, H, j0):
    """qkv with V replaced by one-hot rows over keys j0 .. j0 + 63: ctx[i][c] is then the (dropped) probability p[i][j0 + c]."""
    x = qkv.clone().reshape(B, L, 3, H, 64)
    x[:, :, 2] = 0
    for j in range(j0, min(L, j0 + 64)):
        x[:, j, 2, :, j - j0] = 1.0
    return x.reshape(B * L, 3 * H * 64).contiguous()


def multipliers(pd_lo, p0_lo, pd_hi, p0_hi, B, L, H, p):
    """The dropout multipliers [B][H][L][L] from the forward outputs of the two probes with dropout (pd) and without (p0); where the
    probability underflowed the multiplier is unobservable and reported as 1/(1-p) (it multiplies a zero)."""
    pd = torch.cat([_heads(pd_lo, B, L, H), _heads(pd_hi, B, L, H)], -1)[..., :L].double()
    p0 = torch.cat([_heads(p0_lo, B, L, H), _heads(p0_hi, B, L, H)], -1)[..., :L].double()
    seen = p0 > 1e-20
    return torch.where(seen, pd / p0.clamp_min(1e-30), torch.full_like(p0, 1.0 / (1.0 - p))), seen
