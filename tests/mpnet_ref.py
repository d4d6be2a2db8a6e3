"""Plain-torch restatement of the MPNet text tower (transformers.MPNetModel + sentence-transformers mean pooling), written from the formulas and
evaluated in whatever dtype its inputs have (the tests pass float64). Needs torch only: it is what the GPU tests compare the kernels with, and
the CPU tests check it against fixtures the reference itself produced (tests/golden/make_mpnet_golden.py).

Parameters come as a flat dict with transformers' names relative to the model ("embeddings.word_embeddings.weight",
"encoder.layer.0.attention.attn.q.weight", "encoder.relative_attention_bias.weight", ...)."""
import math

import torch

NEG = torch.finfo(torch.float32).min      # the additive mask value transformers uses for an f32 model


def bucket(rel, num_buckets=32, max_distance=128):
    """MPNetEncoder.relative_position_bucket for one integer offset rel = j - i (key minus query), in float64."""
    half = num_buckets // 2
    n = -rel
    ret = half if n < 0 else 0
    n = abs(n)
    exact = half // 2
    if n < exact:
        return ret + n
    big = exact + int(math.log(n / exact) / math.log(max_distance / exact) * (half - exact))
    return ret + min(big, half - 1)


def bucket_table(span=31):
    return [bucket(r) for r in range(-span, span + 1)]


def position_ids(ids, pad=1):
    """create_position_ids_from_input_ids: pad + cumsum(ids != pad) * (ids != pad)"""
    m = (ids != pad).long()
    return torch.cumsum(m, dim=1) * m + pad


def position_bias(rel_weight, L):
    """[H][L][L]: rel_weight[bucket(j - i)][h]"""
    idx = torch.tensor([[bucket(j - i) for j in range(L)] for i in range(L)], dtype=torch.long)
    return rel_weight[idx].permute(2, 0, 1)


def attention(qkv, mask, bias, heads, keep=None):
    """qkv [B][L][3*heads*64] (q | k | v), mask [B][L] (non-zero = attend) or None, bias [heads][L][L] or None, keep: dropout multiplier
    [B][heads][L][L] or None. Returns ctx [B][L][heads*64]: softmax(q k^T / 8 + bias + (mask == 0) * finfo.min) v."""
    B, L, _ = qkv.shape
    q, k, v = (t.reshape(B, L, heads, 64).permute(0, 2, 1, 3) for t in qkv.split(heads * 64, dim=-1))
    s = q @ k.transpose(-1, -2) / 8.0
    if bias is not None:
        s = s + bias[None]
    if mask is not None:
        s = s + (mask == 0).to(s.dtype)[:, None, None, :] * NEG
    p = torch.softmax(s, dim=-1)
    if keep is not None:
        p = p * keep
    return (p @ v).permute(0, 2, 1, 3).reshape(B, L, heads * 64)


def layer_norm(x, w, b, eps):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * w + b


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def layer(P, pre, h, mask, bias, heads, eps):
    """One MPNetLayer (dropout off): attention with bias -> o -> + h -> LayerNorm -> FFN(GELU) -> + -> LayerNorm"""
    g = lambda n: P[pre + n]
    lin = lambda x, n: x @ g(n + ".weight").T + g(n + ".bias")
    qkv = torch.cat([lin(h, "attention.attn." + n) for n in "qkv"], dim=-1)
    a = lin(attention(qkv, mask, bias, heads), "attention.attn.o")
    h1 = layer_norm(a + h, g("attention.LayerNorm.weight"), g("attention.LayerNorm.bias"), eps)
    f = lin(gelu(lin(h1, "intermediate.dense")), "output.dense")
    return layer_norm(f + h1, g("output.LayerNorm.weight"), g("output.LayerNorm.bias"), eps)


def mean_pool(h, mask):
    """sum(h * mask) / clamp(sum(mask), 1e-9) over the tokens"""
    m = mask.to(h.dtype)[:, :, None]
    return (h * m).sum(1) / m.sum(1).clamp(min=1e-9)


def tower(P, ids, mask, layers, heads=12, eps=1e-12, pad=1):
    """The whole tower: embeddings (no token types, MPNet position ids) -> LayerNorm -> layers sharing one position bias -> masked mean."""
    L = ids.shape[1]
    # both tables are nn.Embedding(..., padding_idx=pad) in transformers: row `pad` is read like any other and receives no gradient
    emb = lambda w, i: torch.nn.functional.embedding(i, w, padding_idx=pad)
    h = emb(P["embeddings.word_embeddings.weight"], ids) + emb(P["embeddings.position_embeddings.weight"], position_ids(ids, pad))
    h = layer_norm(h, P["embeddings.LayerNorm.weight"], P["embeddings.LayerNorm.bias"], eps)
    bias = position_bias(P["encoder.relative_attention_bias.weight"], L)
    for i in range(layers):
        h = layer(P, f"encoder.layer.{i}.", h, mask, bias, heads, eps)
    return mean_pool(h, mask)


def param_shapes(layers, hidden=768, heads=12, inner=3072, vocab=30527, max_pos=512, buckets=32):
    """name -> shape of transformers.MPNetModel's state dict (MPNetConfig() defaults), in its order"""
    s = {"embeddings.word_embeddings.weight": (vocab, hidden), "embeddings.position_embeddings.weight": (max_pos, hidden),
         "embeddings.LayerNorm.weight": (hidden,), "embeddings.LayerNorm.bias": (hidden,)}
    for i in range(layers):
        p = f"encoder.layer.{i}."
        for n in "qkvo":
            s[p + f"attention.attn.{n}.weight"], s[p + f"attention.attn.{n}.bias"] = (hidden, hidden), (hidden,)
        s[p + "attention.LayerNorm.weight"], s[p + "attention.LayerNorm.bias"] = (hidden,), (hidden,)
        s[p + "intermediate.dense.weight"], s[p + "intermediate.dense.bias"] = (inner, hidden), (inner,)
        s[p + "output.dense.weight"], s[p + "output.dense.bias"] = (hidden, inner), (hidden,)
        s[p + "output.LayerNorm.weight"], s[p + "output.LayerNorm.bias"] = (hidden,), (hidden,)
    s["encoder.relative_attention_bias.weight"] = (buckets, heads)
    s["pooler.dense.weight"], s["pooler.dense.bias"] = (hidden, hidden), (hidden,)
    return s


class RefMPNet(torch.nn.Module):
    """The tower above as a module whose state-dict keys are transformers.MPNetModel's (so tests/detfill.py fills it like the reference's)."""

    def __init__(self, layers, **kw):
        super().__init__()
        self.layers = layers
        for name, shape in param_shapes(layers, **kw).items():
            mod, parts = self, name.split(".")
            for part in parts[:-1]:
                if part not in mod._modules:
                    mod.add_module(part, torch.nn.Module())
                mod = mod._modules[part]
            mod.register_parameter(parts[-1], torch.nn.Parameter(torch.zeros(shape)))

    def forward(self, input_ids, attention_mask):
        return tower(dict(self.named_parameters()), input_ids, attention_mask, self.layers)


class RefTextEncoder(torch.nn.Module):
    """reference encoder.TextEncoder(mode="train_sbert", model_name=<MPNet>): `strans` + mean pooling"""

    def __init__(self, layers):
        super().__init__()
        self.strans = RefMPNet(layers)

    def forward(self, x):
        return self.strans(x["input_ids"], x["attention_mask"])
