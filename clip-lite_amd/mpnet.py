"""MPNet text encoder: the module tree of transformers.MPNetModel (what reference encoder.py:171-175 builds with
`AutoModel.from_config(transformers.MPNetConfig())` for MODEL.TEXTUAL.NETWORK_NAME "sentence-transformers/paraphrase-mpnet-base-v2",
configs/done/fs_bs1024_ni250k.yaml), randomly initialised, run by bert.bert_forward / bert.bert_backward.

MPNet is BERT with four differences, each in a kernel of csrc/bert_ops.hip:
  1. every layer's attention scores get `relative_attention_bias[bucket(j - i)][head]`, an Embedding(32, heads) shared by all layers and trained
     (clite_attention_bias_build once per step, clite_attention_bias_fwd / _bwd, clite_attention_bias_grad_reduce);
  2. position ids are `padding_idx + cumsum(ids != pad) * (ids != pad)` with padding_idx = 1 (clite_embed_mpnet_fwd / _bwd);
  3. there are no token-type embeddings;
  4. the output is the masked mean of the last layer's tokens (reference encoder.py:197-198; clite_mean_pool_fwd / _bwd), not the pooler.
State-dict keys equal transformers.MPNetModel's, `pooler.dense.*` included — parameters the reference never gives a gradient, so they are frozen
here (requires_grad False: no weight decay, outside the gradient norm and the fused update, bit-equal after any number of steps)."""
import torch
import torch.nn as nn

from . import hip
from .bert import EmbeddingParams, LayerNormParams, LinearParams, _Intermediate, _Pooler, _SelfOutput


class _MPNetSelfAttention(nn.Module):
    def __init__(self, h):
        super().__init__()
        self.q, self.k, self.v, self.o = (LinearParams(h, h, std=0.02) for _ in range(4))


class _MPNetAttention(nn.Module):
    def __init__(self, h, eps):
        super().__init__()
        self.attn = _MPNetSelfAttention(h)
        self.LayerNorm = LayerNormParams(h, eps)


class MPNetLayer(nn.Module):
    def __init__(self, h, inner, eps):
        super().__init__()
        self.attention = _MPNetAttention(h, eps)
        self.intermediate = _Intermediate(h, inner)
        self.output = _SelfOutput(inner, h, eps)

    def attn_parts(self):
        a = self.attention
        return a.attn.q, a.attn.k, a.attn.v, a.attn.o, a.LayerNorm


class _MPNetEmbeddings(nn.Module):
    def __init__(self, vocab, h, max_pos, eps, padding_idx):
        super().__init__()
        self.word_embeddings = EmbeddingParams(vocab, h, padding_idx=padding_idx)
        self.position_embeddings = EmbeddingParams(max_pos, h, padding_idx=padding_idx)
        self.LayerNorm = LayerNormParams(h, eps)


class _MPNetEncoder(nn.Module):
    def __init__(self, n, h, heads, inner, eps, buckets):
        super().__init__()
        self.layer = nn.ModuleList([MPNetLayer(h, inner, eps) for _ in range(n)])
        self.relative_attention_bias = EmbeddingParams(buckets, heads)


class MPNetModel(nn.Module):
    """MPNetConfig() defaults (transformers) — what the reference constructs: hidden 768, 12 heads, intermediate 3072, vocab 30527, 512 positions,
    GELU(erf), LayerNorm eps 1e-12, hidden/attention dropout 0.1, 32 relative-position buckets, pad_token_id 1. (The published
    paraphrase-mpnet-base-v2 checkpoint's own config has 514 positions and eps 1e-5; the reference never loads it on this branch, so
    `max_pos` / `eps` are constructor arguments for whoever loads such a state dict.) MPNetPreTrainedModel._init_weights: N(0, 0.02), zero
    biases, zeroed padding rows."""

    kind = "mpnet"

    def __init__(self, num_hidden_layers=12, hidden=768, heads=12, inner=3072, vocab=30527, max_pos=512, dropout=0.1, eps=1e-12, padding_idx=1):
        super().__init__()
        assert hidden == heads * 64, "the attention kernel is built for head size 64"
        self.hidden, self.heads, self.inner, self.vocab, self.max_pos, self.padding_idx = hidden, heads, inner, vocab, max_pos, padding_idx
        self.hidden_dropout_prob = self.attention_probs_dropout_prob = dropout
        self.embeddings = _MPNetEmbeddings(vocab, hidden, max_pos, eps, padding_idx)
        self.encoder = _MPNetEncoder(num_hidden_layers, hidden, heads, inner, eps, 32)
        self.pooler = _Pooler(hidden)
        self.freeze_unused()
        # bucket of the relative offsets -31 .. 31: computed once on the host, travels with the module to the device, not part of the state dict
        self.register_buffer("bucket_table", torch.tensor(hip.relative_position_buckets(), dtype=torch.int32), persistent=False)

    def freeze_unused(self):
        for p in self.pooler.parameters():
            p.requires_grad = False

    def contiguous_groups(self, prefix):
        groups = []
        for i in range(len(self.encoder.layer)):
            base = f"{prefix}encoder.layer.{i}.attention.attn."
            groups.append([base + "q.weight", base + "k.weight", base + "v.weight"])
            groups.append([base + "q.bias", base + "k.bias", base + "v.bias"])
        return groups
