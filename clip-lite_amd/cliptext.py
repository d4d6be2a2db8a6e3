"""CLIP text transformer on the HIP kernels: the module tree of open_clip's TextTransformer (parameter names and shapes identical, so checkpoints
interchange) and the hand-scheduled forward/backward executor beside it.

The tower every CLIP / open_clip / FLIP recipe pairs with a ViT: token + positional embeddings (no token types, no LayerNorm behind them), pre-LayerNorm
residual blocks with CAUSAL self-attention, the state of the end-of-text token through `ln_final`, and `x @ text_projection` (no bias) into the
joint width. Per layer it is the loop of vit.vit_forward / vit_backward on the same kernels (clite_layernorm_fwd / _bwd, the GEMM engine's fused
epilogues, the grouped weight gradients) with the causal attention entry points (csrc/bert_ops.hip: clite_attention_causal_fwd / _bwd) in place
of the bidirectional ones; the loop is written out here a second time rather than shared with vit.py, whose launches other tests pin.

Limits: head size 64 (width = 64 heads), at most 128 tokens (context_length <= 128), GELU (open_clip's default; QuickGELU is not built), no
dropout, no pretrained weights. The end-of-text token is found from the attention mask — the last attended token — not by argmax over the ids as
CLIP does with its BPE vocabulary, so it does not depend on the vocabulary's id order: under the loader's WordPiece framing ([CLS] ... [SEP], pad 0)
[SEP] is the last attended token and plays the end-of-text role.
"""
import torch
import torch.nn as nn

from . import hip
from .bert import MAX_TOKENS, EmbeddingParams, LayerNormParams, LinearParams, _alloc, _dgrad, _linear_grads
from .vit import _param_grads, _Params

LN_EPS = 1e-5
SPECS = {"clip_text_b": (77, 512, 8, 12, 512)}      # context_length, width, heads, layers, embed_dim


class _Attn(nn.Module):
    """nn.MultiheadAttention's parameters with CLIP's initialisation."""

    def __init__(self, w, attn_std, proj_std):
        super().__init__()
        self.in_proj_weight = nn.Parameter(torch.empty(3 * w, w).normal_(std=attn_std))
        self.in_proj_bias = nn.Parameter(torch.zeros(3 * w))
        self.out_proj = LinearParams(w, w, std=proj_std)

    def dgrad_weights(self):
        """Bare parameters whose input gradient reads a transposed copy (runtime.DeviceRuntime registers `.weight` of Linear-like modules itself)."""
        return [self.in_proj_weight]


class _Mlp(nn.Module):
    def __init__(self, w, fc_std, proj_std):
        super().__init__()
        self.c_fc = LinearParams(w, 4 * w, std=fc_std)
        self.c_proj = LinearParams(4 * w, w, std=proj_std)


class ResidualAttentionBlock(nn.Module):
    def __init__(self, w, attn_std, proj_std, fc_std):
        super().__init__()
        self.ln_1 = LayerNormParams(w, LN_EPS)
        self.attn = _Attn(w, attn_std, proj_std)
        self.ln_2 = LayerNormParams(w, LN_EPS)
        self.mlp = _Mlp(w, fc_std, proj_std)


class _Transformer(nn.Module):
    def __init__(self, n, w):
        super().__init__()
        # CLIP's init (open_clip TextTransformer.init_parameters): in_proj width^-0.5, out_proj / c_proj width^-0.5 (2 layers)^-0.5, c_fc (2 width)^-0.5
        attn_std, proj_std, fc_std = w ** -0.5, (w ** -0.5) * ((2 * max(n, 1)) ** -0.5), (2 * w) ** -0.5
        self.resblocks = nn.ModuleList([ResidualAttentionBlock(w, attn_std, proj_std, fc_std) for _ in range(n)])


class ClipTextModel(nn.Module):
    """open_clip TextTransformer(context_length, vocab_size, width, heads, layers, output_dim) with its parameter names: token_embedding.weight,
    positional_embedding, transformer.resblocks.{i}.{ln_1, attn.in_proj_weight, attn.in_proj_bias, attn.out_proj, ln_2, mlp.c_fc, mlp.c_proj},
    ln_final, text_projection [width][embed_dim]. The vocabulary defaults to the loader's WordPiece one (30522)."""

    kind = "clip"      # (bert.BertModel: "bert", mpnet.MPNetModel: "mpnet")
    padding_idx = 0    # what the captured step pads caption ids with (train_loop.TrainStep._caption_fill); no embedding row is special

    def __init__(self, vocab=30522, context_length=77, width=512, heads=8, num_hidden_layers=12, embed_dim=512):
        super().__init__()
        assert width == heads * 64, "the attention kernel is built for head size 64"
        assert width % 8 == 0 and width <= 2048 and embed_dim % 8 == 0, "clite_layernorm_fwd needs C % 8 == 0 and C <= 2048"
        if not 1 <= int(context_length) <= MAX_TOKENS:
            raise ValueError(f"clip_lite_amd: the CLIP text tower's context length (MODEL.TEXTUAL.CONTEXT_LENGTH) is {context_length}; the causal "
                             f"attention kernels support 1 to {MAX_TOKENS} tokens")
        self.vocab, self.context_length, self.hidden, self.heads, self.inner = vocab, int(context_length), width, heads, 4 * width
        self.token_embedding = EmbeddingParams(vocab, width, std=0.02)
        self.positional_embedding = nn.Parameter(torch.empty(self.context_length, width).normal_(std=0.01))
        self.transformer = _Transformer(num_hidden_layers, width)
        self.ln_final = LayerNormParams(width, LN_EPS)
        self.text_projection = nn.Parameter(torch.empty(width, embed_dim).normal_(std=width ** -0.5))
        self.out_dim = embed_dim
        # the embeddings are adjacent in the arena (named_parameters() order) and final behind the first layer's backward; the head before the last
        self._stem = _Params([self.token_embedding.weight, self.positional_embedding])
        self._head = _Params([self.ln_final.weight, self.ln_final.bias, self.text_projection])

    def contiguous_groups(self, prefix):
        """What model.attach_runtime asks every text tower for: in_proj_weight is one [3 width][width] parameter already, so nothing needs pulling together."""
        return []


# ---------------------------------------------------------------------------------------------------- executor
def cliptext_forward(rt, net, input_ids, attention_mask, step=None):
    """input_ids / attention_mask: int64 [B][L] on the device, right-padded, L <= net.context_length. Returns (features [B][embed_dim], ctx).
    `step` (the dropout state the other text towers take) is unused: the tower has no dropout."""
    B, L = input_ids.shape
    if L > net.context_length:
        raise RuntimeError(f"clip_lite_amd: a batch of {L}-token captions does not fit the CLIP text tower's context of {net.context_length} tokens "
                           "(MODEL.TEXTUAL.CONTEXT_LENGTH; its positional embedding has that many rows)")
    if rt.fp8_text and rt.lowp:
        raise RuntimeError("clip_lite_amd: the fp8 forward (--fp8) is built for the BERT text encoder only; run the CLIP text tower without it")
    dt, A = rt.dt, rt.arena
    Cc, heads, inner, E = net.hidden, net.heads, net.inner, net.out_dim
    M = B * L
    ids = input_ids.contiguous()
    mask = attention_mask.contiguous().to(torch.int64)
    x = _alloc(rt, M, Cc)
    hip.embed_clip_fwd(dt, ids, A.w(net.token_embedding.weight), A.w(net.positional_embedding), x, M, L, Cc, net.vocab)
    ctx = {"B": B, "L": L, "ids": ids, "mask": mask, "layers": []}
    for layer in net.transformer.resblocks:
        sa, m0, m3 = layer.attn, layer.mlp.c_fc, layer.mlp.c_proj
        y = _alloc(rt, M, Cc)
        st1 = torch.empty(M, 2, device=rt.device, dtype=torch.float32)
        hip.layernorm_fwd(dt, x, layer.ln_1.weight, layer.ln_1.bias, layer.ln_1.eps, y, st1, M, Cc)
        qkv = _alloc(rt, M, 3 * Cc)
        hip.gemm_nt(dt, y, A.w(sa.in_proj_weight), M, 3 * Cc, Cc, hip.epilogue(qkv, 3 * Cc, bias=sa.in_proj_bias))
        ctxt = _alloc(rt, M, Cc)
        hip.attention_causal_fwd(dt, qkv, mask, ctxt, B, L, heads)
        x1 = _alloc(rt, M, Cc)
        hip.gemm_nt(dt, ctxt, A.w(sa.out_proj.weight), M, Cc, Cc, hip.epilogue(x1, Cc, bias=sa.out_proj.bias, residual=x))
        z = _alloc(rt, M, Cc)
        st2 = torch.empty(M, 2, device=rt.device, dtype=torch.float32)
        hip.layernorm_fwd(dt, x1, layer.ln_2.weight, layer.ln_2.bias, layer.ln_2.eps, z, st2, M, Cc)
        f = _alloc(rt, M, inner)      # MLP pre-activation (kept for GELU')
        g = _alloc(rt, M, inner)
        hip.gemm_nt(dt, z, A.w(m0.weight), M, inner, Cc, hip.epilogue(g, inner, bias=m0.bias, act=hip.ACT_GELU, preact=f))
        x2 = _alloc(rt, M, Cc)
        hip.gemm_nt(dt, g, A.w(m3.weight), M, Cc, inner, hip.epilogue(x2, Cc, bias=m3.bias, residual=x1))
        ctx["layers"].append((layer, x, st1, y, qkv, ctxt, x1, st2, z, f, g))
        x = x2
    # ln_final on the B end-of-text rows only: LayerNorm acts row by row and nothing reads the other tokens
    ln = net.ln_final
    xe = _alloc(rt, B, Cc)
    idx = torch.empty(B, device=rt.device, dtype=torch.int32)
    hip.last_token_gather(dt, x, mask, xe, idx, B, L, Cc)
    xn = _alloc(rt, B, Cc)
    stf = torch.empty(B, 2, device=rt.device, dtype=torch.float32)
    hip.layernorm_fwd(dt, xe, ln.weight, ln.bias, ln.eps, xn, stf, B, Cc)
    feat = _alloc(rt, B, E)
    hip.gemm_nn(dt, xn, A.w(net.text_projection), B, E, Cc, hip.epilogue(feat, E))      # x @ text_projection, no bias
    ctx["xe"], ctx["stf"], ctx["xn"], ctx["idx"] = xe, stf, xn, idx
    return feat, ctx


def cliptext_backward(rt, net, ctx, dfeat, defer=None):
    """Parameter gradients into the arena; `defer` and the per-layer grads_ready calls as in vit.vit_backward."""
    dt, A = rt.dt, rt.arena
    B, L = ctx["B"], ctx["L"]
    Cc, heads, inner, E = net.hidden, net.heads, net.inner, net.out_dim
    M = B * L
    own_group = None
    if defer is None and rt.group_wgrad and not rt._capturing:      # (a capture cannot allocate the pinned staging)
        defer = own_group = hip.WgradGroup(rt.dt)
    staged = own_group is not None and getattr(rt, "exchange", None) is not None
    A.ensure_transposed(capturing=rt._capturing)
    ln, tp = net.ln_final, net.text_projection
    dfeat = dfeat.to(rt.tdtype).contiguous()
    if tp.requires_grad:          # d text_projection [width][embed_dim] += xn^T dfeat: B rows, launched in line so that the head is final at once
        hip.gemm_tn(dt, ctx["xn"], dfeat, Cc, E, B, hip.epilogue(A.g(tp), E, atomic=True, out_f32=True))
    dxn = _alloc(rt, B, Cc)
    hip.gemm_nt(dt, dfeat, A.w(tp), B, Cc, E, hip.epilogue(dxn, Cc))          # dfeat @ text_projection^T
    dxe = _alloc(rt, B, Cc)
    hip.layernorm_bwd(dt, dxn, ctx["xe"], ctx["stf"], ln.weight, dxe, None, A.g(ln.weight), A.g(ln.bias), B, Cc)
    if own_group is None or staged:
        rt.grads_ready(net._head)
    dh = torch.zeros(M, Cc, device=rt.device, dtype=rt.tdtype)
    hip.last_token_scatter(dt, dxe, ctx["idx"], dh, B, L, Cc)
    for (layer, x, st1, y, qkv, ctxt, x1, st2, z, f, g) in reversed(ctx["layers"]):
        sa, m0, m3 = layer.attn, layer.mlp.c_fc, layer.mlp.c_proj
        # x2 = x1 + MLP(LN2(x1)): dh is dx2
        _linear_grads(rt, m3, dh, g, M, defer=defer)
        df = _alloc(rt, M, inner)
        fold = m0.bias.requires_grad          # c_fc's bias gradient = the column sums of df, accumulated by the epilogue that stores df
        _dgrad(rt, dh, M, inner, Cc, hip.epilogue(df, inner, dact_aux=f, dact=hip.DACT_GELU, colsum=A.g(m0.bias) if fold else None, colsum_rows=1),
               m3.weight)
        _linear_grads(rt, m0, df, z, M, bias_done=fold, defer=defer)
        dz = _alloc(rt, M, Cc)
        _dgrad(rt, df, M, Cc, inner, hip.epilogue(dz, Cc), m0.weight)
        dln = _alloc(rt, M, Cc)
        hip.layernorm_bwd(dt, dz, x1, st2, layer.ln_2.weight, dln, None, A.g(layer.ln_2.weight), A.g(layer.ln_2.bias), M, Cc)
        dx1 = _alloc(rt, M, Cc)
        hip.add(dt, dln, dh, dx1)             # pre-LayerNorm order: LayerNorm_bwd(...) + the skip gradient
        # x1 = x + out_proj(attention(in_proj(LN1(x))))
        _linear_grads(rt, sa.out_proj, dx1, ctxt, M, defer=defer)
        dctx = _alloc(rt, M, Cc)
        _dgrad(rt, dx1, M, Cc, Cc, hip.epilogue(dctx, Cc), sa.out_proj.weight)
        dqkv = _alloc(rt, M, 3 * Cc)
        hip.attention_causal_bwd(dt, qkv, ctx["mask"], dctx, dqkv, B, L, heads)
        _param_grads(rt, sa.in_proj_weight, sa.in_proj_bias, dqkv, y, M, defer)
        dy = _alloc(rt, M, Cc)
        _dgrad(rt, dqkv, M, Cc, 3 * Cc, hip.epilogue(dy, Cc), sa.in_proj_weight)
        dln = _alloc(rt, M, Cc)
        hip.layernorm_bwd(dt, dy, x, st1, layer.ln_1.weight, dln, None, A.g(layer.ln_1.weight), A.g(layer.ln_1.bias), M, Cc)
        dh = _alloc(rt, M, Cc)
        hip.add(dt, dln, dx1, dh)
        if own_group is None:
            rt.grads_ready(layer)
        elif staged:
            own_group.launch()
            rt.grads_ready(layer)
            defer = own_group = hip.WgradGroup(rt.dt)
    # token assembly: nn.Embedding without a padding row (CLIP has none), the positional rows summed over the batch
    tok, pos = net.token_embedding.weight, net.positional_embedding
    dword = A.g(tok) if tok.requires_grad else None
    dpos = A.g(pos)[:L] if pos.requires_grad else None
    hip.embed_bwd(dt, ctx["ids"], dh, dword, dpos, M, L, Cc, net.vocab, padding_idx=-1)
    if own_group is not None:
        own_group.launch()
        if staged:
            rt.grads_ready(net._stem)
        else:
            rt.grads_ready(net)
    else:
        rt.grads_ready(net._stem)
