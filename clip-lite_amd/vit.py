"""ViT image encoder on the HIP kernels: the module tree of torchvision.models.vit_b_32 / vit_b_16 (parameter names and shapes identical, so
checkpoints interchange; `heads` replaced by the identity as reference encoder.py:41 does to every torchvision model, so there is no `heads.*`
and the output is the class token behind `encoder.ln`, [B][768]) and the hand-scheduled forward/backward executor beside it.

The reference's ImageEncoder cannot build these (its `zero_init_residual=False` argument makes torchvision's ViT constructors fail), so this
tower goes beyond it, as LARS, k-NN and the logistic-regression probe did. Everything but three streaming kernels (csrc/vit_ops.hip) is the text
tower's hot path: the attention kernels of csrc/bert_ops.hip (head size 64, at most 128 tokens: vit_b_32 at 224 pixels has 50, vit_b_16 at 160
has 101, vit_b_16 at 224 would have 197 and is refused), clite_layernorm_fwd / _bwd, the GEMM engine's fused epilogues and the grouped weight
gradients.

Per layer (pre-LayerNorm order, torchvision EncoderBlock): y = LN1(x); qkv = y W_in^T + b_in; ctx = attention(qkv); x1 = x + ctx W_o^T + b_o
(residual in the GEMM epilogue); z = LN2(x1); g = GELU(z W_0^T + b_0) with the pre-activation kept; x2 = x1 + g W_3^T + b_3. Backward is the
mirror; the input gradient of a block half is LayerNorm_bwd(...) + the skip gradient, added by clite_add (clite_layernorm_bwd has no residual
input). Dropout and attention dropout are 0, torchvision's default; another value raises.

Patch dropout (FLIP, Li et al. 2023; `patch_dropout=r`): in training each image keeps kept_patches(P, r) of its P patches, chosen on the device
from the pass's seed (clite_vit_keep_indices), plus the class token, and everything from the patch matrix on runs at that length through the
same code (clite_vit_patchify_keep, clite_vit_tokens_keep_fwd / _bwd in place of the three full kernels). Evaluation sees every token.
"""
import math

import torch
import torch.nn as nn

from . import hip
from .bert import MAX_TOKENS, LayerNormParams, LinearParams, _alloc, _dgrad, _linear_grads

SPECS = {"vit_b_32": (32, 12, 768, 12, 3072), "vit_b_16": (16, 12, 768, 12, 3072)}      # patch, layers, hidden, heads, mlp_dim
LN_EPS = 1e-6


def _hw(image_size):
    if isinstance(image_size, (tuple, list)):
        H, W = image_size
        return int(H), int(W)
    return int(image_size), int(image_size)


def token_count(name, H, W=None):
    """Tokens of a `name` tower on H x W images, class token included: (H / p) (W / p) + 1. Raises where the image is not a whole number of patches
    or the count exceeds what the attention kernels cover. Needs no device."""
    if name not in SPECS:
        raise ValueError(f"unsupported visual backbone {name!r}; supported ViTs: {sorted(SPECS)}")
    W = H if W is None else W
    p = SPECS[name][0]
    if H <= 0 or W <= 0 or H % p or W % p:
        raise ValueError(f"clip_lite_amd: {name} cuts images into {p} x {p} patches; the image size {H} x {W} (DATA.IMAGE_CROP_SIZE) must be a "
                         f"positive multiple of {p}")
    L = (H // p) * (W // p) + 1
    if L > MAX_TOKENS:
        raise ValueError(f"clip_lite_amd: {name} at {H} x {W} pixels has {L} tokens; the attention kernels support at most {MAX_TOKENS} "
                         f"(vit_b_32 up to 352 pixels, vit_b_16 up to 176)")
    return L


def kept_patches(P, r):
    """Patches each image keeps under patch dropout with ratio r (FLIP; open_clip's PatchDropout rule): max(1, int(P (1 - r))). Needs no device."""
    r = float(r)
    if not 0.0 <= r < 1.0:
        raise ValueError(f"clip_lite_amd: patch_dropout (MODEL.VISUAL.PATCH_DROPOUT) is the share of patches dropped in training and must lie in "
                         f"[0, 1); got {r}")
    return max(1, int(P * (1.0 - r)))


class _PatchProj(nn.Module):
    """nn.Conv2d(3, C, p, stride=p)'s state_dict surface. The arena keeps the weight in torch's own [C][3][p][p] order (not the [K][R][S][C] of the
    implicit-GEMM convolutions), so that `.view(C, 3 p p)` is the patch GEMM's operand."""

    def __init__(self, hidden, p):
        super().__init__()
        self.patch = p
        self.weight = nn.Parameter(torch.empty(hidden, 3, p, p))
        self.bias = nn.Parameter(torch.zeros(hidden))
        self.weight._clite_plain = True          # runtime._kernel_shape
        nn.init.trunc_normal_(self.weight, std=math.sqrt(1.0 / (3 * p * p)))


class _SelfAttention(nn.Module):
    """nn.MultiheadAttention's parameters and its default initialisation."""

    def __init__(self, h):
        super().__init__()
        self.in_proj_weight = nn.Parameter(torch.empty(3 * h, h))
        self.in_proj_bias = nn.Parameter(torch.zeros(3 * h))
        nn.init.xavier_uniform_(self.in_proj_weight)
        self.out_proj = LinearParams(h, h)
        self.out_proj.bias.data.zero_()

    def dgrad_weights(self):
        """Bare parameters whose input gradient reads a transposed copy (runtime.DeviceRuntime registers `.weight` of Linear-like modules itself)."""
        return [self.in_proj_weight]


class _Mlp(nn.Module):
    """torchvision MLPBlock: Linear, GELU, Dropout, Linear, Dropout -> parameters under `0` and `3`."""

    def __init__(self, h, inner):
        super().__init__()
        for name, lin in (("0", LinearParams(h, inner)), ("3", LinearParams(inner, h))):
            nn.init.xavier_uniform_(lin.weight)
            nn.init.normal_(lin.bias, std=1e-6)
            self.add_module(name, lin)

    def parts(self):
        return self._modules["0"], self._modules["3"]


class EncoderBlock(nn.Module):
    def __init__(self, h, inner):
        super().__init__()
        self.ln_1 = LayerNormParams(h, LN_EPS)
        self.self_attention = _SelfAttention(h)
        self.ln_2 = LayerNormParams(h, LN_EPS)
        self.mlp = _Mlp(h, inner)


class _Encoder(nn.Module):
    def __init__(self, L, n, h, inner):
        super().__init__()
        self.pos_embedding = nn.Parameter(torch.empty(1, L, h).normal_(std=0.02))
        self.layers = nn.Module()
        for i in range(n):
            self.layers.add_module(f"encoder_layer_{i}", EncoderBlock(h, inner))
        self.ln = LayerNormParams(h, LN_EPS)

    def blocks(self):
        return list(self.layers._modules.values())


class _Params:
    """A set of parameters with the `.parameters()` surface DeviceRuntime.grads_ready reads."""

    def __init__(self, ps):
        self._ps = list(ps)

    def parameters(self):
        return iter(self._ps)


class VisionTransformer(nn.Module):
    """name: "vit_b_32" | "vit_b_16". image_size: the side of the square input, or (H, W). num_layers / hidden / heads / mlp_dim override the spec
    (small test models); hidden == heads * 64 because the attention kernels are built for head size 64. patch_dropout: the share of patches each
    image drops in training (FLIP): the tower then runs on kept_patches(P, r) patches + the class token; evaluation sees every token."""

    kind = "vit"

    def __init__(self, name="vit_b_32", image_size=224, num_layers=None, hidden=None, heads=None, mlp_dim=None, dropout=0.0, attention_dropout=0.0,
                 patch_dropout=0.0):
        super().__init__()
        if name not in SPECS:
            raise ValueError(f"unsupported visual backbone {name!r}; supported ViTs: {sorted(SPECS)}")
        kept_patches(1, patch_dropout)          # (raises for a ratio outside [0, 1))
        self.patch_dropout = float(patch_dropout)
        if dropout != 0.0 or attention_dropout != 0.0:
            raise ValueError(f"clip_lite_amd: the ViT tower runs without dropout (torchvision's default); got dropout={dropout}, "
                             f"attention_dropout={attention_dropout}")
        p, n, h, nh, inner = SPECS[name]
        n = n if num_layers is None else int(num_layers)
        h = h if hidden is None else int(hidden)
        nh = nh if heads is None else int(heads)
        inner = inner if mlp_dim is None else int(mlp_dim)
        assert h == nh * 64, "the attention kernel is built for head size 64"
        assert h % 8 == 0 and h <= 2048 and inner % 8 == 0, "clite_layernorm_fwd needs C % 8 == 0 and C <= 2048"
        self.name, self.patch, self.hidden, self.heads, self.inner = name, p, h, nh, inner
        self.image_hw = _hw(image_size)
        self.seq_length = token_count(name, *self.image_hw)
        self.class_token = nn.Parameter(torch.zeros(1, 1, h))
        self.conv_proj = _PatchProj(h, p)
        self.encoder = _Encoder(self.seq_length, n, h, inner)
        self.out_dim = h          # (torchvision's `heads` is the identity here, reference encoder.py:41: no `heads.*` parameters)
        # class_token, conv_proj.*, encoder.pos_embedding: adjacent in the arena (named_parameters() order), final behind the first layer's backward
        self._stem = _Params([self.class_token, self.conv_proj.weight, self.conv_proj.bias, self.encoder.pos_embedding])


# ---------------------------------------------------------------------------------------------------- executor
def _ones_mask(rt, net, B, L):
    """All-ones int64 [B][L] attention mask (every image token is real). Kept per shape outside a stream capture; a capture makes its own, in the
    graph's memory pool."""
    if rt._capturing:
        return torch.ones(B, L, device=rt.device, dtype=torch.int64)
    cache = net.__dict__.setdefault("_mask_cache", {})
    key = (B, L, str(rt.device))
    m = cache.get(key)
    if m is None:
        cache.clear()
        m = cache[key] = torch.ones(B, L, device=rt.device, dtype=torch.int64)
    return m


def vit_forward(rt, net, image, training=True):
    """image: f32 NCHW [B][3][H][W] on the device, H x W the size the tower was built for. Returns (features [B][hidden], ctx)."""
    if rt.fp8 and rt.lowp:
        raise RuntimeError("clip_lite_amd: the fp8 forward (--fp8) is built for the ResNet image encoders only; run a ViT image encoder without it")
    if image.dim() != 4 or image.shape[1] != 3 or tuple(image.shape[2:]) != net.image_hw:
        raise RuntimeError(f"clip_lite_amd: this {net.name} was built for {net.image_hw[0]} x {net.image_hw[1]} images (its position embedding has "
                           f"{net.seq_length} tokens); got a batch of shape {tuple(image.shape)}")
    dt, A = rt.dt, rt.arena
    B, _, H, W = image.shape
    p, Cc, heads, inner = net.patch, net.hidden, net.heads, net.inner
    L = net.seq_length
    P, K = L - 1, 3 * p * p
    cls, pos, wp = A.w(net.class_token).view(Cc), A.w(net.encoder.pos_embedding).view(L, Cc), A.w(net.conv_proj.weight).view(Cc, K)
    keep = None
    if training and net.patch_dropout > 0:
        # patch dropout: the kept patches are chosen on the device from this pass's seed (inside a captured step from the indirect one, so every
        # replay draws a fresh set), and everything from the patch matrix on runs on Kk patches per image: L is Kk + 1 from here
        Kk = kept_patches(P, net.patch_dropout)
        step = rt.next_step(True)
        idx = torch.empty(B, Kk, device=rt.device, dtype=torch.int32)
        inv = torch.empty(B, P, device=rt.device, dtype=torch.int32)
        hip.vit_keep_indices(idx, inv, B, P, Kk, step.seed, step.site())
        patches = _alloc(rt, B * Kk, K)
        hip.vit_patchify_keep(dt, image, idx, patches, B, H, W, p, Kk)
        e = _alloc(rt, B * Kk, Cc)
        hip.gemm_nt(dt, patches, wp, B * Kk, Cc, K, hip.epilogue(e, Cc, bias=net.conv_proj.bias))
        keep, L = (idx, inv, P, Kk), Kk + 1
        M = B * L
        x = _alloc(rt, M, Cc)
        hip.vit_tokens_keep_fwd(dt, e, cls, pos, idx, x, B, P, Kk, Cc)
    else:
        M = B * L
        patches = _alloc(rt, B * P, K)
        hip.vit_patchify(dt, image, patches, B, H, W, p)
        e = _alloc(rt, B * P, Cc)
        hip.gemm_nt(dt, patches, wp, B * P, Cc, K, hip.epilogue(e, Cc, bias=net.conv_proj.bias))
        x = _alloc(rt, M, Cc)
        hip.vit_tokens_fwd(dt, e, cls, pos, x, B, P, Cc)
    mask = _ones_mask(rt, net, B, L)
    ctx = {"B": B, "L": L, "patches": patches, "mask": mask, "layers": [], "keep": keep, "idx": keep and keep[0], "inv": keep and keep[1]}
    for layer in net.encoder.blocks():
        sa, (m0, m3) = layer.self_attention, layer.mlp.parts()
        y = _alloc(rt, M, Cc)
        st1 = torch.empty(M, 2, device=rt.device, dtype=torch.float32)
        hip.layernorm_fwd(dt, x, layer.ln_1.weight, layer.ln_1.bias, layer.ln_1.eps, y, st1, M, Cc)
        qkv = _alloc(rt, M, 3 * Cc)
        hip.gemm_nt(dt, y, A.w(sa.in_proj_weight), M, 3 * Cc, Cc, hip.epilogue(qkv, 3 * Cc, bias=sa.in_proj_bias))
        ctxt = _alloc(rt, M, Cc)
        hip.attention_fwd(dt, qkv, mask, ctxt, B, L, heads)
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
    # encoder.ln on the B class rows only: LayerNorm acts row by row and nothing reads the other tokens
    ln = net.encoder.ln
    xc = _alloc(rt, B, Cc)
    hip.vit_class_gather(dt, x, xc, B, L, Cc)
    feat = _alloc(rt, B, Cc)
    stf = torch.empty(B, 2, device=rt.device, dtype=torch.float32)
    hip.layernorm_fwd(dt, xc, ln.weight, ln.bias, ln.eps, feat, stf, B, Cc)
    ctx["xc"], ctx["stf"] = xc, stf
    return feat, ctx


def _param_grads(rt, w, b, dy, x, M, defer):
    """bert._linear_grads for a weight / bias pair that is not a LinearParams (in_proj_*, conv_proj.*): dW[N][K] += dy^T x, db += colsum(dy)."""
    N, K = dy.shape[1], x.shape[1]
    dw = rt.arena.g(w).view(N, K) if w.requires_grad else None
    db = rt.arena.g(b) if b.requires_grad else None
    if dw is not None:
        _linear_grads(rt, None, dy, x, M, dw=dw, db=db, defer=defer)
    elif db is not None:
        hip.colsum(rt.dt, dy, db, M, N)


def vit_backward(rt, net, ctx, dfeat, defer=None):
    """Parameter gradients into the arena. defer: a hip.WgradGroup that collects the Linear weight gradients and is left to the caller to launch;
    without one an uncaptured bf16 backward groups them itself and launches once at the end (per layer under eager data parallel, so that the
    layer's region of the gradient arena can be exchanged at once), as bert.bert_backward does."""
    dt, A = rt.dt, rt.arena
    B, L = ctx["B"], ctx["L"]
    Cc, heads, inner = net.hidden, net.heads, net.inner
    P, M = L - 1, B * L
    own_group = None
    if defer is None and rt.group_wgrad and not rt._capturing:      # (a capture cannot allocate the pinned staging)
        defer = own_group = hip.WgradGroup(rt.dt)
    staged = own_group is not None and getattr(rt, "exchange", None) is not None
    A.ensure_transposed(capturing=rt._capturing)
    ln = net.encoder.ln
    dxc = _alloc(rt, B, Cc)
    hip.layernorm_bwd(dt, dfeat.to(rt.tdtype).contiguous(), ctx["xc"], ctx["stf"], ln.weight, dxc, None, A.g(ln.weight), A.g(ln.bias), B, Cc)
    if own_group is None or staged:
        rt.grads_ready(ln)
    dh = torch.zeros(M, Cc, device=rt.device, dtype=rt.tdtype)
    hip.vit_class_scatter(dt, dxc, dh, B, L, Cc)
    for (layer, x, st1, y, qkv, ctxt, x1, st2, z, f, g) in reversed(ctx["layers"]):
        sa, (m0, m3) = layer.self_attention, layer.mlp.parts()
        # x2 = x1 + MLP(LN2(x1)): dh is dx2
        _linear_grads(rt, m3, dh, g, M, defer=defer)
        df = _alloc(rt, M, inner)
        fold = m0.bias.requires_grad          # the first Linear's bias gradient = the column sums of df, accumulated by the epilogue that stores df
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
        hip.attention_bwd(dt, qkv, ctx["mask"], dctx, dqkv, B, L, heads)
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
    # token assembly and the patch projection: conv_proj.weight's gradient is de^T patches, in the 4-D parameter's own [C][3][p][p] order
    # (under patch dropout over the kept patches only: B * Kk rows, the position embedding's gradient scattered through `inv`)
    dpos, dcls = A.g(net.encoder.pos_embedding).view(net.seq_length, Cc), A.g(net.class_token).view(Cc)
    if ctx["keep"] is not None:
        _, inv, Pf, P = ctx["keep"]
        de = _alloc(rt, B * P, Cc)
        hip.vit_tokens_keep_bwd(dt, dh, inv, de, dpos, dcls, B, Pf, P, Cc)
    else:
        de = _alloc(rt, B * P, Cc)
        hip.vit_tokens_bwd(dt, dh, de, dpos, dcls, B, P, Cc)
    _param_grads(rt, net.conv_proj.weight, net.conv_proj.bias, de, ctx["patches"], B * P, defer)
    if own_group is not None:
        own_group.launch()
        if staged:
            rt.grads_ready(net._stem)
        else:
            rt.grads_ready(net)
    else:
        rt.grads_ready(net._stem)
