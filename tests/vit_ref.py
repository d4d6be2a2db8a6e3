"""Plain-torch restatement of the ViT image tower (torchvision.models.vit_b_32 / vit_b_16 with `heads` replaced by the identity), written from
the formulas as functions only and evaluated in whatever dtype its inputs have (the tests pass float64). Needs torch only: the CPU test pins it
to torch's own nn.MultiheadAttention / nn.LayerNorm / nn.Conv2d composition, the GPU tests compare the kernels with it.

Parameters come as a flat dict with torchvision's names relative to the model ("class_token", "conv_proj.weight", "encoder.pos_embedding",
"encoder.layers.encoder_layer_0.self_attention.in_proj_weight", ..., "encoder.ln.weight").

Rounding hooks: `round_to(x, dtype)` rounds a tensor through a storage dtype and returns it in its own (so that bf16-rounded parameters and
inputs are fed identically to the kernels and to this file), and every function that stores an activation takes `rnd`, applied to what the
kernels would store (identity by default)."""
import math

import torch

LN_EPS = 1e-6


def round_to(x, dtype):
    return x.to(dtype).to(x.dtype)


def _id(t):
    return t


def patchify(image, p):
    """[B][3][H][W] -> [B][(H/p)(W/p)][3 p p], patches row-major over (ph, pw), columns (c, i, j): what conv_proj.weight.view(C, -1) contracts with."""
    B, Cin, H, W = image.shape
    x = image.reshape(B, Cin, H // p, p, W // p, p).permute(0, 2, 4, 1, 3, 5)
    return x.reshape(B, (H // p) * (W // p), Cin * p * p)


def tokens(e, class_token, pos):
    """e [B][P][C] -> [B][P + 1][C]: class token in front, position embedding added"""
    B = e.shape[0]
    return torch.cat([class_token.reshape(1, 1, -1).expand(B, -1, -1), e], dim=1) + pos.reshape(1, -1, e.shape[-1])


def layer_norm(x, w, b, eps=LN_EPS):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * w + b


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def attention(qkv, heads):
    """qkv [B][L][3 * heads * 64] (q | k | v) -> [B][L][heads * 64]: softmax(q k^T / 8) v per head, every token attended"""
    B, L, _ = qkv.shape
    q, k, v = (t.reshape(B, L, heads, 64).permute(0, 2, 1, 3) for t in qkv.split(heads * 64, dim=-1))
    p = torch.softmax(q @ k.transpose(-1, -2) / 8.0, dim=-1)
    return (p @ v).permute(0, 2, 1, 3).reshape(B, L, heads * 64)


def block(P, pre, x, heads, rnd=_id):
    """torchvision EncoderBlock, pre-LayerNorm order, dropout off"""
    g = lambda n: P[pre + n]
    y = rnd(layer_norm(x, g("ln_1.weight"), g("ln_1.bias")))
    qkv = rnd(y @ g("self_attention.in_proj_weight").T + g("self_attention.in_proj_bias"))
    ctx = rnd(attention(qkv, heads))
    x1 = rnd(x + ctx @ g("self_attention.out_proj.weight").T + g("self_attention.out_proj.bias"))
    z = rnd(layer_norm(x1, g("ln_2.weight"), g("ln_2.bias")))
    h = rnd(gelu(z @ g("mlp.0.weight").T + g("mlp.0.bias")))
    return rnd(x1 + h @ g("mlp.3.weight").T + g("mlp.3.bias"))


def tower(P, image, layers, heads=12, rnd=_id):
    """features [B][C]: the class token behind encoder.ln"""
    w = P["conv_proj.weight"]
    C, p = w.shape[0], w.shape[-1]
    e = rnd(patchify(image, p) @ w.reshape(C, -1).T + P["conv_proj.bias"])
    x = rnd(tokens(e, P["class_token"], P["encoder.pos_embedding"]))
    for i in range(layers):
        x = block(P, f"encoder.layers.encoder_layer_{i}.", x, heads, rnd)
    return rnd(layer_norm(x[:, 0], P["encoder.ln.weight"], P["encoder.ln.bias"]))


def param_shapes(layers, L, patch=32, hidden=768, inner=3072):
    """name -> shape of torchvision's VisionTransformer state dict without `heads.*`, in its order"""
    s = {"class_token": (1, 1, hidden), "conv_proj.weight": (hidden, 3, patch, patch), "conv_proj.bias": (hidden,),
         "encoder.pos_embedding": (1, L, hidden)}
    for i in range(layers):
        p = f"encoder.layers.encoder_layer_{i}."
        s[p + "ln_1.weight"], s[p + "ln_1.bias"] = (hidden,), (hidden,)
        s[p + "self_attention.in_proj_weight"], s[p + "self_attention.in_proj_bias"] = (3 * hidden, hidden), (3 * hidden,)
        s[p + "self_attention.out_proj.weight"], s[p + "self_attention.out_proj.bias"] = (hidden, hidden), (hidden,)
        s[p + "ln_2.weight"], s[p + "ln_2.bias"] = (hidden,), (hidden,)
        s[p + "mlp.0.weight"], s[p + "mlp.0.bias"] = (inner, hidden), (inner,)
        s[p + "mlp.3.weight"], s[p + "mlp.3.bias"] = (hidden, inner), (hidden,)
    s["encoder.ln.weight"], s["encoder.ln.bias"] = (hidden,), (hidden,)
    return s


def features_and_grads(state_dict, image, layers, heads, dfeat, dtype=torch.float64):
    """(features, {name: gradient}) of sum(features * dfeat), everything in `dtype`"""
    P = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in state_dict.items()}
    feat = tower(P, image.to(dtype), layers, heads)
    (feat * dfeat.to(dtype)).sum().backward()
    return feat.detach(), {k: v.grad for k, v in P.items()}
