"""Patch dropout (FLIP, Li et al. 2023; open_clip's PatchDropout) of the ViT image tower as plain numpy / torch (test infrastructure; shared by
the host, the simulator and the GPU tests). One definition, the one include/clite.h states:

    P patches, ratio r in [0, 1): Kk = max(1, int(P (1 - r))) patches kept per image, the class token always, L' = Kk + 1 tokens.
    key[b][t]   the 24-bit uniform of element b * Ppad + t of the (seed, site) stream of rng_uniform4 (tests/dropout_ref.py: uniform8), Ppad = P
                rounded up to a multiple of 4
    rank[b][t]  #{u : key[b][u] < key[b][t], or key[b][u] == key[b][t] and u < t}; patch t is kept iff rank < Kk (ties to the lower index)
    idx[b]      the kept patches in ascending order; inv[b][t] = the position of t in idx[b], or -1
    tokens      s0[b][0] = class_token + pos[0], s0[b][1 + k] = e[b][idx[b][k]] + pos[1 + idx[b][k]]: all tokens assembled (vit_ref.tokens), then
                the rows [0] + (1 + idx[b]) gathered, which is what PatchDropout does behind the position embedding
and behind it the unchanged tower (vit_ref.block) at L' tokens. Gradients by autograd, in float64 when the inputs are."""
import numpy as np
import torch

import dropout_ref as D
import vit_ref as R


def kept(P, r):
    return max(1, int(P * (1.0 - r)))


def keys(seed, site, B, P):
    """float32 [B][P]"""
    Ppad = (P + 3) // 4 * 4
    return D.uniform8(seed, site, B * Ppad).reshape(B, Ppad)[:, :P].copy()


def select(key, Kk):
    """key [B][P] -> (idx int32 [B][Kk] ascending, inv int32 [B][P]); a stable sort ranks equal keys by index"""
    B, P = key.shape
    order = np.argsort(key, axis=1, kind="stable")
    idx = np.sort(order[:, :Kk], axis=1).astype(np.int32)
    inv = np.full((B, P), -1, np.int32)
    for b in range(B):
        inv[b, idx[b]] = np.arange(Kk, dtype=np.int32)
    return idx, inv


def keep_indices(seed, site, B, P, Kk):
    return select(keys(seed, site, B, P), Kk)


def gather_tokens(s, idx):
    """s [B][P + 1][C], idx [B][Kk] (any integer array / tensor) -> [B][Kk + 1][C]: the class row and the rows 1 + idx[b]"""
    idx = torch.as_tensor(np.asarray(idx), dtype=torch.long)
    rows = torch.cat([torch.zeros(idx.shape[0], 1, dtype=torch.long), 1 + idx], dim=1)
    return torch.gather(s, 1, rows[:, :, None].expand(-1, -1, s.shape[-1]))


def tower(P, image, layers, idx, heads=12, rnd=R._id):
    """vit_ref.tower with the token rows gathered behind the position embedding"""
    w = P["conv_proj.weight"]
    C, p = w.shape[0], w.shape[-1]
    e = rnd(R.patchify(image, p) @ w.reshape(C, -1).T + P["conv_proj.bias"])
    x = gather_tokens(rnd(R.tokens(e, P["class_token"], P["encoder.pos_embedding"])), idx)
    for i in range(layers):
        x = R.block(P, f"encoder.layers.encoder_layer_{i}.", x, heads, rnd)
    return rnd(R.layer_norm(x[:, 0], P["encoder.ln.weight"], P["encoder.ln.bias"]))


def features_and_grads(state_dict, image, layers, heads, dfeat, idx, dtype=torch.float64):
    """(features, {name: gradient}) of sum(features * dfeat) with the patches idx kept, everything in `dtype`"""
    P = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in state_dict.items()}
    feat = tower(P, image.to(dtype), layers, idx, heads)
    (feat * dfeat.to(dtype)).sum().backward()
    return feat.detach(), {k: v.grad for k, v in P.items()}
