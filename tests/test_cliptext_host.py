"""CPU-side tests of the CLIP text tower (clip-lite_amd/cliptext.py): tests/cliptext_ref.py pinned against torch's own modules (so that the GPU
tests compare the kernels with the definition, not with a private restatement), and the host logic - parameter names and shapes, the
initialisation, which name builds which tower, the tokenizer framing, the refusals and the config key. Needs no GPU."""
import math
import os
import types

import pytest
import torch
import torch.nn as nn

import cliptext_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the reference against torch
def _mha_case(B, L, H, seed):
    g = torch.Generator().manual_seed(seed)
    E = 64 * H
    y = torch.randn(B, L, E, generator=g, dtype=torch.float64)
    mha = nn.MultiheadAttention(E, H, batch_first=True).double()
    with torch.no_grad():
        for p in mha.parameters():
            p.copy_(torch.randn(p.shape, generator=g, dtype=torch.float64) * 0.1)
    return y, mha, R.ragged_mask(B, L, seed)


@pytest.mark.parametrize("B,L,H", [(3, 7, 8), (2, 40, 8)])
def test_causal_attention_reference_is_torch_multihead_attention(B, L, H):
    """nn.MultiheadAttention(512, 8, batch_first=True) with a boolean upper-triangular attn_mask and a key_padding_mask, against the reference's
    qkv -> ctx core between torch's own in- and out-projection; forward and, by autograd, the gradient of qkv against the written-out backward."""
    y, mha, mask = _mha_case(B, L, H, 11 * L)
    E = 64 * H
    causal = torch.ones(L, L, dtype=torch.bool).triu(1)
    want, _ = mha(y, y, y, attn_mask=causal, key_padding_mask=mask == 0, need_weights=False)
    qkv = (y @ mha.in_proj_weight.T + mha.in_proj_bias).reshape(B * L, 3 * E).detach().requires_grad_(True)
    ctx = R.causal_attention(qkv, mask, B, L, H)
    got = ctx.reshape(B, L, E) @ mha.out_proj.weight.T + mha.out_proj.bias
    valid = (mask == 1)[:, :, None].expand_as(got)          # (a padded query's row is defined too, but torch may return NaN for it in other versions)
    assert torch.allclose(got[valid], want[valid], rtol=0, atol=1e-12)
    dctx = torch.randn(B * L, E, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    ctx.backward(dctx)
    mine = R.causal_attention_bwd(qkv.detach(), mask, dctx, B, L, H)
    assert (mine - qkv.grad).abs().max() <= 1e-12 * max(1.0, qkv.grad.abs().max().item())
    # nothing flows to a key behind a query's diagonal or to a masked key: the K and V gradients of padded tokens are exactly zero
    d = qkv.grad.reshape(B, L, 3, E)
    pad = (mask == 0)
    assert pad.any() and d[:, :, 1][pad].abs().max() == 0 and d[:, :, 2][pad].abs().max() == 0


class _TorchBlock(nn.Module):
    def __init__(self, w, heads):
        super().__init__()
        self.ln_1, self.ln_2 = nn.LayerNorm(w, eps=1e-5), nn.LayerNorm(w, eps=1e-5)
        self.attn = nn.MultiheadAttention(w, heads, batch_first=True)
        self.mlp = nn.Sequential()
        self.mlp.add_module("c_fc", nn.Linear(w, 4 * w))
        self.mlp.add_module("gelu", nn.GELU())
        self.mlp.add_module("c_proj", nn.Linear(4 * w, w))


class _TorchTower(nn.Module):
    """The tower from torch's own modules, with open_clip's parameter names."""

    def __init__(self, vocab, ctx, w, heads, layers, embed):
        super().__init__()
        self.token_embedding = nn.Embedding(vocab, w)
        self.positional_embedding = nn.Parameter(torch.randn(ctx, w) * 0.01)
        self.transformer = nn.Module()
        self.transformer.resblocks = nn.ModuleList([_TorchBlock(w, heads) for _ in range(layers)])
        self.ln_final = nn.LayerNorm(w, eps=1e-5)
        self.text_projection = nn.Parameter(torch.randn(w, embed) * w ** -0.5)

    def forward(self, ids, mask):
        B, L = ids.shape
        x = self.token_embedding(ids) + self.positional_embedding[:L]
        causal = torch.ones(L, L, dtype=torch.bool).triu(1)
        for blk in self.transformer.resblocks:
            y = blk.ln_1(x)
            x = x + blk.attn(y, y, y, attn_mask=causal, key_padding_mask=mask == 0, need_weights=False)[0]
            x = x + blk.mlp(blk.ln_2(x))
        return self.ln_final(x[torch.arange(B), mask.sum(1) - 1]) @ self.text_projection


def test_tower_reference_is_the_torch_composition():
    """Features and every parameter's gradient (autograd on both sides) at float64 round-off, on a 2-layer tower 128 wide with ragged captions."""
    torch.manual_seed(3)
    vocab, ctx, w, heads, layers, embed = 50, 12, 128, 2, 2, 64
    net = _TorchTower(vocab, ctx, w, heads, layers, embed).double()
    with torch.no_grad():
        for n, p in net.named_parameters():
            if n.endswith("bias"):
                p.normal_(std=0.05)
    B, L = 4, 10
    lens = torch.tensor([10, 1, 6, 3])
    mask = (torch.arange(L)[None, :] < lens[:, None]).long()
    ids = torch.randint(1, vocab, (B, L)) * mask
    dfeat = torch.randn(B, embed, dtype=torch.float64)
    want = net(ids, mask)
    want.backward(dfeat)
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    feat, grads = R.features_and_grads(sd, ids, mask, layers, heads, dfeat)
    assert (feat - want).abs().max() <= 1e-12 * want.abs().max()
    named = dict(net.named_parameters())
    assert sorted(named) == sorted(grads)
    for k, p in named.items():
        assert (grads[k] - p.grad).abs().max() <= 1e-11 * max(p.grad.abs().max().item(), 1e-3), k
    assert grads["token_embedding.weight"][0].abs().max() == 0          # the pad id's row: nothing downstream of a pad reaches a pooled token


# ------------------------------------------------------------------------------------------------ the module tree
def test_state_dict_has_open_clip_names_and_shapes():
    from clip_lite_amd.cliptext import ClipTextModel
    net = ClipTextModel(num_hidden_layers=2)
    assert net.kind == "clip" and net.out_dim == 512 and net.context_length == 77 and (net.hidden, net.heads, net.inner) == (512, 8, 2048)
    want = {"token_embedding.weight": (30522, 512), "positional_embedding": (77, 512), "ln_final.weight": (512,), "ln_final.bias": (512,),
            "text_projection": (512, 512)}
    for i in range(2):
        b = f"transformer.resblocks.{i}."
        want.update({b + "ln_1.weight": (512,), b + "ln_1.bias": (512,), b + "attn.in_proj_weight": (1536, 512), b + "attn.in_proj_bias": (1536,),
                     b + "attn.out_proj.weight": (512, 512), b + "attn.out_proj.bias": (512,), b + "ln_2.weight": (512,), b + "ln_2.bias": (512,),
                     b + "mlp.c_fc.weight": (2048, 512), b + "mlp.c_fc.bias": (2048,), b + "mlp.c_proj.weight": (512, 2048), b + "mlp.c_proj.bias": (512,)})
    assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == want
    assert [k for k, _ in net.named_parameters()] == list(net.state_dict())
    assert net.contiguous_groups("text_encoder.strans.") == []
    assert ClipTextModel(context_length=128, num_hidden_layers=0).positional_embedding.shape == (128, 512)
    with pytest.raises(ValueError, match="129.*128"):
        ClipTextModel(context_length=129, num_hidden_layers=0)


def test_initialisation_is_clips():
    """std of every weight within 5 % of CLIP's (the tensors have 4e4 to 1.5e7 entries: the sample std is within a percent), zeros and ones elsewhere"""
    from clip_lite_amd.cliptext import ClipTextModel
    torch.manual_seed(0)
    layers, w = 12, 512
    net = ClipTextModel(num_hidden_layers=layers)
    near = lambda t, std: abs(t.std().item() / std - 1) < 0.05 and abs(t.mean().item()) < 0.05 * std
    assert near(net.token_embedding.weight, 0.02) and near(net.positional_embedding, 0.01) and near(net.text_projection, w ** -0.5)
    proj = w ** -0.5 * (2 * layers) ** -0.5
    for blk in (net.transformer.resblocks[0], net.transformer.resblocks[layers - 1]):
        assert near(blk.attn.in_proj_weight, w ** -0.5) and near(blk.attn.out_proj.weight, proj)
        assert near(blk.mlp.c_fc.weight, (2 * w) ** -0.5) and near(blk.mlp.c_proj.weight, proj)
        assert blk.attn.in_proj_bias.abs().max() == 0 and blk.attn.out_proj.bias.abs().max() == 0
        assert blk.mlp.c_fc.bias.abs().max() == 0 and blk.mlp.c_proj.bias.abs().max() == 0
        for ln in (blk.ln_1, blk.ln_2):
            assert ln.eps == 1e-5 and (ln.weight == 1).all() and (ln.bias == 0).all()
    assert net.ln_final.eps == 1e-5 and math.isclose(proj, 512 ** -0.5 / math.sqrt(24))


# ------------------------------------------------------------------------------------------------ wiring
def test_name_dispatch(capsys):
    from clip_lite_amd.bert import BertModel
    from clip_lite_amd.cliptext import ClipTextModel
    from clip_lite_amd.encoder import TextEncoder
    from clip_lite_amd.mpnet import MPNetModel
    te = TextEncoder(model_name="clip_text_b", num_hidden_layers=1, txt_enc_dim=512, transform_embedding=True)
    assert type(te.strans) is ClipTextModel and len(te.strans.transformer.resblocks) == 1 and te.strans.context_length == 77
    assert te.fc1.in_features == te.strans.out_dim == 512
    assert TextEncoder(model_name="clip_text_b", num_hidden_layers=0, txt_enc_dim=512, context_length=40).strans.context_length == 40
    assert type(TextEncoder(model_name="bert-base-uncased", num_hidden_layers=0).strans) is BertModel
    mp = TextEncoder(model_name="sentence-transformers/paraphrase-mpnet-base-v2", num_hidden_layers=0, transform_embedding=True)
    assert type(mp.strans) is MPNetModel and mp.fc1.in_features == 768
    with pytest.raises(ValueError, match="clip_text_l"):
        TextEncoder(model_name="clip_text_l", txt_enc_dim=512)
    with pytest.raises(ValueError, match=r"768.*512"):          # both numbers
        TextEncoder(model_name="clip_text_b", txt_enc_dim=768)
    with pytest.raises(RuntimeError, match="download"):
        TextEncoder(model_name="clip_text_b", txt_enc_dim=512, pretrained=True)


def test_factory_reads_the_config_keys():
    from clip_lite_amd.cliptext import ClipTextModel
    from clip_lite_amd.config import Config
    from clip_lite_amd.factories import TextualHeadFactory
    assert Config().MODEL.TEXTUAL.CONTEXT_LENGTH == 77
    cfg = os.path.join(ROOT, "configs", "smoke_random_clip.yaml")
    c = Config(cfg, ["MODEL.TEXTUAL.CONTEXT_LENGTH", 32, "MODEL.TEXTUAL.NUM_HIDDEN_LAYERS", 1])
    te = TextualHeadFactory.from_config(c)
    assert type(te.strans) is ClipTextModel and te.strans.context_length == 32 and len(te.strans.transformer.resblocks) == 1
    assert c.MODEL.LOSS.NAME == "infonce" and c.OPTIM.OPTIMIZER_NAME == "lamb" and c.OPTIM.BATCH_SIZE % 8 == 0
    with pytest.raises(ValueError, match=r"768.*512"):
        TextualHeadFactory.from_config(Config(cfg, ["MODEL.TEXTUAL.FEATURE_SIZE", 768]))
    with pytest.raises(ValueError, match="129"):
        Config(cfg, ["MODEL.TEXTUAL.CONTEXT_LENGTH", 129])
    # the smoke config's NO_DECAY pattern exempts what it says it does, and nothing else of the tower
    import re
    names = ["text_encoder.strans." + k for k in ClipTextModel(num_hidden_layers=1).state_dict()] + ["image_encoder.img_encoder.class_token",
                                                                                                     "image_encoder.img_encoder.encoder.pos_embedding"]
    exempt = {n for n in names if re.match(c.OPTIM.NO_DECAY, n)}
    assert all(n in exempt for n in names if n.endswith("bias") or "ln_" in n or n.endswith(("positional_embedding", "class_token", "pos_embedding")))
    assert not any(n in exempt for n in names if n.endswith(("in_proj_weight", "out_proj.weight", "c_fc.weight", "c_proj.weight", "text_projection",
                                                              "token_embedding.weight")))


def test_text_framing():
    from clip_lite_amd.data import hash_tokenize, text_framing
    assert text_framing("clip_text_b") == "bert" and text_framing("clip_text") == "bert"
    assert text_framing("bert-base-uncased") == "bert" and text_framing(None) == "bert"
    assert text_framing("sentence-transformers/paraphrase-mpnet-base-v2") == "mpnet"
    ids = hash_tokenize("A dog runs.", 16, framing=text_framing("clip_text_b"))
    assert ids[0] == 101 and ids[-1] == 102 and 0 not in ids          # [CLS] ... [SEP]: the last attended token is [SEP]; the pad id occurs nowhere


def _stub_rt(**kw):
    return types.SimpleNamespace(fp8_text=False, lowp=True, **kw)


def test_forward_refusals_name_both_numbers():
    from clip_lite_amd.cliptext import ClipTextModel, cliptext_forward
    net = ClipTextModel(context_length=24, num_hidden_layers=0)
    ids = torch.zeros(2, 25, dtype=torch.long)
    with pytest.raises(RuntimeError, match=r"25.*24"):
        cliptext_forward(_stub_rt(), net, ids, ids)
    rt = _stub_rt()
    rt.fp8_text = True
    with pytest.raises(RuntimeError, match="fp8"):
        cliptext_forward(rt, net, ids[:, :8], ids[:, :8])


def test_bias_eval_length_limit_follows_the_context_length():
    from clip_lite_amd.config import Config
    from clip_lite_amd.downstream import _check_bias_eval_model
    c = Config(os.path.join(ROOT, "configs", "smoke_random_clip.yaml"), ["MODEL.TEXTUAL.CONTEXT_LENGTH", 40, "MODEL.LOSS.TYPE", "dot"])
    _check_bias_eval_model(types.SimpleNamespace(max_length=40), c)
    with pytest.raises(SystemExit, match="41.*40"):
        _check_bias_eval_model(types.SimpleNamespace(max_length=41), c)
