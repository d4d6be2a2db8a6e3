"""CPU-side tests of the ViT image tower's host layer (clip-lite_amd/vit.py): tests/vit_ref.py pinned to torch's own modules in float64,
torchvision's key list and shapes, the initialisation statistics, and the refusals. torchvision is not installed here, so the encoder block is
composed from nn.LayerNorm(eps=1e-6), nn.MultiheadAttention(batch_first=True), nn.Linear, nn.GELU and nn.Conv2d(3, C, p, stride=p), which is
what torchvision.models.vision_transformer builds. Runs without a GPU."""
import math
import os

import pytest
import torch
import torch.nn as nn

import vit_ref as R
from detfill import det_fill, det_tensor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _TorchBlock(nn.Module):
    """torchvision EncoderBlock"""

    def __init__(self, C, heads, inner):
        super().__init__()
        self.ln_1 = nn.LayerNorm(C, eps=1e-6)
        self.self_attention = nn.MultiheadAttention(C, heads, dropout=0.0, batch_first=True)
        self.ln_2 = nn.LayerNorm(C, eps=1e-6)
        self.mlp = nn.Sequential(nn.Linear(C, inner), nn.GELU(), nn.Dropout(0.0), nn.Linear(inner, C), nn.Dropout(0.0))

    def forward(self, x):
        y = self.ln_1(x)
        y, _ = self.self_attention(y, y, y, need_weights=False)
        x = x + y
        return x + self.mlp(self.ln_2(x))


class _TorchViT(nn.Module):
    """torchvision VisionTransformer with heads = Identity, by its own key names"""

    def __init__(self, p, L, layers, C, heads, inner):
        super().__init__()
        self.class_token = nn.Parameter(torch.zeros(1, 1, C))
        self.conv_proj = nn.Conv2d(3, C, p, stride=p)
        self.encoder = nn.Module()
        self.encoder.pos_embedding = nn.Parameter(torch.zeros(1, L, C))
        self.encoder.layers = nn.Sequential()
        for i in range(layers):
            self.encoder.layers.add_module(f"encoder_layer_{i}", _TorchBlock(C, heads, inner))
        self.encoder.ln = nn.LayerNorm(C, eps=1e-6)

    def forward(self, x):
        B = x.shape[0]
        x = self.conv_proj(x).flatten(2).permute(0, 2, 1)          # torchvision _process_input: [B][C][h][w] -> [B][h w][C]
        x = torch.cat([self.class_token.expand(B, -1, -1), x], dim=1)
        x = self.encoder.ln(self.encoder.layers(x + self.encoder.pos_embedding))
        return x[:, 0]


@pytest.mark.parametrize("name,H,W,layers,heads", [("vit_b_32", 64, 96, 2, 2), ("vit_b_16", 48, 32, 1, 1)])
def test_reference_equals_torch_modules_in_float64(name, H, W, layers, heads):
    from clip_lite_amd.vit import VisionTransformer
    C, inner, B = 64 * heads, 96, 3
    net = det_fill(VisionTransformer(name, image_size=(H, W), num_layers=layers, hidden=C, heads=heads, mlp_dim=inner))
    sd = net.state_dict()
    tv = _TorchViT(net.patch, net.seq_length, layers, C, heads, inner).double()
    assert list(tv.state_dict()) == list(sd)
    tv.load_state_dict({k: v.double() for k, v in sd.items()})          # strict: the project's keys and shapes are torch's own
    image = det_tensor("image", (B, 3, H, W), "normal").double()
    dfeat = det_tensor("dfeat", (B, C), "normal").double()
    want = tv(image)
    (want * dfeat).sum().backward()
    feat, grads = R.features_and_grads(sd, image, layers, heads, dfeat)
    rel = lambda a, b: ((a - b).abs().max() / b.abs().max().clamp(min=1e-30)).item()
    assert rel(feat, want.detach()) <= 1e-10
    named = dict(tv.named_parameters())
    assert set(named) == set(grads)
    for k, p in named.items():
        assert p.grad is not None and p.grad.abs().max() > 0, k
        assert rel(grads[k], p.grad) <= 1e-10, k


def test_patchify_reference_is_unfold():
    x = det_tensor("x", (2, 3, 64, 96), "normal")
    for p in (32, 16):
        want = torch.nn.functional.unfold(x, p, stride=p).permute(0, 2, 1)          # unfold's column order is (c, i, j)
        assert torch.equal(R.patchify(x, p), want)


def test_key_list_and_shapes_of_vit_b_32_at_224():
    from clip_lite_amd.vit import VisionTransformer, token_count
    net = VisionTransformer("vit_b_32", image_size=224)
    assert net.out_dim == 768 and net.seq_length == 50 == token_count("vit_b_32", 224, 224)
    want = R.param_shapes(12, 50, 32)
    sd = net.state_dict()
    assert list(sd) == list(want)
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    assert not any(k.startswith("heads") for k in sd)
    assert sum(v.numel() for v in sd.values()) == 87455232          # torchvision vit_b_32: 88 224 232 parameters less heads.head's 769 000
    assert token_count("vit_b_16", 160) == 101
    assert VisionTransformer("vit_b_16", image_size=160, num_layers=1).conv_proj.weight.shape == (768, 3, 16, 16)


def test_initialisation_is_torchvisions():
    from clip_lite_amd.vit import VisionTransformer
    torch.manual_seed(0)
    net = VisionTransformer("vit_b_32", image_size=224, num_layers=2)
    l0 = net.encoder.layers.encoder_layer_0
    assert net.class_token.abs().max() == 0 and l0.self_attention.in_proj_bias.abs().max() == 0
    assert net.conv_proj.bias.abs().max() == 0 and l0.self_attention.out_proj.bias.abs().max() == 0
    assert abs(net.encoder.pos_embedding.std().item() / 0.02 - 1) < 0.05
    assert abs(net.conv_proj.weight.std().item() / math.sqrt(1 / 3072) - 1) < 0.05
    m0, m3 = l0.mlp.parts()
    bound = math.sqrt(6.0 / (768 + 3072))          # Xavier uniform: std = bound / sqrt(3)
    for w in (m0.weight, m3.weight):
        assert w.abs().max() <= bound and abs(w.std().item() / (bound / math.sqrt(3)) - 1) < 0.05
    assert 0 < m0.bias.abs().max() < 1e-5
    b_in = math.sqrt(6.0 / (768 + 2304))
    assert l0.self_attention.in_proj_weight.abs().max() <= b_in
    assert abs(l0.self_attention.in_proj_weight.std().item() / (b_in / math.sqrt(3)) - 1) < 0.05
    assert l0.self_attention.out_proj.weight.abs().max() <= 1 / math.sqrt(768)          # nn.Linear default: U(-1/sqrt(fan_in), 1/sqrt(fan_in))
    assert l0.ln_1.eps == l0.ln_2.eps == net.encoder.ln.eps == 1e-6


def test_refusals():
    from clip_lite_amd.classify import ImageClassifier
    from clip_lite_amd.config import Config
    from clip_lite_amd.encoder import ImageEncoder
    from clip_lite_amd.factories import VisualBackboneFactory
    from clip_lite_amd.vit import VisionTransformer, token_count
    with pytest.raises(ValueError, match=r"197.*128"):
        token_count("vit_b_16", 224, 224)
    with pytest.raises(ValueError, match=r"197.*128"):
        ImageEncoder("vit_b_16", image_size=224)
    with pytest.raises(ValueError, match="multiple of 32"):
        token_count("vit_b_32", 80, 80)
    with pytest.raises(ValueError, match="multiple of 32"):
        ImageEncoder("vit_b_32", image_size=80)
    with pytest.raises(ValueError, match="unsupported visual backbone"):
        ImageEncoder("vit_l_16")
    with pytest.raises(ValueError, match="dropout"):
        VisionTransformer("vit_b_32", dropout=0.1)
    with pytest.raises(ValueError, match="dropout"):
        VisionTransformer("vit_b_32", attention_dropout=0.1)
    with pytest.raises(RuntimeError, match="pretrained"):
        ImageEncoder("vit_b_32", pretrained=True)
    enc = ImageEncoder("vit_b_32", image_size=64)
    assert enc.out_dim == 768 and enc.img_encoder.seq_length == 5
    with pytest.raises(NotImplementedError, match="ViT"):
        enc.detectron2_backbone_state_dict()
    with pytest.raises(ValueError, match="logreg_clf.py"):
        ImageClassifier("vit_b_32", 10)
    cfg = os.path.join(ROOT, "configs", "smoke_random_vit.yaml")
    with pytest.raises(ValueError, match=r"512.*768"):
        VisualBackboneFactory.from_config(Config(cfg, ["MODEL.VISUAL.FEATURE_SIZE", 512]))
    ok = VisualBackboneFactory.from_config(Config(cfg, []))
    assert ok.img_encoder.image_hw == (64, 64) and ok.img_encoder.seq_length == 5
    with pytest.raises(RuntimeError, match="no CPU path"):          # a module that is not on a device runtime has no forward
        ok(torch.zeros(1, 3, 64, 64))


def test_smoke_config_exempts_class_token_and_position_embedding_from_decay():
    import re
    from clip_lite_amd.config import Config
    c = Config(os.path.join(ROOT, "configs", "smoke_random_vit.yaml"), [])
    pat = c.OPTIM.NO_DECAY
    assert re.match(pat, "image_encoder.img_encoder.class_token") and re.match(pat, "image_encoder.img_encoder.encoder.pos_embedding")
    assert not re.match(pat, "image_encoder.img_encoder.conv_proj.weight")
    default = Config(None, []).OPTIM.NO_DECAY
    for n in ("text_encoder.strans.embeddings.LayerNorm.weight", "image_encoder.img_encoder.encoder.ln.bias", "loss.global_d.l0.weight"):
        assert bool(re.match(pat, n)) == bool(re.match(default, n)), n
    assert c.MODEL.VISUAL.FEATURE_SIZE == 768 and c.DATA.IMAGE_CROP_SIZE == 64 and c.OPTIM.BATCH_SIZE == 8
