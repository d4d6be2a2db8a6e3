"""Patch dropout of the ViT tower without a device: the reference of tests/vit_keep_ref.py pinned to tests/vit_ref.py and to its own definition,
a fixed-seed check that the selection is uniform over the patches, and the constructor / config surface (kept_patches, the refusals, eval and
frozen encoders ignoring the ratio)."""
import os

import numpy as np
import pytest
import torch

import vit_keep_ref as K
import vit_ref as R
from detfill import det_tensor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _params(layers, L, patch, hidden, inner):
    return {k: det_tensor("keep-host-" + k, s, "normal").double() * 0.1 for k, s in R.param_shapes(layers, L, patch, hidden, inner).items()}


# ------------------------------------------------------------------------------------------------ the reference
def test_keeping_every_patch_is_the_plain_tower():
    H, W, p, C = 32, 48, 16, 64
    P = (H // p) * (W // p)
    sd = _params(2, P + 1, p, C, 128)
    image = det_tensor("keep-host-image", (3, 3, H, W), "normal").double()
    idx, inv = K.keep_indices(5, 1, 3, P, P)
    assert np.array_equal(idx, np.tile(np.arange(P, dtype=np.int32), (3, 1))) and np.array_equal(inv, idx)
    assert torch.equal(K.tower(sd, image, 2, idx, heads=1), R.tower(sd, image, 2, heads=1))


def test_order_of_the_kept_tokens_does_not_change_the_features():
    """no mask, no causal structure, the position embedding travels with its token: the class token's output is a symmetric function of the others"""
    H, W, p, C = 32, 48, 16, 64
    P = (H // p) * (W // p)
    sd = _params(2, P + 1, p, C, 128)
    image = det_tensor("keep-host-image", (3, 3, H, W), "normal").double()
    idx, _ = K.keep_indices(5, 1, 3, P, 4)
    want = K.tower(sd, image, 2, idx, heads=1)
    perm = np.stack([row[np.random.default_rng(b).permutation(4)] for b, row in enumerate(idx)])
    assert not np.array_equal(perm, idx)
    assert (K.tower(sd, image, 2, perm, heads=1) - want).abs().max() <= 1e-12
    # ... and another kept set does change them
    other = (idx + 1) % P
    assert (K.tower(sd, image, 2, np.sort(other, axis=1), heads=1) - want).abs().max() > 1e-6


@pytest.mark.parametrize("B,P,Kk", [(1, 1, 1), (3, 4, 1), (5, 49, 24), (2, 127, 95), (4, 100, 100)])
def test_indices_are_ascending_and_inv_is_their_inverse(B, P, Kk):
    idx, inv = K.keep_indices(11, 3, B, P, Kk)
    assert idx.shape == (B, Kk) and inv.shape == (B, P) and idx.dtype == inv.dtype == np.int32
    key = K.keys(11, 3, B, P)
    for b in range(B):
        assert (np.diff(idx[b]) > 0).all() and idx[b].min() >= 0 and idx[b].max() < P
        assert np.array_equal(inv[b, idx[b]], np.arange(Kk)) and (inv[b] >= 0).sum() == Kk and inv[b].min() >= -1
        # the definition, literally: rank by (key, index)
        rank = np.array([sum(1 for u in range(P) if key[b, u] < key[b, t] or (key[b, u] == key[b, t] and u < t)) for t in range(P)])
        assert np.array_equal(np.flatnonzero(rank < Kk), idx[b])


def test_ties_go_to_the_lower_index():
    key = np.array([[0.5, 0.25, 0.5, 0.25, 0.75, 0.25]], np.float32)
    idx, inv = K.select(key, 2)
    assert idx.tolist() == [[1, 3]] and inv.tolist() == [[-1, 0, -1, 1, -1, -1]]
    idx, _ = K.select(key, 4)
    assert idx.tolist() == [[0, 1, 3, 5]]


def test_keys_are_the_uniform4_stream_at_a_sample_pitch_of_whole_calls():
    import dropout_ref as D
    B, P = 3, 49          # Ppad = 52
    key = K.keys(9, 2, B, P)
    flat = D.uniform8(9, 2, B * 52)
    assert np.array_equal(key[1], flat[52:52 + 49]) and np.array_equal(key[2, :4], flat[104:108])
    assert (key >= 0).all() and (key < 1).all() and np.array_equal(key * 16777216.0, np.round(key * 16777216.0))          # a 24-bit grid


STAT_SEED = 0


def test_every_patch_is_kept_equally_often():
    """(B, P, Kk) = (4096, 49, 24) with a fixed seed: each patch is kept by B Kk / P = 2006 samples on average, a binomial count with standard
    deviation sqrt(B (Kk / P) (1 - Kk / P)) = 32; every patch within five of them (2006 +- 160). A condition on the reference, not a measurement."""
    B, P, Kk = 4096, 49, 24
    idx, _ = K.keep_indices(STAT_SEED, 1, B, P, Kk)
    counts = np.bincount(idx.reshape(-1), minlength=P)
    assert counts.sum() == B * Kk
    assert (np.abs(counts - B * Kk / P) <= 160).all(), counts


# ------------------------------------------------------------------------------------------------ constructor and config
def test_kept_patches():
    from clip_lite_amd.vit import kept_patches
    assert [kept_patches(49, r) for r in (0.0, 0.25, 0.5, 0.75, 0.99)] == [49, 36, 24, 12, 1]
    assert kept_patches(25, 0.5) == 12 and kept_patches(4, 0.5) == 2 and kept_patches(1, 0.5) == 1 and kept_patches(100, 0.25) == 75
    for P in (1, 4, 16, 49, 100, 127):
        for r in (0.0, 0.1, 0.25, 0.5, 0.75, 0.9):
            assert kept_patches(P, r) == K.kept(P, r)


@pytest.mark.parametrize("r", [1.0, -0.1, 1.5])
def test_ratio_outside_the_unit_interval_is_refused(r):
    from clip_lite_amd.encoder import ImageEncoder
    from clip_lite_amd.vit import VisionTransformer, kept_patches
    with pytest.raises(ValueError, match=str(r)):
        VisionTransformer("vit_b_32", image_size=64, num_layers=1, patch_dropout=r)
    with pytest.raises(ValueError, match=str(r)):
        ImageEncoder("vit_b_32", image_size=64, num_layers=1, patch_dropout=r)
    with pytest.raises(ValueError, match=str(r)):
        kept_patches(49, r)


def test_resnet_with_a_ratio_is_refused_as_a_vit_option():
    from clip_lite_amd.config import Config
    from clip_lite_amd.encoder import ImageEncoder
    from clip_lite_amd.factories import VisualBackboneFactory
    with pytest.raises(ValueError, match="ViT option"):
        ImageEncoder("resnet18", patch_dropout=0.5)
    c = Config(os.path.join(ROOT, "configs", "smoke_random.yaml"), ["MODEL.VISUAL.PATCH_DROPOUT", 0.5])
    assert not c.MODEL.VISUAL.NETWORK_NAME.startswith("vit_")
    with pytest.raises(ValueError, match="ViT option"):
        VisualBackboneFactory.from_config(c)
    assert ImageEncoder("resnet18", patch_dropout=0.0).is_vit is False


def test_config_key_reaches_the_tower():
    from clip_lite_amd.config import Config
    from clip_lite_amd.factories import VisualBackboneFactory
    vit = os.path.join(ROOT, "configs", "smoke_random_vit.yaml")
    assert Config(vit, []).MODEL.VISUAL.PATCH_DROPOUT == 0.0
    assert VisualBackboneFactory.from_config(Config(vit, [])).img_encoder.patch_dropout == 0.0
    assert VisualBackboneFactory.from_config(Config(vit, ["MODEL.VISUAL.PATCH_DROPOUT", 0.25])).img_encoder.patch_dropout == 0.25
    c = Config(os.path.join(ROOT, "configs", "smoke_random_flip.yaml"), [])
    enc = VisualBackboneFactory.from_config(c)
    assert c.MODEL.VISUAL.PATCH_DROPOUT == 0.5 and enc.img_encoder.patch_dropout == 0.5
    assert enc.img_encoder.seq_length - 1 >= 16          # at least 16 patches, so that half of them is a real subset


def test_eval_and_frozen_encoders_run_the_tower_in_eval_mode(monkeypatch):
    """the one switch the tower sees is vit_forward's `training`: False in eval mode and for a frozen encoder whatever train() says"""
    from clip_lite_amd import encoder
    seen = []

    def fake_forward(rt, net, image, training=True):
        seen.append(training)
        return torch.zeros(image.shape[0], net.hidden), None

    monkeypatch.setattr(encoder, "vit_forward", fake_forward)
    monkeypatch.setattr(encoder, "_runtime_of", lambda m: None)
    image = torch.zeros(2, 3, 64, 64)
    with torch.no_grad():
        enc = encoder.ImageEncoder("vit_b_32", image_size=64, num_layers=1, patch_dropout=0.5)
        enc.train()(image)
        enc.eval()(image)
        frozen = encoder.ImageEncoder("vit_b_32", image_size=64, num_layers=1, patch_dropout=0.5, frozen=True)
        frozen.train()(image)
    assert seen == [True, False, False]
