"""CPU-side tests of GPU augmentation's host half (clip_lite_amd/augment.py, data.py): planner invariants, the canvas rule, the collate layout,
tests/augment_ref.py against PIL, the validation transform list against load_image, bit-identity of the batches with everything off, and the
keys the self-supervised switches add. No GPU, no kernels."""
import json
import math
import os

import numpy as np
import pytest
import torch
from PIL import Image

import augment_ref as R
from clip_lite_amd import augment as A
from clip_lite_amd import data as D

TRAIN = ("random_resized_crop", "horizontal_flip", "color_jitter", "normalize")
VAL = ("smallest_resize", "center_crop", "normalize")


def _gen(seed, idx):
    return torch.Generator().manual_seed(seed * 1000003 + idx)


def test_planner_invariants_over_200_seeds():
    h, w, S = 256, 341, 224
    flips = jitters = 0
    for idx in range(200):
        r = A.plan_transforms(h, w, TRAIN, S, _gen(0, idx))
        assert torch.equal(r, A.plan_transforms(h, w, TRAIN, S, _gen(0, idx)))           # same (seed, idx), same row
        x0, y0, cw, ch = (float(r[k]) for k in range(4))
        assert x0 >= 0 and y0 >= 0 and x0 + cw <= w and y0 + ch <= h and cw >= 1 and ch >= 1
        assert x0 == int(x0) and y0 == int(y0) and cw == int(cw) and ch == int(ch)
        # area fraction in [0.2, 1] and ratio in [0.75, 1.333], up to the rounding of the sides to whole pixels (half a pixel each)
        frac, ratio = cw * ch / (w * h), cw / ch
        assert (cw - 0.5) * (ch - 0.5) / (w * h) <= 1.0 and (cw + 0.5) * (ch + 0.5) / (w * h) >= 0.2, frac
        assert (cw + 0.5) / (ch - 0.5) >= 0.75 and (cw - 0.5) / (ch + 0.5) <= 1.333, ratio
        assert r[A.PLAN_NORMALIZE] == 1 and r[A.PLAN_VIEW_SIZE] == S
        assert sorted(int(o) for o in r[A.PLAN_ORDER:A.PLAN_ORDER + 4]) == [0, 1, 2, 3]
        if r[A.PLAN_JITTER]:
            jitters += 1
            assert all(0.6 <= float(r[k]) <= 1.4 for k in (A.PLAN_FB, A.PLAN_FC, A.PLAN_FS)) and abs(float(r[A.PLAN_FH])) <= 0.1
        flips += int(r[A.PLAN_FLIP])
    assert 70 <= flips <= 130 and 140 <= jitters <= 180          # p = 0.5 and p = 0.8 over 200 draws (4 sigma: 28 and 23)


def test_planner_fallback_and_kwargs():
    # no try fits (every ratio makes the box wider than the canvas): the centred square
    r = A.plan_transforms(100, 60, ("random_resized_crop::{'scale': (0.9, 1.0), 'ratio': (3.0, 4.0)}",), 32, _gen(0, 1))
    assert [float(v) for v in r[:4]] == [0.0, 20.0, 60.0, 60.0]
    for idx in range(50):
        r = A.plan_transforms(80, 100, ("random_resized_crop::{'scale': (0.5, 0.6), 'ratio': (1.0, 1.0)}", "horizontal_flip::{'p': 1.0}",
                                        "color_jitter::{'p': 1.0, 'brightness': 0.1, 'hue': 0.0}"), 32, _gen(3, idx))
        assert abs(float(r[2]) - float(r[3])) <= 1 and 0.45 <= float(r[2] * r[3]) / 8000 <= 0.65
        assert r[A.PLAN_FLIP] == 1 and r[A.PLAN_JITTER] == 1 and 0.9 <= float(r[A.PLAN_FB]) <= 1.1 and r[A.PLAN_FH] == 0 and r[A.PLAN_NORMALIZE] == 0
    assert A.plan_transforms(80, 100, ("horizontal_flip::{'p': 0.0}", "center_crop"), 64, _gen(0, 0))[A.PLAN_FLIP] == 0
    r = A.plan_transforms(81, 101, ("center_crop", "normalize"), 64, None)               # the integer centred box at scale 1
    assert [float(v) for v in r[:4]] == [18.0, 8.0, 64.0, 64.0] and r[A.PLAN_JITTER] == 0
    with pytest.raises(ValueError):                                                      # more than 9 taps on an axis
        A.plan_transforms(200, 300, ("global_resize",), 32, None)
    with pytest.raises(KeyError):
        A.plan_transforms(64, 64, ("no_such_transform",), 64, None)


def test_canvas_rule():
    rng = np.random.default_rng(0)
    wide = Image.fromarray(rng.integers(0, 256, (120, 400, 3), dtype=np.uint8))
    c = A.make_canvas(wide, 64)
    assert c.shape == (64, 96, 3) and c.dtype == np.uint8                                # shorter side 64, longer trimmed from 213 to 96
    full = np.asarray(wide.resize((213, 64), Image.BILINEAR))
    np.testing.assert_array_equal(c, full[:, (213 - 96) // 2:(213 - 96) // 2 + 96])
    tall = Image.fromarray(rng.integers(0, 256, (90, 70, 3), dtype=np.uint8))
    assert A.make_canvas(tall, 64).shape == (82, 64, 3)                                  # inside the 1.5 limit: untrimmed
    small = Image.fromarray(rng.integers(0, 256, (20, 30, 3), dtype=np.uint8))
    assert A.make_canvas(small, 64).shape == (64, 96, 3)                                 # upscaled
    assert A.canvas_short_side(VAL, 224, 256) == 224 and A.canvas_short_side(("smallest_resize::256", "center_crop"), 224, 300) == 256
    assert A.canvas_short_side(TRAIN, 224, 256) == 256 and A.canvas_capacity(256) == 256 * 384 * 3


def test_collate_layout_and_fixed_shapes():
    ds = D.RandomDataset(mode="train_sbert", image_size=32, image_transform=TRAIN, length=16, gpu_augment=True, source_size=40,
                         visual_self_supervised=True)
    shapes = None
    for lo in (0, 4):
        items = [ds[i] for i in range(lo, lo + 4)]
        b = ds.collate_fn(items)
        assert b["image_u8"].shape == (4, 40 * 60 * 3) and b["image_u8"].dtype == torch.uint8
        assert b["image_hw"].dtype == torch.int32 and b["image_plan"].shape == (4, A.PLAN_W) == b["aug_image_plan"].shape
        for n, it in enumerate(items):
            h, w = it["image_u8"].shape[:2]
            assert tuple(b["image_hw"][n]) == (h, w)
            assert torch.equal(b["image_u8"][n, :h * w * 3].reshape(h, w, 3), it["image_u8"]) and not b["image_u8"][n, h * w * 3:].any()
        s = {k: (v.shape, v.dtype) for k, v in b.items() if "image" in k}
        assert shapes is None or s == shapes
        shapes = s
    assert not torch.equal(b["image_plan"], b["aug_image_plan"])


def test_reference_resample_against_pil():
    """resize-only plans on noisy canvases, scales 0.35 .. 1.6: PIL rounds to uint8 after each of its two passes, so the bound is 1.0 level plus
    float slack"""
    rng = np.random.default_rng(5)
    S, worst = 24, 0.0
    for k, scale in enumerate(np.linspace(0.35, 1.6, 12)):
        canvas = rng.integers(0, 256, (60, 70, 3), dtype=np.uint8)
        c = scale * S
        x0, y0 = rng.uniform(0, 70 - c), rng.uniform(0, 60 - c * 0.9)
        row = np.zeros(16)
        row[:4] = (x0, y0, c, c * 0.9)
        got = R.resample(canvas, row, S)
        want = np.asarray(Image.fromarray(canvas).resize((S, S), Image.BILINEAR, box=(x0, y0, x0 + c, y0 + c * 0.9)), dtype=np.float64)
        worst = max(worst, np.abs(got - want).max())
    print("worst difference from PIL, levels:", worst)
    assert worst <= 1.01


def _png(tmp_path, h=300, w=420, name="img.png"):
    rng = np.random.default_rng(9)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([(xx * 255 / w), (yy * 255 / h), rng.integers(0, 256, (h, w))], -1).astype(np.uint8)
    path = os.path.join(tmp_path, name)
    Image.fromarray(img).save(path)
    return path


def test_validation_list_equals_load_image(tmp_path):
    """smallest_resize, center_crop, normalize: an integer crop at scale 1, so canvas + plan + augment_ref differ from load_image only by the f32
    rounding of the normalisation. rtol 1e-6 as the comparison of record; where (v / 255 - mean) cancels (v = 124 against 0.485: a result of
    1e-3) the f32 steps of load_image - v / 255, the f32 mean and std constants, the subtraction - leave up to 3 * 2^-24 of absolute error in front of the
    division by std >= 0.224, i.e. 8e-7, which no relative bound on the result can absorb: atol 1e-6."""
    path = _png(str(tmp_path))
    S = 224
    want = D.load_image(path, VAL, S).numpy()
    canvas = A.make_canvas(Image.open(path), A.canvas_short_side(VAL, S, 256))
    row = A.plan_transforms(canvas.shape[0], canvas.shape[1], VAL, S, None)
    got = R.view(canvas, row.numpy(), S)
    print("max abs difference", np.abs(got - want).max())
    np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-6)


def _records(tmp_path):
    p1 = _png(str(tmp_path), 90, 130, "a.png")
    recs = [{"image": p1, "caption": ["a cat on the left of a dog", "two animals"]}, {"image": p1, "caption": ["one caption", "one caption"]},
            {"image": "missing.jpg", "caption": "a single string"}]
    f = os.path.join(str(tmp_path), "recs.json")
    with open(f, "w") as fh:
        json.dump(recs, fh)
    return f


def test_everything_off_is_the_parent_batch(tmp_path):
    f = _records(tmp_path)
    ds = D.JsonCaptionDataset([f], image_size=32, image_transform=("smallest_resize::40",) + TRAIN, seed=2)
    items = [ds[i] for i in range(3)]
    assert all(list(i) == ["image_id", "image", "caption_tokens"] for i in items)
    b = ds.collate_fn(items)
    assert list(b) == ["image_id", "image", "input_ids", "attention_mask"]
    for idx in range(2):
        g = _gen(2, idx)
        want, flipped = D.load_image(ds.image_path(idx), ds.image_transform, 32, g, return_flipped=True)
        assert torch.equal(b["image"][idx], want)
        cap = ds.caption(idx)
        assert items[idx]["caption_tokens"].tolist() == D.hash_tokenize(D.swap_left_right(cap) if flipped else cap, 30)
    assert torch.equal(b["image"][2], torch.randn(3, 32, 32, generator=_gen(2, 2)))
    sb = D.RandomDataset(mode="sbert", image_size=16, length=4, seed=1)[3]
    g = _gen(1, 3)
    assert torch.equal(sb["image"], torch.randn(3, 16, 16, generator=g)) and torch.equal(sb["caption_encodings"], torch.randn(768, generator=g))


@pytest.mark.parametrize("gpu", [False, True])
def test_switches_emit_exactly_the_expected_keys(tmp_path, gpu):
    f = _records(tmp_path)
    ds = D.JsonCaptionDataset([f], image_size=32, image_transform=("smallest_resize::40",) + TRAIN, seed=2, gpu_augment=gpu,
                              visual_self_supervised=True, textual_self_supervised=True)
    items = [ds[i] for i in range(3)]
    b = ds.collate_fn(items)
    image_keys = ["image_u8", "image_hw", "image_plan", "aug_image_plan"] if gpu else ["image", "aug_image"]
    assert list(b) == ["image_id"] + image_keys + ["input_ids", "attention_mask", "aug_input_ids", "aug_attention_mask"]
    tok = lambda i, k: items[i][k].tolist()
    assert tok(0, "aug_caption_tokens") == D.hash_tokenize("two animals", 30) != tok(0, "caption_tokens")          # two distinct captions
    assert tok(1, "aug_caption_tokens") == tok(1, "caption_tokens") and tok(2, "aug_caption_tokens") == tok(2, "caption_tokens")
    if gpu:
        assert b["image_u8"].shape == (3, 40 * 60 * 3) and tuple(b["image_hw"][0]) == (40, 58) and tuple(b["image_hw"][2]) == (40, 40)
        # the flip flag still swaps left and right in the caption
        flipped = bool(items[0]["image_plan"][A.PLAN_FLIP])
        assert tok(0, "caption_tokens") == D.hash_tokenize(D.swap_left_right("a cat on the left of a dog") if flipped else "a cat on the left of a dog", 30)
    else:
        assert b["aug_image"].shape == b["image"].shape and not torch.equal(b["aug_image"], b["image"])
        g = _gen(2, 0)
        first = D.load_image(ds.image_path(0), ds.image_transform, 32, g)
        assert torch.equal(b["image"][0], first) and torch.equal(b["aug_image"][0], D.load_image(ds.image_path(0), ds.image_transform, 32, g))
    rd = D.RandomDataset(image_size=16, length=8, textual_self_supervised=True)
    assert rd[2]["aug_caption_tokens"].tolist() == D.hash_tokenize(D.CAPTIONS[3], 30)


def test_factory_passes_the_switches_and_clustered_base_carries_canvases(tmp_path):
    from clip_lite_amd.config import Config
    from clip_lite_amd.factories import PretrainingDatasetFactory
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    _C = Config(os.path.join(root, "configs", "smoke_random_gpuaug.yaml"), ["DATA.IMAGE_CROP_SIZE", 32, "DATA.GPU_AUGMENT_SOURCE_SIZE", 40])
    assert _C.DATA.GPU_AUGMENT is True and Config().DATA.GPU_AUGMENT is False and Config().DATA.GPU_AUGMENT_SOURCE_SIZE == 256
    ds = PretrainingDatasetFactory.from_config(_C, "train")
    b = ds.collate_fn([ds[0], ds[1]])
    assert {"image_u8", "image_hw", "image_plan", "aug_image_plan", "aug_input_ids", "aug_attention_mask"} <= set(b) and "image" not in b
    assert "image" in PretrainingDatasetFactory.from_config(Config(os.path.join(root, "configs", "smoke_random.yaml")), "train")[0]
    import pickle
    with open(os.path.join(str(tmp_path), "img_id_cluster_map_train_2.pkl"), "wb") as fh:
        pickle.dump({i: i % 2 for i in range(8)}, fh)
    base = D.RandomDataset(image_size=32, length=8, image_transform=TRAIN, gpu_augment=True, source_size=40)
    cd = D.ClusteredDataset(base, str(tmp_path), total_iters=10)
    b = cd.collate_fn([cd[0], cd[1]])
    assert {"neg_image_u8", "neg_image_hw", "neg_image_plan", "neg_input_ids", "neg_attention_mask"} <= set(b) and "neg_image" not in b


def test_colour_ops_against_pil_imageenhance_recorded_not_gated():
    """The measured distance between augment_ref's brightness / contrast / saturation and PIL's ImageEnhance on a noisy image (PIL rounds to
    uint8, blends with integer arithmetic and rounds the contrast mean to an integer): printed and written into DESIGN.md section 3.3f, not a bound."""
    from PIL import ImageEnhance
    rng = np.random.default_rng(2)
    img = rng.integers(0, 256, (48, 48, 3), dtype=np.uint8)
    pil = Image.fromarray(img)
    worst = {}
    for name, op, enh in (("brightness", 0, ImageEnhance.Brightness), ("contrast", 1, ImageEnhance.Contrast), ("saturation", 2, ImageEnhance.Color)):
        for f in (0.6, 0.85, 1.2, 1.4):
            row = np.zeros(16)
            row[[R.FB, R.FC, R.FS]] = 1.0
            row[R.FB + op] = f
            row[R.ORD:R.ORD + 4] = [op] + [k for k in range(4) if k != op]
            got = R.jitter(img.astype(np.float64), row)[0]
            want = np.asarray(enh(pil).enhance(f), dtype=np.float64)
            worst[name] = max(worst.get(name, 0.0), float(np.abs(got - want).max()))
    print("levels of 255 between augment_ref and ImageEnhance:", worst)
    assert all(np.isfinite(v) for v in worst.values())
