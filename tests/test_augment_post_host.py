"""CPU-side tests of the host half of `random_gray` and `blur` (clip_lite_amd/augment.py, data.py): load_image's two branches, the distribution of
the blur's kernel size, the agreement of load_image and the planner on every decision and on the generator's state, the refusals, the keys the
datasets add, and the measured distance between the CPU recipe and tests/augment_post_ref.py. No GPU, no kernels."""
import os
import pickle

import numpy as np
import pytest
import torch
from PIL import Image

import augment_post_ref as PR
from clip_lite_amd import augment as A
from clip_lite_amd import data as D

SIMCLR = ("random_resized_crop", "horizontal_flip", "color_jitter8", "random_gray", "blur", "normalize")
PLAIN = ("random_resized_crop", "horizontal_flip", "color_jitter", "normalize")


def _gen(seed, idx=0):
    return torch.Generator().manual_seed(seed * 1000003 + idx)


def _save(tmp_path, arr, name="img.png"):
    path = os.path.join(str(tmp_path), name)
    Image.fromarray(arr).save(path)
    return path


def _noise(h=48, w=48, seed=3):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def test_both_names_were_unknown_transforms_and_now_load(tmp_path):
    path = _save(tmp_path, _noise())
    for spec in ("random_gray", "blur"):
        assert D.load_image(path, (spec,), 48, _gen(0)).shape == (3, 48, 48)
        assert A.needs_post((spec,)) and A.needs_post(("center_crop", spec + "::{'p': 1.0}"))
    assert not A.needs_post(PLAIN)


def test_load_image_gray_is_pils_l_image(tmp_path):
    arr = _noise()
    path = _save(tmp_path, arr)
    d = {}
    x = D.load_image(path, ("random_gray::{'p': 1.0}",), 48, _gen(1), decisions=d)
    assert d == {"flipped": False, "gray": True, "blur": 0}
    assert torch.equal(x[0], x[1]) and torch.equal(x[1], x[2])
    want = np.asarray(Image.fromarray(arr).convert("L"), dtype=np.float32) / 255.0
    np.testing.assert_array_equal(x[0].numpy(), want)
    d = {}
    y = D.load_image(path, ("random_gray::{'p': 0.0}",), 48, _gen(1), decisions=d)
    assert d["gray"] is False and np.array_equal(np.rint(y.numpy() * 255).astype(np.uint8).transpose(1, 2, 0), arr)


def test_load_image_blur_of_one_bright_pixel(tmp_path):
    arr = np.zeros((9, 11, 3), np.uint8)
    arr[4, 6] = (255, 200, 100)
    path = _save(tmp_path, arr)
    d = {}
    x = D.load_image(path, ("blur::{'p': 1.0, 'blur_limit': (3, 3)}",), 9, _gen(0), decisions=d)
    assert d["blur"] == 3
    got = np.rint(x.numpy() * 255).astype(np.int64)
    k = np.outer((0.25, 0.5, 0.25), (0.25, 0.5, 0.25))
    for c, peak in enumerate((255, 200, 100)):
        want = np.zeros((9, 11), np.int64)
        want[3:6, 5:8] = np.rint(k * peak)
        np.testing.assert_array_equal(got[c], want)


def test_blur_border_is_reflect_101(tmp_path):
    """a bright pixel one step inside the left and the bottom border: coordinate -1 mirrors 1 (and S mirrors S - 2), so the border pixel
    receives the 0.25 tap twice - 0.5 of the peak along that axis, where a replicated border would give 0.25"""
    arr = np.zeros((8, 8, 3), np.uint8)
    arr[4, 1] = arr[6, 5] = 200
    path = _save(tmp_path, arr)
    x = D.load_image(path, ("blur::{'p': 1.0, 'blur_limit': (3, 3)}",), 8, _gen(0))
    got = np.rint(x[0].numpy() * 255)
    assert got[4, 0] == 50 and got[4, 1] == 50 and got[4, 2] == 25 and got[3, 0] == 25          # 200 (0.5 vertical) (0.25 + 0.25), ...
    assert got[7, 5] == 50 and got[6, 5] == 50 and got[5, 5] == 25 and got[7, 4] == 25


def test_kernel_size_shares_over_2000_seeds():
    """default blur_limit (3, 7): k = 3 + int(5 u), even going up: 3, 5, 7 with 1/5, 2/5, 2/5. Bounds: 4.5 sigma of a binomial over 2000 draws -
    0.2 +- 0.04, 0.4 +- 0.05"""
    n = {3: 0, 5: 0, 7: 0}
    for seed in range(2000):
        g = _gen(seed)
        k = A.draw_blur(lambda: float(torch.rand((), generator=g)), {"p": 1.0})
        n[k] += 1
    share = {k: v / 2000 for k, v in n.items()}
    print("kernel size shares", share)
    assert 0.16 <= share[3] <= 0.24
    assert 0.35 <= share[5] <= 0.45 and 0.35 <= share[7] <= 0.45
    fired = sum(A.draw_blur(lambda g=_gen(s): float(torch.rand((), generator=g)), {}) != 0 for s in range(2000)) / 2000
    grayed = sum(A.draw_gray(lambda g=_gen(s): float(torch.rand((), generator=g)), {}) for s in range(2000)) / 2000
    print("blur fired", fired, "gray fired", grayed)
    assert 0.45 <= fired <= 0.55 and 0.16 <= grayed <= 0.24          # p = 0.5 and p = 0.2 by default, the same 4.5 sigma


def test_load_image_and_planner_agree_for_32_seeds(tmp_path):
    path = _save(tmp_path, _noise(40, 56))
    S = 32
    seen = set()
    for seed in range(32):
        g1, g2, d = _gen(seed), _gen(seed), {}
        D.load_image(path, SIMCLR, S, g1, decisions=d)
        row, post = A.plan_transforms(40, 56, SIMCLR, S, g2, return_post=True)
        assert post.shape == (A.POST_W,) and post.dtype == torch.float32
        assert bool(row[A.PLAN_FLIP]) == d["flipped"] and bool(post[A.POST_GRAY]) == d["gray"] and bool(post[A.POST_BLUR]) == (d["blur"] != 0)
        want = A.BLUR_WEIGHTS[d["blur"]] if d["blur"] else (0.0, 0.0, 0.0, 0.0)
        assert tuple(post[A.POST_W0:A.POST_W0 + 4].tolist()) == want and not post[A.POST_W0 + 4:].any()
        assert float(torch.rand((), generator=g1)) == float(torch.rand((), generator=g2))          # the same number of draws
        seen.add((d["gray"], d["blur"]))
    assert len({b for _, b in seen}) >= 3 and {g for g, _ in seen} == {False, True}, seen          # the 32 seeds exercise the branches


def test_refusals():
    ok = A.plan_transforms(40, 56, SIMCLR, 32, _gen(0), return_post=True)
    assert len(ok) == 2
    for bad in (("random_gray", "random_resized_crop", "normalize"), ("random_resized_crop", "blur", "color_jitter8"),
                ("random_resized_crop", "random_gray", "color_jitter"), ("blur", "center_crop")):
        with pytest.raises(ValueError, match="ahead of"):
            A.plan_transforms(40, 56, bad, 32, _gen(0), return_post=True)
    for order in (("center_crop", "blur", "random_gray", "horizontal_flip"), ("center_crop", "random_gray", "blur")):      # either order of the two
        A.plan_transforms(40, 56, order, 32, _gen(0), return_post=True)
    for name in ("random_gray", "blur"):
        with pytest.raises(ValueError, match="return_post"):
            A.plan_transforms(40, 56, ("center_crop", name), 32, _gen(0))
    for lim in ("(2, 7)", "(3, 9)", "(3, 4)", "(1, 3)", "(7, 3)", "(3.0, 7)"):
        with pytest.raises(ValueError, match="blur_limit"):
            A.plan_transforms(40, 56, ("center_crop", "blur::{'blur_limit': %s}" % lim), 32, _gen(0), return_post=True)
    for sig in ("1.5", "(0.1, 2.0)"):
        with pytest.raises(ValueError, match="sigma_limit"):
            A.plan_transforms(40, 56, ("center_crop", "blur::{'sigma_limit': %s}" % sig), 32, _gen(0), return_post=True)
    A.plan_transforms(40, 56, ("center_crop", "blur::{'sigma_limit': 0, 'blur_limit': (5, 5), 'p': 1.0}"), 32, _gen(0), return_post=True)
    with pytest.raises(ValueError):
        A.plan_transforms(3, 3, ("blur::{'p': 1.0}",), 3, _gen(0), return_post=True)          # a blurred view needs S >= 4
    good = torch.zeros(2, A.POST_W)
    good[0, A.POST_BLUR], good[0, A.POST_W0:A.POST_W0 + 4] = 1.0, torch.tensor(A.BLUR_WEIGHTS[7])
    A.check_post(good, 4)
    for col, v in ((A.POST_GRAY, 2.0), (A.POST_BLUR, 0.5), (A.POST_W0 + 1, -0.1), (A.POST_W0, float("nan")), (A.POST_W0, 0.29)):
        bad = good.clone()
        bad[0, col] = v
        with pytest.raises(ValueError):
            A.check_post(bad, 32)
    with pytest.raises(ValueError):
        A.check_post(good, 3)
    with pytest.raises(ValueError):
        A.check_post(torch.zeros(2, A.POST_W + 1), 32)


def test_datasets_emit_the_post_keys_exactly_when_the_list_names_a_transform(tmp_path):
    with open(os.path.join(str(tmp_path), "img_id_cluster_map_train_2.pkl"), "wb") as fh:
        pickle.dump({i: i % 2 for i in range(8)}, fh)
    keys = {}
    for name, tf in (("plain", PLAIN), ("simclr", SIMCLR), ("gray", PLAIN[:3] + ("random_gray",)), ("blur", PLAIN[:3] + ("blur",))):
        ds = D.RandomDataset(mode="train_sbert", image_size=32, image_transform=tf, length=8, gpu_augment=True, source_size=40,
                             visual_self_supervised=True)
        b = ds.collate_fn([ds[i] for i in range(4)])
        keys[name] = list(b)
        if name == "plain":
            assert list(b) == ["image_id", "image_u8", "image_hw", "image_plan", "aug_image_plan", "input_ids", "attention_mask"]      # today's
        else:
            assert list(b) == ["image_id", "image_u8", "image_hw", "image_plan", "aug_image_plan", "image_post", "aug_image_post", "input_ids",
                               "attention_mask"]
            assert b["image_post"].shape == (4, A.POST_W) == b["aug_image_post"].shape and b["image_post"].dtype == torch.float32
        single = D.RandomDataset(mode="train_sbert", image_size=32, image_transform=tf, length=8, gpu_augment=True, source_size=40)
        assert ("image_post" in single[0]) == (name != "plain") and "aug_image_post" not in single[0]
        cd = D.ClusteredDataset(single, str(tmp_path), total_iters=10)
        nb = cd.collate_fn([cd[0], cd[1]])
        assert ("neg_image_post" in nb) == ("image_post" in nb) == (name != "plain")
        if name != "plain":
            assert nb["neg_image_post"].shape == (2, A.POST_W)
    cpu = D.RandomDataset(mode="train_sbert", image_size=32, image_transform=SIMCLR, length=8, visual_self_supervised=True)
    assert list(cpu.collate_fn([cpu[0], cpu[1]])) == ["image_id", "image", "aug_image", "input_ids", "attention_mask"]
    # the post rows of the items are the planner's, drawn behind the plan row from the per-index generator
    ds = D.RandomDataset(mode="train_sbert", image_size=32, image_transform=SIMCLR, length=8, seed=5, gpu_augment=True, source_size=40,
                         visual_self_supervised=True)
    it = ds[3]
    g = _gen(5, 3)
    A.synthetic_canvas(40, g)
    for pre in ("", "aug_"):
        row, post = A.plan_transforms(40, 40, SIMCLR, 32, g, return_post=True)
        assert torch.equal(it[pre + "image_plan"], row) and torch.equal(it[pre + "image_post"], post)


def test_simclr_config_reaches_the_loader():
    from clip_lite_amd.config import Config
    from clip_lite_amd.factories import PretrainingDatasetFactory
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    _C = Config(os.path.join(root, "configs", "smoke_random_simclr.yaml"), ["DATA.IMAGE_CROP_SIZE", 32, "DATA.GPU_AUGMENT_SOURCE_SIZE", 40])
    assert tuple(_C.DATA.IMAGE_TRANSFORM_TRAIN) == SIMCLR
    ds = PretrainingDatasetFactory.from_config(_C, "train")
    b = ds.collate_fn([ds[0], ds[1]])
    assert {"image_post", "aug_image_post", "aug_image_plan", "aug_input_ids"} <= set(b)


def test_cpu_recipe_against_the_reference_restatement_recorded(tmp_path):
    """The measured distance, in levels of 255, between load_image's gray / blur (PIL's integer `L` weights; the blur's rounding to uint8) and
    steps 3b / 3c of tests/augment_post_ref.py on a noisy 48 x 48 image: printed and written into DESIGN.md section 3.3f. Only gray is gated,
    at 1 level: PIL's integer weights are within 0.5 level of the f32 formula, and PIL rounds to uint8 (another 0.5)."""
    arr = _noise()
    path = _save(tmp_path, arr)
    v = arr.astype(np.float64)
    got = D.load_image(path, ("random_gray::{'p': 1.0}",), 48, _gen(0)).numpy().transpose(1, 2, 0).astype(np.float64) * 255
    worst = np.abs(got - PR.to_gray(v)).max()
    print("gray: worst difference, levels:", worst)
    assert worst <= 1.0
    for k in (3, 5, 7):
        got = D.load_image(path, ("blur::{'p': 1.0, 'blur_limit': (%d, %d)}" % (k, k),), 48, _gen(0)).numpy().transpose(1, 2, 0).astype(np.float64) * 255
        print("blur k = %d: worst difference, levels:" % k, np.abs(got - PR.blur(v, PR.WEIGHTS[k])).max())
