"""clite_augment_apply_post (csrc/augment_ops.hip: gray and blur behind the colour jitter) on the GPU against tests/augment_post_ref.py, an
all-zero table against the plain entry, bitwise reproducibility, the stem form against hip.image_to_nhwc4 of the f32 form, and the consumers:
VLInfoModel.forward and the captured TrainStep fed `image_post` batches must compute what they compute on the pre-augmented images; train.py
on configs/smoke_random_simclr.yaml. Tolerance as in tests/test_wavesim_augment_post.py: 0.02 level of 255 (blur, a convex combination, does not
amplify the incoming error and adds about 2e-4 level)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import augment_post_ref as PR
from detfill import det_fill

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEVEL = 0.02 / 255.0
SIMCLR = ("random_resized_crop", "horizontal_flip", "color_jitter8::{'p': 1.0}", "random_gray::{'p': 1.0}", "blur::{'p': 1.0}", "normalize")
DRAWN = ("random_resized_crop", "horizontal_flip", "color_jitter8", "random_gray::{'p': 0.5}", "blur", "normalize")       # a mix of plain, gray and blurred rows


def _batch(N, S, extents, transforms=SIMCLR, seed=0):
    """(canvases, packed u8, hw, plan, post) on the host: random canvases of the given extents, rows drawn by the planner"""
    from clip_lite_amd import augment
    rng = np.random.default_rng(seed)
    canv = [rng.integers(0, 256, extents[n % len(extents)] + (3,), dtype=np.uint8) for n in range(N)]
    cap = max(c.size for c in canv)
    u8, hw = augment.pack_canvases(canv, cap)
    rows = [augment.plan_transforms(c.shape[0], c.shape[1], transforms, S, torch.Generator().manual_seed(seed * 100 + n), return_post=True)
            for n, c in enumerate(canv)]
    return canv, u8, hw, torch.stack([r[0] for r in rows]), torch.stack([r[1] for r in rows])


_cache = {}


def _case(name):
    if name not in _cache:
        N, S, ext = {"small": (5, 36, [(40, 61), (70, 47), (36, 36)]), "full": (2, 224, [(256, 341)])}[name]
        canv, u8, hw, plan, post = _batch(N, S, ext)
        _cache[name] = (S, u8, hw, plan, post, PR.views(canv, plan.numpy(), post.numpy(), S))
    return _cache[name]


@pytest.mark.parametrize("name", ["small", "full"])
def test_views_match_reference(name):
    from clip_lite_amd import augment
    S, u8, hw, plan, post, want = _case(name)
    assert bool(post[:, augment.POST_GRAY].all()) and bool(post[:, augment.POST_BLUR].all())
    print("kernel weights of the rows", post[:, augment.POST_W0].tolist())
    got = augment.views(u8.cuda(), hw.cuda(), plan.cuda(), S, plan_host=plan, hw_host=hw, post=post.cuda(), post_host=post).cpu().numpy()
    err = np.abs(got - want).max()
    print(name, "max error in normalised units", err, "bound", LEVEL / 0.224)
    assert err <= LEVEL / 0.224


def test_all_zero_post_is_bit_equal_to_views_without_post():
    from clip_lite_amd import augment
    S, u8, hw, plan, post, _ = _case("small")
    d = [t.cuda() for t in (u8, hw, plan)]
    want = augment.views(*d, S)
    got = augment.views(*d, S, post=torch.zeros_like(post).cuda())
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert not torch.equal(augment.views(*d, S, post=post.cuda()), want)


def test_runs_are_bit_identical_in_both_deterministic_settings():
    from clip_lite_amd import augment, hip
    S, u8, hw, plan, post, _ = _case("small")
    d = [t.cuda() for t in (u8, hw, plan)]
    q = post.cuda()
    outs = []
    try:
        for det in (False, False, True, True):
            hip.set_deterministic(det)
            outs.append(augment.views(*d, S, post=q).cpu())
    finally:
        hip.set_deterministic(False)
    for v in outs[1:]:
        assert torch.equal(v.view(torch.int32), outs[0].view(torch.int32))


@pytest.mark.parametrize("dt", [0, 1])
def test_stem_form_equals_image_to_nhwc4_of_the_f32_form(dt):
    from clip_lite_amd import augment, hip
    S, u8, hw, plan, _, _ = _case("small")
    _, _, _, _, post = _batch(5, S, [(40, 61), (70, 47), (36, 36)], transforms=DRAWN, seed=4)          # the same canvases' extents, mixed rows
    d = [t.cuda() for t in (u8, hw, plan)]
    q = post.cuda()
    N = u8.shape[0]
    f32 = augment.views(*d, S, post=q)
    Hp, Wp = S + 6, S + 8
    want = torch.full((N, Hp, Wp, 4), float("nan"), device="cuda", dtype=hip.TORCH_DTYPE[dt])
    hip.image_to_nhwc4(dt, f32, want, N, S, S, 3, Hp, Wp)
    got = torch.full((N, Hp, Wp, 4), float("nan"), device="cuda", dtype=hip.TORCH_DTYPE[dt])
    hip.augment_apply_post(hip.AUGMENT_NHWC4, dt, *d, q, augment.gray_means(*d, S), S, got, 3, Hp, Wp)
    bits = torch.int16 if dt == 0 else torch.int32
    assert torch.equal(got.view(bits), want.view(bits))


def _model(layers=1, amp=False, vssl=False):
    from clip_lite_amd.encoder import ImageEncoder, TextEncoder
    from clip_lite_amd.loss import JSDInfoMaxLoss
    from clip_lite_amd.model import VLInfoModel
    torch.manual_seed(7)
    te = TextEncoder(mode="train_sbert", num_hidden_layers=layers)
    te.strans.hidden_dropout_prob = te.strans.attention_probs_dropout_prob = 0.0
    L = JSDInfoMaxLoss(512, 768, "dot", 0.1, True, True, visual_self_supervised=vssl, textual_self_supervised=False)
    return det_fill(VLInfoModel(te, ImageEncoder("resnet18"), L, "train_sbert", is_amp=amp)).to("cuda").train()


def _captions(B, L, seed):
    ids = torch.randint(1000, 30522, (B, L), generator=torch.Generator().manual_seed(seed))
    ids[:, 0], ids[:, -1] = 101, 102
    return {"input_ids": ids.cuda(), "attention_mask": torch.ones(B, L, dtype=torch.long).cuda()}


def test_forward_on_canvases_with_post_equals_forward_on_their_views(deterministic_reductions):
    """`image_u8` + `image_plan` + `image_post` against the f32 output as `image`, and `aug_image_plan` + `aug_image_post` against `aug_image`"""
    from clip_lite_amd import augment
    from clip_lite_amd.model import VLInfoModel
    B, S = 4, 64
    _, u8, hw, plan, post = _batch(B, S, [(72, 96), (80, 72)], transforms=DRAWN, seed=1)
    _, _, _, plan2, post2 = _batch(B, S, [(72, 96), (80, 72)], transforms=DRAWN, seed=2)
    assert post.any() and post2.any()
    u8, hw, plan, plan2, post, post2 = (t.cuda() for t in (u8, hw, plan, plan2, post, post2))
    cap = _captions(B, 9, 1)
    noise = torch.rand(B, 512, generator=torch.Generator().manual_seed(3)).cuda(), torch.rand(B, 768, generator=torch.Generator().manual_seed(4)).cuda()
    losses = []
    for form in ("u8", "f32", "u8+aug", "f32+aug"):
        M = _model(vssl=form.endswith("aug"))
        M.loss.set_prior_noise(*noise)
        batch = dict(cap)
        if form.startswith("u8"):
            batch.update(image_u8=u8, image_hw=hw, image_plan=plan, image_post=post)
            if form.endswith("aug"):
                batch.update(aug_image_plan=plan2, aug_image_post=post2)
            assert not any(k.endswith("_post") or k.endswith("_plan") for k in VLInfoModel.materialize_views(batch, size=S))
        else:
            batch["image"] = augment.views(u8, hw, plan, S, post=post)
            if form.endswith("aug"):
                batch["aug_image"] = augment.views(u8, hw, plan2, S, post=post2)
        out = M(batch)
        losses.append((out["loss"].item(), out["loss_components"]["visual_loss"].item()))
    assert losses[0] == losses[1] and losses[2] == losses[3], losses
    assert losses[2][1] != 0 and losses[2] != losses[0]
    plain = _model()
    plain.loss.set_prior_noise(*noise)
    assert plain(dict(cap, image_u8=u8, image_hw=hw, image_plan=plan))["loss"].item() != losses[0][0]          # the post rows are not ignored


def test_replayed_train_steps_on_post_batches_equal_those_on_views(deterministic_reductions):
    """ResNet-18 / 2-layer BERT at batch 8: two eager warm-up steps, then the capture and three replays; the canvases go straight into the staged
    stem input (augment.stage_views with post), the pre-augmented images through stage_image - the losses must be bit-equal"""
    from clip_lite_amd import augment
    from clip_lite_amd.optim import FusedSGD, Lookahead
    from clip_lite_amd.optim.lr_scheduler import LinearWarmupCosineAnnealingLR
    from clip_lite_amd.train_loop import TrainStep
    from clip_lite_amd.utils.common import GradScaler
    B, S = 8, 64
    batches = []
    for i in range(3):
        _, u8, hw, plan, post = _batch(B, S, [(72, 96), (80, 72)], transforms=DRAWN, seed=10 + i)
        assert post.any()
        batches.append(dict(_captions(B, 12, i), image_u8=u8.cuda(), image_hw=hw.cuda(), image_plan=plan.cuda(), image_post=post.cuda()))
    results = []
    for form in ("u8", "f32"):
        M = _model(layers=2, amp=True)
        groups = [{"params": [p], "lr": 1e-3 if "image_encoder" in n else 1e-4, "weight_decay": 1e-4} for n, p in M.named_parameters()]
        opt = Lookahead(FusedSGD(groups, momentum=0.9), k=3, alpha=0.5)
        sched = LinearWarmupCosineAnnealingLR(opt, total_steps=40, warmup_steps=3)
        step = TrainStep(M, opt, sched, GradScaler(True), 10.0, None, graph=True, graph_warmup=2)
        losses = []
        for s in range(5):          # two eager warm-up steps; the third call captures and replays, then two more replays
            b = batches[s % 3]
            if form == "f32":
                b = {"input_ids": b["input_ids"], "attention_mask": b["attention_mask"],
                     "image": augment.views(b["image_u8"], b["image_hw"], b["image_plan"], S, post=b["image_post"])}
            losses.append(step(b)["loss"].item())
        assert step.replays == 3 and step._graphs is not None, (step.replays, step.eager_steps)
        results.append(losses)
    assert all(np.isfinite(results[0]))
    assert results[0] == results[1], results


def test_train_cli_on_the_simclr_recipe(tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--config", os.path.join(ROOT, "configs", "smoke_random_simclr.yaml"),
           "--num-gpus-per-machine", "1", "--checkpoints-dir", str(tmp_path) + "/", "--checkpoint-every", "100", "--log-every", "2",
           "--config-override", "OPTIM.NUM_ITERATIONS", "6", "DATA.IMAGE_CROP_SIZE", "64", "DATA.GPU_AUGMENT_SOURCE_SIZE", "80", "OPTIM.BATCH_SIZE", "16"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    assert "capture of the train step failed" not in (r.stdout + r.stderr)
    lines = re.findall(r"train total_loss=(\S+) cross_modal_loss=(\S+) visual_loss=(\S+) textual_loss=(\S+)", r.stdout + r.stderr)
    assert lines, r.stdout[-1500:]
    total, _, visual, textual = (float(x) for x in lines[-1])
    assert np.isfinite(total) and visual != 0 and textual != 0, lines[-1]
