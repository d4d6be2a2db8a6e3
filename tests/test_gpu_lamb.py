"""FusedLAMB on the GPU, host level (optim/fused_sgd.py over csrc/update_ops.hip): tests/test_gpu_lars.py's small arena of hand-picked tensors with
random fixed gradients against the float64 reference (tests/lamb_ref.py) through Lookahead, clipping, the checkpoint layout, span launches and the
factory; then configs/smoke_random_lamb.yaml through TrainStep, eager and captured. The step bounds are those of tests/test_gpu_lamb_ops.py: p and
slow per element within 2e-6 * max(1, max|ref|) + 2e-5 * |delta_ref|, delta_ref = lr q r, the moments within 1e-5 * max|ref|, every step's
reference evaluated on the f32 state the device held before that step; the norms' bound is 1e-5 * max(1, sum of terms).

Tensors of the small arena (padded to 64 elements each, pads zero): w5 [1, 5] (one item of 8 elements, 3 of them padding), w8195 [5, 1639] (two
items: 8192 + 4, one element of padding), w3 [130, 129] (three items), conv [8, 4, 3, 3] (stored permuted), frozen [6, 50] (no item), and the 1-D
b300, scale [7], bias [1028], which LAMB never adapts.

Measured on an MI355X (`pytest -s`, LAMBERR lines; no figure feeds a bound):
  four steps      max error / bound: p 0.034   slow 0.034   m 0.0083   v2 0.016
  trust ratios    squared norms, error / max(1, sum of terms): |p| w5 1.5e-08, w8195 9.8e-09, conv 8.9e-08, w3 1.9e-08; |r| w5 1.1e-07,
                  w8195 1.2e-07, conv 1.0e-07, w3 1.1e-07 (bound 1e-5); q: 0.264756199 against 0.264756208 (w5), 4.98680559 against 4.98680606 (conv)
  smoke config    captured against eager, deterministic reductions: losses and parameters bit-identical on both capture forms (parameter
                  movement over four steps 0.711 with the ViT, 0.457 with the ResNet-18)
"""
import copy
import os

import numpy as np
import pytest
import torch

import lamb_ref as L
import loss_ref as R
from test_gpu_lars import _bits_equal, _np, _tiny, _write_grads

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B1, B2, EPS = 0.9, 0.999, 1e-6
ADAPTED = ("w5", "w8195", "conv", "w3")


def _groups(M):
    return [{"params": [p], "lr": 3e-3 if p.dim() == 4 else 1e-3, "weight_decay": 0.0 if n in ("scale", "bias") else 1e-2} for n, p in M.named_parameters()]


def _tensors(M, A):
    out, lr, wd = [], np.zeros(A.total), np.zeros(A.total)
    for grp in _groups(M):
        p = grp["params"][0]
        if not p.requires_grad:
            continue
        o, numel = A.index[p._clite[1]]
        out.append(L.Tensor(o, numel, p.dim() >= 2))
        lr[o:o + numel], wd[o:o + numel] = np.float32(grp["lr"]), np.float32(grp["weight_decay"])
    inside = np.zeros(A.total, bool)
    for t in out:
        inside[t.start:t.start + t.n] = True
    return out, lr, wd, inside


def _reference(p0, g0, m0, v0, s0, lr, wd, max_norm, sync, step, ss, trust_clip, tensors):
    """lamb_step_ref on the f32 values FusedLAMB.upload_hp uploads for optimizer step `step` (1-based): lr multiplier 1, alpha 0.5, pre-scale 1."""
    f = L.f32
    return L.lamb_step_ref(p0, g0, m0, v0, s0, lr, wd, max_norm, sync, 0.5, 1.0, f(B2), f(EPS), f(1 - B1 ** step), f(1 - B2 ** step), f(1 - B1), f(1 - B2),
                           ss, trust_clip, tensors)


def test_four_steps_with_lookahead_and_clipping_track_float64():
    """FusedLAMB + Lookahead(k = 2, alpha = 0.5), four steps; the gradient scale alternates so that the global norm (about 1.7 / 0.17) is clipped at
    1 on steps 0 and 2 and not on 1 and 3. After every step: p, slow and both moments within the step bounds, the gradient arena zero, the bf16
    copy the round-to-nearest-even of p, the frozen tensor and the pads bit for bit what they were."""
    from clip_lite_amd.optim import FusedLAMB, Lookahead
    M, A = _tiny()
    opt = FusedLAMB(_groups(M))
    wrapped = Lookahead(opt, k=2, alpha=0.5)
    tensors, lr, wd, inside = _tensors(M, A)
    fo, fn = A.index["frozen"]
    worst = {}
    for step in range(4):
        _write_grads(M, A, 100 + step, 0.01 if step % 2 == 0 else 0.001)
        p0, m0, v0, s0 = _np(A.flat_p), _np(opt.flat_v), _np(opt.flat_v2), _np(opt.flat_slow)
        total = wrapped.clip_grad_norm(1.0)
        g0 = _np(A.flat_g)
        assert not g0[fo:fo + fn].any(), "the frozen tensor's gradient must not enter the norm"
        ss = float(opt.sumsq.item())
        R.scalar(f"step {step} sumsq", ss, (g0[inside].astype(np.float64) ** 2).sum(), g0[inside].astype(np.float64) ** 2)
        assert (float(total) > 1.0) == (step % 2 == 0)
        wrapped.step()
        torch.cuda.synchronize()
        assert opt.steps == step + 1
        sync = step % 2 == 1
        ref = _reference(p0, g0, m0, v0, s0, lr, wd, 1.0, sync, step + 1, ss, False, tensors)
        assert all((ref.q[t.start] != 1.0) == t.adapted for t in tensors)
        delta = np.abs(lr * ref.q * ref.r)
        for name, got, r, before, d in (("p", A.flat_p, ref.p, p0, delta), ("slow", opt.flat_slow, ref.slow, s0, delta if sync else 0 * delta),
                                        ("m", opt.flat_v, ref.m, m0, None), ("v2", opt.flat_v2, ref.v2, v0, None)):
            err = np.abs(_np(got).astype(np.float64) - r)
            bound = 1e-5 * np.abs(r[inside]).max() + 0 * err if d is None else 2e-6 * max(1.0, np.abs(r[inside]).max()) + 2e-5 * d
            worst[name] = max(worst.get(name, 0.0), float((err / bound)[inside].max()))
            print(f"LAMBERR host step {step} {name}: max err / bound = {(err / bound)[inside].max():.4f}, running max {worst[name]:.4f}")
            assert (err[inside] <= bound[inside]).all(), (step, name, float((err / bound)[inside].max()))
            assert R.same_bits(_np(got)[~inside], before[~inside]), f"{name}: the frozen tensor or a pad changed"
        assert not A.flat_g.any()
        assert np.array_equal(_np(A.flat_lp.view(torch.int16)).view(np.uint16)[inside], R.to_bf16_bits(_np(A.flat_p))[inside])
        if sync:
            assert np.array_equal(_np(opt.flat_slow)[inside], _np(A.flat_p)[inside])


@pytest.mark.parametrize("trust_clip", [False, True])
def test_tensor_norms_and_trust_ratio_against_float64_ignore_the_padding(trust_clip):
    """The items of w5 and w8195 cover 3 and 1 elements of arena padding: the norms the update used are those of the tensors themselves (float64:
    |p| before the update, |r| from the reference's moments after it), within the sumsq bound on their squares; trust_ratio is their quotient
    (within 2e-5: LARS's trust-ratio term), capped at 1 under trust_clip. conv's parameters are scaled up (the others' ratios are about 0.5 at
    step 1, where |u| = 1 per element) so that ratios on both sides of 1 occur."""
    from clip_lite_amd.optim import FusedLAMB
    M, A = _tiny()
    o, numel = A.index["conv"]
    A.flat_p[o:o + numel] *= 10.0
    opt = FusedLAMB(_groups(M), trust_clip=trust_clip)
    tensors, lr, wd, inside = _tensors(M, A)
    _write_grads(M, A, 7, 0.3)
    p0, g0 = _np(A.flat_p), _np(A.flat_g)
    zeros = np.zeros(A.total, np.float32)
    opt.step()
    torch.cuda.synchronize()
    ref = _reference(p0, g0, zeros, zeros, p0, lr, wd, 0.0, False, 1, float("nan"), trust_clip, tensors)
    free = []
    for n in ADAPTED:
        o, numel = A.index[n]
        pn, rn = np.linalg.norm(p0[o:o + numel].astype(np.float64)), np.linalg.norm(ref.r[o:o + numel])
        got = opt.tensor_norms(getattr(M, n))
        for what, a, b in (("|p|", got[0], pn), ("|r|", got[1], rn)):
            err = abs(a * a - b * b) / max(1.0, b * b)
            print(f"LAMBERR host norms {n} {what}: {a:.9g} against {b:.9g}, squares' error / max(1, sum of terms) = {err:.2e}")
            assert err <= 1e-5, (n, what, a, b)
        q = opt.trust_ratio(getattr(M, n))
        free.append(pn / rn)
        print(f"LAMBERR host trust ratio {n}: {q:.9g} against {ref.q[o]:.9g}")
        assert abs(q - ref.q[o]) <= 2e-5 * ref.q[o] and (not trust_clip or q <= 1.0)
    assert min(free) < 1.0 < max(free)
    assert opt._slots.keys() == {id(getattr(M, n)) for n in ADAPTED + ("frozen",)}


def test_one_dimensional_tensors_move_exactly_as_under_fused_adamw():
    """Same parameters, same gradients, hence the same clip factor: biases and scales are bit-identical to FusedAdamW's after two steps (moments
    and bf16 copy too), the adapted tensors are not."""
    from clip_lite_amd.optim import FusedAdamW, FusedLAMB
    res = []
    for cls in (FusedAdamW, FusedLAMB):
        M, A = _tiny()
        opt = cls(_groups(M), eps=EPS, weight_decay=0.0)
        for step in range(2):
            _write_grads(M, A, 20 + step, 0.01)
            assert float(opt.clip_grad_norm(1.0)) > 1.0
            opt.step()
        torch.cuda.synchronize()
        res.append((A, A.flat_p.clone(), opt.flat_v.clone(), opt.flat_v2.clone(), A.flat_lp.clone().view(torch.int16)))
    (A, p0, m0, v0, c0), (_, p1, m1, v1, c1) = res
    assert _bits_equal(m0, m1) and _bits_equal(v0, v1), "the moments do not depend on the trust ratio"
    for n in ("b300", "scale", "bias"):
        o, numel = A.index[n]
        assert _bits_equal(p0[o:o + numel], p1[o:o + numel]) and torch.equal(c0[o:o + numel], c1[o:o + numel]), n
    for n in ADAPTED:
        o, numel = A.index[n]
        assert not torch.equal(p0[o:o + numel], p1[o:o + numel]), n


def test_frozen_tensor_is_untouched_and_keeps_a_zero_gradient():
    from clip_lite_amd.optim import FusedLAMB
    M, A = _tiny()
    opt = FusedLAMB(_groups(M))
    o, numel = A.index["frozen"]
    before = A.flat_p[o:o + numel].clone()
    others = A.flat_p.clone()
    for step in range(2):
        _write_grads(M, A, 30 + step, 0.1)
        assert A.flat_g[o:o + numel].any()
        opt.clip_grad_norm(1.0)
        opt.step()
        torch.cuda.synchronize()
        assert not A.flat_g.any()
    assert _bits_equal(A.flat_p[o:o + numel], before) and not opt.flat_v[o:o + numel].any() and not opt.flat_v2[o:o + numel].any()
    assert not torch.equal(A.flat_p[:o], others[:o])


def test_state_dict_round_trip_continues_bit_identically():
    """torch.optim.AdamW's layout (step, exp_avg, exp_avg_sq per parameter); a fresh optimizer on a fresh arena that loads it takes the next step
    bit for bit as the uninterrupted run does - which it only does if the step counter (the bias corrections' exponent) came along."""
    from clip_lite_amd.optim import FusedLAMB
    M, A = _tiny()
    opt = FusedLAMB(_groups(M))
    for step in range(2):
        _write_grads(M, A, 40 + step, 0.01)
        opt.clip_grad_norm(1.0)
        opt.step()
    sd, p_saved = copy.deepcopy(opt.state_dict()), A.flat_p.clone()
    assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"} and len(sd["state"]) == len(sd["param_groups"]) == 8
    assert sd["state"][3]["exp_avg"].shape == (8, 4, 3, 3) and float(sd["state"][3]["step"]) == 2.0
    assert sd["param_groups"][0]["betas"] == (B1, B2) and sd["param_groups"][0]["eps"] == EPS
    M2, A2 = _tiny()
    A2.flat_p.copy_(p_saved)
    A2.refresh_lowp()
    opt2 = FusedLAMB(_groups(M2))
    opt2.load_state_dict(sd)
    assert opt2.steps == 2 and _bits_equal(opt2.flat_v, opt.flat_v) and _bits_equal(opt2.flat_v2, opt.flat_v2)
    for (m, a, o) in ((M, A, opt), (M2, A2, opt2)):
        _write_grads(m, a, 42, 0.01)
        o.clip_grad_norm(1.0)
        o.step()
    torch.cuda.synchronize()
    assert _bits_equal(A.flat_p, A2.flat_p) and _bits_equal(opt.flat_v, opt2.flat_v) and _bits_equal(opt.flat_v2, opt2.flat_v2)
    assert torch.equal(A.flat_lp.view(torch.int16), A2.flat_lp.view(torch.int16)) and not _bits_equal(A.flat_p, p_saved)


def test_two_span_launches_on_a_tensor_boundary_equal_one_launch_bitwise():
    from clip_lite_amd.optim import FusedLAMB
    res = []
    for split in (False, True):
        M, A = _tiny()
        opt = FusedLAMB(_groups(M))
        k = A.index["conv"][0]
        for step in range(2):
            _write_grads(M, A, 50 + step, 0.01)
            opt.clip_grad_norm(1.0)
            opt.upload_hp(lookahead_sync=step == 1, alpha=0.5)
            for span in (((0, k), (k, A.total)) if split else (None,)):
                opt.launch(span)
        torch.cuda.synchronize()
        assert opt.steps == 2 and not A.flat_g.any()
        res.append((A.flat_p.clone(), opt.flat_v.clone(), opt.flat_v2.clone(), opt.flat_slow.clone(), opt.norms.clone(), A.flat_lp.clone().view(torch.int16)))
    assert 0 < k < res[0][0].numel()
    for a, b in zip(*res):
        assert torch.equal(a, b) if a.dtype == torch.int16 else _bits_equal(a, b)


def test_optimizer_factory_builds_lookahead_over_fused_lamb():
    from clip_lite_amd.config import Config
    from clip_lite_amd.factories import OptimizerFactory
    from clip_lite_amd.optim import FusedAdamW, FusedLAMB, Lookahead
    M, _ = _tiny()
    cfg = Config(override_list=["OPTIM.OPTIMIZER_NAME", "lamb", "OPTIM.LAMB.BETA2", 0.98, "OPTIM.LAMB.EPS", 1e-7, "OPTIM.LAMB.TRUST_CLIP", True,
                                "OPTIM.LR", 2e-3, "OPTIM.WEIGHT_DECAY", 0.02, "OPTIM.NO_DECAY", ".*(scale|bias)"])
    opt = OptimizerFactory.from_config(cfg, M.named_parameters())
    assert isinstance(opt, Lookahead) and type(opt.optimizer) is FusedLAMB and opt.k == cfg.OPTIM.LOOKAHEAD.STEPS
    inner = opt.optimizer
    assert isinstance(inner, FusedAdamW) and inner.trust_clip is True and "momentum" not in inner.param_groups[0]
    assert all(g["betas"] == (0.9, 0.98) and g["eps"] == 1e-7 and g["lr"] == 2e-3 for g in inner.param_groups)
    names = [n for n, _ in M.named_parameters()]
    assert [g["weight_decay"] for g in inner.param_groups] == [0.0 if n in ("scale", "bias") else 0.02 for n in names]
    L_ = Config().OPTIM.LAMB
    assert (L_.BETA1, L_.BETA2, L_.EPS, L_.TRUST_CLIP) == (0.9, 0.999, 1e-6, False)
    M2, _ = _tiny()
    plain = OptimizerFactory.from_config(Config(override_list=["OPTIM.OPTIMIZER_NAME", "lamb", "OPTIM.LOOKAHEAD.USE", False]), M2.named_parameters())
    assert type(plain) is FusedLAMB and plain.trust_clip is False and plain.param_groups[0]["eps"] == 1e-6 and plain.param_groups[0]["betas"] == (0.9, 0.999)


@pytest.mark.usefixtures("deterministic_reductions")
@pytest.mark.parametrize("tower", ["vit_b_32", "resnet18"])
def test_lamb_smoke_config_captured_step_tracks_eager_and_repeats_bitwise(tower):
    """configs/smoke_random_lamb.yaml (64-pixel crops, batch 8) through TrainStep as train_loop.main builds it - the factories' model, LAMB under
    Lookahead, the cosine schedule, clipping, defer_update - for four steps: eager, captured (two eager warm-up steps, the capture, two replays)
    and captured again. As configured the image tower is a ViT, which TrainStep captures as ONE graph (the update is one launch over the whole
    table); overridden to resnet18 / FEATURE_SIZE 512 the same configuration takes the per-phase graphs, where the update is three span launches
    and the text encoder's and the heads' share is deferred to the next step - the case in which the step counter (one increment per upload_hp,
    not per launch) and the per-span partials can go wrong. The bar of tests/test_gpu_train_step.py's captured-versus-eager run, as
    tests/test_gpu_lars.py takes it: every loss within 2e-3, the total parameter movement within 2 % (relative L2) and above 1e-3. The two captured
    runs end bit-identical in parameters and both moments."""
    from clip_lite_amd.config import Config
    from clip_lite_amd.factories import LRSchedulerFactory, OptimizerFactory, PretrainingDatasetFactory, PretrainingModelFactory
    from clip_lite_amd.optim import FusedLAMB, Lookahead
    from clip_lite_amd.train_loop import TrainStep
    from clip_lite_amd.utils.common import GradScaler
    B = 8
    _C = Config(os.path.join(ROOT, "configs", "smoke_random_lamb.yaml"),
                [] if tower == "vit_b_32" else ["MODEL.VISUAL.NETWORK_NAME", "resnet18", "MODEL.VISUAL.FEATURE_SIZE", 512, "MODEL.VISUAL.SELF_SUPERVISED", False,
                                                "MODEL.TEXTUAL.SELF_SUPERVISED", False])
    assert _C.OPTIM.OPTIMIZER_NAME == "lamb" and _C.DATA.IMAGE_CROP_SIZE == 64 and _C.OPTIM.BATCH_SIZE == B and _C.MODEL.VISUAL.NETWORK_NAME == tower
    ds = PretrainingDatasetFactory.from_config(_C, "train")
    batches = [{k: v.cuda() for k, v in ds.collate_fn([ds[i * B + j] for j in range(B)]).items() if torch.is_tensor(v)} for i in range(3)]
    # the captured step pads captions to pad_to columns and dropout-mask indices depend on the caption length: the eager run gets the same padded
    # tensors (the step's own padding is then the identity), so that both runs draw the same masks
    for b in batches:
        for k in TrainStep._CAPTION_KEYS:
            if k in b:
                b[k] = torch.nn.functional.pad(b[k], (0, int(_C.DATA.MAX_CAPTION_LENGTH) - b[k].shape[1]))          # BERT's pad id, and mask, 0
    assert all(b["input_ids"].shape[1] == _C.DATA.MAX_CAPTION_LENGTH for b in batches)
    results = []
    for graph in (False, True, True):
        torch.manual_seed(7)          # initial weights, and the runtime's base seed (dropout, prior noise) comes from torch.initial_seed()
        M = PretrainingModelFactory.from_config(_C).to("cuda").train()
        p_init = M.runtime.arena.flat_p.clone()
        opt = OptimizerFactory.from_config(_C, M.named_parameters())
        assert isinstance(opt, Lookahead) and type(opt.optimizer) is FusedLAMB
        sched = LRSchedulerFactory.from_config(_C, opt)
        step = TrainStep(M, opt, sched, GradScaler(_C.AMP), _C.OPTIM.CLIP_GRAD_NORM, None, graph=graph, graph_warmup=2,
                         pad_to=int(_C.DATA.MAX_CAPTION_LENGTH), defer_update=True)
        losses = [step(batches[s % 3])["loss"].item() for s in range(4)]
        if graph:
            assert step.replays == 2 and step.eager_steps == 2, (step.replays, step.eager_steps)
            if tower == "vit_b_32":
                assert step._g is not None and step._graphs is None
            else:
                assert step._graphs is not None and step._pending_rest
        else:
            assert step.replays == 0 and step.eager_steps == 4
        step.finish()
        torch.cuda.synchronize()
        A = M.runtime.arena
        assert not A.flat_g.any() and all(np.isfinite(l) for l in losses)
        assert opt.optimizer.steps == 4 and opt.optimizer.norms.sum().item() > 0          # one count per step; the per-tensor norms were taken
        results.append((losses, A.flat_p - p_init, A.flat_p.clone(), opt.optimizer.flat_v.clone(), opt.optimizer.flat_v2.clone()))
    (l0, d0, _, _, _), (l1, d1, p1, m1, v1), (l2, _, p2, m2, v2) = results
    print(f"LAMBERR smoke config {tower}: losses eager", l0, "captured", l1)
    assert max(abs(a - b) for a, b in zip(l0, l1)) < 2e-3, (l0, l1)
    rel = ((d0 - d1).norm() / d0.norm()).item()
    print(f"LAMBERR smoke config {tower}: parameter movement {d0.norm().item():.3e}, captured against eager {rel:.2e} of it")
    assert d0.norm().item() > 1e-3 and rel < 2e-2, (d0.norm().item(), rel)
    assert l1 == l2 and _bits_equal(p1, p2) and _bits_equal(m1, m2) and _bits_equal(v1, v2)
