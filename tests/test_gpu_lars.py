"""FusedLARS on the GPU, host level (optim/fused_sgd.py over csrc/update_ops.hip): a small arena of hand-picked tensors with random fixed gradients
against the float64 reference (tests/lars_ref.py) through Lookahead, clipping, the checkpoint layout and the factory; then
configs/smoke_random_lars.yaml through TrainStep, eager and captured. The step bounds are those of tests/test_gpu_lars_ops.py: per element
1e-6 * max(1, |ref|) + 2e-5 * |delta_ref|, every step's reference evaluated on the f32 state the device held before that step; the norms' bound is
1e-5 * max(1, sum of terms).

Tensors of the small arena (padded to 64 elements each, pads zero): w5 [1, 5] (one item of 8 elements, 3 of them padding), w8195 [5, 1639] (two
items: 8192 + 4, one element of padding), w3 [130, 129] (three items), conv [8, 4, 3, 3] (stored permuted), frozen [6, 50] (no item), and the 1-D
b300, scale [7], bias [1028], which LARS never adapts.

Measured on an MI355X (`pytest -s`, LARSERR lines; no figure feeds a bound):
  four steps      max error / bound: p 0.077   v 0.046   slow 0.077
  trust ratios    squared norms, error / max(1, sum of terms): w5 2.7e-08, w8195 3.0e-08, conv 9.9e-08, w3 5.5e-08            (bound 1e-5)
  smoke config    captured against eager, deterministic reductions: losses and parameters bit-identical on both capture forms
"""
import copy
import os

import numpy as np
import pytest
import torch

import lars_ref as L
import loss_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ETA, EPS = 0.5, 1e-8          # a trust coefficient large enough that a wrong ratio cannot hide under the SGD bound


class Tiny(torch.nn.Module):
    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(5)
        for name, shape in (("w5", (1, 5)), ("b300", (300,)), ("w8195", (5, 1639)), ("conv", (8, 4, 3, 3)), ("scale", (7,)), ("w3", (130, 129)),
                            ("frozen", (6, 50)), ("bias", (1028,))):
            setattr(self, name, torch.nn.Parameter(torch.randn(*shape, generator=g) * 0.5))


def _tiny(lowp=True):
    from clip_lite_amd.runtime import Arena
    M = Tiny()
    A = Arena(list(M.named_parameters()), "cuda", lowp)
    M.frozen.requires_grad_(False)
    return M, A


def _groups(M):
    return [{"params": [p], "lr": 0.1 if p.dim() == 4 else 0.02, "weight_decay": 0.0 if n in ("scale", "bias") else 1e-2} for n, p in M.named_parameters()]


def _write_grads(M, A, seed, scale):
    """Random fixed gradients into the arena's gradient buffer (frozen tensor included; the pads stay zero)."""
    g = torch.Generator().manual_seed(seed)
    for n, _ in M.named_parameters():
        o, numel = A.index[n]
        A.flat_g[o:o + numel] = (torch.randn(numel, generator=g) * scale).cuda()


def _tensors(M, A):
    out, lr, wd = [], np.zeros(A.total), np.zeros(A.total)
    for grp in _groups(M):
        p = grp["params"][0]
        if not p.requires_grad:
            continue
        o, numel = A.index[p._clite[1]]
        out.append(L.Tensor(o, numel, p.dim() >= 2))
        lr[o:o + numel], wd[o:o + numel] = np.float32(grp["lr"]), np.float32(grp["weight_decay"])
    return out, lr, wd


def _np(t):
    return t.detach().cpu().numpy().copy()


def _bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def test_four_steps_with_lookahead_and_clipping_track_float64():
    """FusedLARS + Lookahead(k = 2, alpha = 0.5), four steps; the gradient scale alternates so that the global norm (about 1.7 / 0.17) is clipped at
    1 on steps 0 and 2 and not on 1 and 3. After every step: p, v, slow within the step bounds, the gradient arena zero, the bf16 copy the
    round-to-nearest-even of p, the frozen tensor and the pads bit for bit what they were."""
    from clip_lite_amd.optim import FusedLARS, Lookahead
    M, A = _tiny()
    opt = FusedLARS(_groups(M), momentum=0.9, trust_coefficient=ETA, eps=EPS)
    wrapped = Lookahead(opt, k=2, alpha=0.5)
    tensors, lr, wd = _tensors(M, A)
    inside = np.zeros(A.total, bool)
    for t in tensors:
        inside[t.start:t.start + t.n] = True
    fo, fn = A.index["frozen"]
    worst = {}
    for step in range(4):
        _write_grads(M, A, 100 + step, 0.01 if step % 2 == 0 else 0.001)
        p0, v0, s0 = _np(A.flat_p), _np(opt.flat_v), _np(opt.flat_slow)
        total = wrapped.clip_grad_norm(1.0)
        g0 = _np(A.flat_g)
        assert not g0[fo:fo + fn].any(), "the frozen tensor's gradient must not enter the norm"
        ss = float(opt.sumsq.item())
        R.scalar(f"step {step} sumsq", ss, (g0[inside].astype(np.float64) ** 2).sum(), g0[inside].astype(np.float64) ** 2)
        assert (float(total) > 1.0) == (step % 2 == 0)
        wrapped.step()
        torch.cuda.synchronize()
        sync = step % 2 == 1
        ref = L.lars_step_ref(p0, g0, v0, s0, lr, wd, L.f32(0.9), 1.0, sync, 0.5, 1.0, ss, L.f32(ETA), L.f32(EPS), tensors)
        assert all((ref.q[t.start] != 1.0) == t.adapted for t in tensors)
        dv = np.abs(ref.u)
        for name, got, r, delta in (("p", A.flat_p, ref.p, lr * dv), ("v", opt.flat_v, ref.v, dv), ("slow", opt.flat_slow, ref.slow, lr * dv if sync else 0 * dv)):
            err = np.abs(_np(got).astype(np.float64) - r)
            bound = 1e-6 * np.maximum(1.0, np.abs(r)) + 2e-5 * delta
            worst[name] = max(worst.get(name, 0.0), float((err / bound)[inside].max()))
            print(f"LARSERR host step {step} {name}: max err / bound = {(err / bound)[inside].max():.3f}, running max {worst[name]:.3f}")
            assert (err[inside] <= bound[inside]).all(), (step, name, float((err / bound)[inside].max()))
            assert R.same_bits(_np(got)[~inside], (p0 if name == "p" else v0 if name == "v" else s0)[~inside]), f"{name}: the frozen tensor or a pad changed"
        assert not A.flat_g.any()
        assert np.array_equal(_np(A.flat_lp.view(torch.int16)).view(np.uint16)[inside], R.to_bf16_bits(_np(A.flat_p))[inside])
        if sync:
            assert np.array_equal(_np(opt.flat_slow)[inside], _np(A.flat_p)[inside])


def test_trust_ratio_norms_of_a_5_and_an_8195_element_tensor_ignore_the_padding():
    """The items of w5 and w8195 cover 3 and 1 elements of arena padding: the norms the update used are p.norm() / grad.norm() of the tensors
    themselves (float64), within the sumsq bound on their squares."""
    from clip_lite_amd.optim import FusedLARS
    M, A = _tiny()
    opt = FusedLARS(_groups(M), momentum=0.9, trust_coefficient=ETA, eps=EPS)
    _write_grads(M, A, 7, 0.3)
    want = {n: (getattr(M, n).detach().double().norm().item(), getattr(M, n).grad.detach().double().norm().item()) for n in ("w5", "w8195", "conv", "w3")}
    opt.step()
    torch.cuda.synchronize()
    for n, (pn, gn) in want.items():
        got = opt.tensor_norms(getattr(M, n))
        for what, a, b in (("|p|", got[0], pn), ("|g|", got[1], gn)):
            err = abs(a * a - b * b) / max(1.0, b * b)
            print(f"LARSERR host norms {n} {what}: {a:.9g} against {b:.9g}, squares' error / max(1, sum of terms) = {err:.2e}")
            assert err <= 1e-5, (n, what, a, b)
    assert opt._slots.keys() == {id(getattr(M, n)) for n in ("w5", "w8195", "conv", "w3", "frozen")}


def test_one_dimensional_tensors_move_exactly_as_under_fused_sgd():
    """Same parameters, same gradients, hence the same clip factor: biases and scales are bit-identical to FusedSGD's after two steps (momentum
    and bf16 copy too), the adapted tensors are not."""
    from clip_lite_amd.optim import FusedLARS, FusedSGD
    res = []
    for cls, kw in ((FusedSGD, {}), (FusedLARS, dict(trust_coefficient=ETA, eps=EPS))):
        M, A = _tiny()
        opt = cls(_groups(M), momentum=0.9, **kw)
        for step in range(2):
            _write_grads(M, A, 20 + step, 0.01)
            assert float(opt.clip_grad_norm(1.0)) > 1.0
            opt.step()
        torch.cuda.synchronize()
        res.append((A, A.flat_p.clone(), opt.flat_v.clone(), A.flat_lp.clone().view(torch.int16)))
    (A, p0, v0, c0), (_, p1, v1, c1) = res
    for n in ("b300", "scale", "bias"):
        o, numel = A.index[n]
        assert _bits_equal(p0[o:o + numel], p1[o:o + numel]) and _bits_equal(v0[o:o + numel], v1[o:o + numel]), n
        assert torch.equal(c0[o:o + numel], c1[o:o + numel]), n
    for n in ("w5", "w8195", "conv", "w3"):
        o, numel = A.index[n]
        assert not torch.equal(p0[o:o + numel], p1[o:o + numel]), n


def test_frozen_tensor_is_untouched_and_keeps_a_zero_gradient():
    from clip_lite_amd.optim import FusedLARS
    M, A = _tiny()
    opt = FusedLARS(_groups(M), momentum=0.9, trust_coefficient=ETA, eps=EPS)
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
    assert _bits_equal(A.flat_p[o:o + numel], before) and not opt.flat_v[o:o + numel].any()
    assert not torch.equal(A.flat_p[:o], others[:o])


def test_state_dict_round_trip_continues_bit_identically():
    """torch.optim.SGD's layout (`momentum_buffer` per parameter); a fresh optimizer on a fresh arena that loads it takes the next step bit for bit as
    the uninterrupted run does."""
    from clip_lite_amd.optim import FusedLARS
    M, A = _tiny()
    opt = FusedLARS(_groups(M), momentum=0.9, trust_coefficient=ETA, eps=EPS)
    for step in range(2):
        _write_grads(M, A, 40 + step, 0.01)
        opt.clip_grad_norm(1.0)
        opt.step()
    sd, p_saved = copy.deepcopy(opt.state_dict()), A.flat_p.clone()
    assert set(sd["state"][0]) == {"momentum_buffer"} and len(sd["state"]) == len(sd["param_groups"]) == 8
    assert sd["state"][3]["momentum_buffer"].shape == (8, 4, 3, 3)
    M2, A2 = _tiny()
    A2.flat_p.copy_(p_saved)
    A2.refresh_lowp()
    opt2 = FusedLARS(_groups(M2), momentum=0.9, trust_coefficient=ETA, eps=EPS)
    opt2.load_state_dict(sd)
    assert _bits_equal(opt2.flat_v, opt.flat_v)
    for (m, a, o) in ((M, A, opt), (M2, A2, opt2)):
        _write_grads(m, a, 42, 0.01)
        o.clip_grad_norm(1.0)
        o.step()
    torch.cuda.synchronize()
    assert _bits_equal(A.flat_p, A2.flat_p) and _bits_equal(opt.flat_v, opt2.flat_v) and torch.equal(A.flat_lp.view(torch.int16), A2.flat_lp.view(torch.int16))
    assert not _bits_equal(A.flat_p, p_saved)


def test_optimizer_factory_builds_lookahead_over_fused_lars():
    from clip_lite_amd.config import Config
    from clip_lite_amd.factories import OptimizerFactory
    from clip_lite_amd.optim import FusedLARS, FusedSGD, Lookahead
    M, _ = _tiny()
    cfg = Config(override_list=["OPTIM.OPTIMIZER_NAME", "lars", "OPTIM.LARS.TRUST_COEFFICIENT", 0.002, "OPTIM.SGD_MOMENTUM", 0.8])
    opt = OptimizerFactory.from_config(cfg, M.named_parameters())
    assert isinstance(opt, Lookahead) and type(opt.optimizer) is FusedLARS and opt.k == cfg.OPTIM.LOOKAHEAD.STEPS
    inner = opt.optimizer
    assert inner.trust_coefficient == 0.002 and inner.eps == 1e-8 and inner.param_groups[0]["momentum"] == 0.8
    assert Config().OPTIM.LARS.TRUST_COEFFICIENT == 0.001 and Config().OPTIM.LARS.EPS == 1e-8
    M2, _ = _tiny()
    plain = OptimizerFactory.from_config(Config(override_list=["OPTIM.LOOKAHEAD.USE", False]), M2.named_parameters())
    assert type(plain) is FusedSGD


@pytest.mark.usefixtures("deterministic_reductions")
@pytest.mark.parametrize("second_views", [True, False])
def test_lars_smoke_config_captured_step_tracks_eager_and_repeats_bitwise(second_views):
    """configs/smoke_random_lars.yaml (at 64-pixel crops and batch 8) through TrainStep as train_loop.main builds it - the factories' model, LARS under
    Lookahead, the cosine schedule, clipping, defer_update - for four steps: eager, captured (two eager warm-up steps, the capture, two replays)
    and captured again. As configured, the batches carry the self-supervised second views, which TrainStep captures as ONE graph (the update is one
    launch over the whole table; defer_update is without effect there); with the second views switched off the same configuration takes the
    per-phase graphs, where the update is three span launches and the text encoder's and the heads' share is deferred to the next step. The bar
    of tests/test_gpu_train_step.py's captured-versus-eager run of the SGD step: every loss within 2e-3, the total parameter movement within 2 %
    (relative L2). The two captured runs end bit-identical."""
    from clip_lite_amd.config import Config
    from clip_lite_amd.factories import LRSchedulerFactory, OptimizerFactory, PretrainingDatasetFactory, PretrainingModelFactory
    from clip_lite_amd.optim import FusedLARS, Lookahead
    from clip_lite_amd.train_loop import TrainStep
    from clip_lite_amd.utils.common import GradScaler
    B = 8
    _C = Config(os.path.join(ROOT, "configs", "smoke_random_lars.yaml"), ["DATA.IMAGE_CROP_SIZE", 64, "DATA.GPU_AUGMENT_SOURCE_SIZE", 80, "OPTIM.BATCH_SIZE", B] +
                ([] if second_views else ["MODEL.VISUAL.SELF_SUPERVISED", False, "MODEL.TEXTUAL.SELF_SUPERVISED", False]))
    assert _C.OPTIM.OPTIMIZER_NAME == "lars"
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
        assert isinstance(opt, Lookahead) and type(opt.optimizer) is FusedLARS
        sched = LRSchedulerFactory.from_config(_C, opt)
        step = TrainStep(M, opt, sched, GradScaler(_C.AMP), _C.OPTIM.CLIP_GRAD_NORM, None, graph=graph, graph_warmup=2,
                         pad_to=int(_C.DATA.MAX_CAPTION_LENGTH), defer_update=True)
        losses = [step(batches[s % 3])["loss"].item() for s in range(4)]
        if graph:
            assert step.replays == 2 and step.eager_steps == 2, (step.replays, step.eager_steps)
            if second_views:
                assert step._g is not None and step._graphs is None and "aug_image_plan" in batches[0]
            else:
                assert step._graphs is not None and step._pending_rest
        else:
            assert step.replays == 0 and step.eager_steps == 4
        step.finish()
        torch.cuda.synchronize()
        A = M.runtime.arena
        assert not A.flat_g.any() and all(np.isfinite(l) for l in losses)
        assert opt.optimizer.norms.sum().item() > 0          # the per-tensor norms were taken
        results.append((losses, A.flat_p - p_init, A.flat_p.clone(), opt.optimizer.flat_v.clone()))
    (l0, d0, _, _), (l1, d1, p1, v1), (l2, _, p2, v2) = results
    print("LARSERR smoke config: losses eager", l0, "captured", l1)
    assert max(abs(a - b) for a, b in zip(l0, l1)) < 2e-3, (l0, l1)
    rel = ((d0 - d1).norm() / d0.norm()).item()
    print(f"LARSERR smoke config: parameter movement {d0.norm().item():.3e}, captured against eager {rel:.2e} of it")
    assert d0.norm().item() > 1e-3 and rel < 2e-2, (d0.norm().item(), rel)
    assert l1 == l2 and _bits_equal(p1, p2) and _bits_equal(v1, v2)
