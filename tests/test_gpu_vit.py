"""The ViT image tower on the MI355X (clip-lite_amd/vit.py, csrc/vit_ops.hip): the three streaming kernels, the tower against tests/vit_ref.py in
float64 (exact-f32 mode and bf16), the frozen / eval path, the train step of configs/smoke_random_vit.yaml eager and captured, and the
checkpoint round trip."""
import os

import numpy as np
import pytest
import torch

import vit_ref as R
from detfill import det_fill, det_tensor

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16, F32 = 0, 1
TD = {BF16: torch.bfloat16, F32: torch.float32}


def _hip():
    from clip_lite_amd import hip
    return hip


# ------------------------------------------------------------------------------------------------ the kernels
@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("H,W,p", [(64, 96, 32), (48, 32, 16)])
def test_patchify_is_unfold_in_c_i_j_order(dt, H, W, p):
    hip = _hip()
    B = 2
    img = torch.randn(B, 3, H, W, generator=torch.Generator().manual_seed(H + p))
    out = torch.full((B * (H // p) * (W // p), 3 * p * p), float("nan"), device="cuda", dtype=TD[dt])
    hip.vit_patchify(dt, img.cuda(), out, B, H, W, p)
    want = torch.nn.functional.unfold(img, p, stride=p).permute(0, 2, 1).reshape(out.shape)          # non-square: a row / column swap shows
    assert torch.equal(out.cpu(), want.to(TD[dt]))          # a copy: exact after the dtype cast


@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("C", [128, 768])
def test_tokens_forward_and_backward(dt, C):
    hip = _hip()
    B, P = 3, 6
    L = P + 1
    g = torch.Generator().manual_seed(C)
    e, cls, pos = (torch.randn(s, generator=g).to(TD[dt]) for s in ((B * P, C), (C,), (L, C)))
    s0 = torch.full((B * L, C), float("nan"), device="cuda", dtype=TD[dt])
    hip.vit_tokens_fwd(dt, e.cuda(), cls.cuda(), pos.cuda(), s0, B, P, C)
    want = R.tokens(e.double().view(B, P, C), cls.double(), pos.double()).reshape(B * L, C)
    assert torch.equal(s0.cpu(), want.float().to(TD[dt]))          # exact to one rounding of the sum (float64 -> f32 of two addends is the f32 sum)

    ds0 = torch.randn(B * L, C, generator=g).to(TD[dt])
    runs = []
    for _ in range(2):
        de = torch.full((B * P, C), float("nan"), device="cuda", dtype=TD[dt])
        dpos, dcls = torch.zeros(L, C, device="cuda"), torch.zeros(C, device="cuda")
        hip.vit_tokens_bwd(dt, ds0.cuda(), de, dpos, dcls, B, P, C)
        runs.append((de.cpu(), dpos.cpu(), dcls.cpu()))
    de, dpos, dcls = runs[0]
    d3 = ds0.view(B, L, C)
    assert torch.equal(de.view(B, P, C), d3[:, 1:])
    # f32-exact against float64 on the stored inputs: B - 1 = 2 additions per slot, each within half an ulp of its partial sum
    d64 = d3.double()
    tol = (B - 1) * torch.from_numpy(np.spacing(d64.abs().sum(0).float().numpy()))
    assert ((dpos.double() - d64.sum(0)).abs() <= tol).all() and ((dcls.double() - d64.sum(0)[0]).abs() <= tol[0]).all()
    assert torch.equal(dpos, (d3[0].float() + d3[1].float()) + d3[2].float()) and torch.equal(dcls, dpos[0])          # index order
    assert all(torch.equal(a, b) for a, b in zip(runs[0], runs[1]))          # bit-identical across two runs
    # ... in the deterministic mode too, and with the same bits (no atomics in either); the accumulators are added to
    hip.set_deterministic(True)
    try:
        dpos2, dcls2 = torch.ones(L, C, device="cuda"), torch.ones(C, device="cuda")
        hip.vit_tokens_bwd(dt, ds0.cuda(), torch.empty_like(de, device="cuda"), dpos2, dcls2, B, P, C)
    finally:
        hip.set_deterministic(False)
    assert torch.equal(dpos2.cpu(), 1.0 + dpos) and torch.equal(dcls2.cpu(), 1.0 + dcls)


@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_tokens_backward_in_unrolled_rounds_and_tail(dt):
    """B = 19: one round of 16 batch rows with all loads in flight, then 3 rows one by one - the same index order throughout"""
    hip = _hip()
    B, P, C = 19, 2, 128
    L = P + 1
    ds0 = torch.randn(B * L, C, generator=torch.Generator().manual_seed(19)).to(TD[dt])
    d3 = ds0.view(B, L, C).float()
    de = torch.full((B * P, C), float("nan"), device="cuda", dtype=TD[dt])
    dpos, dcls = torch.zeros(L, C, device="cuda"), torch.zeros(C, device="cuda")
    hip.vit_tokens_bwd(dt, ds0.cuda(), de, dpos, dcls, B, P, C)
    assert torch.equal(de.cpu().view(B, P, C), ds0.view(B, L, C)[:, 1:])
    seq = torch.zeros(L, C)
    for b in range(B):
        seq = seq + d3[b]
    assert torch.equal(dpos.cpu(), seq) and torch.equal(dcls.cpu(), seq[0])
    tol = (B - 1) * torch.from_numpy(np.spacing(d3.double().abs().sum(0).float().numpy()))
    assert ((dpos.cpu().double() - d3.double().sum(0)).abs() <= tol).all()


@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_class_rows_gather_and_scatter(dt):
    hip = _hip()
    B, L, C = 3, 7, 768
    x = torch.randn(B * L, C, generator=torch.Generator().manual_seed(3)).to(TD[dt])
    out = torch.full((B, C), float("nan"), device="cuda", dtype=TD[dt])
    hip.vit_class_gather(dt, x.cuda(), out, B, L, C)
    assert torch.equal(out.cpu(), x.view(B, L, C)[:, 0])
    dx = torch.zeros(B * L, C, device="cuda", dtype=TD[dt])
    hip.vit_class_scatter(dt, out, dx, B, L, C)
    want = torch.zeros(B, L, C, dtype=TD[dt])
    want[:, 0] = x.view(B, L, C)[:, 0]
    assert torch.equal(dx.cpu().view(B, L, C), want)


# ------------------------------------------------------------------------------------------------ the tower against float64
class _Holder(torch.nn.Module):
    """Gives a lone ImageEncoder the `image_encoder` slot the runtime looks for."""

    def __init__(self, enc):
        super().__init__()
        self.image_encoder = enc


def _fill(enc, salt="clite"):
    """det_fill by torchvision's key names: class_token, in_proj_bias and every other bias get non-zero values (their defaults are zero)."""
    det_fill(enc, salt)
    sd = enc.img_encoder.state_dict()
    assert all(v.abs().max() > 0 for v in sd.values())
    return enc


def _tower(layers, H, W, lowp, frozen=False, salt="clite", round_bf16=False):
    from clip_lite_amd.encoder import ImageEncoder
    from clip_lite_amd.model import attach_runtime
    enc = _fill(ImageEncoder("vit_b_32", image_size=(H, W), frozen=frozen, num_layers=layers), salt)
    if round_bf16:
        with torch.no_grad():
            for p in enc.parameters():
                p.copy_(R.round_to(p, torch.bfloat16))
    sd = {k: v.clone() for k, v in enc.img_encoder.state_dict().items()}
    holder = _Holder(enc).to("cuda")
    holder.rt = attach_runtime(holder, torch.device("cuda", torch.cuda.current_device()), lowp)
    return holder, sd


_REF = {}


def _reference(key, sd, image, layers, dfeat):
    """float64 features and gradients, computed once per case"""
    if key not in _REF:
        _REF[key] = R.features_and_grads(sd, image, layers, 12, dfeat)
    return _REF[key]


CASES = {"a_7_tokens": (1, 3, 64, 96), "b_37_tokens": (2, 3, 192, 192), "c_50_tokens": (1, 2, 224, 224)}


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.usefixtures("deterministic_reductions")
def test_f32_tower_matches_float64(case):
    """Exact-f32 mode, width 768, 12 heads: (a) the one-tile attention, (b) the four-key-tile kernels with a ragged second tile, (c) ViT-B/32's own
    50 tokens. The bounds tests/test_gpu_model.py / test_gpu_mpnet.py hold model-level f32 parity to: features within 1e-4 of max |ref|, every
    parameter's gradient within 2e-3 of its max, gradient norms within 2e-3 of max(norm, 1e-3 of the largest)."""
    layers, B, H, W = CASES[case]
    holder, sd = _tower(layers, H, W, lowp=False)
    holder.train()
    image, dfeat = det_tensor("image" + case, (B, 3, H, W), "normal"), det_tensor("dfeat" + case, (B, 768), "normal")
    feat = holder.image_encoder(image.cuda())
    feat.backward(dfeat.cuda())
    torch.cuda.synchronize()
    want, grads = _reference(case, sd, image, layers, dfeat)
    err = ((feat.detach().cpu().double() - want).abs().max() / want.abs().max()).item()
    print(f"{case}: features max |err| / max |ref| = {err:.3e}")
    assert err <= 1e-4
    named = dict(holder.image_encoder.img_encoder.named_parameters())
    assert sorted(named) == sorted(grads)
    gmax = max(g.norm().item() for g in grads.values())
    for k, p in named.items():
        got, g = p.grad.detach().cpu().double(), grads[k]
        assert got.shape == g.shape and g.abs().max() > 0, k
        assert (got - g).abs().max() <= 2e-3 * g.abs().max(), (k, ((got - g).abs().max() / g.abs().max()).item())
        assert abs(got.norm().item() - g.norm().item()) <= 2e-3 * max(g.norm().item(), 1e-3 * gmax), k


# Measured on the MI355X, case (b) on bf16-rounded parameters and input against float64, seeds 0 / 1 / 2 (bf16_figures below):
BF16_MEASURED_FWD = (9.805e-3, 7.809e-3, 1.1318e-2)          # max |features - ref| / max |ref|
BF16_MEASURED_COS = (0.99984142, 0.99990242, 0.99988271)     # cosine of the flattened parameter gradient
# The bounds: twice the worst forward error; and for the cosine twice the worst distance from 1. (Read to the letter, "halfway between the
# worst value and 1" is (worst + 1) / 2 = 0.99992: above the worst measured value itself, so the measurement it is derived from would fail it
# whatever the code does. The distance from 1 is the cosine's error, and twice the worst error is the rule the forward bound follows.)
BF16_FWD_BOUND = 2 * max(BF16_MEASURED_FWD)                  # 2.264e-2
BF16_COS_BOUND = 1 - 2 * (1 - min(BF16_MEASURED_COS))        # 0.99968


def bf16_figures(seed):
    """(forward error / max |ref|, cosine of the flattened parameter gradient) of case (b) in bf16 against float64 on the same bf16-rounded
    parameters and input"""
    layers, B, H, W = CASES["b_37_tokens"]
    holder, sd = _tower(layers, H, W, lowp=True, salt=f"bf16-{seed}", round_bf16=True)
    holder.train()
    image = R.round_to(det_tensor(f"image-bf16-{seed}", (B, 3, H, W), "normal"), torch.bfloat16)
    dfeat = R.round_to(det_tensor(f"dfeat-bf16-{seed}", (B, 768), "normal"), torch.bfloat16)
    feat = holder.image_encoder(image.cuda())
    feat.backward(dfeat.cuda().to(feat.dtype))
    torch.cuda.synchronize()
    want, grads = _reference(("bf16", seed), sd, image, layers, dfeat)
    fwd = ((feat.detach().cpu().double() - want).abs().max() / want.abs().max()).item()
    named = dict(holder.image_encoder.img_encoder.named_parameters())
    a = torch.cat([named[k].grad.detach().cpu().double().flatten() for k in sorted(named)])
    b = torch.cat([grads[k].flatten() for k in sorted(named)])
    return fwd, (a @ b / (a.norm() * b.norm())).item()


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_bf16_tower_tracks_float64(seed):
    """bf16 mode, case (b): 2 layers, B = 3, 37 tokens. Measured on the MI355X (seeds 0, 1, 2): forward error / max |ref| 9.8e-3, 7.8e-3,
    1.13e-2; gradient cosine 0.999841, 0.999902, 0.999883. Bounds: twice the worst error (2.26e-2), and for the cosine twice the worst distance
    from 1 (0.99968; see BF16_COS_BOUND for why not the midpoint) - and never below the 0.93 the project holds the whole-model bf16 backward to."""
    fwd, cos = bf16_figures(seed)
    print(f"bf16 seed {seed}: forward error {fwd:.4e}, gradient cosine {cos:.6f}")
    assert fwd <= BF16_FWD_BOUND
    assert cos >= BF16_COS_BOUND and cos >= 0.93


# ------------------------------------------------------------------------------------------------ frozen and eval
@pytest.mark.parametrize("lowp", [False, True], ids=["f32", "bf16"])
def test_frozen_encoder_equals_eval_mode_and_writes_no_gradients(lowp):
    H = W = 96
    image = det_tensor("frozen-image", (3, 3, H, W), "normal").cuda()
    trainable, _ = _tower(1, H, W, lowp)
    trainable.eval()
    with torch.no_grad():
        want = trainable.image_encoder(image)
    frozen, _ = _tower(1, H, W, lowp, frozen=True)
    frozen.train()          # (ImageEncoder.frozen keeps the tower in eval mode whatever train() says)
    got = frozen.image_encoder(image)
    torch.cuda.synchronize()
    assert not got.requires_grad and torch.equal(got, want)
    assert all(not p.requires_grad for p in frozen.image_encoder.parameters())
    assert frozen.rt.arena.flat_g.abs().max().item() == 0
    # the trainable tower in train mode computes the same features (no BatchNorm, no dropout) and does write gradients
    trainable.train()
    feat = trainable.image_encoder(image)
    assert feat.requires_grad and torch.equal(feat.detach(), want)
    feat.backward(torch.ones_like(feat))
    torch.cuda.synchronize()
    assert trainable.rt.arena.flat_g.abs().max().item() > 0


# ------------------------------------------------------------------------------------------------ the train step of configs/smoke_random_vit.yaml
_BATCHES = {}


def _batches_of(c):
    """the config's own dataset and collate: 6 batches (computed once, shared by the runs)"""
    from clip_lite_amd.factories import PretrainingDatasetFactory
    key = (c.OPTIM.BATCH_SIZE, c.DATA.IMAGE_CROP_SIZE)
    if key not in _BATCHES:
        ds = PretrainingDatasetFactory.from_config(c, split="train")
        B = c.OPTIM.BATCH_SIZE
        _BATCHES[key] = [ds.collate_fn([ds[i * B + j] for j in range(B)]) for i in range(c.OPTIM.NUM_ITERATIONS)]
        for b in _BATCHES[key]:
            b.pop("image_id", None)
    return _BATCHES[key]


def _run_config(graph, overrides, steps):
    """train_loop.main's objects for the config; returns (losses, model, step, the image tower's initial state)"""
    from clip_lite_amd.config import Config
    from clip_lite_amd.factories import LRSchedulerFactory, OptimizerFactory, PretrainingModelFactory
    from clip_lite_amd.train_loop import TrainStep
    from clip_lite_amd.utils.common import GradScaler
    from clip_lite_amd.vit import VisionTransformer
    c = Config(os.path.join(ROOT, "configs", "smoke_random_vit.yaml"), overrides)
    batches = _batches_of(c)
    torch.manual_seed(7)          # (behind the dataset: every run starts from the same parameters and the same dropout seeds)
    model = PretrainingModelFactory.from_config(c).to("cuda").train()
    assert isinstance(model.image_encoder.img_encoder, VisionTransformer) and model.image_encoder.img_encoder.seq_length == 5
    optimizer = OptimizerFactory.from_config(c, model.named_parameters())
    decay = {id(p): g["weight_decay"] for g in optimizer.param_groups for p in g["params"]}
    vt = model.image_encoder.img_encoder
    assert decay[id(vt.class_token)] == 0.0 and decay[id(vt.encoder.pos_embedding)] == 0.0 and decay[id(vt.conv_proj.weight)] > 0          # OPTIM.NO_DECAY
    init = {k: v.detach().clone() for k, v in vt.state_dict().items()}
    scheduler = LRSchedulerFactory.from_config(c, optimizer)
    step = TrainStep(model, optimizer, scheduler, GradScaler(enabled=c.AMP), c.OPTIM.CLIP_GRAD_NORM, None, graph=graph, graph_warmup=2,
                     defer_update=True)
    assert not step._direct_ok()          # a ViT model takes the one-graph capture
    losses = [step({k: v.cuda() for k, v in batches[s].items()})["loss"].item() for s in range(steps)]
    step.finish()
    torch.cuda.synchronize()
    return losses, model, step, init


def test_config_runs_three_eager_steps():
    """configs/smoke_random_vit.yaml as it is (bf16), launched eagerly: a finite, changing loss, and every ViT tensor moves."""
    losses, model, step, init = _run_config(False, [], 3)
    print("eager losses", losses)
    assert all(np.isfinite(losses)) and len(set(losses)) == 3 and step.eager_steps == 3 and step.replays == 0
    for k, v in model.image_encoder.img_encoder.state_dict().items():
        assert torch.isfinite(v).all() and not torch.equal(v, init[k]), k


@pytest.mark.usefixtures("deterministic_reductions")
def test_captured_step_is_bit_identical_to_eager_steps():
    """graph=True takes TrainStep._capture_single (replays > 0, no per-phase graphs), and in the deterministic mode the replayed steps leave
    bit-identical parameters to the same six steps launched eagerly: same kernels, same arguments, the device-side dropout seeds continuing the
    host sequence. Exact-f32 kernels, as in the MPNet captured-step test (in bf16 the eager step groups its weight gradients into one launch and
    the captured one launches them in line: other kernels, other summation orders)."""
    ov = ["AMP", False]
    (l0, m0, s0, _), (l1, m1, s1, _) = (_run_config(graph, ov, 6) for graph in (False, True))
    print("eager", l0, "captured", l1)
    assert s0.replays == 0 and s0.eager_steps == 6
    assert s1.replays == 4 and s1.eager_steps == 2 and s1._g is not None and s1._graphs is None
    assert all(np.isfinite(l1)) and len(set(l1)) >= 3
    assert l0 == l1
    assert torch.equal(m0.runtime.arena.flat_p, m1.runtime.arena.flat_p)
    assert not torch.equal(m0.runtime.arena.flat_p, torch.zeros_like(m0.runtime.arena.flat_p))


# ------------------------------------------------------------------------------------------------ checkpoint
def test_state_dict_round_trip_reproduces_the_features_bit_for_bit():
    from clip_lite_amd.config import Config
    from clip_lite_amd.factories import PretrainingModelFactory
    c = Config(os.path.join(ROOT, "configs", "smoke_random_vit.yaml"), [])
    image = det_tensor("ckpt-image", (4, 3, 64, 64), "normal").cuda()
    torch.manual_seed(1)
    M1 = PretrainingModelFactory.from_config(c)
    _fill(M1.image_encoder)
    M1 = M1.to("cuda").eval()
    sd = {k: v.detach().cpu().clone() for k, v in M1.state_dict().items()}
    w = sd["image_encoder.img_encoder.conv_proj.weight"]
    assert tuple(w.shape) == (768, 3, 32, 32) and w.is_contiguous()
    assert tuple(sd["image_encoder.img_encoder.class_token"].shape) == (1, 1, 768)
    torch.manual_seed(2)
    M2 = PretrainingModelFactory.from_config(c).to("cuda").eval()
    with torch.no_grad():
        f1 = M1.image_encoder(image)
        assert not torch.equal(M2.image_encoder(image), f1)          # another initialisation
        M2.load_state_dict(sd)
        f2 = M2.image_encoder(image)
    torch.cuda.synchronize()
    assert torch.isfinite(f1).all() and torch.equal(f1, f2)
    for k, v in M2.state_dict().items():
        assert torch.equal(v.cpu(), sd[k]), k
