"""GPU tests of the SigLIP pairwise sigmoid loss: the two kernels (csrc/siglip_ops.hip) through clip_lite_amd.hip with the shared checks of
tests/siglip_ref.py (float64 reference, the bounds of tests/loss_ref.py), the critic chain (loss.siglip_critic_fwd / _bwd) against float64 autograd,
and SigLIPLoss inside the train step: configs/smoke_random_siglip.yaml eager, captured and resumed, and a ResNet-18 + 1-layer BERT model whose
captured step takes the per-phase graphs and so loss.jsd_join.

Kernel shapes (B, ld, ldd), as tests/test_wavesim_siglip.py: (8, 8, 8) one live lane; (24, 32, 24) padded ld; (72, 72, 72) nine live lanes;
(136, 144, 136) ld > ldd; (520, 520, 520) in f32: lane 0 takes a second trip over the columns (the device build's grid cap of 2048 workgroups is
out of a test's reach: a second pass over the rows needs B > 8192, a 268 MB matrix; the simulator build caps at 128 and runs it).

The critic chain's bound is relative to the InfoNCE chain, which shares every kernel but the element-wise middle: INFONCE_CHAIN holds that chain's
errors measured the same way (infonce_chain_figures below: same shapes, same stored inputs, against loss_ref.infonce_ref composed with float64
normalisation; error over max|ref|), and SigLIP is held to twice each. dbias has no InfoNCE counterpart; it is the sum dtemp is without the
factor t C[i][j], |t C| <= 10 at the initial temperature, and is held to twice the dtemp figure."""
import os
import types

import numpy as np
import pytest
import torch

import loss_ref as R
import siglip_ref as S
from loss_backends import BF16, F32

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "configs", "smoke_random_siglip.yaml")
DTS = [BF16, F32]
SHAPES = [(8, 8, 8), (24, 32, 24), (72, 72, 72), (136, 144, 136)]
POINTS = [(S.T_INIT, S.B_INIT), (S.T100, -3.0)]


@pytest.fixture(scope="module")
def be():
    return S.SiglipHipBackend()


# ------------------------------------------------------------------------------------------------ the kernels
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("t,b", POINTS)
@pytest.mark.parametrize("B,ld,ldd", SHAPES)
def test_siglip_matches_float64_and_repeats_bitwise(be, dt, B, ld, ldd, t, b):
    S.check_siglip(be, dt, B, ld, ldd, t, b, repeat=True)


@pytest.mark.parametrize("t,b", POINTS)
def test_siglip_second_column_sweep(be, t, b):
    S.check_siglip(be, F32, 520, 520, 520, t, b, repeat=True)


@pytest.mark.parametrize("dt", DTS)
def test_siglip_scalar_gradients_are_optional(be, dt):
    S.check_siglip_no_scalar_grads(be, dt)


def test_siglip_refusals(be):
    S.check_siglip_refusals(be)


# ------------------------------------------------------------------------------------------------ the critic chain
CHAIN = [(8, 64), (24, 128), (136, 2048)]
GOUT, SCALE = 1.0, 0.9

# infonce_chain_figures(B, U, dt) measured on the MI355X with the package of the commit before SigLIPLoss existed: error over max|ref| of
# (loss, df1, df2, dtemp). (The InfoNCE kernels add with float atomics, so a second run moves the last digits: dtemp at (8, 64) in f32 came out as
# 1.771e-06 and 1.859e-06. SigLIP's figures: at most 7.9e-07 in f32, and in bf16 at most 6.9e-03 on df1 / df2 and 5.1e-05 on the scalars; they repeat to the digit.)
INFONCE_CHAIN = {
    (F32, 8, 64): (6.519e-07, 6.295e-07, 5.85e-07, 1.771e-06),
    (F32, 24, 128): (5.7e-07, 7.909e-07, 6.758e-07, 8.732e-07),
    (F32, 136, 2048): (2.408e-07, 6.196e-06, 5.396e-06, 3.272e-07),
    (BF16, 8, 64): (0.0025, 0.004458, 0.004282, 0.0009568),
    (BF16, 24, 128): (0.000214, 0.004837, 0.007322, 0.0001111),
    (BF16, 136, 2048): (0.0001338, 0.009364, 0.007675, 9.383e-05),
}


def _chain_inputs(B, U, dt):
    rng = R._rng(B, U, 31)
    f1 = rng.standard_normal((B, U))
    f2 = rng.standard_normal((B, U)) + 0.5 * f1          # correlated: the diagonal cosines stand out
    return R.stored(f1, dt), R.stored(f2, dt)


class _Slots:
    """stands in for the parameter arena: one zeroed f32 gradient slot per parameter"""

    def __init__(self):
        self.slots = {}

    def g(self, p):
        return self.slots.setdefault(id(p), torch.zeros((), device="cuda", dtype=torch.float32))


def _stub_rt(dt):
    return types.SimpleNamespace(dt=dt, tdtype=torch.bfloat16 if dt == BF16 else torch.float32, device=torch.device("cuda"), arena=_Slots())


def _dev(x, dt):
    t = torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()
    return t.bfloat16() if dt == BF16 else t


def _rel(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(got - ref).max() / np.abs(ref).max())


def _normalized64(f):
    f = torch.tensor(np.asarray(f, np.float64), requires_grad=True)
    return f, f / f.norm(dim=1, keepdim=True).clamp_min(1e-12)


def infonce_chain_figures(B, U, dt):
    """The InfoNCE critic as loss.jsd_forward / jsd_backward launch it (l2_normalize -> gemm_nt -> infonce_fwd, infonce_bwd -> gemm_nn / gemm_tn ->
    l2_normalize_bwd) at the temperature it starts with, against float64 on the same stored inputs."""
    from clip_lite_amd import hip
    f1, f2 = _chain_inputs(B, U, dt)
    tdt = torch.bfloat16 if dt == BF16 else torch.float32
    d1, d2 = _dev(f1, dt), _dev(f2, dt)
    new = lambda *s: torch.empty(*s, device="cuda", dtype=tdt)
    temp = torch.tensor([R.T_CLIP], device="cuda")
    acc, gout, dtemp = torch.zeros(8, device="cuda"), torch.full((1,), GOUT, device="cuda"), torch.zeros(1, device="cuda")
    a, b, Cm, lse = new(B, U), new(B, U), torch.empty(B, B, device="cuda"), torch.empty(2, B, device="cuda")
    hip.l2_normalize(dt, d1, a, B, U)
    hip.l2_normalize(dt, d2, b, B, U)
    hip.gemm_nt(dt, a, b, B, B, U, hip.epilogue(Cm, B, out_f32=True))
    hip.infonce_fwd(Cm, B, B, temp, lse[0], lse[1], acc)
    dC, da, db, df1, df2 = new(B, B), new(B, U), new(B, U), new(B, U), new(B, U)
    hip.infonce_bwd(dt, Cm, B, B, temp, lse[0], lse[1], gout, SCALE, dC, B, dtemp)
    hip.gemm_nn(dt, dC, b, B, U, B, hip.epilogue(da, U))
    hip.gemm_tn(dt, dC, a, B, U, B, hip.epilogue(db, U))
    hip.l2_normalize_bwd(dt, d1, a, da, df1, B, U)
    hip.l2_normalize_bwd(dt, d2, b, db, df2, B, U)
    torch.cuda.synchronize()
    (x1, n1), (x2, n2) = _normalized64(f1), _normalized64(f2)
    t = torch.tensor(np.float64(np.float32(R.T_CLIP)), requires_grad=True)
    sr, sc, _ = R.infonce_loss(n1 @ n2.T, t)
    g1, g2, gt = torch.autograd.grad((sr + sc) * GOUT * float(np.float32(SCALE)), (x1, x2, t))
    return (_rel(acc[0].item() + acc[1].item(), (sr + sc).item()), _rel(df1.float().cpu().numpy(), g1.numpy()),
            _rel(df2.float().cpu().numpy(), g2.numpy()), _rel(dtemp.item(), gt.item()))


def siglip_chain_figures(B, U, dt):
    """loss.siglip_critic_fwd / _bwd at the initial temperature and bias: error over max|ref| of (loss, df1, df2, dtemp, dbias)."""
    from clip_lite_amd import loss as L
    f1, f2 = _chain_inputs(B, U, dt)
    rt = _stub_rt(dt)
    gd = types.SimpleNamespace(temperature=torch.tensor(S.T_INIT, device="cuda"), bias=torch.tensor(S.B_INIT, device="cuda"))
    acc, gout = torch.zeros(8, device="cuda"), torch.full((1,), GOUT, device="cuda")
    d1, d2 = _dev(f1, dt), _dev(f2, dt)
    work = L.siglip_critic_fwd(rt, gd, d1, d2, acc)
    df1, df2 = L.siglip_critic_bwd(rt, gd, d1, d2, work, gout, SCALE)
    torch.cuda.synchronize()
    assert acc[1:].abs().max().item() == 0 and df1.dtype == rt.tdtype and tuple(df1.shape) == tuple(df2.shape) == (B, U)
    (x1, n1), (x2, n2) = _normalized64(f1), _normalized64(f2)
    t = torch.tensor(np.float64(np.float32(S.T_INIT)), requires_grad=True)
    b = torch.tensor(np.float64(S.B_INIT), requires_grad=True)
    loss = S.siglip_loss(n1 @ n2.T, t, b)[0]
    g1, g2, gt, gb = torch.autograd.grad(loss * GOUT * float(np.float32(SCALE)), (x1, x2, t, b))
    return (_rel(acc[0].item(), loss.item()), _rel(df1.float().cpu().numpy(), g1.numpy()), _rel(df2.float().cpu().numpy(), g2.numpy()),
            _rel(rt.arena.g(gd.temperature).item(), gt.item()), _rel(rt.arena.g(gd.bias).item(), gb.item()))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("B,U", CHAIN)
def test_critic_chain_against_float64_autograd(dt, B, U):
    got = siglip_chain_figures(B, U, dt)
    base = INFONCE_CHAIN[(dt, B, U)]
    print(f"CHAIN ({B}, {U}) {'bf16' if dt == BF16 else 'f32'}: siglip loss/df1/df2/dtemp/dbias " + " ".join(f"{v:.3e}" for v in got)
          + "  infonce loss/df1/df2/dtemp " + " ".join(f"{v:.3e}" for v in base))
    for name, v, ref in zip(("loss", "df1", "df2", "dtemp", "dbias"), got, base + (base[3],)):
        assert v <= 2 * ref, f"{name}: {v:.3e} > 2 x {ref:.3e}"


def test_batch_not_a_multiple_of_8_is_refused_by_name():
    from clip_lite_amd import loss as L
    rt = _stub_rt(F32)
    gd = types.SimpleNamespace(temperature=torch.tensor(S.T_INIT, device="cuda"), bias=torch.tensor(S.B_INIT, device="cuda"))
    f = torch.zeros(12, 64, device="cuda")
    with pytest.raises(RuntimeError, match="SigLIPLoss needs a batch that is a multiple of 8"):
        L.siglip_critic_fwd(rt, gd, f, f, torch.zeros(8, device="cuda"))


# ------------------------------------------------------------------------------------------------ the train step of configs/smoke_random_siglip.yaml
_BATCHES = {}


def _batches_of(c):
    """the config's own dataset and collate: 3 batches (computed once, shared by the runs), the captions right-padded to DATA.MAX_CAPTION_LENGTH
    columns as the captured step pads them, so that eager and captured steps see the same tensors"""
    from clip_lite_amd.factories import PretrainingDatasetFactory
    if "b" not in _BATCHES:
        ds = PretrainingDatasetFactory.from_config(c, split="train")
        B, W = c.OPTIM.BATCH_SIZE, int(c.DATA.MAX_CAPTION_LENGTH)
        _BATCHES["b"] = [ds.collate_fn([ds[i * B + j] for j in range(B)]) for i in range(3)]
        for b in _BATCHES["b"]:
            b.pop("image_id", None)
            for k in ("input_ids", "attention_mask"):
                w = torch.zeros(B, W, dtype=b[k].dtype)
                w[:, :b[k].shape[1]] = b[k]
                b[k] = w
    return _BATCHES["b"]


def _build(c, graph, seed=7):
    from clip_lite_amd.factories import LRSchedulerFactory, OptimizerFactory, PretrainingModelFactory
    from clip_lite_amd.loss import SigLIPLoss
    from clip_lite_amd.train_loop import TrainStep
    from clip_lite_amd.utils.common import GradScaler
    torch.manual_seed(seed)
    model = PretrainingModelFactory.from_config(c).to("cuda").train()
    assert type(model.loss) is SigLIPLoss
    optimizer = OptimizerFactory.from_config(c, model.named_parameters())
    decay = {id(p): g["weight_decay"] for g in optimizer.param_groups for p in g["params"]}
    assert decay[id(model.loss.global_d.bias)] == 0.0 and decay[id(model.loss.global_d.temperature)] == 0.0
    scheduler = LRSchedulerFactory.from_config(c, optimizer)
    scaler = GradScaler(enabled=c.AMP)
    step = TrainStep(model, optimizer, scheduler, scaler, c.OPTIM.CLIP_GRAD_NORM, None, graph=graph, graph_warmup=1,
                     pad_to=min(int(c.DATA.MAX_CAPTION_LENGTH), model.text_encoder.strans.context_length), defer_update=True)
    return model, optimizer, scheduler, scaler, step


def _run(step, batches, which):
    losses = [step({k: v.cuda() for k, v in batches[s].items()})["loss"].item() for s in which]
    step.finish()
    torch.cuda.synchronize()
    return losses


@pytest.mark.usefixtures("deterministic_reductions")
def test_config_three_steps_eager_and_captured_are_bit_identical():
    from clip_lite_amd.config import Config
    c = Config(CFG, ["AMP", False])
    batches = _batches_of(c)
    res = []
    for graph in (False, True):
        model, _, _, _, step = _build(c, graph)
        gd = model.loss.global_d
        b0, t0 = gd.bias.item(), gd.temperature.item()
        losses = _run(step, batches, range(3))
        assert (step.replays, step.eager_steps) == ((2, 1) if graph else (0, 3))
        assert gd.bias.item() != b0 and gd.temperature.item() != t0, "global_d.bias and global_d.temperature must both move"
        res.append((losses, model.runtime.arena.flat_p.clone(), gd.bias.item(), gd.temperature.item()))
    (l0, p0, b0, t0), (l1, p1, b1, t1) = res
    print("eager", l0, "captured", l1, "bias", b0, "temperature", t0)
    assert all(np.isfinite(l0)) and l0 == l1 and torch.equal(p0, p1) and (b0, t0) == (b1, t1)


@pytest.mark.usefixtures("deterministic_reductions")
def test_config_checkpoint_after_step_2_resumes_step_3_bit_for_bit(tmp_path):
    from clip_lite_amd.config import Config
    from clip_lite_amd.utils.checkpointing import CheckpointManager
    c = Config(CFG, ["AMP", False])
    batches = _batches_of(c)
    model, opt, sched, scaler, step = _build(c, False)
    _run(step, batches, range(2))
    CheckpointManager(str(tmp_path), model=model, optimizer=opt, scheduler=sched, scaler=scaler).step(2)
    ck = torch.load(tmp_path / "checkpoint_2.pth", weights_only=False)
    assert ck["model"]["loss.global_d.bias"].shape == () and ck["model"]["loss.global_d.bias"].item() != -10.0
    seeds_drawn = model.runtime.steps          # the runtime's seed counter (prior noise) is not checkpoint state: the resumed run continues it by hand
    want_loss = _run(step, batches, [2])
    want = model.runtime.arena.flat_p.clone()

    model2, opt2, sched2, scaler2, step2 = _build(c, False, seed=7)
    with torch.no_grad():
        for p in model2.parameters():
            p.add_(0.123)                       # make sure the load really restores
    assert CheckpointManager(model=model2, optimizer=opt2, scheduler=sched2, scaler=scaler2).load(str(tmp_path / "checkpoint_2.pth")) == 2
    model2.runtime.steps = seeds_drawn
    got_loss = _run(step2, batches, [2])
    assert got_loss == want_loss and torch.equal(model2.runtime.arena.flat_p, want)


@pytest.mark.usefixtures("deterministic_reductions")
def test_first_step_cross_modal_loss_is_the_reference_on_the_device_cosines(monkeypatch):
    from clip_lite_amd import hip
    from clip_lite_amd.config import Config
    c = Config(CFG, ["AMP", False])
    seen = []
    real = hip.siglip_fwd

    def spy(Cm, ld, B, temperature, bias, part, acc):
        seen.append((Cm.detach().cpu().numpy().copy(), temperature.item(), bias.item(), B, ld))
        real(Cm, ld, B, temperature, bias, part, acc)

    monkeypatch.setattr(hip, "siglip_fwd", spy)
    model, _, _, _, step = _build(c, False)
    out = step({k: v.cuda() for k, v in _batches_of(c)[0].items()})
    cross = out["loss_components"]["cross_modal_loss"].item()
    step.finish()
    torch.cuda.synchronize()
    assert len(seen) == 1
    Cm, t, b, B, ld = seen[0]
    assert B == ld == c.OPTIM.BATCH_SIZE and np.abs(Cm).max() <= 1 + 1e-5 and t == np.float32(np.log(10.0)) and b == -10.0
    ref = S.siglip_ref(Cm, np.float32(t), np.float32(b))
    R.scalar("first step cross_modal_loss", cross, ref.loss, ref.row_terms)


# ------------------------------------------------------------------------------------------------ ResNet-18 + 1-layer BERT: the per-phase graphs
def _rn18_run(loss_cls, graph, steps=3):
    from detfill import det_fill, det_tensor
    from clip_lite_amd.encoder import ImageEncoder, TextEncoder
    from clip_lite_amd.model import VLInfoModel
    from clip_lite_amd.optim import FusedSGD, Lookahead
    from clip_lite_amd.optim.lr_scheduler import LinearWarmupCosineAnnealingLR
    from clip_lite_amd.train_loop import TrainStep
    from clip_lite_amd.utils.common import GradScaler
    B, L = 8, 12
    batches = []
    for i in range(3):
        ids = torch.randint(1000, 30522, (B, L), generator=torch.Generator().manual_seed(i))
        batches.append({"image": det_tensor(f"gimg{i}", (B, 3, 64, 64), "normal").cuda(), "input_ids": ids.cuda(),
                        "attention_mask": torch.ones(B, L, dtype=torch.long).cuda()})
    torch.manual_seed(7)          # the runtime's base seed comes from torch.initial_seed()
    te = TextEncoder(mode="train_sbert", num_hidden_layers=1)
    M = det_fill(VLInfoModel(te, ImageEncoder("resnet18"), loss_cls(512, 768, "dot", 0.1, True, True), "train_sbert", is_amp=False)).to("cuda").train()
    groups = [{"params": [p], "lr": 1e-3 if "image_encoder" in n else 1e-4, "weight_decay": 1e-4} for n, p in M.named_parameters()]
    opt = Lookahead(FusedSGD(groups, momentum=0.9), k=5, alpha=0.5)
    sched = LinearWarmupCosineAnnealingLR(opt, total_steps=40, warmup_steps=1)
    step = TrainStep(M, opt, sched, GradScaler(False), 10.0, None, graph=graph, graph_warmup=1)
    losses = [step(batches[s % 3])["loss"].item() for s in range(steps)]
    step.finish()
    torch.cuda.synchronize()
    return losses, M, step


@pytest.mark.usefixtures("deterministic_reductions")
def test_resnet18_bert_per_phase_capture_goes_through_jsd_join_and_equals_eager(monkeypatch):
    from clip_lite_amd import loss as L
    from clip_lite_amd.loss import SigLIPLoss
    joins = []
    real = L.jsd_join

    def counting(rt, mod, *a, **k):
        joins.append(mod.estimator)
        return real(rt, mod, *a, **k)

    monkeypatch.setattr(L, "jsd_join", counting)
    l0, m0, s0 = _rn18_run(SigLIPLoss, False)
    assert joins == [] and s0.eager_steps == 3
    l1, m1, s1 = _rn18_run(SigLIPLoss, True)
    assert joins == ["siglip"] and s1._graphs is not None and s1.replays == 2          # one capture of the join, replayed with the phase graphs
    print("eager", l0, "captured", l1)
    gd = m1.loss.global_d
    assert gd.bias.item() != -10.0 and abs(gd.temperature.item() - np.log(10.0)) > 0
    assert all(np.isfinite(l0)) and l0 == l1
    assert torch.equal(m0.runtime.arena.flat_p, m1.runtime.arena.flat_p)
