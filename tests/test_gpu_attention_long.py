"""GPU tests of captions of 33..128 tokens: the attention kernels through the C ABI against tests/attention_long_ref.py in float64 (the shapes and
bounds of tests/test_wavesim_attention_long.py at bench-like head counts), and the layers above them — padding invariance of the loss and the
text-encoder gradients, parity with the oracle at L = 48, a step captured at pad_to = 64 against the eager run, and the refusals with their
messages.

Bounds: kernels as tests/test_gpu_ops.py (f32 1e-5 of max|ref|; bf16 1e-2 forward, 2e-2 backward); padding invariance 1e-5 relative (the loss, and
per text-encoder tensor the largest gradient difference over the tensor's largest gradient: the padded columns add exact zeros to every sum, so
only the f32 summation order of the longer reductions differs); oracle parity as tests/test_gpu_model.py's fixture tests (loss 1e-4, gradient
norms 2e-3)."""
import pytest
import torch

import attention_long_ref as R
from detfill import det_fill, det_tensor

pytestmark = pytest.mark.gpu
BF16, F32 = 0, 1
TOL = {BF16: (1e-2, 2e-2), F32: (1e-5, 1e-5)}


def _hip():
    from clip_lite_amd import hip
    return hip


def _problem(B, L, H, seed):
    g = torch.Generator().manual_seed(seed)
    qkv = (torch.randn(B * L, 3 * H * 64, generator=g) * 0.7).bfloat16().float()
    dctx = torch.randn(B * L, H * 64, generator=g).bfloat16().float()
    return qkv, dctx, R.masks(B, L, seed)


def _run(dtype, qkv, mask, dctx, B, L, H, drop=None, backward=True):
    hip = _hip()
    td = torch.bfloat16 if dtype == BF16 else torch.float32
    q, m = qkv.to("cuda", td).contiguous(), mask.cuda()
    ctx = torch.empty(B * L, H * 64, device="cuda", dtype=td)
    args = () if drop is None else (drop,)
    hip.attention_fwd(dtype, q, m, ctx, B, L, H, *args)
    dqkv = None
    if backward:
        dqkv = torch.empty_like(q)
        hip.attention_bwd(dtype, q, m, dctx.to("cuda", td).contiguous(), dqkv, B, L, H, *args)
        dqkv = dqkv.float().cpu()
    return ctx.float().cpu(), dqkv


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("B,L,H", [(5, 33, 12), (3, 64, 4), (2, 100, 12), (4, 128, 12)])
def test_kernels_match_float64(dtype, B, L, H):
    qkv, dctx, mask = _problem(B, L, H, L)
    ref_ctx, ref_dqkv = R.reference(qkv, mask, dctx, B, L, H)
    ctx, dqkv = _run(dtype, qkv, mask, dctx, B, L, H)
    ef, eb = R.rel_err(ctx, ref_ctx), R.rel_err(dqkv, ref_dqkv)
    print(f"dtype {dtype} (B, L, H) = {(B, L, H)}: forward {ef:.3e}, backward {eb:.3e}")
    assert ef < TOL[dtype][0]
    assert eb < TOL[dtype][1]
    again = _run(dtype, qkv, mask, dctx, B, L, H)
    assert torch.equal(again[0], ctx) and torch.equal(again[1], dqkv)      # no atomics, fixed order: the same bits


def test_dropout_same_mask_in_both_families_and_directions():
    """p = 0.1 at (6, 80, 4): the multipliers recovered from the exact-f32 forward through two one-hot probes of V (keys 0..63, then 64..79) are
    0 or 1/0.9 at a keep rate within 0.02 of 0.9, and the float64 reference with that mask matches forward and backward of both families."""
    B, L, H, p = 6, 80, 4, 0.1
    drop = (p, 1234567, 9)
    qkv, dctx, _ = _problem(B, L, H, 80)
    mask = torch.ones(B, L, dtype=torch.long)
    mask[2, 70:] = 0
    outs = []
    for j0 in (0, 64):
        probe = R.one_hot_probe(qkv, B, L, H, j0)
        outs.append(_run(F32, probe, mask, dctx, B, L, H, drop, backward=False)[0])
        outs.append(_run(F32, probe, mask, dctx, B, L, H, backward=False)[0])
    mult, _ = R.multipliers(outs[0], outs[1], outs[2], outs[3], B, L, H, p)
    assert (((mult - 1 / 0.9).abs() < 1e-3) | (mult.abs() < 1e-6)).all()
    keep = (mult > 0.5).double().mean().item()
    assert abs(keep - 0.9) < 0.02, keep
    ref_ctx, ref_dqkv = R.reference(qkv, mask, dctx, B, L, H, keep=(mult > 0.5).double() / 0.9)
    for dtype in (BF16, F32):
        ctx, dqkv = _run(dtype, qkv, mask, dctx, B, L, H, drop)
        ef, eb = R.rel_err(ctx, ref_ctx), R.rel_err(dqkv, ref_dqkv)
        print(f"dropout, dtype {dtype}: forward {ef:.3e}, backward {eb:.3e}")
        assert ef < TOL[dtype][0] and eb < TOL[dtype][1], (dtype, ef, eb)


def _model(lowp=False, dropout=False):
    from clip_lite_amd.encoder import ImageEncoder, TextEncoder
    from clip_lite_amd.loss import JSDInfoMaxLoss
    from clip_lite_amd.model import VLInfoModel
    te = TextEncoder(mode="train_sbert", num_hidden_layers=2)
    if not dropout:
        te.strans.hidden_dropout_prob = te.strans.attention_probs_dropout_prob = 0.0
    return det_fill(VLInfoModel(te, ImageEncoder("resnet18"), JSDInfoMaxLoss(512, 768, "dot", 0.1, True, True), "train_sbert", is_amp=lowp)).to("cuda").train()


def _captions(B, L, lens, seed):
    ids = torch.randint(1000, 30522, (B, L), generator=torch.Generator().manual_seed(seed))
    ids[:, 0] = 101
    mask = (torch.arange(L)[None, :] < torch.tensor(lens)[:, None]).long()
    for b, n in enumerate(lens):
        ids[b, n - 1] = 102 if n > 1 else 101
    ids[mask == 0] = 0
    return ids, mask


@pytest.mark.usefixtures("deterministic_reductions")
def test_padding_to_64_and_128_changes_nothing():
    """ResNet-18 + 2 BERT layers, 64-pixel images, B = 4, exact-f32 kernels, dropout off: a batch whose longest caption has 40 tokens gives the
    same loss and text-encoder gradients padded to 40, 64 and 128 columns (three kernel instantiations: two, two and four key tiles)."""
    B = 4
    ids, mask = _captions(B, 40, [40, 1, 33, 17], 3)
    image = det_tensor("plimg", (B, 3, 64, 64), "normal").cuda()
    u = (det_tensor("plu1", (B, 512), "uniform").cuda(), det_tensor("plu2", (B, 768), "uniform").cuda())
    runs = []
    for L in (40, 64, 128):
        pi, pm = torch.zeros(B, L, dtype=torch.long), torch.zeros(B, L, dtype=torch.long)
        pi[:, :40], pm[:, :40] = ids, mask
        M = _model()          # the same deterministic fill every time
        M.loss.set_prior_noise(*u)
        out = M({"image": image, "input_ids": pi.cuda(), "attention_mask": pm.cuda()})
        out["loss"].backward()
        torch.cuda.synchronize()
        runs.append((out["loss"].item(), {n: p.grad.detach().double().cpu().clone() for n, p in M.named_parameters() if n.startswith("text_encoder.")}))
    l0, g0 = runs[0]
    assert len(g0) > 30 and max(g.abs().max().item() for g in g0.values()) > 0
    for L, (l1, g1) in zip((64, 128), runs[1:]):
        worst = max(((g1[n] - g0[n]).abs().max().item() / max(g0[n].abs().max().item(), 1e-30), n) for n in g0 if g0[n].abs().max().item() > 0)
        print(f"pad {L}: loss {l1:.8f} vs {l0:.8f}; worst gradient {worst[0]:.3e} ({worst[1]})")
        assert abs(l1 - l0) <= 1e-5 * abs(l0), (L, l0, l1)
        assert worst[0] <= 1e-5, (L, worst)
        for n in g0:
            if g0[n].abs().max().item() == 0:
                assert g1[n].abs().max().item() == 0, n


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.usefixtures("deterministic_reductions")
def test_f32_model_at_48_tokens_matches_oracle(ragged):
    """The small model of tests/test_gpu_model.py at L = 48 (two key tiles, the second ragged) against oracle/ref_model.py: one short row, or every
    caption its own length (1, 6, 11, 16). Loss within 1e-4; every parameter's gradient norm within 2e-3 of the float64 evaluation's."""
    from test_gpu_model import run_case
    M, Mo, Md, out, ref = run_case("resnet18", "train_sbert", 2, False, 4, 64, 48, 512, ragged=ragged)
    assert abs(out["loss"].item() - ref["loss"].item()) < 1e-4, (out["loss"].item(), ref["loss"].item())
    truth = {k: p.grad.norm().item() for k, p in Md.named_parameters()}
    gmax = max(truth.values())
    for k, p in M.named_parameters():
        got = p.grad.detach().double().norm().item()
        assert abs(got - truth[k]) <= 2e-3 * max(truth[k], 1e-3 * gmax), (k, got, truth[k])


def test_step_captured_at_64_tokens_replays_the_eager_bits(deterministic_reductions):
    """TrainStep(pad_to=64) in the deterministic mode, exact-f32 kernels, dropout and prior noise on, three steps on 64-column batches: the
    captured run (one eager warm-up step, the capture, a replay) gives the losses and parameters of the eager run bit for bit. A 65-column batch
    does not fit the captured step and takes the eager path (TrainStep._fits), on the 65-token kernels."""
    from clip_lite_amd.optim import FusedSGD, Lookahead
    from clip_lite_amd.optim.lr_scheduler import LinearWarmupCosineAnnealingLR
    from clip_lite_amd.train_loop import TrainStep
    from clip_lite_amd.utils.common import GradScaler
    B, L = 8, 64
    batches = []
    for i in range(3):
        ids, mask = _captions(B, L, [64, 40, 33, 64, 5, 1, 50, 64 - i], 20 + i)
        batches.append({"image": det_tensor(f"climg{i}", (B, 3, 64, 64), "normal").cuda(), "input_ids": ids.cuda(), "attention_mask": mask.cuda()})
    res = []
    for graph in (False, True):
        torch.manual_seed(7)
        M = _model(dropout=True)
        groups = [{"params": [p], "lr": 1e-3 if "image_encoder" in n else 1e-4, "weight_decay": 1e-4} for n, p in M.named_parameters()]
        opt = Lookahead(FusedSGD(groups, momentum=0.9), k=3, alpha=0.5)
        sched = LinearWarmupCosineAnnealingLR(opt, total_steps=40, warmup_steps=3)
        step = TrainStep(M, opt, sched, GradScaler(True), 10.0, None, graph=graph, graph_warmup=1, pad_to=L)
        losses = [step(b)["loss"].item() for b in batches]
        step.finish()
        torch.cuda.synchronize()
        if graph:
            assert step.eager_steps == 1 and step.replays == 2, (step.eager_steps, step.replays)
        res.append((losses, M.runtime.arena.flat_p.clone()))
    (l0, p0), (l1, p1) = res
    print(f"eager {l0}\ncaptured {l1}\nparameters differ in {(p0 != p1).sum().item()} of {p0.numel()}")
    assert l0 == l1
    assert torch.equal(p0, p1)
    ids, mask = _captions(B, 65, [65, 40, 33, 64, 5, 1, 50, 65], 30)
    before = step.eager_steps
    out = step({"image": batches[0]["image"], "input_ids": ids.cuda(), "attention_mask": mask.cuda()})
    torch.cuda.synchronize()
    assert step.eager_steps == before + 1 and torch.isfinite(out["loss"]).item()


class _Holder(torch.nn.Module):
    def __init__(self, te):
        super().__init__()
        self.text_encoder = te


def _tower(lowp, **kw):
    from clip_lite_amd.encoder import TextEncoder
    from clip_lite_amd.model import attach_runtime
    te = TextEncoder(mode="train_sbert", num_hidden_layers=1, **kw)
    holder = _Holder(det_fill(te)).to("cuda").train()
    return te, attach_runtime(holder, torch.device("cuda", torch.cuda.current_device()), lowp)


def _forward(te, rt, L, pad=0):
    from clip_lite_amd.bert import bert_forward
    ids = torch.full((2, L), 2000, dtype=torch.long, device="cuda")
    ids[1, L - 3:] = pad
    with torch.no_grad():
        return bert_forward(rt, te.strans, ids, (ids != pad).long(), rt.next_step(False))[0]


def test_refusals_name_their_limits():
    te, rt = _tower(False)
    assert torch.isfinite(_forward(te, rt, 128).float()).all()
    with pytest.raises(RuntimeError, match="at most 128 tokens"):
        _forward(te, rt, 129)
    hip = _hip()
    q = torch.zeros(2 * 129, 3 * 64, device="cuda")
    with pytest.raises(RuntimeError):
        hip.attention_fwd(F32, q, None, torch.zeros(2 * 129, 64, device="cuda"), 2, 129, 1)
    mp, rtm = _tower(False, model_name="sentence-transformers/paraphrase-mpnet-base-v2")
    assert torch.isfinite(_forward(mp, rtm, 32, pad=1).float()).all()
    with pytest.raises(RuntimeError, match="MPNet text encoder supports captions of at most 32 tokens"):
        _forward(mp, rtm, 33, pad=1)
    t8, rt8 = _tower(True)
    rt8.fp8_text = True
    with pytest.raises(RuntimeError, match="fp8 forward .* at most 32 tokens"):
        _forward(t8, rt8, 40)
