"""GPU tests of the MPNet text tower (through the C ABI): attention with the relative-position bias in both kernel families and the bias
table's gradient, the bias build and its gradient reduce, the embedding with MPNet position ids, the masked mean pool, the whole tower and
model against fixtures the reference itself produced, and the captured train step of configs/smoke_random_mpnet.yaml.

References: tests/mpnet_ref.py in float64 on the same (bf16-rounded) inputs. Bounds are the ones tests/test_gpu_ops.py holds the attention
kernels to (f32 below 1e-5 relative, bf16 forward below 1e-2 and backward below 2e-2 of max|ref|) and the ones tests/test_gpu_model.py applies to
the reference's fixtures (loss within 1e-4; gradient norms within 2e-3 of max(norm, 1e-3 of the largest); stored gradients within 2e-3 of
their max), restated here."""
import os

import numpy as np
import pytest
import torch

import mpnet_ref as R
from detfill import det_fill

pytestmark = pytest.mark.gpu
BF16, F32 = 0, 1
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MPNET = "sentence-transformers/paraphrase-mpnet-base-v2"
TD = {BF16: torch.bfloat16, F32: torch.float32}


def _hip():
    from clip_lite_amd import hip
    return hip


def _rel(got, ref):
    return ((got.double().cpu() - ref.double().cpu()).abs().max() / ref.double().abs().max().clamp_min(1e-6)).item()


def _table():
    return torch.tensor(_hip().relative_position_buckets(), dtype=torch.int32, device="cuda")


def _attn_problem(B, L, H, seed):
    """bf16-rounded qkv / dctx, a ragged mask (first caption full, one of a single token), a bias of order 1"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    qkv = (torch.randn(B * L, 3 * H * 64, device="cuda", generator=g) * 0.7).bfloat16()
    dctx = torch.randn(B * L, H * 64, device="cuda", generator=g).bfloat16()
    bias = torch.randn(H, 32, 32, device="cuda", generator=g)
    lens = torch.randint(1, L + 1, (B,), generator=torch.Generator().manual_seed(L))
    lens[0], lens[-1] = L, 1
    mask = (torch.arange(L)[None, :] < lens[:, None]).long().cuda()
    return qkv, dctx, bias, mask


def _bucket_sums(dbias, L):
    """[H][L][L] gradient of the bias -> [32][H] gradient of the table: sum over the (i, j) of each bucket"""
    H = dbias.shape[0]
    out = torch.zeros(32, H, dtype=dbias.dtype)
    for i in range(L):
        for j in range(L):
            out[R.bucket(j - i)] += dbias[:, i, j]
    return out


def _attn_ref(qkv, dctx, bias, mask, B, L, H, keep=None):
    q = qkv.double().cpu().view(B, L, 3 * H * 64).requires_grad_(True)
    b = bias.double().cpu()[:, :L, :L].clone().requires_grad_(True)
    ctx = R.attention(q, mask.cpu(), b, H, keep=keep)
    ctx.backward(dctx.double().cpu().view(B, L, H * 64))
    return ctx.detach().view(B * L, H * 64), q.grad.view(B * L, 3 * H * 64), _bucket_sums(b.grad, L)


def _run_bias_kernels(dt, qkv, dctx, bias, mask, B, L, H, drop=None):
    hip = _hip()
    drop = drop or hip.NO_DROP
    x, d = qkv.to(TD[dt]), dctx.to(TD[dt])
    ctx = torch.empty(B * L, H * 64, device="cuda", dtype=TD[dt])
    hip.attention_bias_fwd(dt, x, mask, bias, ctx, B, L, H, drop)
    dqkv = torch.empty_like(x)
    partials = torch.full((B * H, 32), float("nan"), device="cuda")
    hip.attention_bias_bwd(dt, x, mask, bias, _table(), d, dqkv, partials, B, L, H, drop)
    drel = torch.zeros(32, H, device="cuda")
    hip.attention_bias_grad_reduce(partials, drel, B, H)
    torch.cuda.synchronize()
    return ctx, dqkv, drel


SHAPES = [(3, 7, 1), (2, 30, 2), (2, 32, 12)]      # B*H = 3 fills neither the 4-wave forward nor the 2-wave backward block; the full tile at 12 heads


@pytest.mark.parametrize("dt", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("B,L,H", SHAPES)
def test_attention_with_bias_matches_ref(dt, B, L, H):
    qkv, dctx, bias, mask = _attn_problem(B, L, H, 100 * B + L)
    ctx, dqkv, drel = _run_bias_kernels(dt, qkv, dctx, bias, mask, B, L, H)
    rctx, rdqkv, rdrel = _attn_ref(qkv, dctx, bias, mask, B, L, H)
    e = (_rel(ctx, rctx), _rel(dqkv, rdqkv), _rel(drel, rdrel))
    print(f"{'bf16' if dt == BF16 else 'f32'} B={B} L={L} H={H}: ctx {e[0]:.3e} dqkv {e[1]:.3e} drel {e[2]:.3e} (max|drel| {rdrel.abs().max():.3e})")
    assert torch.isfinite(drel).all()
    fwd, bwd = (1e-2, 2e-2) if dt == BF16 else (1e-5, 1e-5)
    assert e[0] < fwd and e[1] < bwd and e[2] < bwd
    # no float atomics on the bias-gradient path: a second run gives the same bits
    _, dqkv2, drel2 = _run_bias_kernels(dt, qkv, dctx, bias, mask, B, L, H)
    assert torch.equal(drel, drel2) and torch.equal(dqkv, dqkv2)


@pytest.mark.parametrize("dt", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("B,L,H", SHAPES)
def test_zero_bias_equals_the_kernels_without_bias_bitwise(dt, B, L, H):
    hip = _hip()
    qkv, dctx, _, mask = _attn_problem(B, L, H, 7 * B + L)
    for drop in (hip.NO_DROP, (0.1, 424242, 5)):
        ctx, dqkv, drel = _run_bias_kernels(dt, qkv, dctx, torch.zeros(H, 32, 32, device="cuda"), mask, B, L, H, drop)
        x, d = qkv.to(TD[dt]), dctx.to(TD[dt])
        ctx0, dqkv0 = torch.empty_like(ctx), torch.empty_like(dqkv)
        hip.attention_fwd(dt, x, mask, ctx0, B, L, H, drop)
        hip.attention_bwd(dt, x, mask, d, dqkv0, B, L, H, drop)
        assert torch.equal(ctx, ctx0) and torch.equal(dqkv, dqkv0)


def test_dropout_masks_are_those_of_the_kernels_without_bias():
    """Dropout ON: the mask is recovered from the existing f32 kernel (V = identity columns makes ctx the dropped probabilities: the method of
    test_gpu_ops.test_attention_mfma_dropout_masks_regenerate_in_backward); the reference with that mask and the bias must then match the
    forward and the backward of both bias kernels, which therefore regenerate the same mask."""
    hip = _hip()
    B, L, H = 2, 30, 2
    qkv, dctx, bias, _ = _attn_problem(B, L, H, 77)
    mask = torch.ones(B, L, dtype=torch.long, device="cuda")
    mask[1, 20:] = 0
    drop = (0.1, 1234567, 9)
    probe = qkv.float().view(B, L, 3, H, 64).clone()
    probe[:, :, 2] = 0
    for j in range(L):
        probe[:, j, 2, :, j] = 1.0
    probe = probe.view(B * L, 3 * H * 64).contiguous()
    pd, p0 = torch.empty(B * L, H * 64, device="cuda"), torch.empty(B * L, H * 64, device="cuda")
    hip.attention_fwd(F32, probe, mask, pd, B, L, H, drop)
    hip.attention_fwd(F32, probe, mask, p0, B, L, H)
    pd, p0 = pd.view(B, L, H, 64)[..., :L].permute(0, 2, 1, 3), p0.view(B, L, H, 64)[..., :L].permute(0, 2, 1, 3)
    mult = torch.where(p0 > 1e-20, pd / p0.clamp_min(1e-30), torch.full_like(p0, 1.0 / 0.9))
    assert abs((mult > 0.5).float().mean().item() - 0.9) < 0.03
    keep = ((mult > 0.5).double() / 0.9).cpu()
    rctx, rdqkv, rdrel = _attn_ref(qkv, dctx, bias, mask, B, L, H, keep=keep)
    for dt, fwd, bwd in ((BF16, 1e-2, 2e-2), (F32, 1e-5, 1e-5)):
        ctx, dqkv, drel = _run_bias_kernels(dt, qkv, dctx, bias, mask, B, L, H, drop)
        assert _rel(ctx, rctx) < fwd and _rel(dqkv, rdqkv) < bwd and _rel(drel, rdrel) < bwd


@pytest.mark.parametrize("L", [1, 7, 32])
def test_bias_build_and_gradient_reduce_are_exact(L):
    hip = _hip()
    H = 12
    g = torch.Generator(device="cuda").manual_seed(L)
    rel = torch.randn(32, H, device="cuda", generator=g)
    bias = torch.full((H, 32, 32), float("nan"), device="cuda")
    hip.attention_bias_build(rel, _table(), bias, H, L)
    want = torch.zeros(H, 32, 32, dtype=torch.float32)
    want[:, :L, :L] = R.position_bias(rel.cpu(), L)
    assert torch.equal(bias.cpu(), want)          # a gather: exact, and zero outside the L x L corner
    # the reduce over rows (layers x batch), on integer-valued partials so that every summation order gives the same f32
    for rows in (1, 5, 70):
        partials = torch.randint(-8, 9, (rows, H, 32), device="cuda", generator=g).float()
        drel = torch.randint(-3, 4, (32, H), device="cuda", generator=g).float()
        want = drel + partials.sum(0).t()
        hip.attention_bias_grad_reduce(partials, drel, rows, H)
        assert torch.equal(drel, want)


def _embed_problem():
    B, L, C = 3, 7, 768
    ids = torch.tensor([[5, 1, 1, 1, 1, 1, 1],             # captions of 1, 4 and 7 tokens, pad id 1 behind them
                        [0, 11, 12, 2, 1, 1, 1],
                        [0, 21, 1, 23, 24, 25, 2]])        # ... and a pad id in the middle: its position id is 1, the ones behind it keep counting
    return B, L, C, ids


@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_embedding_forward_with_mpnet_position_ids(dt):
    hip = _hip()
    B, L, C, ids = _embed_problem()
    vocab, max_pos = 64, 20
    g = torch.Generator().manual_seed(3)
    word, pos = torch.randn(vocab, C, generator=g).to(TD[dt]), torch.randn(max_pos, C, generator=g).to(TD[dt])
    pid = R.position_ids(ids)
    assert pid.tolist() == [[2, 1, 1, 1, 1, 1, 1], [2, 3, 4, 5, 1, 1, 1], [2, 3, 1, 4, 5, 6, 7]]
    out = torch.full((B * L, C), float("nan"), device="cuda", dtype=TD[dt])
    pids = torch.full((B * L,), -7, device="cuda", dtype=torch.int32)
    hip.embed_mpnet_fwd(dt, ids.cuda(), word.cuda(), pos.cuda(), out, pids, B * L, L, C, vocab, max_pos, 1)
    assert pids.cpu().view(B, L).tolist() == pid.tolist()
    want = (word.float()[ids] + pos.float()[pid]).view(B * L, C)
    if dt == F32:
        assert torch.equal(out.cpu(), want)          # one f32 add per element: exact
    else:
        assert torch.equal(out.cpu(), want.bfloat16())


@pytest.mark.usefixtures("deterministic_reductions")
@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_embedding_backward_skips_both_padding_rows_and_repeats_bitwise(dt):
    hip = _hip()
    assert hip.is_deterministic()
    B, L, C, ids = _embed_problem()
    vocab, max_pos = 64, 20
    pid = R.position_ids(ids)
    d = torch.randn(B * L, C, generator=torch.Generator().manual_seed(4)).to(TD[dt])
    runs = []
    for _ in range(2):
        dword, dpos = torch.zeros(vocab, C, device="cuda"), torch.zeros(max_pos, C, device="cuda")
        hip.embed_mpnet_bwd(dt, ids.cuda(), pid.to(torch.int32).cuda(), d.cuda(), dword, dpos, B * L, L, C, vocab, max_pos, 1)
        runs.append((dword.cpu(), dpos.cpu()))
    (dword, dpos), (dword2, dpos2) = runs
    assert torch.equal(dword, dword2) and torch.equal(dpos, dpos2)
    rw, rp = torch.zeros(vocab, C, dtype=torch.float64), torch.zeros(max_pos, C, dtype=torch.float64)
    rw.index_add_(0, ids.view(-1), d.double())
    rp.index_add_(0, pid.view(-1), d.double())
    assert rw[1].abs().max() > 0 and rp[1].abs().max() > 0          # the problem does send gradient towards both padding rows ...
    rw[1], rp[1] = 0, 0
    assert dword[1].abs().max() == 0 and dpos[1].abs().max() == 0          # ... and neither row accumulates it (nn.Embedding(padding_idx=1))
    assert _rel(dword, rw) < 1e-6 and _rel(dpos, rp) < 1e-6


@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_masked_mean_pool_forward_backward(dt):
    hip = _hip()
    B, L, C = 4, 7, 768
    g = torch.Generator().manual_seed(5)
    h = torch.randn(B, L, C, generator=g).to(TD[dt])
    dy = torch.randn(B, C, generator=g).to(TD[dt])
    mask = torch.zeros(B, L, dtype=torch.long)
    for b, n in enumerate((1, 3, 7, 0)):          # one row whose mask is all zero: its output is 0, not NaN
        mask[b, :n] = 1
    out = torch.full((B, C), float("nan"), device="cuda", dtype=TD[dt])
    inv = torch.full((B,), float("nan"), device="cuda")
    hip.mean_pool_fwd(dt, h.cuda(), mask.cuda(), out, inv, B, L, C)
    dh = torch.full((B, L, C), float("nan"), device="cuda", dtype=TD[dt])
    hip.mean_pool_bwd(dt, dy.cuda(), mask.cuda(), inv, dh, B, L, C)
    h64 = h.double().requires_grad_(True)
    ref = R.mean_pool(h64, mask)
    ref.backward(dy.double())
    out, dh = out.cpu().double(), dh.cpu().double()
    assert torch.isfinite(out).all() and torch.isfinite(dh).all() and out[3].abs().max() == 0 and dh[3].abs().max() == 0
    assert torch.allclose(inv.cpu(), torch.tensor([1.0, 1.0 / 3.0, 1.0 / 7.0, 1e9]), rtol=1e-6, atol=0)          # 1 / clamp(count, 1e-9)
    if dt == F32:
        assert (out - ref.detach()).abs().max() < 1e-6 * ref.abs().max() and (dh - h64.grad).abs().max() < 1e-6 * h64.grad.abs().max()
    else:
        # f32 accumulation of bf16 inputs, one rounding to bf16 at the store: half a bf16 ulp of each element - at most 2^-8 relative, bf16
        # keeping 8 significant bits - plus the f32 noise
        for got, want in ((out, ref.detach()), (dh, h64.grad)):
            assert ((got - want).abs() <= 2.0 ** -8 * want.abs() + 1e-6 * want.abs().max()).all()


# ------------------------------------------------------------------------------------------------ tower and model against the reference's fixtures
class _Holder(torch.nn.Module):
    """Gives a lone TextEncoder the `text_encoder` slot model.attach_runtime looks for."""

    def __init__(self, te):
        super().__init__()
        self.text_encoder = te


def _text_tower(layers):
    from clip_lite_amd.encoder import TextEncoder
    from clip_lite_amd.model import attach_runtime
    te = TextEncoder(mode="train_sbert", model_name=MPNET, num_hidden_layers=layers)
    te.strans.hidden_dropout_prob = te.strans.attention_probs_dropout_prob = 0.0
    det_fill(te)          # by the reference's key names ("strans. ..."), before the holder prefixes them
    holder = _Holder(te).to("cuda").train()
    holder.rt = attach_runtime(holder, torch.device("cuda", torch.cuda.current_device()), False)
    return holder


def _check_gnorms(g, fx, sfx=""):
    names = [str(n) for n in fx["gnames"]]
    assert sorted(g) == names
    gmax = float(fx["gnorms" + sfx].max())
    for n, ref in zip(names, fx["gnorms" + sfx]):
        assert abs(g[n].norm().item() - ref) <= 2e-3 * max(ref, 1e-3 * gmax), (n, g[n].norm().item(), ref)


@pytest.mark.parametrize("name,layers,mask", [("mpnet_l1_b3_len30", 1, "mask"), ("mpnet_l2_b4_len7_ragged", 2, "mask"), ("mpnet_l2_b4_len7_ragged", 2, "ones")])
@pytest.mark.usefixtures("deterministic_reductions")
def test_f32_tower_matches_reference_fixture(name, layers, mask):
    """Exact-f32 mode against the reference's own TextEncoder(model_name=<MPNet>): the pooled output within 1e-4, every gradient norm and the
    bias table's gradient under test_gpu_model's bounds. The ragged fixture also under the all-ones mask the reference's collate produces."""
    fx = dict(np.load(os.path.join(G, name + ".npz")))
    sfx = "_ones" if mask == "ones" else ""
    holder = _text_tower(layers)
    ids = torch.tensor(fx["ids"]).cuda()
    m = torch.ones_like(ids) if sfx else torch.tensor(fx["mask"]).cuda()
    out = holder.text_encoder({"input_ids": ids, "attention_mask": m})
    (out.float() * torch.tensor(fx["w"]).cuda()).sum().backward()
    torch.cuda.synchronize()
    err = (out.float().cpu() - torch.tensor(fx["out" + sfx])).abs().max().item()
    print(f"{name}{sfx}: max |out - reference| {err:.3e}")
    assert err < 1e-4
    g = {k: p.grad for k, p in holder.text_encoder.named_parameters() if p.requires_grad}
    _check_gnorms(g, fx, sfx)
    rel = g["strans.encoder.relative_attention_bias.weight"].cpu().numpy()
    assert np.abs(rel - fx["g_rel" + sfx]).max() <= 2e-3 * np.abs(fx["g_rel" + sfx]).max()
    pooler = [p for k, p in holder.text_encoder.named_parameters() if "pooler" in k]
    assert len(pooler) == 2 and all(p.grad.abs().max().item() == 0 for p in pooler)


@pytest.mark.usefixtures("deterministic_reductions")
def test_f32_model_matches_reference_fixture():
    """tests/test_gpu_model.py::test_f32_mode_matches_reference_golden with the 2-layer MPNet tower: fixture of the reference's own model.py /
    loss.py / encoder.TextEncoder."""
    from clip_lite_amd.encoder import ImageEncoder, TextEncoder
    from clip_lite_amd.loss import JSDInfoMaxLoss
    from clip_lite_amd.model import VLInfoModel
    fx = dict(np.load(os.path.join(G, "model_rn18_mpnet2_b4.npz")))
    te = TextEncoder(mode="train_sbert", model_name=MPNET, num_hidden_layers=2)
    te.strans.hidden_dropout_prob = te.strans.attention_probs_dropout_prob = 0.0
    M = det_fill(VLInfoModel(te, ImageEncoder("resnet18"), JSDInfoMaxLoss(512, 768, "dot", 0.1, True, True), "train_sbert", is_amp=False)).to("cuda").train()
    batch = {k: torch.tensor(fx[k]).cuda() for k in ("image", "input_ids", "attention_mask")}
    M.loss.set_prior_noise(torch.tensor(fx["u_img"]).cuda(), torch.tensor(fx["u_txt"]).cuda())
    out = M(batch)
    out["loss"].backward()
    assert abs(out["loss"].item() - float(fx["total"])) < 1e-4
    assert abs(out["loss_components"]["cross_modal_loss"].item() - float(fx["cross"])) < 1e-4
    g = {k: p.grad for k, p in M.named_parameters() if p.requires_grad}
    _check_gnorms(g, fx)
    c1 = g["image_encoder.img_encoder.conv1.weight"].float().cpu().numpy()
    assert np.abs(c1 - fx["g_conv1"]).max() <= 2e-3 * np.abs(fx["g_conv1"]).max()
    rel = g["text_encoder.strans.encoder.relative_attention_bias.weight"].cpu().numpy()
    assert np.abs(rel - fx["g_rel"]).max() <= 2e-3 * np.abs(fx["g_rel"]).max()


# ------------------------------------------------------------------------------------------------ the train step of configs/smoke_random_mpnet.yaml
def _run_config(graph, overrides, batches_of, pad=True):
    """train_loop.main's objects for the config, `len(batches)` steps; returns (losses, model, initial pooler / bias-table copies, the step).
    pad: capture at DATA.MAX_CAPTION_LENGTH as train_loop.main does (TrainStep pad_to)."""
    from clip_lite_amd.config import Config
    from clip_lite_amd.factories import LRSchedulerFactory, OptimizerFactory, PretrainingModelFactory
    from clip_lite_amd.train_loop import TrainStep
    from clip_lite_amd.utils.common import GradScaler
    torch.manual_seed(7)
    c = Config(os.path.join(ROOT, "configs", "smoke_random_mpnet.yaml"), overrides)
    batches = batches_of(c)
    model = PretrainingModelFactory.from_config(c).to("cuda").train()
    st = model.text_encoder.strans
    init = {k: v.detach().clone() for k, v in st.state_dict().items() if "pooler" in k or "relative_attention_bias" in k}
    optimizer = OptimizerFactory.from_config(c, model.named_parameters())
    scheduler = LRSchedulerFactory.from_config(c, optimizer)
    step = TrainStep(model, optimizer, scheduler, GradScaler(enabled=c.AMP), c.OPTIM.CLIP_GRAD_NORM, None, graph=graph, graph_warmup=2,
                     pad_to=min(int(c.DATA.MAX_CAPTION_LENGTH), 32) if pad else None, defer_update=True)
    losses = [step({k: v.cuda() for k, v in b.items()})["loss"].item() for b in batches]
    step.finish()
    torch.cuda.synchronize()
    return losses, model, init, step, c


_BATCHES = {}


def _batches_of(c):
    """the config's own dataset and collate: 6 batches (computed once, shared by the runs)"""
    from clip_lite_amd.factories import PretrainingDatasetFactory
    key = (c.OPTIM.BATCH_SIZE, c.DATA.IMAGE_CROP_SIZE)
    if key not in _BATCHES:
        ds = PretrainingDatasetFactory.from_config(c, split="train")
        assert ds.framing == "mpnet"
        B = c.OPTIM.BATCH_SIZE
        _BATCHES[key] = [ds.collate_fn([ds[i * B + j] for j in range(B)]) for i in range(c.OPTIM.NUM_ITERATIONS)]
        for b in _BATCHES[key]:
            b.pop("image_id", None)
            assert (b["input_ids"][b["attention_mask"] == 0] == 1).all()
    return _BATCHES[key]


def _check_step_run(losses, model, init, step, c, graph):
    assert c.OPTIM.NUM_ITERATIONS == 6 == len(losses) and all(np.isfinite(losses)), losses
    if graph:
        assert step._graphs is not None and step.replays == 4 and step.eager_steps == 2          # the per-phase captured step took over after the warm-up
    sd = model.text_encoder.strans.state_dict()
    assert c.OPTIM.WEIGHT_DECAY > 0
    for k, v in init.items():
        if "pooler" in k:
            assert torch.equal(sd[k], v), k          # never decayed, never updated: bit-equal
        else:
            assert not torch.equal(sd[k], v) and torch.isfinite(sd[k]).all(), k          # the shared bias table is trained


def test_config_runs_six_captured_steps_and_leaves_the_pooler_alone():
    """configs/smoke_random_mpnet.yaml as it is (bf16) through train_loop's captured per-phase step."""
    _check_step_run(*_run_config(True, [], _batches_of), True)


def test_captured_step_tracks_eager_step():
    """The same six steps captured and eager, loss by loss, to the tolerance of test_gpu_train_step.test_graph_replay_matches_eager_steps (2e-3) and
    under its conditions, which that test explains: the exact-f32 kernels (AMP false: two EAGER bf16 runs already differ by float-atomic order)
    and its small learning rates (a small randomly initialised problem amplifies that noise ~10x per step at the reference's rates). Dropout
    stays on: the replayed steps must reproduce the eager seed sequence - which is why the captured run is not padded to DATA.MAX_CAPTION_LENGTH
    here (the hidden-state dropout masks are indexed by row = b * L + l, so a padded L draws other masks: test_gpu_train_step's padded-replay test
    switches dropout off for the same reason); every batch of the synthetic dataset has the same longest caption, so all of them replay. The padded
    capture itself runs in the test above."""
    ov = ["AMP", False, "OPTIM.CNN_LR", 1e-3, "OPTIM.TRANS_LR", 1e-4, "OPTIM.LR", 1e-4, "OPTIM.BATCH_SIZE", 8, "DATA.IMAGE_CROP_SIZE", 64]
    runs = [_run_config(graph, ov, _batches_of, pad=False) for graph in (False, True)]
    for (losses, model, init, step, c), graph in zip(runs, (False, True)):
        _check_step_run(losses, model, init, step, c, graph)
    l0, l1 = runs[0][0], runs[1][0]
    print("eager", l0, "captured", l1)
    assert max(abs(a - b) for a, b in zip(l0, l1)) < 2e-3, (l0, l1)
    assert len(set(round(x, 3) for x in l1)) >= 3
