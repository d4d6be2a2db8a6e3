"""Downstream classification on the MI355X (classify.py, csrc/cls_ops.hip): the linear probe and the fine-tune against the oracle's
torchvision ResNet + nn.Linear + F.cross_entropy, the bf16 form against the f32 form, learning on the synthetic labelled source, zero-shot
counts against the oracle's embeddings, and the linear_clf.py command line end to end."""
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from detfill import det_fill, det_tensor

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pair(name, C, frozen, is_amp=False):
    """(ImageClassifier on the GPU, f32 oracle, f64 oracle) with identical weights and buffers."""
    from oracle.ref_model import OracleResNet
    from clip_lite_amd.classify import ImageClassifier
    m = ImageClassifier(name, C, frozen=frozen, is_amp=is_amp)
    D = m.out_dim
    m = det_fill(m)
    with torch.no_grad():
        m.fc.weight.mul_(0.05)                  # logits of order 1
    ref = OracleResNet(name)
    ref.fc = nn.Linear(D, C)
    ref.load_state_dict(m.state_dict(), strict=True)
    ref64 = OracleResNet(name)
    ref64.fc = nn.Linear(D, C)
    ref64.load_state_dict(m.state_dict(), strict=True)
    ref64 = ref64.double()
    m = m.to("cuda")
    if frozen:
        ref.eval(), ref64.eval()
    else:
        m.train(), ref.train(), ref64.train()
    return m, ref, ref64


def _batch(B, C, S=64, key="cimg"):
    img = det_tensor(key, (B, 3, S, S), "normal")
    y = torch.randint(0, C, (B,), generator=torch.Generator().manual_seed(C + B))
    return img, y


def _grads(m, ref, ref64, img, y):
    from clip_lite_amd.classify import cross_entropy
    loss = cross_entropy(m(img.cuda()), y.cuda())
    loss.backward()
    lo = F.cross_entropy(ref(img), y)
    lo.backward()
    l64 = F.cross_entropy(ref64(img.double()), y)
    l64.backward()
    torch.cuda.synchronize()
    return loss, lo, l64


def _bad_grads(m, ref, ref64):
    """test_f32_mode_matches_oracle's bar: err vs fp64 <= max(2e-3 * max(scale, 1e-3 * largest scale), 16 * the fp32 oracle's own err)."""
    got = dict(m.named_parameters())
    rows = []
    for (k, p32), (_, p64) in zip(ref.named_parameters(), ref64.named_parameters()):
        if p32.grad is None:
            continue
        g64 = p64.grad
        e = (got[k].grad.float().cpu().double() - g64).abs().max().item()
        eo = (p32.grad.double() - g64).abs().max().item()
        rows.append((e, eo, g64.abs().max().item(), k))
    gmax = max(r[2] for r in rows)
    return [r for r in rows if r[0] > max(2e-3 * max(r[2], 1e-3 * gmax), 16 * r[1])], rows


@pytest.mark.parametrize("C", [10, 1003])
@pytest.mark.usefixtures("deterministic_reductions")
def test_frozen_probe_matches_oracle(C):
    from clip_lite_amd.optim import FusedSGD
    B = 6
    m, ref, ref64 = _pair("resnet18", C, frozen=True)
    before = {k: v.detach().float().cpu().clone() for k, v in m.state_dict().items() if not k.startswith("fc.")}
    img, y = _batch(B, C)
    y[2] = -100                                           # ignore_index: not in the mean
    opt = FusedSGD([{"params": [p], "lr": 0.1, "weight_decay": 1e-4} for p in m.parameters()], momentum=0.9)
    ropt = torch.optim.SGD([ref.fc.weight, ref.fc.bias], lr=0.1, momentum=0.9, weight_decay=1e-4)
    opt.zero_grad()
    loss, lo, l64 = _grads(m, ref, ref64, img, y)
    assert loss.dim() == 0 and loss.is_cuda
    assert abs(loss.item() - l64.item()) < 1e-4, (loss.item(), l64.item())
    for k in ("weight", "bias"):
        g, g64 = getattr(m.fc, k).grad.float().cpu(), getattr(ref64.fc, k).grad.float()
        assert (g - g64).abs().max().item() <= 2e-3 * g64.abs().max().item(), k
    opt.step()
    ropt.step()
    torch.cuda.synchronize()
    for k in ("weight", "bias"):
        assert torch.allclose(getattr(m.fc, k).detach().cpu(), getattr(ref.fc, k).detach(), rtol=1e-5, atol=1e-6), k
    after = m.state_dict()
    for k, v in before.items():                          # backbone weights, BatchNorm buffers and counters: bitwise unchanged
        assert torch.equal(after[k].float().cpu(), v), k


@pytest.mark.parametrize("C", [10, 1003])
@pytest.mark.usefixtures("deterministic_reductions")
def test_fine_tune_matches_oracle(C):
    B = 6
    m, ref, ref64 = _pair("resnet18", C, frozen=False)
    img, y = _batch(B, C, key="fimg")
    loss, lo, l64 = _grads(m, ref, ref64, img, y)
    assert abs(loss.item() - l64.item()) < 1e-4
    bad, rows = _bad_grads(m, ref, ref64)
    for e, eo, s, k in sorted(bad, reverse=True)[:10]:
        print(f"  {k}: err {e:.3e} (fp32 oracle err {eo:.3e}) scale {s:.3e}")
    assert len(rows) == len(list(ref.parameters())) and not bad
    sd, sdo = m.state_dict(), ref.state_dict()
    for k in sdo:
        if "running_" in k or "num_batches" in k:
            assert torch.allclose(sd[k].float().cpu(), sdo[k].float(), rtol=1e-4, atol=1e-5), k


def test_bf16_fine_tune_tracks_f32():
    """ResNet-50, C = 1000, B = 32: the bf16 fine-tune step against the exact-f32 step on the same weights (the classifier's own torchvision
    initialisation). Loss within 2e-2. Gradient direction: cosine >= 0.93 on the classifier's own gradient (fc, the product of clite_xent_bwd's bf16
    logit gradient); the whole-model cosine is printed, not held to 0.93: a bf16 backward through 50 train-mode BatchNorm layers at random init
    decorrelates from fp32 even in PyTorch with bf16 storage emulated (tests/test_gpu_model.py test_bf16_mode_resnet50_bert_forward: cosine ~0.1)."""
    from clip_lite_amd.classify import ImageClassifier, cross_entropy
    C, B = 1000, 32
    img, y = _batch(B, C, S=128, key="bimg")
    torch.manual_seed(3)
    state = ImageClassifier("resnet50", C, frozen=False, is_amp=False).state_dict()
    out = {}
    for amp in (False, True):
        m = ImageClassifier("resnet50", C, frozen=False, is_amp=amp)
        m.load_state_dict(state)
        m = m.to("cuda").train()
        loss = cross_entropy(m(img.cuda()), y.cuda())
        loss.backward()
        torch.cuda.synchronize()
        g = torch.cat([p.grad.detach().float().reshape(-1) for p in m.parameters()])
        gfc = m.fc.weight.grad.detach().float().reshape(-1).clone()
        out[amp] = (loss.item(), g, gfc)
    cos = F.cosine_similarity(out[True][1], out[False][1], dim=0).item()
    cfc = F.cosine_similarity(out[True][2], out[False][2], dim=0).item()
    print(f"bf16 loss {out[True][0]:.5f} vs f32 {out[False][0]:.5f}; gradient cosine {cos:.4f} (fc alone {cfc:.4f})")
    assert abs(out[True][0] - out[False][0]) < 2e-2, (out[True][0], out[False][0])
    assert cfc >= 0.93


@pytest.mark.usefixtures("deterministic_reductions")
def test_logit_gradient_reaches_autograd():
    """The gradient w.r.t. the logits is autograd's own: retain_grad sees it, two losses on the same logits add up (a mixup-style sum),
    torch.autograd.grad returns it without touching the parameter gradients. Against the fp64 oracle, with class padding (C = 1003)."""
    from clip_lite_amd.classify import cross_entropy
    C, B = 1003, 6
    m, ref, ref64 = _pair("resnet18", C, frozen=True)
    img, y = _batch(B, C, key="gimg")
    y2 = (y * 7 + 3) % C
    y2[4] = -100
    z = m(img.cuda())
    z.retain_grad()
    loss = 0.5 * cross_entropy(z, y.cuda()) + 0.5 * cross_entropy(z, y2.cuda())
    loss.backward()
    zo = ref64(img.double())
    zo.retain_grad()
    lo = 0.5 * F.cross_entropy(zo, y) + 0.5 * F.cross_entropy(zo, y2)
    lo.backward()
    torch.cuda.synchronize()
    assert abs(loss.item() - lo.item()) < 1e-4
    assert (z.grad.cpu().double() - zo.grad).abs().max().item() <= 1e-3 * zo.grad.abs().max().item()
    for k in ("weight", "bias"):
        g, g64 = getattr(m.fc, k).grad.double().cpu(), getattr(ref64.fc, k).grad
        assert (g - g64).abs().max().item() <= 2e-3 * g64.abs().max().item(), k
    before = m.fc.weight.grad.clone()
    z2 = m(img.cuda())
    (g,) = torch.autograd.grad(cross_entropy(z2, y.cuda()), z2)
    zo2 = ref64(img.double()).detach().requires_grad_(True)
    (go,) = torch.autograd.grad(F.cross_entropy(zo2, y), zo2)
    assert (g.cpu().double() - go).abs().max().item() <= 1e-3 * go.abs().max().item()
    torch.cuda.synchronize()
    assert torch.equal(m.fc.weight.grad, before)


@pytest.mark.usefixtures("deterministic_reductions")
def test_bf16_fine_tune_backbone_matches_image_encoder_backward():
    """The bf16 fine-tune's backbone backward (ResNet-50, C = 1000, B = 32) against the pretraining image encoder's bf16 backward (the executor
    VLInfoModel trains with, DeviceRuntime registering its transposed dgrad weights) on the same weights, images and feature gradient. Every
    backbone gradient and running statistic agrees, and every convolution whose dgrad can read a transposed copy has one registered."""
    from clip_lite_amd import hip
    from clip_lite_amd.classify import ImageClassifier
    from clip_lite_amd.encoder import ImageEncoder
    from clip_lite_amd.model import attach_runtime
    C, B = 1000, 32
    img, _ = _batch(B, C, S=128, key="eimg")
    gl = det_tensor("elogit_grad", (B, C), "normal") * 1e-3
    torch.manual_seed(4)
    m = ImageClassifier("resnet50", C, frozen=False, is_amp=True)
    state = m.state_dict()
    m = m.to("cuda").train()
    A = m.runtime.arena
    convs = [mod for mod in m.modules() if hasattr(mod, "in_channels")]
    assert all(A.has_wt(c.weight) for c in convs if c.in_channels % 8 == 0 and c.out_channels % 8 == 0)

    class Holder(nn.Module):
        def __init__(self):
            super().__init__()
            self.image_encoder = ImageEncoder("resnet50")

    h = Holder()
    h.image_encoder.img_encoder.load_state_dict({k: v for k, v in state.items() if not k.startswith("fc.")}, strict=True)
    h = h.to("cuda")
    attach_runtime(h, torch.device("cuda", torch.cuda.current_device()), True)
    h.train()

    m(img.cuda()).backward(gl.cuda())
    feat = h.image_encoder(img.cuda())
    D = m.out_dim
    dpad = torch.zeros(B, C, device="cuda", dtype=torch.bfloat16)
    dpad.copy_(gl.cuda())
    dfeat = torch.empty(B, D, device="cuda", dtype=torch.bfloat16)
    hip.gemm_nn(hip.BF16, dpad, A.w(m.fc.weight), B, D, C, hip.epilogue(dfeat, D), lda=C, ldb=D)
    feat.backward(dfeat)
    torch.cuda.synchronize()
    got = {n: p.grad.detach().float().reshape(-1) for n, p in m.named_parameters() if not n.startswith("fc.")}
    want = {n: p.grad.detach().float().reshape(-1) for n, p in h.image_encoder.img_encoder.named_parameters()}
    assert set(got) == set(want)
    same = sum(torch.equal(got[n], want[n]) for n in got)
    gc, wc = torch.cat([got[n] for n in sorted(got)]), torch.cat([want[n] for n in sorted(want)])
    cos = F.cosine_similarity(gc, wc, dim=0).item()
    print(f"bf16 fine-tune backbone vs image encoder: {same}/{len(got)} tensors bit-identical, global cosine {cos:.6f}")
    assert cos >= 0.999
    for n in got:
        assert (got[n] - want[n]).abs().max().item() <= 1e-2 * max(want[n].abs().max().item(), 1e-3 * wc.abs().max().item()), n
    sd, sdh = m.state_dict(), h.image_encoder.img_encoder.state_dict()
    for k in sdh:
        if "running_" in k or "num_batches" in k:
            assert torch.allclose(sd[k].float(), sdh[k].float(), rtol=1e-3, atol=1e-4), k


def _probe_top1(amp, steps=300, strength=None):
    from clip_lite_amd.classify import ImageClassifier, TopkAccuracy, cross_entropy
    from clip_lite_amd.data import RandomLabelledDataset
    from clip_lite_amd.optim import FusedSGD
    torch.manual_seed(0)
    kw = {} if strength is None else {"strength": strength}
    tr = RandomLabelledDataset(10, 32, 256, "train", 0, **kw)
    va = RandomLabelledDataset(10, 32, 200, "val", 0, **kw)
    X = torch.stack([tr[i]["image"] for i in range(len(tr))]).cuda()
    Y = torch.stack([tr[i]["label"] for i in range(len(tr))]).cuda()
    Xv = torch.stack([va[i]["image"] for i in range(len(va))]).cuda()
    Yv = torch.stack([va[i]["label"] for i in range(len(va))]).cuda()
    m = ImageClassifier("resnet18", 10, frozen=True, is_amp=amp).to("cuda")
    opt = FusedSGD([{"params": [p], "lr": 0.05, "weight_decay": 0.0} for p in m.parameters()], momentum=0.9)
    g = torch.Generator().manual_seed(1)
    for _ in range(steps):
        idx = torch.randint(0, len(tr), (64,), generator=g).cuda()
        opt.zero_grad()
        cross_entropy(m(X[idx]), Y[idx]).backward()
        opt.step()
    top1 = TopkAccuracy(1)
    with torch.no_grad():
        for i in range(0, len(va), 64):
            top1(m(Xv[i:i + 64]), Yv[i:i + 64])
    return 100.0 * top1.get_metric()


def test_probe_learns_random_labelled_source():
    """A frozen random ResNet-18 probe, 300 steps of 64 on 256 synthetic 32 x 32 images, top-1 on 200 held-out ones. Calibrated on the f32
    path at the source's default pattern strength 1.0: 97 % (strength 0.5: 51.5 %, 0.25: 16.5 %; chance 10 %)."""
    f32 = _probe_top1(False)
    bf16 = _probe_top1(True)
    print(f"frozen probe top-1 on RandomLabelledDataset: f32 {f32:.1f} %, bf16 {bf16:.1f} % (chance 10 %)")
    assert f32 >= 80.0
    assert abs(bf16 - f32) <= 2.0 or bf16 >= f32


@pytest.mark.usefixtures("deterministic_reductions")
def test_zero_shot_counts_match_oracle():
    from oracle import ref_model as O
    from clip_lite_amd.classify import zero_shot_accuracy
    from clip_lite_amd.encoder import ImageEncoder, TextEncoder
    from clip_lite_amd.loss import JSDInfoMaxLoss
    from clip_lite_amd.model import VLInfoModel
    te = TextEncoder(mode="train_sbert", num_hidden_layers=2)
    M = det_fill(VLInfoModel(te, ImageEncoder("resnet18"), JSDInfoMaxLoss(512, 768, "dot", 0.1, True, True), "train_sbert", is_amp=False)).to("cuda").train()
    Mo = det_fill(O.build_oracle_model("resnet18", "train_sbert", 2, dropout=0.0)).eval()
    N, Cc, L = 24, 11, 9
    img = det_tensor("zimg", (N, 3, 64, 64), "normal")
    ids = torch.randint(1000, 30522, (Cc, L), generator=torch.Generator().manual_seed(9))
    mask = torch.ones(Cc, L, dtype=torch.long)
    mask[4, 5:] = 0
    with torch.no_grad():
        ie = F.normalize(Mo.loss.global_d.img_block(Mo.image_encoder(img)), p=2, dim=-1).double()
        tt = F.normalize(Mo.loss.global_d.text_block(Mo.text_encoder({"input_ids": ids, "attention_mask": mask})), p=2, dim=-1).double()
    S = ie @ tt.t()
    order = S.argsort(1, descending=True)
    labels = torch.empty(N, dtype=torch.long)
    for i in range(N):                                    # labels at ranks 0 .. 7, each away from its neighbours in the ranking (tie-free)
        for r in [i % 8] + list(range(Cc)):
            s = S[i, order[i]]
            gaps = [abs(s[r] - s[q]).item() for q in (r - 1, r + 1) if 0 <= q < Cc]
            if min(gaps) > 2e-3:
                labels[i] = order[i, r]
                break
        else:
            pytest.fail(f"image {i} has no tie-free class")
    want1 = (S.argmax(1) == labels).sum().item()
    want5 = (S.topk(5, 1).indices == labels[:, None]).any(1).sum().item()
    res = zero_shot_accuracy(M, img.cuda(), labels.cuda(), ids.cuda(), mask.cuda(), topk=5, batch_size=10)
    assert M.training and M.image_encoder.img_encoder.training
    assert round(res["top1"] * N / 100) == want1 and round(res["top5"] * N / 100) == want5, (res, want1, want5)
    assert 0 < want1 < want5 < N


def test_linear_clf_cli_end_to_end(tmp_path):
    out = str(tmp_path / "run")
    cmd = [sys.executable, os.path.join(ROOT, "linear_clf.py"), "--down-config", os.path.join(ROOT, "configs", "downstream_random.yaml"),
           "--down-config-override", "OPTIM.BATCH_SIZE", "32", "--weight-init", "random", "--checkpoint-every", "10", "--log-every", "10",
           "--cpu-workers", "0", "--serialization-dir", out, "--checkpoints-dir", str(tmp_path / "logs"), "--num-gpus-per-machine", "1"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    print(r.stdout[-3000:], r.stderr[-3000:])
    assert r.returncode == 0
    assert re.search(r"Top-1 accuracy: [0-9.]+", r.stdout + r.stderr)
    from oracle.ref_model import OracleResNet
    ck = torch.load(os.path.join(out, "checkpoint_30.pth"), map_location="cpu", weights_only=False)
    ref = OracleResNet("resnet18")
    ref.fc = nn.Linear(512, 10)
    ref.load_state_dict(ck["model"], strict=True)
    assert ck["iteration"] == 30 and "optimizer" in ck and "scheduler" in ck
