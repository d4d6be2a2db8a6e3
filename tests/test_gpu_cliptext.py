"""The CLIP text tower on the MI355X (clip-lite_amd/cliptext.py; csrc/bert_ops.hip: the causal attention families, token assembly, end-of-text
gather / scatter): the kernel checks of tests/cliptext_checks.py on every shape, the 2-layer tower against tests/cliptext_ref.py in float64
(exact-f32 mode and bf16), padding invariance, the train step of configs/smoke_random_clip.yaml eager and captured, the checkpoint round trip,
the frozen path and one retrieval evaluation."""
import json
import os

import numpy as np
import pytest
import torch

import cliptext_checks as K
import cliptext_ref as R
from loss_backends import BF16, F32

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "configs", "smoke_random_clip.yaml")


@pytest.fixture(scope="module")
def be():
    return K.Hip()


# ------------------------------------------------------------------------------------------------ the kernels
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("B,L,H", K.SHAPES)
def test_causal_attention_matches_float64(be, dtype, B, L, H):
    K.check_against_float64(be, dtype, B, L, H)


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("L,i0", [(77, 40), (77, 31), (20, 9), (128, 95)])
def test_nothing_behind_a_token_reaches_it(be, dtype, L, i0):
    """i0 = 40 sits inside the second tile of 77 tokens, 31 on a tile edge; one tile; the last edge of four tiles"""
    K.check_causality(be, dtype, L, i0)


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("L", [20, 77])
def test_null_mask_is_the_all_ones_mask(be, dtype, L):
    K.check_null_mask(be, dtype, L)


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
def test_last_token_gather_and_scatter(be, dtype):
    K.check_gather_scatter(be, dtype)
    K.check_gather_scatter(be, dtype, Cc=512)


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
def test_token_assembly(be, dtype):
    K.check_embed(be, dtype)
    K.check_embed(be, dtype, Cc=512)


def test_refusals(be):
    K.check_refusals(be)


# ------------------------------------------------------------------------------------------------ the tower against float64
LENS, L_PAD = [24, 1, 13, 7], 24          # (the longest caption fills the padded width; the others are 1, 13 and 7 tokens)


def _case():
    ids, mask = K.captions([min(n, L_PAD) for n in LENS], L_PAD, seed=4)
    dfeat = torch.randn(4, 512, generator=torch.Generator().manual_seed(2))
    return ids, mask, dfeat


@pytest.mark.usefixtures("deterministic_reductions")
def test_f32_tower_matches_float64():
    """2 layers, B = 4, 24 columns, lengths 24 / 1 / 13 / 7, exact-f32 mode: pooled output within 1e-4, every parameter's gradient norm within 2e-3
    (the bars of tests/test_gpu_model.py), and an exactly zero gradient for the pad id's embedding row."""
    holder, sd = K.build_tower(2, "cuda", False)
    ids, mask, dfeat = _case()
    K.check_tower_f32(holder, sd, 2, 8, ids, mask, dfeat)


# the bounds tests/test_gpu_vit.py holds the 2-layer bf16 ViT tower to (BF16_FWD_BOUND, BF16_COS_BOUND there)
BF16_FWD_BOUND = 2 * 1.1318e-2
BF16_COS_BOUND = 1 - 2 * (1 - 0.99984142)


@pytest.mark.parametrize("seed", [0, 1])
def test_bf16_tower_tracks_float64(seed):
    """bf16 mode on bf16-rounded parameters against float64 on the same values: forward error / max |ref| and the cosine of the flattened
    parameter gradient inside the bounds of the 2-layer bf16 ViT tower; the pad row's gradient is exactly zero here too."""
    holder, sd = K.build_tower(2, "cuda", True, salt=f"bf16-{seed}", round_bf16=True)
    ids, mask, dfeat = _case()
    dfeat = dfeat.bfloat16().float()
    feat, grads = K.tower_pass(holder, ids, mask, dfeat)
    want, ref = R.features_and_grads(sd, ids, mask, 2, 8, dfeat)
    fwd = ((feat.double() - want).abs().max() / want.abs().max()).item()
    a = torch.cat([grads[k].double().flatten() for k in sorted(grads)])
    b = torch.cat([ref[k].flatten() for k in sorted(grads)])
    cos = (a @ b / (a.norm() * b.norm())).item()
    print(f"bf16 seed {seed}: forward error {fwd:.4e}, gradient cosine {cos:.6f}")
    assert fwd <= BF16_FWD_BOUND
    assert cos >= BF16_COS_BOUND and cos >= 0.93
    assert grads["token_embedding.weight"][0].abs().max() == 0


@pytest.mark.usefixtures("deterministic_reductions")
def test_padding_to_24_32_and_40_columns_changes_nothing():
    """The same captions padded to 24, 32 and 40 columns (a partial tile, a full tile, the two-tile kernels): the same pooled output and text
    gradients within 1e-5 relative - the bound and the reasoning of test_padding_to_64_and_128_changes_nothing (exact-f32 kernels, one contribution
    per address: only the order inside a few sums differs between the instantiations)."""
    ids, mask, dfeat = _case()
    runs = []
    for L in (24, 32, 40):
        pi, pm = torch.zeros(4, L, dtype=torch.long), torch.zeros(4, L, dtype=torch.long)
        pi[:, :L_PAD], pm[:, :L_PAD] = ids, mask
        holder, _ = K.build_tower(2, "cuda", False)
        runs.append(K.tower_pass(holder, pi, pm, dfeat))
    f0, g0 = runs[0]
    for L, (f1, g1) in zip((32, 40), runs[1:]):
        ef = ((f1 - f0).abs().max() / f0.abs().max()).item()
        worst = max(((g1[n] - g0[n]).abs().max().item() / g0[n].abs().max().item(), n) for n in g0)
        print(f"pad {L}: features {ef:.3e}; worst gradient {worst[0]:.3e} ({worst[1]})")
        assert ef <= 1e-5 and worst[0] <= 1e-5, (L, ef, worst)
        assert g1["token_embedding.weight"][0].abs().max() == 0


# ------------------------------------------------------------------------------------------------ the train step of configs/smoke_random_clip.yaml
_BATCHES = {}


def _batches_of(c):
    """the config's own dataset and collate: 3 batches (computed once, shared by the runs), the captions right-padded to DATA.MAX_CAPTION_LENGTH
    columns as train.py's captured step pads them - an eager step takes a batch at the width it comes with, and the weight gradients' sums over
    the B L rows are not bitwise the same at two widths"""
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


def _run_config(graph, overrides, steps=3):
    from clip_lite_amd.cliptext import ClipTextModel
    from clip_lite_amd.config import Config
    from clip_lite_amd.factories import LRSchedulerFactory, OptimizerFactory, PretrainingModelFactory
    from clip_lite_amd.train_loop import TrainStep
    from clip_lite_amd.utils.common import GradScaler
    c = Config(CFG, overrides)
    batches = _batches_of(c)
    torch.manual_seed(7)
    model = PretrainingModelFactory.from_config(c).to("cuda").train()
    st = model.text_encoder.strans
    assert isinstance(st, ClipTextModel) and len(st.transformer.resblocks) == 2 and model.loss.estimator == "infonce"
    optimizer = OptimizerFactory.from_config(c, model.named_parameters())
    decay = {id(p): g["weight_decay"] for g in optimizer.param_groups for p in g["params"]}
    assert decay[id(st.positional_embedding)] == 0.0 and decay[id(st.ln_final.weight)] == 0.0 and decay[id(st.text_projection)] > 0
    init = {k: v.detach().clone() for k, v in st.state_dict().items()}
    scheduler = LRSchedulerFactory.from_config(c, optimizer)
    step = TrainStep(model, optimizer, scheduler, GradScaler(enabled=c.AMP), c.OPTIM.CLIP_GRAD_NORM, None, graph=graph, graph_warmup=1,
                     pad_to=min(int(c.DATA.MAX_CAPTION_LENGTH), st.context_length), defer_update=True)
    assert not step._direct_ok()          # this tower takes the one-graph capture whatever the image tower is
    losses = [step({k: v.cuda() for k, v in batches[s].items()})["loss"].item() for s in range(steps)]
    step.finish()
    torch.cuda.synchronize()
    return losses, model, step, init


def test_config_runs_three_eager_steps():
    """configs/smoke_random_clip.yaml as it is (bf16), launched eagerly: finite losses, and every tensor of the text tower moves."""
    losses, model, step, init = _run_config(False, [])
    print("eager losses", losses)
    assert all(np.isfinite(losses)) and step.eager_steps == 3 and step.replays == 0
    for k, v in model.text_encoder.strans.state_dict().items():
        assert torch.isfinite(v).all(), k
        if k != "token_embedding.weight":
            assert not torch.equal(v, init[k]), k
    tok = model.text_encoder.strans.state_dict()["token_embedding.weight"]
    assert not torch.equal(tok[101], init["token_embedding.weight"][101])          # [CLS] occurs in every caption


def test_config_runs_captured_in_bf16():
    losses, model, step, _ = _run_config(True, [])
    print("captured losses", losses)
    assert all(np.isfinite(losses)) and step.replays == 2 and step.eager_steps == 1 and step._g is not None and step._graphs is None


@pytest.mark.usefixtures("deterministic_reductions")
def test_captured_step_is_bit_identical_to_eager_steps():
    """graph=True takes TrainStep._capture_single; in the deterministic exact-f32 mode the losses and the parameter arena after three steps are
    bit-identical between the eager and the captured run."""
    ov = ["AMP", False]
    (l0, m0, s0, _), (l1, m1, s1, _) = (_run_config(graph, ov) for graph in (False, True))
    print("eager", l0, "captured", l1)
    assert s0.replays == 0 and s0.eager_steps == 3
    assert s1.replays == 2 and s1.eager_steps == 1 and s1._g is not None and s1._graphs is None
    assert all(np.isfinite(l1))
    assert l0 == l1
    assert torch.equal(m0.runtime.arena.flat_p, m1.runtime.arena.flat_p)
    assert not torch.equal(m0.runtime.arena.flat_p, torch.zeros_like(m0.runtime.arena.flat_p))


def test_frozen_text_tower_stays_bit_equal_after_a_step():
    from clip_lite_amd.config import Config
    from clip_lite_amd.factories import LRSchedulerFactory, OptimizerFactory, PretrainingModelFactory
    from clip_lite_amd.train_loop import TrainStep
    from clip_lite_amd.utils.common import GradScaler
    c = Config(CFG, [])
    batch = _batches_of(c)[0]
    torch.manual_seed(3)
    model = PretrainingModelFactory.from_config(c).to("cuda").train()
    model.text_encoder.dont_train_enc()
    st = model.text_encoder.strans
    before = {k: v.detach().clone() for k, v in st.state_dict().items()}
    img0 = model.image_encoder.img_encoder.conv_proj.weight.detach().clone()
    optimizer = OptimizerFactory.from_config(c, model.named_parameters())
    step = TrainStep(model, optimizer, LRSchedulerFactory.from_config(c, optimizer), GradScaler(enabled=c.AMP), c.OPTIM.CLIP_GRAD_NORM, None,
                     graph=False, defer_update=True)
    losses = [step({k: v.cuda() for k, v in batch.items()})["loss"].item() for _ in range(2)]          # (the warm-up's first step has a zero rate)
    step.finish()
    torch.cuda.synchronize()
    assert all(np.isfinite(losses))
    for k, v in st.state_dict().items():
        assert torch.equal(v, before[k]), k
    assert not torch.equal(model.image_encoder.img_encoder.conv_proj.weight, img0)


def test_state_dict_round_trip_reproduces_the_features_bit_for_bit():
    from detfill import det_fill
    from clip_lite_amd.config import Config
    from clip_lite_amd.factories import PretrainingModelFactory
    c = Config(CFG, [])
    ids, mask, _ = _case()
    text = {"input_ids": ids.cuda(), "attention_mask": mask.cuda()}
    torch.manual_seed(1)
    M1 = PretrainingModelFactory.from_config(c)
    det_fill(M1.text_encoder)
    M1 = M1.to("cuda").eval()
    sd = {k: v.detach().cpu().clone() for k, v in M1.state_dict().items()}
    assert tuple(sd["text_encoder.strans.text_projection"].shape) == (512, 512)
    assert tuple(sd["text_encoder.strans.transformer.resblocks.1.attn.in_proj_weight"].shape) == (1536, 512)
    torch.manual_seed(2)
    M2 = PretrainingModelFactory.from_config(c).to("cuda").eval()
    with torch.no_grad():
        f1 = M1.text_encoder(text)
        assert not torch.equal(M2.text_encoder(text), f1)
        M2.load_state_dict(sd)
        f2 = M2.text_encoder(text)
    torch.cuda.synchronize()
    assert torch.isfinite(f1).all() and torch.equal(f1, f2)
    for k, v in M2.state_dict().items():
        assert torch.equal(v.cpu(), sd[k]), k


def test_retrieval_cli_takes_the_tower(tmp_path):
    """retrieval.py's evaluation on a generated image / caption tree with the randomly initialised model (--weight-init random) and the tower
    selected by overrides: it returns its result dict."""
    from PIL import Image
    from clip_lite_amd.downstream import retrieval_cli
    root = os.path.join(str(tmp_path), "flickr30k")
    rng = np.random.default_rng(0)
    os.makedirs(os.path.join(root, "images"))
    os.makedirs(os.path.join(root, "data"))
    words = ["dog", "cat", "red", "blue", "runs", "sits", "on", "grass", "a", "the", "ball"]
    ann = []
    for i in range(8):
        name = f"images/{i:04d}.jpg"
        Image.fromarray(rng.integers(0, 255, (72, 80, 3)).astype(np.uint8)).save(os.path.join(root, name))
        ann.append({"image": name, "caption": [" ".join(rng.choice(words, rng.integers(3, 9))) + "." for _ in range(2)]})
    with open(os.path.join(root, "data", "flickr30k_test.json"), "w") as f:
        json.dump(ann, f)
    over = ["MODEL.TEXTUAL.NETWORK_NAME", "clip_text_b", "MODEL.TEXTUAL.FEATURE_SIZE", 512, "MODEL.TEXTUAL.NUM_HIDDEN_LAYERS", 1]
    argv = ["--config", CFG, "--config-override", *[str(v) for v in over], "--down-config", os.path.join(ROOT, "configs", "downstream_coco_itm.yaml"),
            "--down-config-override", "DATA.ROOT", root, "DATA.IMAGE_CROP_SIZE", "64", "OPTIM.BATCH_SIZE", "8",
            "--checkpoint-path", os.path.join(str(tmp_path), "missing.pth"), "--weight-init", "random", "--cpu-workers", "0",
            "--checkpoints-dir", os.path.join(str(tmp_path), "logs") + "/"]
    res = retrieval_cli(argv)
    assert isinstance(res, dict) and len(res) >= 6 and all(0.0 <= v <= 100.0 for v in res.values())
