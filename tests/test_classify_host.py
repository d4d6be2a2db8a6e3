"""CPU checks of the downstream classification host layer: torchvision names and shapes of ImageClassifier, loading a pretraining
backbone, the optimizer groups, the image-folder dataset and the two command lines."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from torch import nn

from oracle.ref_model import OracleResNet
from clip_lite_amd.classify import ImageClassifier
from clip_lite_amd.config import Config
from clip_lite_amd.data import ImageFolderDataset, RandomLabelledDataset
from clip_lite_amd.downstream import build_linear_clf_parser, build_zero_shot_parser, linear_clf_main, tokenize_prompts
from clip_lite_amd.factories import DownstreamDatasetFactory, OptimizerFactory

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name,D", [("resnet18", 512), ("resnet50", 2048)])
def test_state_dict_matches_torchvision_classifier(name, D):
    ref = OracleResNet(name)
    ref.fc = nn.Linear(D, 10)
    m = ImageClassifier(name, 10, frozen=False, is_amp=False)
    want = {k: tuple(v.shape) for k, v in ref.state_dict().items()}
    got = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert got == want
    assert list(got) == list(want)
    assert [n for n, _ in m.named_parameters()] == [n for n, _ in ref.named_parameters()]
    # fc re-initialised N(0, 0.01) / 0 (reference linear_clf.py:159-160)
    w = m.fc.weight.detach()
    assert abs(w.std().item() - 0.01) < 2e-3 and not m.fc.bias.detach().any()
    m.load_state_dict(ref.state_dict(), strict=True)
    ref.load_state_dict(m.state_dict(), strict=True)


def test_frozen_sets_eval_and_no_grad():
    m = ImageClassifier("resnet18", 10, frozen=True, is_amp=False)
    assert not m.training
    assert all(not p.requires_grad for n, p in m.named_parameters() if not n.startswith("fc."))
    assert m.fc.weight.requires_grad and m.fc.bias.requires_grad
    m.train()
    assert not m.layer1.training and not m.bn1.training


def test_from_pretraining_copies_backbone():
    from clip_lite_amd.encoder import ImageEncoder, TextEncoder
    from clip_lite_amd.loss import JSDInfoMaxLoss
    from clip_lite_amd.model import VLInfoModel
    te = TextEncoder(mode="train_sbert", num_hidden_layers=1)
    vl = VLInfoModel(te, ImageEncoder("resnet18"), JSDInfoMaxLoss(512, 768, "dot", 0.1, True, True), "train_sbert", is_amp=False)
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for n, t in list(vl.named_parameters()) + list(vl.named_buffers()):
            if t.dtype.is_floating_point:
                t.copy_(torch.randn(t.shape, generator=g))
            else:
                t.fill_(7)
    sd = vl.state_dict()
    m = ImageClassifier.from_pretraining({"model": sd, "iteration": 5}, "resnet18", 10, frozen=True, is_amp=False)
    pre = "image_encoder.img_encoder."
    n = 0
    for k, v in m.state_dict().items():
        if k.startswith("fc."):
            continue
        assert torch.equal(v, sd[pre + k]), k
        n += 1
    assert n == len([k for k in sd if k.startswith(pre)])
    m2 = ImageClassifier.from_pretraining(vl, "resnet18", 10)
    assert torch.equal(m2.state_dict()["layer3.0.bn1.running_var"], sd[pre + "layer3.0.bn1.running_var"])
    with pytest.raises(KeyError):
        ImageClassifier.from_pretraining(sd, "resnet50", 10)


def test_optimizer_factory_puts_every_tensor_at_lr():
    _C = Config(None, ["OPTIM.LR", 0.3, "OPTIM.CNN_LR", 0.9, "OPTIM.LOOKAHEAD.USE", False])
    m = ImageClassifier("resnet18", 10, frozen=False, is_amp=False)
    named = list(m.named_parameters())
    assert not any("image_encoder" in n for n, _ in named)
    # FusedSGD needs the device arena; check the grouping the factory would hand it
    import clip_lite_amd.factories as F
    seen = []
    orig = F.OptimizerFactory.create
    try:
        F.OptimizerFactory.create = classmethod(lambda cls, name, groups, **kw: seen.extend(groups))
        OptimizerFactory.from_config(_C, named)
    finally:
        F.OptimizerFactory.create = orig
    assert len(seen) == len(named) and all(g["lr"] == 0.3 for g in seen)


def _write_tree(root, classes, per_class, size=(20, 16)):
    from PIL import Image
    rng = np.random.default_rng(0)
    for split in ("train", "val"):
        for ci, c in enumerate(classes):
            d = os.path.join(root, split, c)
            os.makedirs(d)
            for k in range(per_class):
                a = rng.integers(0, 255, (size[1], size[0], 3), dtype=np.uint8)
                Image.fromarray(a).save(os.path.join(d, f"img{k:02d}.png"))
            open(os.path.join(d, "notes.txt"), "w").close()            # not an image: skipped


def test_image_folder_dataset(tmp_path):
    classes = ["zebra", "ant", "moth"]
    _write_tree(str(tmp_path), classes, 8)
    ds = ImageFolderDataset(str(tmp_path), "train", ("global_resize::12", "normalize"), 12)
    assert ds.classes == ["ant", "moth", "zebra"] and ds.num_classes == 3
    assert len(ds) == 24 and ds.targets == [0] * 8 + [1] * 8 + [2] * 8
    assert ds.samples[8][0].endswith(os.path.join("moth", "img00.png"))
    item = ds[9]
    assert item["image"].shape == (3, 12, 12) and item["image"].dtype == torch.float32 and item["label"].item() == 1
    cut = ImageFolderDataset(str(tmp_path), "train", ("global_resize::12",), 12, percentage=25)
    assert len(cut) == 6 and cut.targets == [0, 0, 1, 1, 2, 2]
    assert [s for s, _ in cut.samples][:2] == [s for s, _ in ds.samples][:2]
    val = ImageFolderDataset(str(tmp_path), "val", ("global_resize::12",), 12, percentage=25)
    assert len(val) == 24                                          # the cut is train-only
    batch = ds.collate_fn([ds[i] for i in (0, 9, 23)])
    assert batch["image"].shape == (3, 3, 12, 12) and batch["image"].dtype == torch.float32
    assert batch["label"].dtype == torch.int64 and batch["label"].tolist() == [0, 1, 2]


def test_downstream_factory(tmp_path):
    root = os.path.join(str(tmp_path), "imagenet")
    _write_tree(root, ["a", "b"], 2)
    _C = Config(None, ["DATA.ROOT", root, "DATA.IMAGE_CROP_SIZE", 8, "DATA.IMAGE_TRANSFORM_TRAIN", ["global_resize"]])
    with pytest.raises(ValueError, match="1000"):
        DownstreamDatasetFactory.from_config(_C, "train")
    other = os.path.join(str(tmp_path), "flowers")
    _write_tree(other, ["a", "b"], 2)
    _C = Config(None, ["DATA.ROOT", other, "DATA.IMAGE_CROP_SIZE", 8, "DATA.IMAGE_TRANSFORM_TRAIN", ["global_resize"]])
    assert DownstreamDatasetFactory.from_config(_C, "train").num_classes == 2
    r = DownstreamDatasetFactory.from_config(Config(None, ["DATA.ROOT", "random", "DATA.IMAGE_CROP_SIZE", 16]), "val")
    assert isinstance(r, RandomLabelledDataset) and r.num_classes == 10 and r[3]["image"].shape == (3, 16, 16)
    assert torch.equal(r[3]["image"], r[3]["image"])
    with pytest.raises(NotImplementedError):
        DownstreamDatasetFactory.from_config(Config(None, ["DATA.ROOT", "datasets/VOC2007"]), "train")


def test_linear_clf_arguments_and_errors():
    p = build_linear_clf_parser()
    a = p.parse_args(["--config", "c.yaml", "--down-config", "d.yaml", "--down-config-override", "OPTIM.LR", "0.1", "--weight-init", "random",
                      "--checkpoint-every", "10", "--log-every", "5", "--cpu-workers", "0", "--serialization-dir", "/x", "--resume-from", "r.pth",
                      "--checkpoint-path", "k.pth"])
    assert a.down_config_override == ["OPTIM.LR", "0.1"] and a.weight_init == "random" and a.checkpoint_every == 10
    assert a.num_gpus_per_machine == 1 and a.serialization_dir == "/x" and a.resume_from == "r.pth"
    with pytest.raises(SystemExit, match="one GPU"):
        linear_clf_main(p.parse_args(["--weight-init", "random", "--num-gpus-per-machine", "2"]))
    with pytest.raises(SystemExit, match="clip package"):
        linear_clf_main(p.parse_args(["--weight-init", "clip", "--checkpoint-path", "x"]))
    with pytest.raises(SystemExit, match="downloads"):
        linear_clf_main(p.parse_args(["--weight-init", "imagenet"]))
    with pytest.raises(SystemExit, match="not supported"):
        linear_clf_main(p.parse_args(["--weight-init", "torchvision", "--checkpoint-path", "x"]))


def test_linear_clf_script_refuses_several_gpus():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "linear_clf.py"), "--weight-init", "random", "--num-gpus-per-machine", "4"],
                       capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode != 0 and "one GPU" in r.stderr


def test_zero_shot_arguments_and_prompts():
    a = build_zero_shot_parser().parse_args(["--config", "c.yaml", "--checkpoint-path", "k.pth", "--data-root", "/d"])
    assert a.prompt == "a picture of a {}." and a.max_length == 30
    ids, mask = tokenize_prompts(["plane", "sea_turtle"], a.prompt, a.max_length)
    assert ids.shape == (2, 30) and ids.dtype == torch.int64 and ids[0, 0] == 101
    assert mask.sum(1).tolist() == [(ids[i] != 0).sum().item() for i in range(2)]
    assert not torch.equal(ids[0], ids[1])


def test_forward_refuses_graph_capture(monkeypatch):
    """hipGraph capture of the classification step is out of scope and says so before anything is launched."""
    from clip_lite_amd.classify import cross_entropy
    m = ImageClassifier("resnet18", 10, frozen=True, is_amp=False)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="capture"):
        m(torch.zeros(2, 3, 32, 32))
    with pytest.raises(RuntimeError, match="capture"):
        cross_entropy(torch.zeros(2, 10), torch.zeros(2, dtype=torch.long))
