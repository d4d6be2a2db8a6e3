"""Host side of the image-text retrieval evaluation (retrieval.py): the reference's caption cleanup, both dataset layouts, the factory's
routing, recalls against itm_eval, gpu_ranks' index validation, the shared tokenisation and every command-line refusal. Runs without a GPU."""
import json
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pre_caption_restated(caption, max_words):
    """reference data/dataloader.py:1027-1052, restated"""
    caption = re.sub(r"([,.'!?\"()*#:;~])", "", caption.lower()).replace("-", " ").replace("/", " ").replace("<person>", "person")
    caption = re.sub(r"\s{2,}", " ", caption)
    caption = caption.rstrip("\n")
    caption = caption.strip(" ")
    caption_words = caption.split(" ")
    if len(caption_words) > max_words:
        caption = " ".join(caption_words[:max_words])
    return caption


def test_pre_caption_matches_reference():
    from clip_lite_amd.data import normalize_caption, pre_caption
    cases = ["A man, riding a horse!", "  Two <person>s  on a half-pipe/ramp.\n", "Café  crème (\"good\") #1; ok: ~yes~ *", "word " * 40,
             "UPPER lower\tTab", "a--b //c", ""]
    for c in cases:
        for k in (30, 5):
            assert pre_caption(c, k) == _pre_caption_restated(c, k)
    assert pre_caption("Café") == "café" and normalize_caption("Café") == "cafe"        # accents stay


def _jpeg(path, seed, size=(40, 32)):
    from PIL import Image
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(np.random.default_rng(seed).integers(0, 255, (size[1], size[0], 3)).astype(np.uint8)).save(path)


def test_json_layout(tmp_path):
    from clip_lite_amd.data import RetrievalEvalDataset, load_image, pre_caption
    root = str(tmp_path)
    ann = [{"image": "a/1.jpg", "caption": ["One dog.", "A DOG running!"]}, {"image": "b/2.jpg", "caption": []},
           {"image": "c.jpg", "caption": ["Third-image caption"]}]
    for k, a in enumerate(ann):
        _jpeg(os.path.join(root, a["image"]), k)
    with open(os.path.join(root, "ann.json"), "w") as f:
        json.dump(ann, f)
    tfm = ("smallest_resize", "center_crop", "normalize")
    ds = RetrievalEvalDataset(root, os.path.join(root, "ann.json"), image_transform=tfm, image_size=24)
    assert ds.text == [pre_caption(c) for c in ["One dog.", "A DOG running!", "Third-image caption"]]
    assert ds.img2txt == {0: [0, 1], 1: [], 2: [2]} and ds.txt2img == {0: 0, 1: 0, 2: 2}
    assert ds.image == [os.path.join(root, a["image"]) for a in ann] and ds.image_ids == [0, 1, 2] and len(ds) == 3
    item = ds[2]
    assert item["index"] == 2 and item["image"].dtype == torch.float32 and item["image"].shape == (3, 24, 24)
    assert torch.equal(item["image"], load_image(os.path.join(root, "c.jpg"), tfm, 24))
    b = ds.collate_fn([ds[0], ds[2]])
    assert b["image"].shape == (2, 3, 24, 24) and b["index"].tolist() == [0, 2]
    with open(os.path.join(root, "bad.json"), "w") as f:
        json.dump([{"image": "c.jpg", "caption": "not a list"}], f)
    with pytest.raises(ValueError):
        RetrievalEvalDataset(root, os.path.join(root, "bad.json"))


def _coco_tree(root):
    for img_id in (42, 7, 1000):
        _jpeg(os.path.join(root, "val2017", f"{img_id:012d}.jpg"), img_id)
    anns = [{"image_id": 1000, "id": 1, "caption": "Last one."}, {"image_id": 7, "id": 2, "caption": "Seven, first."},
            {"image_id": 99, "id": 3, "caption": "no image"}, {"image_id": 7, "id": 4, "caption": "Seven, second."}]
    os.makedirs(os.path.join(root, "annotations"))
    with open(os.path.join(root, "annotations", "captions_val2017.json"), "w") as f:
        json.dump({"annotations": anns}, f)


def test_coco_layout(tmp_path):
    from clip_lite_amd.data import RetrievalEvalDataset
    root = os.path.join(str(tmp_path), "coco")
    _coco_tree(root)
    ds = RetrievalEvalDataset(root, split="val", image_transform=("smallest_resize", "center_crop", "normalize"), image_size=16)
    assert ds.image_ids == [7, 42, 1000]                               # sorted file names
    assert ds.text == ["seven first", "seven second", "last one"]
    assert ds.img2txt == {0: [0, 1], 1: [], 2: [2]} and ds.txt2img == {0: 0, 1: 0, 2: 2}
    assert ds[1]["image"].shape == (3, 16, 16) and ds[1]["index"] == 1


def test_factory_routing(tmp_path):
    from clip_lite_amd.config import Config
    from clip_lite_amd.factories import DownstreamDatasetFactory, RetrievalDatasetFactory
    coco = os.path.join(str(tmp_path), "coco")
    _coco_tree(coco)
    flickr = os.path.join(str(tmp_path), "flickr30k")
    _jpeg(os.path.join(flickr, "img", "x.jpg"), 1)
    os.makedirs(os.path.join(flickr, "data"))
    with open(os.path.join(flickr, "data", "flickr30k_test.json"), "w") as f:
        json.dump([{"image": "img/x.jpg", "caption": ["A.", "B."]}], f)
    cfg = os.path.join(ROOT, "configs", "downstream_coco_itm.yaml")
    ds = RetrievalDatasetFactory.from_config(Config(cfg, ["DATA.ROOT", coco]))
    assert ds.image_ids == [7, 42, 1000] and ds.image_size == 224
    ds = RetrievalDatasetFactory.from_config(Config(cfg, ["DATA.ROOT", flickr]))
    assert ds.text == ["a", "b"] and ds.image == [os.path.join(flickr, "img/x.jpg")] and ds.img2txt == {0: [0, 1]}
    ds = RetrievalDatasetFactory.from_config(Config(cfg, ["DATA.ROOT", flickr]), ann_file=os.path.join(flickr, "data", "flickr30k_test.json"))
    assert len(ds) == 1
    other = os.path.join(str(tmp_path), "imagenet")
    with pytest.raises(ValueError, match="COCO 2017"):
        RetrievalDatasetFactory.from_config(Config(cfg, ["DATA.ROOT", other]))
    # the classification factory keeps its meaning for such roots: an image folder
    with pytest.raises(FileNotFoundError):
        DownstreamDatasetFactory.from_config(Config(cfg, ["DATA.ROOT", coco]), split="val")


def test_recalls_equal_itm_eval():
    from clip_lite_amd.retrieval import host_ranks, itm_eval, recalls
    rng = np.random.default_rng(1)
    for Ni, per in ((17, 5), (40, 3)):
        Nt = Ni * per
        owners = rng.permutation(np.repeat(np.arange(Ni), per))
        img2txt = [list(np.flatnonzero(owners == i)) for i in range(Ni)]
        s = np.round(rng.standard_normal((Ni, Nt)), 1).astype(np.float32)
        want = itm_eval(s, s.T, owners.tolist(), {i: c for i, c in enumerate(img2txt)}, list(range(Ni)))
        assert recalls(*host_ranks(s, img2txt, owners.tolist())) == want
    r_i, r_t = rng.integers(0, 30, 50), rng.integers(0, 30, 200)
    got = recalls(r_i, r_t)
    assert got["txt_r5"] == 100.0 * np.mean(r_i < 5) and got["img_r10"] == 100.0 * np.mean(r_t < 10)
    assert got["r_mean"] == (got["txt_r_mean"] + got["img_r_mean"]) / 2


def test_gpu_ranks_validates_before_any_launch():
    """a CPU tensor reaches no kernel: every index is checked first (ValueError), and only then the device (RuntimeError)"""
    from clip_lite_amd.retrieval import gpu_ranks
    s = torch.zeros(3, 5)
    bad = [([[0], [1, 5], [2]], [0, 1, 2, 0, 1]), ([[0], [1, -1], [2]], [0, 1, 2, 0, 1]), ([[0], [1], [2]], [0, 1, 3, 0, 1]),
           ([[0], [1], [2]], [0, 1, 2, 0]), ([[0], [1]], [0, 1, 1, 0, 1])]
    for img2txt, txt2img in bad:
        with pytest.raises(ValueError):
            gpu_ranks(s, img2txt, txt2img)
    with pytest.raises(ValueError):
        gpu_ranks(torch.zeros(3, 5, dtype=torch.float64), [[0], [1], [2]], [0, 1, 2, 0, 1])
    with pytest.raises(RuntimeError, match="GPU"):
        gpu_ranks(s, [[0, 3], [1, 4], [2]], [0, 1, 2, 0, 1])


def test_tokenize_prompts_unchanged():
    from clip_lite_amd.data import hash_tokenize
    from clip_lite_amd.downstream import tokenize_prompts, tokenize_texts
    names = ["golden_retriever", "cat", "a_very_long_name_" * 8]
    ids, mask = tokenize_prompts(names, "a picture of a {}.", 12)
    for i, n in enumerate(names):                      # what the loop computed before it moved into tokenize_texts
        t = hash_tokenize("a picture of a {}.".format(n.replace("_", " ")), 12)[:12]
        assert ids[i, :len(t)].tolist() == t and not ids[i, len(t):].any()
        assert mask[i].tolist() == [1] * len(t) + [0] * (12 - len(t))
    ids2, mask2 = tokenize_texts(["a picture of a {}.".format(n.replace("_", " ")) for n in names], 12)
    assert torch.equal(ids, ids2) and torch.equal(mask, mask2) and ids.dtype == torch.long


def _argv(*extra):
    return ["--config", os.path.join(ROOT, "configs", "smoke_random.yaml"), "--down-config", os.path.join(ROOT, "configs", "downstream_coco_itm.yaml"),
            "--checkpoint-path", "unused.pth", *extra]


@pytest.mark.parametrize("extra,msg", [(["--weight-init", "clip"], "clip"), (["--weight-init", "imagenet"], "download"),
                                       (["--weight-init", "torchvision"], "download"), (["--num-gpus-per-machine", "2"], "one GPU"),
                                       (["--num-gpus-per-machine", "0"], "MI355X")])
def test_cli_refusals(extra, msg):
    from clip_lite_amd.downstream import retrieval_cli
    with pytest.raises(SystemExit, match=msg):
        retrieval_cli(_argv(*extra))


def test_cli_refuses_without_a_gpu(monkeypatch):
    from clip_lite_amd.downstream import retrieval_cli
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(SystemExit, match="no GPU visible"):
        retrieval_cli(_argv())


def test_cli_parser_matches_reference():
    from clip_lite_amd.downstream import build_retrieval_parser
    p = build_retrieval_parser()
    with pytest.raises(SystemExit):
        p.parse_args(["--config", "x"])                # --checkpoint-path is required
    a = p.parse_args(_argv("--ann-file", "f.json", "--down-config-override", "DATA.ROOT", "datasets/flickr30k"))
    assert a.weight_init == "vlinfo" and a.ann_file == "f.json" and a.num_gpus_per_machine == 1
    assert a.down_config_override == ["DATA.ROOT", "datasets/flickr30k"]
