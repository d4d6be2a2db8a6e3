"""Image-text retrieval on the GPU: the rank kernels (gpu_ranks) against the host ranks of itm_eval's stable argsorts, exactly, on a tie-heavy,
a random and a COCO-5k-scale matrix out of similarity() (padded row stride), in both deterministic-reduction modes; and retrieval.py end to end
on a Flickr-format dataset, against the library composition on the host and against the oracle's modules."""
import json
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _check(sims, img2txt, txt2img):
    from clip_lite_amd import retrieval as R
    host = sims.cpu().numpy()
    got = R.gpu_ranks(sims, img2txt, txt2img)
    want = R.host_ranks(host, img2txt, txt2img)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    if all(len(c) for c in img2txt):
        ref = R.itm_eval(host, host.T, txt2img, {i: c for i, c in enumerate(img2txt)}, list(range(len(img2txt))))
        assert R.recalls(*got) == ref
    return got


def _layout(rng, Ni, Nt):
    owners = rng.integers(0, Ni, Nt)
    owners[:min(Ni, Nt)] = np.arange(min(Ni, Nt))      # every image has a caption when Nt >= Ni
    rng.shuffle(owners)
    return [list(rng.permutation(np.flatnonzero(owners == i))) for i in range(Ni)], [int(o) for o in owners]


@pytest.mark.gpu
def test_gpu_ranks_exact_on_ties_and_random():
    rng = np.random.default_rng(0)
    for Ni, Nt, ld in ((300, 1501, 1504), (129, 77, 77)):
        vals = np.array([-1.0, -0.0, 0.0, 0.5, 2.0], np.float32)
        full = torch.from_numpy(vals[rng.integers(0, 5, (Ni, ld))]).cuda()
        img2txt, txt2img = _layout(rng, Ni, Nt)
        _check(full[:, :Nt], img2txt, txt2img)
        s = rng.standard_normal((Ni, Nt)).astype(np.float32)
        for t, i in enumerate(txt2img):
            s[i, t] += 2.0
        _check(torch.from_numpy(s).cuda(), img2txt, txt2img)


@pytest.mark.gpu
def test_gpu_ranks_exact_at_coco_scale_in_both_modes():
    from clip_lite_amd import hip
    from clip_lite_amd import retrieval as R
    from clip_lite_amd.encoder import ImageEncoder, TextEncoder
    from clip_lite_amd.loss import JSDInfoMaxLoss
    from clip_lite_amd.model import VLInfoModel
    sys_path_tools = os.path.join(ROOT, "tools")
    import sys
    sys.path.insert(0, sys_path_tools)
    try:
        from bench_retrieval import coco_scale_sims
    finally:
        sys.path.remove(sys_path_tools)
    M = VLInfoModel(TextEncoder(mode="train_sbert", num_hidden_layers=1), ImageEncoder("resnet18"), JSDInfoMaxLoss(512, 768, "dot", 0.1, True, True),
                    "train_sbert", is_amp=False).cuda()
    sims, img2txt, txt2img = coco_scale_sims(M)
    assert sims.shape == (5000, 25014) and sims.stride(0) == 25016
    first = _check(sims, img2txt, txt2img)
    was = hip.is_deterministic()
    hip.set_deterministic(not was)
    try:
        again = R.gpu_ranks(sims, img2txt, txt2img)
    finally:
        hip.set_deterministic(was)
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])


@pytest.mark.gpu
def test_gpu_ranks_rejects_bad_indices():
    from clip_lite_amd import retrieval as R
    s = torch.zeros(3, 5, device="cuda")
    with pytest.raises(ValueError):
        R.gpu_ranks(s, [[0], [1, 5], [2]], [0, 1, 2, 0, 1])
    with pytest.raises(ValueError):
        R.gpu_ranks(s, [[0], [1], [2]], [0, 1, 2, 3, 1])


def _flickr_tree(root, n_img=24, per=5, seed=0):
    from PIL import Image
    rng = np.random.default_rng(seed)
    os.makedirs(os.path.join(root, "images"))
    os.makedirs(os.path.join(root, "data"))
    words = ["dog", "cat", "red", "blue", "runs", "sits", "on", "grass", "a", "the", "ball", "man", "woman", "street", "water"]
    ann = []
    for i in range(n_img):
        name = f"images/{i:04d}.jpg"
        Image.fromarray(rng.integers(0, 255, (72, 80, 3)).astype(np.uint8)).save(os.path.join(root, name))
        caps = [" ".join(rng.choice(words, rng.integers(3, 9))).capitalize() + "." for _ in range(per)]
        ann.append({"image": name, "caption": caps})
    with open(os.path.join(root, "data", "flickr30k_test.json"), "w") as f:
        json.dump(ann, f)


@pytest.mark.gpu
def test_retrieval_cli_end_to_end(tmp_path, capsys):
    from detfill import det_fill
    from oracle import ref_model as O
    from clip_lite_amd import retrieval as R
    from clip_lite_amd.config import Config
    from clip_lite_amd.data import RetrievalEvalDataset
    from clip_lite_amd.downstream import retrieval_cli, tokenize_texts
    from clip_lite_amd.factories import PretrainingModelFactory
    from clip_lite_amd.utils.checkpointing import CheckpointManager
    root = os.path.join(str(tmp_path), "flickr30k")
    _flickr_tree(root)
    over = ["MODEL.VISUAL.NETWORK_NAME", "resnet18", "MODEL.VISUAL.FEATURE_SIZE", 512, "MODEL.TEXTUAL.NUM_HIDDEN_LAYERS", 2, "AMP", False]
    cfg = os.path.join(ROOT, "configs", "smoke_random.yaml")
    _C = Config(cfg, over)
    M = det_fill(PretrainingModelFactory.from_config(_C))
    ck = os.path.join(str(tmp_path), "ck")
    os.makedirs(ck)
    CheckpointManager(ck, model=M).step(7)
    argv = ["--config", cfg, "--config-override", *[str(v) for v in over], "--down-config", os.path.join(ROOT, "configs", "downstream_coco_itm.yaml"),
            "--down-config-override", "DATA.ROOT", root, "DATA.IMAGE_CROP_SIZE", "64", "OPTIM.BATCH_SIZE", "10",
            "--checkpoint-path", os.path.join(ck, "checkpoint_7.pth"), "--cpu-workers", "0", "--checkpoints-dir", os.path.join(str(tmp_path), "logs") + "/"]
    got = retrieval_cli(argv)
    out = capsys.readouterr().out
    assert str(got) in out and str({f"val_{k}": v for k, v in got.items()}) in out

    # the library composition, ranked on the host
    ds = RetrievalEvalDataset(root, os.path.join(root, "data", "flickr30k_test.json"), image_transform=("smallest_resize", "center_crop", "normalize"),
                              image_size=64)
    assert len(ds) == 24 and len(ds.text) == 120
    Mg = PretrainingModelFactory.from_config(_C)
    CheckpointManager(model=Mg).load(os.path.join(ck, "checkpoint_7.pth"))
    Mg = Mg.cuda()
    imgs = torch.stack([ds[i]["image"] for i in range(len(ds))], 0)
    ids, mask = tokenize_texts(ds.text, 30)
    ie = R.embed_images(Mg, imgs.cuda())
    te = R.embed_texts(Mg, ids.cuda(), mask.cuda())
    sims = R.similarity(Mg, ie, te).cpu().numpy()
    want = R.itm_eval(sims, sims.T, [ds.txt2img[t] for t in range(120)], ds.img2txt, ds.image_ids)
    assert got == want

    # the oracle's modules on the same weights: ranks may differ only where the oracle's score gap at the positive is below 1e-3
    Mo = det_fill(O.build_oracle_model("resnet18", "train_sbert", 2, dropout=0.0)).eval()
    with torch.no_grad():
        ie_o = torch.nn.functional.normalize(Mo.loss.global_d.img_block(Mo.image_encoder(imgs)), p=2, dim=-1)
        te_o = torch.nn.functional.normalize(Mo.loss.global_d.text_block(Mo.text_encoder({"input_ids": ids, "attention_mask": mask})), p=2, dim=-1)
    so = (ie_o @ te_o.t()).double().numpy()
    img2txt, txt2img = [ds.img2txt[i] for i in range(24)], [ds.txt2img[t] for t in range(120)]
    r_g = R.host_ranks(sims, img2txt, txt2img)
    r_o = R.host_ranks(so, img2txt, txt2img)
    for i in np.flatnonzero(r_g[0] != r_o[0]):
        best = max(so[i, c] for c in img2txt[i])
        others = np.delete(so[i], img2txt[i])
        assert np.min(np.abs(others - best)) < 1e-3, (i, r_g[0][i], r_o[0][i])
    for t in np.flatnonzero(r_g[1] != r_o[1]):
        col = so[:, t]
        gap = np.abs(np.delete(col, txt2img[t]) - col[txt2img[t]])
        assert gap.min() < 1e-3, (t, r_g[1][t], r_o[1][t])

    # --weight-init random evaluates the randomly initialised model without reading the checkpoint
    argv_r = [a if a != os.path.join(ck, "checkpoint_7.pth") else os.path.join(ck, "missing.pth") for a in argv] + ["--weight-init", "random"]
    res = retrieval_cli(argv_r)
    assert set(res) == set(got) and all(0.0 <= v <= 100.0 for v in res.values())
