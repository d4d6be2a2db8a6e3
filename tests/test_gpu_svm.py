"""VOC07 SVM evaluation on the MI355X (svm.py, csrc/svm_ops.hip): the batched solver against the float64 optimum of a fixture problem and the
reference protocol's results, the VOC-scale solve (320 problems on 5011 x 2048 features), the feature path against the oracle, and voc_clf.py
end to end."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from detfill import det_fill, det_tensor
import svm_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "svm_voc_small.npz")

pytestmark = pytest.mark.gpu


def test_fixture_problem_matches_optimum_and_reference_protocol():
    from clip_lite_amd import svm
    g = np.load(GOLDEN)
    xtr, xte = g["x_train"].astype(np.float32), g["x_test"].astype(np.float32)
    ttr, tte = g["t_train"].astype(np.int64), g["t_test"].astype(np.int64)
    costs = tuple(g["costs"])
    Y, Cw, folds = svm.voc07_problems(ttr, costs)
    assert np.array_equal(folds, g["folds"])
    Xg = torch.from_numpy(xtr).cuda()
    sol = svm.fit_squared_hinge(Xg, torch.from_numpy(Y).cuda(), torch.from_numpy(Cw).cuda())
    W, b = sol["W"].cpu().double().numpy(), sol["b"].cpu().double().numpy()
    print(f"newton {sol['newton'].min().item()}-{sol['newton'].max().item()}, max rel grad {sol['rel_grad'].max().item():.2e}, "
          f"CG launched {sol['cg_launched']}")
    X64 = xtr.astype(np.float64)
    for p in range(Y.shape[1]):
        y, c = Y[:, p].astype(np.float64), Cw[:, p].astype(np.float64)
        wo, bo = g["w_opt"][p].astype(np.float64), float(g["b_opt"][p])
        dz = np.abs((X64 @ W[p] + b[p]) - (X64 @ wo + bo)).max()
        assert dz <= 2e-3, (p, dz)
        fo, fg = svm_ref.objective(X64, y, c, wo, bo), svm_ref.objective(X64, y, c, W[p], b[p])
        assert abs(fg - fo) <= 1e-5 * abs(fo), (p, fg, fo)
    res = svm.voc07_svm_eval(Xg, ttr, torch.from_numpy(xte).cuda(), tte, costs)
    assert np.abs(res["cv_ap"] - g["cv_ap"]).max() <= 2e-3
    for k in range(ttr.shape[1]):
        if g["cv_margin"][k] > 5e-3:
            assert res["cost_index"][k] == g["cost_index"][k], k
    ok = res["cost_index"] == g["cost_index"]
    assert np.abs(res["test_ap"][ok] - g["test_ap"][ok]).max() <= 2e-3
    assert abs(100 * res["map"] - 100 * float(g["map"])) <= 0.1, (res["map"], float(g["map"]))


def _voc_scale_problem(seed=0, N=5011, D=2048, K=20):
    g = torch.Generator().manual_seed(seed)
    present = torch.rand(N, K, generator=g) < torch.linspace(0.03, 0.3, K)
    protos = torch.randn(K, D, generator=g) * 0.04
    f = torch.relu(0.3 + torch.randn(N, D, generator=g) * 0.5 + present.float() @ protos)
    f = f / f.norm(dim=1, keepdim=True)
    t = present.to(torch.int64)
    t[(~present) & (torch.rand(N, K, generator=g) < 0.03)] = -1
    return f, t.numpy()


def test_voc_scale_solve_converges_and_is_reproducible():
    from clip_lite_amd import hip, svm
    f, t = _voc_scale_problem()
    Y, Cw, _ = svm.voc07_problems(t)
    assert Y.shape == (5011, 320)
    X, Yg, Cg = f.cuda(), torch.from_numpy(Y).cuda(), torch.from_numpy(Cw).cuda()
    svm.fit_squared_hinge(X[:512], Yg[:512], Cg[:512], max_newton=2)          # warm-up (first launches)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sol = svm.fit_squared_hinge(X, Yg, Cg)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(f"VOC-scale solve: {dt * 1e3:.1f} ms, Newton {sol['newton'].min().item()}-{sol['newton'].max().item()}, CG launched "
          f"{sol['cg_launched']}, device max rel grad {sol['rel_grad'].max().item():.2e}")
    Xt = np.concatenate([f.double().numpy(), np.ones((5011, 1))], 1)
    Wt = np.concatenate([sol["W"].cpu().double().numpy(), sol["b"].cpu().double().numpy()[:, None]], 1)
    Z = Xt @ Wt.T
    Y64, C64 = Y.astype(np.float64), Cw.astype(np.float64)
    act = (Y64 * Z < 1) & (C64 > 0)
    G = Wt + 2 * (np.where(act, C64 * (Z - Y64), 0.0)).T @ Xt
    G0 = 2 * (-(C64 * Y64)).T @ Xt
    rel = np.linalg.norm(G, axis=1) / np.linalg.norm(G0, axis=1)
    print(f"host float64 relative gradient norm: max {rel.max():.2e}, median {np.median(rel):.2e}")
    assert rel.max() <= 1e-3
    hip.set_deterministic(True)
    try:
        a = svm.fit_squared_hinge(X, Yg, Cg)
        b = svm.fit_squared_hinge(X, Yg, Cg)
    finally:
        hip.set_deterministic(False)
    assert torch.equal(a["W"], b["W"]) and torch.equal(a["b"], b["b"]) and torch.equal(a["newton"], b["newton"])


def test_features_match_oracle_f32():
    from oracle import ref_model as O
    from clip_lite_amd.downstream import extract_features
    from clip_lite_amd.encoder import ImageEncoder, TextEncoder
    from clip_lite_amd.loss import JSDInfoMaxLoss
    from clip_lite_amd.model import VLInfoModel
    te = TextEncoder(mode="train_sbert", num_hidden_layers=1)
    M = det_fill(VLInfoModel(te, ImageEncoder("resnet18"), JSDInfoMaxLoss(512, 768, "dot", 0.1, True, True), "train_sbert", is_amp=False))
    M = M.to("cuda").train()
    Mo = det_fill(O.build_oracle_model("resnet18", "train_sbert", 1, dropout=0.0)).eval()
    img = det_tensor("vocimg", (10, 3, 64, 64), "normal")
    loader = [{"image": img[:6], "label": torch.zeros(6, 3, dtype=torch.long)}, {"image": img[6:], "label": torch.ones(4, 3, dtype=torch.long)}]
    feats, tg = extract_features(M, loader, torch.device("cuda"))
    assert M.image_encoder.training                     # the mode is restored
    with torch.no_grad():
        want = F.normalize(Mo.image_encoder(img), p=2, dim=-1)
    assert feats.dtype == torch.float32 and feats.shape == (10, 512) and tg.shape == (10, 3)
    err = (feats.cpu() - want).abs().max().item()
    print(f"feature error vs oracle: {err:.2e}")
    assert err <= 1e-4


def _voc_tree(root, classes, names, seed):
    from PIL import Image
    rng = np.random.default_rng(seed)
    os.makedirs(os.path.join(root, "ImageSets", "Main"), exist_ok=True)
    os.makedirs(os.path.join(root, "JPEGImages"), exist_ok=True)
    for split, ns in names.items():
        lab = {}
        for n in ns:
            present = rng.random(len(classes)) < 0.4
            lab[n] = [1 if pr else (0 if rng.random() < 0.1 else -1) for pr in present]
            base = rng.integers(0, 255, (64, 64, 3))
            for k, pr in enumerate(present):                # a class leaves a colour cast, so the SVM has something to find
                if pr:
                    base[..., k % 3] = np.clip(base[..., k % 3] + 30, 0, 255)
            Image.fromarray(base.astype(np.uint8)).save(os.path.join(root, "JPEGImages", f"{n}.jpg"))
        for k, c in enumerate(classes):
            with open(os.path.join(root, "ImageSets", "Main", f"{c}_{split}.txt"), "w") as f:
                for n in ns:
                    f.write(f"{n} {lab[n][k]}\n")


def test_voc_clf_end_to_end(tmp_path):
    from clip_lite_amd.config import Config
    from clip_lite_amd.data import VOC07ClassificationDataset
    from clip_lite_amd.downstream import extract_features
    from clip_lite_amd.factories import PretrainingModelFactory
    from clip_lite_amd.utils.checkpointing import CheckpointManager
    root = os.path.join(str(tmp_path), "VOC2007")
    classes = ["bird", "car", "dog"]
    _voc_tree(root, classes, {"trainval": [f"{i:06d}" for i in range(48)], "test": [f"{i:06d}" for i in range(100, 132)]}, 0)
    ck = os.path.join(str(tmp_path), "ck")
    os.makedirs(ck)
    over = ["MODEL.VISUAL.NETWORK_NAME", "resnet18", "MODEL.VISUAL.FEATURE_SIZE", 512, "MODEL.TEXTUAL.NUM_HIDDEN_LAYERS", 1, "AMP", False]
    for it, seed in ((100, 1), (150, 2)):
        torch.manual_seed(seed)
        m = PretrainingModelFactory.from_config(Config(os.path.join(ROOT, "configs", "smoke_random.yaml"), over))
        torch.save({"model": m.state_dict(), "iteration": it}, os.path.join(ck, f"checkpoint_{it}.pth"))
    down = ["DATA.ROOT", root, "DATA.IMAGE_CROP_SIZE", 64, "OPTIM.BATCH_SIZE", 16]
    cmd = [sys.executable, os.path.join(ROOT, "voc_clf.py"), "--config", os.path.join(ROOT, "configs", "smoke_random.yaml"), "--config-override",
           *[str(v) for v in over], "--down-config", os.path.join(ROOT, "configs", "downstream_voc07.yaml"), "--down-config-override",
           *[str(v) for v in down], "--checkpoint-dir", ck, "--start-iter", "100", "--freq", "50", "--cpu-workers", "0",
           "--checkpoints-dir", os.path.join(str(tmp_path), "logs") + "/"]
    r = subprocess.run(cmd, cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    print(r.stdout[-2000:], r.stderr[-3000:])
    assert r.returncode == 0
    assert r.stdout.count("Test mAP: ") == 2 and "Completed!" in r.stdout
    with open(os.path.join(ck, "voc07_mAP.txt")) as f:
        got = json.load(f)
    assert sorted(got) == ["100", "150"]
    # the float64 reference protocol on the same extracted features
    _C = Config(os.path.join(ROOT, "configs", "smoke_random.yaml"), over)
    tfm = ("smallest_resize", "center_crop", "normalize")
    dss = [VOC07ClassificationDataset(root, s, tfm, 64) for s in ("trainval", "test")]
    for it in (100, 150):
        m = PretrainingModelFactory.from_config(_C).cuda()
        CheckpointManager(model=m).load(os.path.join(ck, f"checkpoint_{it}.pth"))
        out = []
        for ds in dss:
            loader = torch.utils.data.DataLoader(ds, batch_size=16, shuffle=False, collate_fn=ds.collate_fn)
            out.append(extract_features(m, loader, torch.device("cuda")))
        ref = svm_ref.voc07_protocol(out[0][0].cpu().numpy(), out[0][1].numpy(), out[1][0].cpu().numpy(), out[1][1].numpy())
        print(f"iteration {it}: voc_clf {got[str(it)]:.4f}, float64 reference {100 * ref['map']:.4f}")
        assert abs(got[str(it)] - 100 * ref["map"]) <= 0.1
