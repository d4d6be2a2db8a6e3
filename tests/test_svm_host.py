"""CPU tests of the VOC07 SVM evaluation's host layer: the float64 reference solver and AP pinned to sklearn, StratifiedKFold folds, the label
handling and cost selection of the reference protocol, the VOC reader, the dataset factory's VOC splits, the voc_clf command line and its
checkpoint loop (evaluation stubbed). Runs without a GPU."""
import json
import os

import numpy as np
import pytest
import torch

import svm_ref
from clip_lite_amd import svm
from clip_lite_amd.config import Config
from clip_lite_amd.data import VOC07ClassificationDataset
from clip_lite_amd.downstream import build_voc_clf_parser, run_checkpoint_loop, voc_clf_main
from clip_lite_amd.factories import DownstreamDatasetFactory

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("y", [
    np.array([1, -1] * 10),
    np.r_[np.ones(7), -np.ones(93)],                                   # imbalanced
    np.random.default_rng(0).choice([-1, 1], 101, p=[0.9, 0.1]),
    np.r_[-np.ones(50), np.ones(3), -np.ones(10)],                       # exactly n_splits positives
    np.random.default_rng(1).choice([0, 1, 2], 64),                      # three classes
])
def test_stratified_kfold_masks_match_sklearn(y):
    from sklearn.model_selection import StratifiedKFold
    got = svm.stratified_kfold_masks(y, 3)
    X = np.zeros((len(y), 1))
    for f, (_, test) in enumerate(StratifiedKFold(3).split(X, y)):
        want = np.zeros(len(y), bool)
        want[test] = True
        assert np.array_equal(got[f], want), f
    assert (got.sum(0) == 1).all()


def test_reference_solver_matches_liblinear():
    from sklearn.svm import LinearSVC
    rng = np.random.default_rng(2)
    X = np.abs(rng.standard_normal((200, 15)))
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    y = np.where(X[:, 0] + 0.2 * rng.standard_normal(200) > 0.3, 1, -1)
    keep = rng.random(200) > 0.3
    for C in (0.01, 1.0, 10.0):
        c = C * np.where(y > 0, 2.0, 1.0) * keep
        w, b, _ = svm_ref.solve_primal(X, y, c)
        clf = LinearSVC(C=C, class_weight={1: 2, -1: 1}, dual=False, tol=1e-12, max_iter=100000).fit(X[keep], y[keep])
        np.testing.assert_allclose(w, clf.coef_[0], rtol=1e-5, atol=1e-6)
        assert abs(b - clf.intercept_[0]) < 1e-5
        assert np.linalg.norm(svm_ref.gradient(X, y, c, w, b)) < 1e-8


def test_reference_ap_matches_sklearn_with_ties_and_ignored_rows():
    from sklearn.metrics import average_precision_score
    rng = np.random.default_rng(3)
    for n, q in ((50, 0), (400, 3), (1000, 1)):
        s = rng.standard_normal(n)
        if q:
            s = np.round(s * q) / q
        t = (rng.random(n) < 0.3).astype(np.int64)
        t[rng.random(n) < 0.1] = -1
        keep = t >= 0
        assert abs(svm_ref.average_precision(t, s) - average_precision_score(t[keep] > 0, s[keep])) < 1e-12


def test_protocol_labels_weights_and_cost_selection():
    T = np.array([[1, 0], [0, -1], [-1, 1], [1, 1], [0, 0], [0, 1], [1, -1], [0, 0], [1, 0]])
    assert svm.svm_labels(T[:, 0]).tolist() == [1, -1, -1, 1, -1, -1, 1, -1, 1]        # difficult trains as a negative
    Y, Cw, folds = svm.voc07_problems(T, (0.5, 2.0))
    assert Y.shape == (9, 2 * 2 * 4) and folds.shape == (2, 3, 9)
    p = (1 * 2 + 1) * 4 + 0                         # class 1, cost 2.0, fold 0
    y1 = svm.svm_labels(T[:, 1])
    assert np.array_equal(Y[:, p], y1)
    assert np.array_equal(Cw[:, p], 2.0 * np.where(y1 > 0, 2.0, 1.0) * ~folds[1, 0])
    assert np.array_equal(Cw[:, p + 3], 2.0 * np.where(y1 > 0, 2.0, 1.0))          # the full fit keeps every row
    assert svm.select_cost(np.array([[0.5, 0.5, 0.5], [0.6, 0.6, 0.6], [0.6, 0.6, 0.6], [0.2, 0.2, 0.2]]))[0] == 1   # strict >, first wins
    with pytest.raises(RuntimeError, match="no SVM cost"):
        svm.select_cost(np.zeros((4, 3)))


def test_reference_protocol_matches_golden_on_confident_classes():
    """tests/svm_ref.voc07_protocol (float64 optimum, NumPy AP) on the fixture against the sklearn protocol recorded in it."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "svm_voc_small.npz"))
    r = svm_ref.voc07_protocol(g["x_train"], g["t_train"].astype(np.int64), g["x_test"], g["t_test"].astype(np.int64), tuple(g["costs"]))
    P = r["W"].shape[0]
    for p in range(0, P, 7):
        assert np.abs(r["W"][p] - g["w_opt"][p]).max() < 1e-4 * max(1.0, np.abs(g["w_opt"][p]).max())
    assert np.abs(r["cv_ap"] - g["cv_ap"]).max() < 2e-3
    sure = g["cv_margin"] > 5e-3
    assert sure.any() and np.array_equal(r["cost_index"][sure], g["cost_index"][sure])


def _voc_tree(root, split, table):
    os.makedirs(os.path.join(root, "ImageSets", "Main"), exist_ok=True)
    os.makedirs(os.path.join(root, "JPEGImages"), exist_ok=True)
    from PIL import Image
    for cls, lines in table.items():
        with open(os.path.join(root, "ImageSets", "Main", f"{cls}_{split}.txt"), "w") as f:
            for name, lab in lines:
                f.write(f"{name} {lab:2d}\n")
                Image.new("RGB", (12, 10), (len(name) * 20 % 255, 40, 90)).save(os.path.join(root, "JPEGImages", f"{name}.jpg"))


def test_voc_reader_order_labels_and_collate(tmp_path):
    root = os.path.join(str(tmp_path), "VOC2007")
    # written out of class order; "dog" has an image the other classes do not list
    _voc_tree(root, "trainval", {"dog": [("000009", 1), ("000005", -1), ("000012", 0)],
                                 "cat": [("000005", 1), ("000009", 0), ("000007", -1)]})
    ds = VOC07ClassificationDataset(root, "trainval", ("global_resize", "normalize"), 8)
    assert ds.class_names == ["cat", "dog"]
    names = [os.path.basename(p)[:-4] for p, _ in ds.instances]
    assert names == ["000005", "000009", "000007", "000012"]                  # first appearance over the sorted class files
    labels = {n: lab for n, (_, lab) in zip(names, ds.instances)}
    assert labels == {"000005": [1, 0], "000009": [-1, 1], "000007": [0, -1], "000012": [-1, -1]}
    b = ds.collate_fn([ds[0], ds[1]])
    assert b["image"].shape == (2, 3, 8, 8) and b["label"].dtype == torch.long and b["label"].tolist() == [[1, 0], [-1, 1]]
    with pytest.raises(FileNotFoundError):
        VOC07ClassificationDataset(root, "test")


def test_downstream_factory_voc_splits(tmp_path):
    root = os.path.join(str(tmp_path), "VOC2007")
    _voc_tree(root, "trainval", {"cat": [("000001", 1)]})
    _voc_tree(root, "test", {"cat": [("000002", -1)]})
    over = ["DATA.ROOT", root, "DATA.IMAGE_CROP_SIZE", 8, "DATA.IMAGE_TRANSFORM_TRAIN", ["global_resize"],
            "DATA.IMAGE_TRANSFORM_VAL", ["global_resize", "normalize"]]
    tr = DownstreamDatasetFactory.from_config(Config(None, over), "trainval")
    te = DownstreamDatasetFactory.from_config(Config(None, over), "test")
    assert isinstance(tr, VOC07ClassificationDataset) and tr.image_transform == ("global_resize",)
    assert te.image_transform == ("global_resize", "normalize") and te.instances[0][1] == [0]
    for split in ("train", "val"):
        with pytest.raises(NotImplementedError, match="voc_clf"):
            DownstreamDatasetFactory.from_config(Config(None, over), split)


def test_voc_clf_arguments_and_errors():
    p = build_voc_clf_parser()
    a = p.parse_args(["--checkpoint-dir", "d"])
    assert (a.freq, a.start_iter, a.weight_init, a.loss_type, a.num_gpus_per_machine) == (46200, 46200, "vlinfo", "dot", 1)
    a = p.parse_args(["--config", "c.yaml", "--down-config", "d.yaml", "--down-config-override", "OPTIM.BATCH_SIZE", "8", "--weight-init",
                      "random", "--loss-type", "concat", "--checkpoint-dir", "x", "--freq", "10", "--start-iter", "20", "--cpu-workers", "0"])
    assert a.down_config_override == ["OPTIM.BATCH_SIZE", "8"] and (a.freq, a.start_iter, a.loss_type) == (10, 20, "concat")
    with pytest.raises(SystemExit):
        p.parse_args([])                                # --checkpoint-dir is required
    with pytest.raises(SystemExit):
        p.parse_args(["--checkpoint-dir", "x", "--weight-init", "clip"])
    for args, msg in ((["--num-gpus-per-machine", "0"], "no CPU path"), (["--num-gpus-per-machine", "2"], "one GPU"),
                      (["--weight-init", "imagenet"], "not supported"), (["--weight-init", "torchvision"], "not supported")):
        with pytest.raises(SystemExit, match=msg):
            voc_clf_main(p.parse_args(["--checkpoint-dir", "x"] + args))


def test_checkpoint_loop_merges_results(tmp_path, capsys):
    d = str(tmp_path)
    with open(os.path.join(d, "voc07_mAP.txt"), "w") as f:
        json.dump({"10": 1.5}, f)
    for it in (30, 40):
        open(os.path.join(d, f"checkpoint_{it}.pth"), "w").close()
    loaded, maps = [], iter([0.25, 0.5, 0.75])

    def load(path):
        if not os.path.exists(path):
            raise FileNotFoundError(path)
        loaded.append(os.path.basename(path))

    res = run_checkpoint_loop(d, 20, 10, lambda: next(maps), load)
    assert loaded == ["checkpoint_30.pth", "checkpoint_40.pth"]
    with open(os.path.join(d, "voc07_mAP.txt")) as f:
        got = json.load(f)
    assert got == res == {"10": 1.5, "20": 25.0, "30": 50.0, "40": 75.0}
    out = capsys.readouterr().out
    assert out.count("Test mAP: ") == 3 and out.rstrip().endswith("Completed!")
