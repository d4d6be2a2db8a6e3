"""k-NN evaluation on the MI355X (knn.py, csrc/knn_ops.hip): the streaming selection against the stable argsort (ties, chunkings, padded tiles,
a 300 x 70 001 random matrix), knn.topk end to end on exact lattice features, knn_eval against float64 on clustered features, and knn_clf.py
end to end."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import knn_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def _feed(s, K, chunk, pad=0, fill=1e30):
    """knn_ref.feed on the device: s [Q][N] in chunks of `chunk` columns, tiles of row stride Nc + pad (pad None: Nc rounded up to a multiple of
    8, as knn.topk pads) with `fill` in the padding."""
    from clip_lite_amd import hip
    Q, N = s.shape
    sd = torch.from_numpy(np.ascontiguousarray(s)).cuda()
    top_s = torch.full((Q, K), -7.0, device="cuda")
    top_i = torch.full((Q, K), -7, device="cuda", dtype=torch.int32)
    for base in range(0, N, chunk):
        nc = min(chunk, N - base)
        lds = nc + ((-nc) % 8 if pad is None else pad)
        tile = torch.full((Q, lds), fill, device="cuda")
        tile[:, :nc] = sd[:, base:base + nc]
        hip.knn_topk_merge(tile, lds, Q, nc, base, K, min(K, base), top_s, top_i)
    return top_s[:, :min(K, N)].cpu().numpy(), top_i[:, :min(K, N)].cpu().numpy()


@pytest.mark.parametrize("Q,N,K", knn_ref.SELECTION_SHAPES)
def test_selection_is_the_stable_argsort_under_every_chunking(Q, N, K):
    s = knn_ref.tie_scores(Q, N)
    want_s, want_i = knn_ref.topk_ref(s, K)
    for chunk, pad in [(N, 0), (N, 5), (N, 4 + (-N) % 4), (64, 0), (100, 0), (1, 0)]:
        got_s, got_i = _feed(s, K, chunk, pad)
        np.testing.assert_array_equal(got_i, want_i, err_msg=f"chunk {chunk} pad {pad}")
        np.testing.assert_array_equal(got_s, want_s, err_msg=f"chunk {chunk} pad {pad}")


def test_selection_with_signed_zeros_and_rows_that_keep_improving():
    rng = np.random.default_rng(5)
    vals = np.array([-0.5, -0.0, 0.0, 0.25, -0.0, 0.0], np.float32)
    s = vals[rng.integers(0, len(vals), (2, 300))]
    up = np.arange(3000, dtype=np.float32)[None, :].repeat(2, 0)
    up[1] = -up[1]
    for m, chunks in ((s, (300, 64, 7)), (up, (3000, 1024))):
        want_s, want_i = knn_ref.topk_ref(m, 200)
        for chunk in chunks:
            got_s, got_i = _feed(m, 200, chunk)
            np.testing.assert_array_equal(got_i, want_i)
            np.testing.assert_array_equal(got_s, want_s)


def test_selection_on_random_scores_is_exact_and_repeats_bitwise():
    """300 x 70 001 random f32 scores in three chunks (tiles padded to a multiple of 8 columns: the 16-byte path): the lists equal the stable
    sort of the given scores, and a second run gives the same bits."""
    Q, N, K = 300, 70001, 200
    s = torch.randn(Q, N, generator=torch.Generator().manual_seed(7))
    order = torch.sort(s, dim=1, descending=True, stable=True)      # equal scores keep their index order: np.argsort(-s, kind="stable")
    want_s, want_i = order.values[:, :K].numpy(), order.indices[:, :K].numpy().astype(np.int32)
    chunk = 23336
    runs = [_feed(s.numpy(), K, chunk, pad=None) for _ in range(2)]
    np.testing.assert_array_equal(runs[0][1], want_i)
    np.testing.assert_array_equal(runs[0][0], want_s)
    assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][1].tobytes() == runs[1][1].tobytes()


def test_topk_end_to_end_on_lattice_features():
    """Integer features in -2 .. 2, D = 32: every product and sum is exact in f32, so the GEMM adds no error and the lists must equal the
    reference's exactly; 3 query blocks x 3 bank chunks, the last of both ragged."""
    from clip_lite_amd import knn
    rng = np.random.default_rng(11)
    X, Z = knn_ref.lattice(rng, 700), knn_ref.lattice(rng, 33)
    want_s, want_i = knn_ref.topk_ref(Z @ X.T, 200)
    got_s, got_i = knn.topk(torch.from_numpy(Z).cuda(), torch.from_numpy(X).cuda(), 200, query_rows=16, bank_rows=256)
    np.testing.assert_array_equal(got_i.cpu().numpy(), want_i)
    np.testing.assert_array_equal(got_s.cpu().numpy(), want_s)
    one_s, one_i = knn.topk(torch.from_numpy(Z).cuda(), torch.from_numpy(X).cuda(), 200)          # one block, one chunk
    assert torch.equal(one_s, got_s) and torch.equal(one_i, got_i)
    with pytest.raises(ValueError, match="non-finite"):
        bad = torch.from_numpy(X).cuda()
        bad[5, 3] = float("nan")
        knn.topk(torch.from_numpy(Z).cuda(), bad, 10)


@pytest.mark.parametrize("N,Q,D,C,noise", [(3000, 97, 64, 10, 1.5), (5000, 128, 256, 100, 2.0)])
def test_knn_eval_matches_float64_on_clustered_features(N, Q, D, C, noise):
    """Predictions equal float64's for every query whose relative float64 margin between its two best class scores is at least 1e-3 (a
    neighbour swapped at the k-th place by f32 rounding moves a class score by far less); at most 2 % of the queries may fall under that
    margin (the float64 reference alone: none, at every k, for these shapes and seeds), and top-1 / top-5 agree to within that share."""
    from clip_lite_amd import knn
    ks = (1, 10, 20, 200)
    for seed in range(3):
        xb, yb, xq, yq = knn_ref.clustered(seed, N, Q, D, C, noise)
        want_scores, want_pred, want_acc = knn_ref.knn_eval_ref(xb, yb, xq, yq, C, ks, 0.07)
        res, pred, kept = knn.knn_eval(torch.from_numpy(xb).cuda(), torch.from_numpy(yb), torch.from_numpy(xq).cuda(), torch.from_numpy(yq), C, ks,
                                       0.07, query_rows=64, bank_rows=2048, return_pred=True)
        assert kept == list(ks)
        pred = pred.cpu().numpy()
        top = -np.sort(-want_scores, axis=-1)[..., :2]
        sure = (top[..., 0] - top[..., 1]) >= 1e-3 * top[..., 0]
        for j, k in enumerate(ks):
            excluded = float((~sure[j]).mean())
            print(f"seed {seed} k {k}: excluded {excluded:.4f}, top1 {res[k]['top1']:.3f} (float64 {want_acc[k]['top1']:.3f}), "
                  f"top5 {res[k]['top5']:.3f} (float64 {want_acc[k]['top5']:.3f})")
            assert excluded <= 0.02
            np.testing.assert_array_equal(pred[j, sure[j], 0], want_pred[j, sure[j], 0])
            assert abs(res[k]["top1"] - want_acc[k]["top1"]) <= 100 * excluded + 1e-9
            assert abs(res[k]["top5"] - want_acc[k]["top5"]) <= 100 * excluded + 1e-9


def test_knn_eval_drops_a_k_beyond_the_bank_and_reports_top5_only_with_five_classes():
    from clip_lite_amd import knn
    xb, yb, xq, yq = knn_ref.clustered(0, 40, 9, 16, 3, 0.5)
    res = knn.knn_eval(torch.from_numpy(xb).cuda(), torch.from_numpy(yb), torch.from_numpy(xq).cuda(), torch.from_numpy(yq), 3, (10, 20, 100, 200))
    assert sorted(res) == [10, 20] and all(set(v) == {"top1"} for v in res.values())
    _, _, want = knn_ref.knn_eval_ref(xb, yb, xq, yq, 3, [10, 20], 0.07)
    assert res[10]["top1"] == pytest.approx(want[10]["top1"]) and res[20]["top1"] == pytest.approx(want[20]["top1"])


def test_classify_returns_class_scores_within_1e5_of_float64():
    """knn.classify(..., return_scores=True) on the real build, on the wave-simulator test's vote cases: f32 sums of at most 256 terms in
    (0, 1] against float64 at 1e-5 relative, unvoted classes exactly 0, and the same predictions with and without the scores."""
    from clip_lite_amd import knn
    for Q, K, N, C in [(4, 200, 700, 10), (3, 20, 50, 3), (2, 256, 300, 1000)]:
        top_s, top_i, labels = knn_ref.vote_inputs(0, Q, K, N, C)
        ks = sorted({min(k, K) for k in (1, 10, 20, 200)})
        want, want_pred = knn_ref.vote_ref(top_s, top_i, labels, C, ks, float(np.float32(1.0 / 0.07)))
        ds, di = torch.from_numpy(top_s).cuda(), torch.from_numpy(top_i).cuda()
        pred, cs = knn.classify(ds, di, torch.from_numpy(labels), C, ks, 0.07, return_scores=True)
        got = cs.cpu().numpy()
        err = np.abs(got - want) / np.maximum(want, 1e-300)
        print(f"C = {C}: class score error vs float64 {err[want > 0].max():.2e}")
        assert got.shape == want.shape and np.all(got[want == 0] == 0) and err[want > 0].max() <= 1e-5
        ok = knn_ref.separated(want, 1e-4)
        assert (~ok).mean() <= 0.02
        np.testing.assert_array_equal(pred.cpu().numpy()[ok], want_pred[ok])
        assert torch.equal(knn.classify(ds, di, torch.from_numpy(labels), C, ks, 0.07), pred)


def test_selection_passes_over_nan_scores():
    s = knn_ref.tie_scores(2, 300)
    s[0, ::2] = np.nan                                   # 150 scores left for a list of 200
    s[0, :40] = np.nan
    for chunk in (300, 40):
        got_s, got_i = _feed(s, 200, chunk)
        keep = np.flatnonzero(~np.isnan(s[0]))
        want_s, want_i = knn_ref.topk_ref(s[0, keep][None, :], 200)
        n = want_i.shape[1]
        np.testing.assert_array_equal(got_i[0, :n], keep[want_i[0]])
        np.testing.assert_array_equal(got_s[0, :n], want_s[0])
        assert np.all(got_i[0, n:] == 2**31 - 1) and np.all(np.isneginf(got_s[0, n:]))
        want1 = knn_ref.topk_ref(s[1:], 200)
        np.testing.assert_array_equal(got_i[1:], want1[1])


def _image_folder(root, classes, per_class, seed):
    from PIL import Image
    rng = np.random.default_rng(seed)
    for split, n in per_class.items():
        for c, name in enumerate(classes):
            os.makedirs(os.path.join(root, split, name), exist_ok=True)
            for i in range(n):
                img = rng.integers(0, 255, (40, 40, 3))
                img[..., c % 3] = np.clip(img[..., c % 3] + 60, 0, 255)      # a class leaves a colour cast
                Image.fromarray(img.astype(np.uint8)).save(os.path.join(root, split, name, f"{i:03d}.png"))


def test_knn_clf_end_to_end(tmp_path):
    """knn_clf.py on configs/downstream_knn.yaml over an image folder of 36 + 12 images, ResNet-18 at crop 32 with random weights, --k 1 5:
    one evaluation, a well-formed knn_acc.txt, and `Completed!` when the next checkpoint is missing."""
    root = os.path.join(str(tmp_path), "folder")
    _image_folder(root, ["ant", "bee", "cat", "dog", "eel", "fox"], {"train": 6, "val": 2}, 0)
    ck = os.path.join(str(tmp_path), "ck")
    os.makedirs(ck)
    over = ["MODEL.VISUAL.NETWORK_NAME", "resnet18", "MODEL.VISUAL.FEATURE_SIZE", 512, "MODEL.TEXTUAL.NUM_HIDDEN_LAYERS", 1]
    cmd = [sys.executable, os.path.join(ROOT, "knn_clf.py"), "--config", os.path.join(ROOT, "configs", "smoke_random.yaml"), "--config-override",
           *[str(v) for v in over], "--down-config", os.path.join(ROOT, "configs", "downstream_knn.yaml"), "--down-config-override", "DATA.ROOT", root,
           "OPTIM.BATCH_SIZE", "16", "--weight-init", "random", "--checkpoint-dir", ck, "--start-iter", "100", "--freq", "50", "--k", "1", "5",
           "--cpu-workers", "0", "--checkpoints-dir", os.path.join(str(tmp_path), "logs") + "/"]
    r = subprocess.run(cmd, cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    print(r.stdout[-2000:], r.stderr[-3000:])
    assert r.returncode == 0
    assert r.stdout.count("k-NN top-1 (k = ") == 2 and "k-NN top-1 (k = 5): " in r.stdout and r.stdout.rstrip().endswith("Completed!")
    with open(os.path.join(ck, "knn_acc.txt")) as f:
        got = json.load(f)
    assert sorted(got) == ["100"] and sorted(got["100"]) == ["1", "5"]
    for acc in got["100"].values():
        assert set(acc) == {"top1", "top5"} and all(0.0 <= v <= 100.0 for v in acc.values())
        assert acc["top5"] >= acc["top1"]
