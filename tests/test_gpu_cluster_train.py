"""GPU checks of clustered negative sampling end to end: cluster.py's CLI on a small generated JSON dataset (every file written, maps against
tests/kmeans_ref.py on the embeddings it saved, --encodings reproducing them), and train_loop.main on configs/smoke_random_clusters.yaml
with the captured graphs on (the switch, the re-capture, bit-identical steps before the switch, resume onto the clustered loader)."""
import json
import os
import pickle

import numpy as np
import pytest
import torch

import kmeans_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _json_dataset(tmp_path, n=60, seed=0):
    rng = np.random.default_rng(seed)
    words = ["dog", "cat", "red", "blue", "runs", "sits", "on", "grass", "a", "the", "ball", "man", "woman", "street", "water"]
    recs = [{"image": "", "caption": " ".join(rng.choice(words, rng.integers(3, 9)))} for _ in range(n)]
    path = tmp_path / "train.json"
    path.write_text(json.dumps(recs))
    cfg = tmp_path / "c.yaml"
    cfg.write_text("RANDOM_SEED: 0\nAMP: false\nMODEL:\n  NAME: json\n  VISUAL:\n    NETWORK_NAME: resnet18\n    FEATURE_SIZE: 512\n"
                   f"  TEXTUAL:\n    NUM_HIDDEN_LAYERS: 2\nDATA:\n  JSON_FILES_TRAIN: ['{path}']\n  JSON_FILES_VAL: ['{path}']\n")
    return recs, str(cfg)


def test_cluster_cli_writes_the_reference_layout(tmp_path):
    from clip_lite_amd import kmeans
    from clip_lite_amd.downstream import cluster_cli
    recs, cfg = _json_dataset(tmp_path)
    n = len(recs)
    # the text encoder of a deterministically filled checkpoint (tests/detfill.py). (The default initialisation puts all 60 embeddings so close
    # together that 1.7 - 6.7 % of the rows sit under tau_n at the result, over the cap before any kernel has run; with this fill no row does.)
    from clip_lite_amd.config import Config
    from clip_lite_amd.factories import PretrainingModelFactory
    from clip_lite_amd.utils.checkpointing import CheckpointManager
    from detfill import det_fill
    os.makedirs(tmp_path / "ck")
    CheckpointManager(str(tmp_path / "ck"), model=det_fill(PretrainingModelFactory.from_config(Config(cfg, [])))).step(1)
    args = ["--config", cfg, "--checkpoint-path", str(tmp_path / "ck" / "checkpoint_1.pth"), "--cluster-root", str(tmp_path / "out"),
            "--min-clusters", "2", "--max-clusters", "4"]
    results = cluster_cli(args)
    out = tmp_path / "out" / "clusters_4"
    load = lambda name: pickle.load(open(out / name, "rb"))
    assert sorted(os.listdir(out)) == sorted([f"img_id_cluster_map_train_{k}.pkl" for k in (2, 3, 4)] +
                                             [f"img_id_{m}_map_train.pkl" for m in ("caption", "filename", "encoding")])
    caps, enc = load("img_id_caption_map_train.pkl"), load("img_id_encoding_map_train.pkl")
    assert caps == {i: [recs[i]["caption"]] for i in range(n)} and sorted(enc) == list(range(n))
    X = np.stack([enc[i] for i in range(n)])
    assert X.dtype == np.float32 and X.shape == (n, 768)
    np.testing.assert_allclose(np.linalg.norm(X.astype(np.float64), axis=1), 1.0, atol=1e-5)
    for K in (2, 3, 4):
        cmap = load(f"img_id_cluster_map_train_{K}.pkl")
        assert sorted(cmap) == list(range(n)) and all(type(k) is int and type(v) is int for k, v in cmap.items())
        got = np.array([cmap[i] for i in range(n)])
        np.testing.assert_array_equal(got, results[K]["assign"].cpu().numpy())
        ref = R.lloyd(X, X[kmeans.init_rows(n, K, 1234).numpy()])
        print(f"K = {K}: reference {ref['iterations']} iterations, largest share under tau_n {100 * ref['max_exempt_share']:.3f} %")
        if ref["max_exempt_share"] == 0.0:
            np.testing.assert_array_equal(got, ref["assign"])
        else:                                   # a boundary row at some iteration: the two runs may part; the result must still be a fixed point
            C = results[K]["centroids"].cpu().numpy()
            a64, _, gap = R.assign_step(X, C)
            ex = R.exempt_rows(X, C, gap)
            print(f"K = {K}: rows under tau_n at the result: {100 * ex.mean():.3f} %")
            assert ex.mean() <= R.EXEMPT_CAP
            np.testing.assert_array_equal(got[~ex], a64[~ex])
    again = cluster_cli(["--config", cfg, "--cluster-root", str(tmp_path / "out2"), "--min-clusters", "2", "--max-clusters", "4",
                         "--encodings", str(out / "img_id_encoding_map_train.pkl")])
    for K in (2, 3, 4):
        a = pickle.load(open(tmp_path / "out2" / "clusters_4" / f"img_id_cluster_map_train_{K}.pkl", "rb"))
        assert a == load(f"img_id_cluster_map_train_{K}.pkl")
        assert torch.equal(again[K]["centroids"], results[K]["centroids"])


def _maps(root, split, n, ks):
    os.makedirs(root, exist_ok=True)
    for k in ks:
        with open(os.path.join(root, f"img_id_cluster_map_{split}_{k}.pkl"), "wb") as fh:
            pickle.dump({i: i % k for i in range(n)}, fh, protocol=pickle.HIGHEST_PROTOCOL)
    return str(root)


def _run_main(monkeypatch, tmp_path, tag, overrides, resume=None, snapshot_at=2):
    from clip_lite_amd import train_loop
    log = {"calls": [], "snap": None, "recaptures": 0}

    class Recording(train_loop.TrainStep):
        def __call__(self, batch):
            out = super().__call__(batch)
            log["calls"].append({"keys": sorted(batch), "rows": int(batch["image"].shape[0]), "replays": self.replays, "eager": self.eager_steps,
                                 "loss": float(out["loss"].detach())})
            if len(log["calls"]) == snapshot_at:
                self.finish()
                torch.cuda.synchronize()
                log["snap"] = {n: p.detach().clone() for n, p in self.model.named_parameters()}
            return out

        def recapture(self):
            log["recaptures"] += 1
            log["at_recapture"] = (self.replays, self.eager_steps)
            return super().recapture()

    monkeypatch.setattr(train_loop, "TrainStep", Recording)
    argv = ["--config", os.path.join(ROOT, "configs", "smoke_random_clusters.yaml"), "--config-override", "DATA.IMAGE_CROP_SIZE", "64"] + \
        [str(o) for o in overrides] + ["--checkpoints-dir", str(tmp_path / tag), "--num-gpus-per-machine", "1", "--cpu-workers", "0",
                                       "--checkpoint-every", "4", "--log-every", "100"]
    if resume:
        argv += ["--resume-from", resume]
    _A = train_loop.build_parser().parse_args(argv)
    train_loop.main(_A)
    return log


def _check_switch(log, start, total=8):
    """Batches, and which launch path every step took, for a switch at iteration `start` (graph warm-up: 2 eager steps, then capture)."""
    calls = log["calls"]
    assert len(calls) == total and all(np.isfinite(c["loss"]) for c in calls)
    for c in calls[:start - 1]:                        # before the switch: the normal loader
        assert c["rows"] == 32 and "neg_image" not in c["keys"]
    for c in calls[start - 1:]:                        # from the switch on: half the rows plus their negatives
        assert c["rows"] == 16 and {"neg_image", "neg_input_ids", "neg_attention_mask"} <= set(c["keys"])
    assert log["recaptures"] == 1
    r0, e0 = log["at_recapture"]
    assert (r0, e0) == (max(start - 3, 0), 2)          # replays before the switch: every step after the two warm-up steps
    eager_after = [c["eager"] - e0 for c in calls[start - 1:]]
    replays_after = [c["replays"] - r0 for c in calls[start - 1:]]
    print(f"switch at {start}: eager steps after it {eager_after}, replays after it {replays_after}")
    n = total - start + 1
    assert eager_after == [1] + [2] * (n - 1)          # the eager count stops at the warm-up count
    assert replays_after == [0, 0] + list(range(1, n - 1))        # and the re-captured step is replayed from the third clustered step on


def test_train_switches_recaptures_and_resumes(monkeypatch, tmp_path, deterministic_reductions):
    """configs/smoke_random_clusters.yaml as written (switch at iteration 3 of 8), graphs on."""
    cpath = _maps(tmp_path / "clusters", "train", 118000, [2, 3, 4])
    log = _run_main(monkeypatch, tmp_path, "a", ["DATA.CLUSTER_PATH", cpath])
    _check_switch(log, 3)

    normal = _run_main(monkeypatch, tmp_path, "b", ["DATA.NEGATIVE_SAMPLING", "normal"])
    assert all("neg_image" not in c["keys"] and c["rows"] == 32 for c in normal["calls"]) and normal["recaptures"] == 0
    for name, p in log["snap"].items():                # the parameters after iteration 2 are those of a run without the switch, bit for bit
        assert torch.equal(p, normal["snap"][name]), name

    ckpts = [os.path.join(d, f) for d, _, fs in os.walk(tmp_path / "a") for f in fs if f == "checkpoint_4.pth"]
    assert len(ckpts) == 1
    resumed = _run_main(monkeypatch, tmp_path, "a", ["DATA.CLUSTER_PATH", cpath], resume=ckpts[0], snapshot_at=-1)
    assert len(resumed["calls"]) == 4 and resumed["recaptures"] == 0
    assert all(c["rows"] == 16 and "neg_image" in c["keys"] for c in resumed["calls"])      # directly on the clustered loader
    assert [c["eager"] for c in resumed["calls"]] == [1, 2, 2, 2] and [c["replays"] for c in resumed["calls"]] == [0, 0, 1, 2]


def test_recapture_drops_live_graphs_at_a_later_switch(monkeypatch, tmp_path, deterministic_reductions):
    """Switch at iteration 5: iterations 3 and 4 replay the captured normal step, so recapture() has live graphs (and a deferred update) to drop."""
    cpath = _maps(tmp_path / "clusters", "train", 118000, [2, 3, 4])
    log = _run_main(monkeypatch, tmp_path, "a", ["DATA.CLUSTER_PATH", cpath, "DATA.NEGATIVE_SAMPLING_START_ITERATION", 5], snapshot_at=4)
    _check_switch(log, 5)
    normal = _run_main(monkeypatch, tmp_path, "b", ["DATA.NEGATIVE_SAMPLING", "normal"], snapshot_at=4)
    for name, p in log["snap"].items():                # replayed steps before the switch as well
        assert torch.equal(p, normal["snap"][name]), name


def test_missing_cluster_path_stops_the_run_at_start_up(monkeypatch, tmp_path):
    with pytest.raises(FileNotFoundError, match="cluster.py"):
        _run_main(monkeypatch, tmp_path, "c", ["DATA.NEGATIVE_SAMPLING_START_ITERATION", 250000])
