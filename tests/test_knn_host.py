"""CPU-side checks of the k-NN evaluation's host layer: the knn_clf command line (defaults, launch refusals and their messages), the merging
of knn_acc.txt over checkpoints, the unchanged voc_clf.py loop, and knn.topk / knn.classify refusing what has no kernel path."""
import json
import os

import pytest
import torch

from clip_lite_amd import knn
from clip_lite_amd.downstream import _report_knn, build_knn_parser, knn_clf_main, run_checkpoint_loop

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_knn_clf_arguments_and_errors():
    p = build_knn_parser()
    a = p.parse_args(["--checkpoint-dir", "d"])
    assert (a.freq, a.start_iter, a.weight_init, a.num_gpus_per_machine, a.k, a.temperature) == (46200, 46200, "vlinfo", 1, [10, 20, 100, 200], 0.07)
    a = p.parse_args(["--config", "c.yaml", "--down-config", "d.yaml", "--down-config-override", "OPTIM.BATCH_SIZE", "8", "--weight-init", "random",
                      "--checkpoint-dir", "x", "--freq", "10", "--start-iter", "20", "--cpu-workers", "0", "--k", "1", "5", "--temperature", "0.1"])
    assert a.down_config_override == ["OPTIM.BATCH_SIZE", "8"] and (a.freq, a.start_iter, a.k, a.temperature) == (10, 20, [1, 5], 0.1)
    with pytest.raises(SystemExit):
        p.parse_args([])                                # --checkpoint-dir is required
    with pytest.raises(SystemExit):
        p.parse_args(["--checkpoint-dir", "x", "--weight-init", "clip"])
    for args, msg in ((["--num-gpus-per-machine", "0"], "no CPU path"), (["--num-gpus-per-machine", "2"], "one GPU"),
                      (["--weight-init", "imagenet"], "not supported"), (["--weight-init", "torchvision"], "not supported"),
                      (["--k", "257"], r"\[1, 256\]"), (["--k", "0", "5"], r"\[1, 256\]"), (["--k"] + [str(k) for k in range(1, 10)], "at most 8"),
                      (["--temperature", "0"], "positive")):
        with pytest.raises(SystemExit, match=msg):
            knn_clf_main(p.parse_args(["--checkpoint-dir", "x"] + args))


def test_knn_clf_needs_a_gpu(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(SystemExit, match="no GPU visible"):
        knn_clf_main(build_knn_parser().parse_args(["--checkpoint-dir", "x", "--weight-init", "random"]))


def _fake_checkpoints(d, its):
    for it in its:
        open(os.path.join(d, f"checkpoint_{it}.pth"), "w").close()
    loaded = []

    def load(path):
        if not os.path.exists(path):
            raise FileNotFoundError(path)
        loaded.append(os.path.basename(path))
    return loaded, load


def test_knn_acc_file_merges_over_checkpoints(tmp_path, capsys):
    d = str(tmp_path)
    with open(os.path.join(d, "knn_acc.txt"), "w") as f:
        json.dump({"10": {"20": {"top1": 1.5}}}, f)
    loaded, load = _fake_checkpoints(d, (30,))
    evals = iter([{1: {"top1": 25.0, "top5": 50.0}, 20: {"top1": 30.0, "top5": 60.0}}, {1: {"top1": 35.0}, 20: {"top1": 40.125}}])
    res = run_checkpoint_loop(d, 20, 10, lambda: next(evals), load, filename="knn_acc.txt", report=_report_knn)
    assert loaded == ["checkpoint_30.pth"]
    with open(os.path.join(d, "knn_acc.txt")) as f:
        got = json.load(f)
    assert got == res == {"10": {"20": {"top1": 1.5}}, "20": {"1": {"top1": 25.0, "top5": 50.0}, "20": {"top1": 30.0, "top5": 60.0}},
                          "30": {"1": {"top1": 35.0}, "20": {"top1": 40.125}}}
    out = capsys.readouterr().out
    assert "k-NN top-1 (k = 20): 30.00 | top-5: 60.00" in out and "k-NN top-1 (k = 20): 40.12\n" in out
    assert out.count("k-NN top-1 (k = ") == 4 and "Test mAP" not in out and out.rstrip().endswith("Completed!")
    assert not os.path.exists(os.path.join(d, "voc07_mAP.txt"))


def test_voc_loop_output_is_unchanged(tmp_path, capsys):
    """run_checkpoint_loop as voc_clf_main calls it: voc07_mAP.txt, `Test mAP: <mAP x 100>` and `Completed!`, byte for byte."""
    d = str(tmp_path)
    loaded, load = _fake_checkpoints(d, (150,))
    maps = iter([0.25, 1 / 3])
    res = run_checkpoint_loop(d, 100, 50, lambda: next(maps), load)
    assert loaded == ["checkpoint_150.pth"]
    assert capsys.readouterr().out == "Test mAP: 25.0\nTest mAP: " + str(1 / 3 * 100) + "\nCompleted!\n"
    with open(os.path.join(d, "voc07_mAP.txt")) as f:
        raw = f.read()
    assert raw == json.dumps({"100": 25.0, "150": 1 / 3 * 100}) and json.loads(raw) == res
    assert os.listdir(d).count("knn_acc.txt") == 0


def test_topk_and_classify_refuse_what_has_no_kernel_path():
    x, z = torch.zeros(4, 16), torch.zeros(300, 16)
    with pytest.raises(RuntimeError, match="no CPU path"):
        knn.topk(x, z, 3)
    with pytest.raises(ValueError, match=r"\[1, 256\]"):
        knn.topk(x, z, 257)
    with pytest.raises(ValueError, match=r"\[1, 256\]"):
        knn.topk(x, z, 0)
    with pytest.raises(ValueError, match="exceeds the bank's 3 rows"):
        knn.topk(x, z[:3], 4)
    with pytest.raises(ValueError, match="multiple of 8"):
        knn.topk(torch.zeros(4, 12), torch.zeros(30, 12), 3)
    with pytest.raises(ValueError, match="features"):
        knn.topk(x, torch.zeros(30, 24), 3)
    with pytest.raises(ValueError, match="f32"):
        knn.topk(x.double(), z.double(), 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        knn.classify(torch.zeros(2, 4), torch.zeros(2, 4, dtype=torch.int32), torch.zeros(9, dtype=torch.long), 3, [1, 4])
    with pytest.raises(ValueError, match="no k"):
        knn.knn_eval(z[:5], torch.zeros(5), x, torch.zeros(4), 3, ks=(10, 20))


def test_knn_config_and_entry_script():
    from clip_lite_amd.config import Config
    c = Config(os.path.join(ROOT, "configs", "downstream_knn.yaml"), [])
    assert c.DATA.ROOT == "random" and c.DATA.IMAGE_CROP_SIZE == 32
    assert list(c.DATA.IMAGE_TRANSFORM_TRAIN) == list(c.DATA.IMAGE_TRANSFORM_VAL)       # the bank is not augmented
    src = open(os.path.join(ROOT, "knn_clf.py")).read()
    assert "knn_clf_cli" in src


def test_hip_wrappers_on_the_simulator_build(monkeypatch):
    """hip.knn_topk_merge / hip.knn_vote (their asserts and argument order) on host tensors through the wave-simulator build of the same
    sources: the lists equal the stable argsort and the class scores float64's, with and without the class_scores output."""
    import ctypes as C
    import numpy as np
    import knn_ref
    import simlib
    from clip_lite_amd import hip
    simlib.build_sim()
    monkeypatch.setattr(hip, "_lib", hip._bind(C.CDLL(simlib.SIM_SO)))
    monkeypatch.setattr(hip, "_allow_host_tensors", True)
    Q, N, K, Cn = 2, 40, 8, 6
    s = knn_ref.tie_scores(Q, N)
    top_s, top_i = torch.empty(Q, K), torch.empty(Q, K, dtype=torch.int32)
    for base in (0, 24):
        nc = min(24, N - base)
        hip.knn_topk_merge(torch.from_numpy(np.ascontiguousarray(s[:, base:base + nc])), nc, Q, nc, base, K, min(K, base), top_s, top_i)
    want_s, want_i = knn_ref.topk_ref(s, K)
    assert np.array_equal(top_i.numpy(), want_i) and np.array_equal(top_s.numpy(), want_s)
    labels = torch.arange(N, dtype=torch.int32) % Cn
    unit = (top_s / 64).contiguous()
    want, want_pred = knn_ref.vote_ref(unit.numpy(), want_i, labels.numpy(), Cn, [1, 8], float(np.float32(1 / 0.07)))
    pred, cs = torch.empty(2, Q, 5, dtype=torch.int32), torch.empty(2, Q, Cn)
    hip.knn_vote(unit, top_i, labels, Q, K, N, Cn, [1, 8], float(np.float32(1 / 0.07)), cs, pred)
    np.testing.assert_allclose(cs.numpy(), want, rtol=1e-5, atol=0)
    pred2 = torch.empty_like(pred)
    hip.knn_vote(unit, top_i, labels, Q, K, N, Cn, [1, 8], float(np.float32(1 / 0.07)), None, pred2)
    assert torch.equal(pred, pred2) and np.array_equal(pred.numpy()[1][:, 0], want_pred[1][:, 0])
    with pytest.raises(AssertionError):
        hip.knn_vote(unit, top_i, labels, Q, K, N, Cn, [1, 8], 1.0, torch.empty(2, Q, Cn - 1), pred)       # class_scores too small
