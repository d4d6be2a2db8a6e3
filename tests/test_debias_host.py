"""CPU-side checks of the bias evaluation's host layer: the bias_eval command line (defaults, every refusal and its message), the pairs /
queries / gender-annotation readers, the assembly of the result from top-k lists, debias.py refusing what has no kernel path, and the
unchanged defaults of retrieval.embed_images / embed_texts. Runs without a GPU."""
import inspect
import json
import os
import pickle

import numpy as np
import pytest
import torch

from clip_lite_amd import debias, retrieval
from clip_lite_amd.data import GenderAnnotationDataset, read_gender_records
from clip_lite_amd.downstream import (DEFINITIONAL_PAIRS, bias_eval_main, build_bias_eval_parser, read_pairs, read_queries, report_bias)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMOKE = os.path.join(ROOT, "configs", "smoke_random.yaml")
DOWN = os.path.join(ROOT, "configs", "downstream_bias.yaml")


def test_bias_eval_arguments_and_defaults():
    p = build_bias_eval_parser()
    a = p.parse_args(["--query", "a doctor"])
    assert (a.weight_init, a.num_gpus_per_machine, a.split, a.num_results, a.components, a.max_length) == ("vlinfo", 1, "train", 10, 1, 30)
    assert (a.pairs, a.queries, a.output, a.gender_data_path, a.checkpoint_path, a.query) == (None, None, None, None, None, ["a doctor"])
    a = p.parse_args(["--config", "c.yaml", "--config-override", "AMP", "False", "--down-config", "d.yaml", "--down-config-override", "OPTIM.BATCH_SIZE",
                      "8", "--weight-init", "random", "--split", "val", "--pairs", "p.json", "--query", "a doctor", "a nurse", "--queries", "q.txt",
                      "--num-results", "5", "--components", "2", "--max-length", "16", "--output", "o.json", "--gender-data-path", "g"])
    assert a.query == ["a doctor", "a nurse"] and (a.num_results, a.components, a.max_length, a.split) == (5, 2, 16, "val")
    assert a.down_config_override == ["OPTIM.BATCH_SIZE", "8"] and (a.pairs, a.queries, a.output, a.gender_data_path) == ("p.json", "q.txt", "o.json", "g")
    assert len(DEFINITIONAL_PAIRS) == 10 and DEFINITIONAL_PAIRS[0] == ("woman", "man") and DEFINITIONAL_PAIRS[-1] == ("mary", "john")


def test_bias_eval_refusals(tmp_path):
    p = build_bias_eval_parser()
    base = ["--weight-init", "random", "--query", "a doctor", "--config", SMOKE, "--down-config", DOWN]
    two = tmp_path / "two.json"
    two.write_text(json.dumps([["she", "he"], ["her", "his"]]))
    many = tmp_path / "many.json"
    many.write_text(json.dumps([[f"a{i}", f"b{i}"] for i in range(65)]))
    for args, msg in ((["--num-gpus-per-machine", "2"], "one GPU"), (["--num-machines", "2"], "one GPU"),
                      (["--num-gpus-per-machine", "0"], "no CPU path"),
                      (["--weight-init", "imagenet"], "not supported"), (["--weight-init", "torchvision"], "not supported"),
                      (["--weight-init", "clip"], "clip package"), (["--weight-init", "vlinfo"], "needs --checkpoint-path"),
                      (["--components", "0"], r"\[1, 8\]"), (["--components", "9"], r"\[1, 8\]"),
                      (["--pairs", str(two), "--components", "3"], r"\[1, 2\] for 2 pairs"), (["--pairs", str(many)], "at most 64 pairs"),
                      (["--num-results", "0"], r"\[1, 256\]"), (["--num-results", "257"], r"\[1, 256\]"),
                      (["--config-override", "MODEL.LOSS.TYPE", "concat"], "no projection heads"),
                      (["--config-override", "MODEL.LOSS.TYPE", "condot"], "no projection heads"),
                      (["--max-length", "129"], "exceeds the 128 tokens"), (["--max-length", "0"], "exceeds"),
                      (["--max-length", "33", "--config-override", "MODEL.TEXTUAL.NETWORK_NAME", "microsoft/mpnet-base"], "exceeds the 32 tokens")):
        with pytest.raises(SystemExit, match=msg):
            bias_eval_main(p.parse_args(base + args))
    with pytest.raises(SystemExit, match="at least one prompt"):
        bias_eval_main(p.parse_args(["--weight-init", "random", "--config", SMOKE, "--down-config", DOWN]))
    with pytest.raises(SystemExit):
        p.parse_args(base + ["--weight-init", "glove"])


def test_bias_eval_needs_a_gpu(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(SystemExit, match="no GPU visible"):
        bias_eval_main(build_bias_eval_parser().parse_args(["--weight-init", "random", "--query", "a doctor", "--config", SMOKE, "--down-config", DOWN]))


def test_pairs_and_queries_readers(tmp_path):
    f = tmp_path / "pairs.json"
    f.write_text(json.dumps([["woman", "man"], ["girl", "boy"]]))
    assert read_pairs(str(f)) == [("woman", "man"), ("girl", "boy")]
    for bad in ([], [["woman"]], [["woman", "man", "x"]], [["woman", 3]], {"woman": "man"}, [["woman", " "]]):
        f.write_text(json.dumps(bad))
        with pytest.raises(SystemExit, match="two-string lists"):
            read_pairs(str(f))
    q = tmp_path / "queries.txt"
    q.write_text("a doctor\n\n  a nurse  \na person cooking\n")
    assert read_queries(str(q)) == ["a doctor", "a nurse", "a person cooking"]


def test_gender_annotation_reader(tmp_path):
    """The reference's <split>.data: a pickled list of {image_id, file_name, gender}; the image is <root>/<split>2017/<file_name.split("_")[-1]>."""
    records = [{"image_id": 9, "file_name": "COCO_train2014_000000000009.jpg", "gender": [1, 0]},
               {"image_id": 25, "file_name": "COCO_train2014_000000000025.jpg", "gender": np.array([0, 1])},
               {"image_id": 30, "file_name": "000000000030.jpg", "gender": torch.tensor([1, 0])}]
    d = tmp_path / "gender"
    d.mkdir()
    with open(d / "train.data", "wb") as fh:
        pickle.dump(records, fh)
    assert read_gender_records(str(d / "train.data")) == [(9, "000000000009.jpg", 0), (25, "000000000025.jpg", 1), (30, "000000000030.jpg", 0)]
    ds = GenderAnnotationDataset("/data/coco", str(d), "train", image_size=32)
    assert len(ds) == 3 and ds.classes == ["men", "women"] and ds.targets == [0, 1, 0] and ds.image_ids == [9, 25, 30]
    assert ds.samples[1][0] == os.path.join("/data/coco", "train2017", "000000000025.jpg")
    for bad in ([{"image_id": 1, "file_name": "a.jpg", "gender": [1, 1]}], [{"image_id": 1, "file_name": "a.jpg"}], [], {"a": 1}):
        with open(d / "val.data", "wb") as fh:
            pickle.dump(bad, fh)
        with pytest.raises(ValueError):
            read_gender_records(str(d / "val.data"))
    from clip_lite_amd.config import Config
    from clip_lite_amd.factories import DownstreamDatasetFactory
    ds = DownstreamDatasetFactory.from_config(Config(DOWN, ["DATA.ROOT", "/data/coco"]), split="train", gender_data_path=str(d))
    assert isinstance(ds, GenderAnnotationDataset) and ds.image_transform == ("smallest_resize", "center_crop", "normalize")
    with pytest.raises(ValueError, match="COCO"):
        DownstreamDatasetFactory.from_config(Config(DOWN, []), split="train", gender_data_path=str(d))
    two = DownstreamDatasetFactory.from_config(Config(DOWN, []), split="val", num_classes=2)
    assert two.num_classes == 2 and len(two) == 500 and {two.label(i) for i in range(len(two))} == {0, 1}
    assert DownstreamDatasetFactory.from_config(Config(DOWN, []), split="val").num_classes == 10          # the default is unchanged


def test_result_assembly_from_given_lists():
    groups = np.array([0, 1, 0, 1, 1, 0])
    gs = np.array([[[0.9, 0.5], [0.8, 0.2]]], np.float32)                # one prompt, two groups, k = 2
    gi = np.array([[[0, 2], [1, 4]]])
    lists = {"biased": (gs, gi, np.array([[0, 1]])), "debiased": (gs / 2, gi[:, :, ::-1], np.array([[3, 4]]))}
    res = debias.assemble(groups, 2, 2, lists, [1.5, -0.5], [0.75])
    assert res["k"] == 2 and res["num_groups"] == 2 and res["num_images"] == 6 and res["group_sizes"] == [3, 3]
    assert res["prior"] == [1.5, -0.5] and res["explained_variance_ratio"] == [0.75]
    np.testing.assert_allclose(res["mean_alignment"]["biased"], [[0.7, 0.5]], rtol=1e-6)
    np.testing.assert_allclose(res["mean_alignment"]["debiased"], [[0.35, 0.25]], rtol=1e-6)
    assert res["share"] == {"biased": [[0.5, 0.5]], "debiased": [[0.0, 1.0]]}
    assert res["top_indices"]["debiased"] == [[[2, 0], [4, 1]]]
    np.testing.assert_allclose(res["top_scores"]["biased"], gs.astype(np.float64))
    assert json.loads(json.dumps(res)) == res                           # plain Python all the way down
    lines = report_bias(res, ["a doctor"], ["men", "women"])
    assert lines[0] == "prompt 'a doctor'" and "Mean Alignment | men | Biased: 0.700000 | Debiased: 0.350000" in lines[1]
    assert "Mean Alignment | women | Biased: 0.500000 | Debiased: 0.250000" in lines[2] and "0.500 -> 1.000 (prior 0.500)" in lines[2]
    with pytest.raises(ValueError, match="shapes"):
        debias.assemble(groups, 2, 3, lists, [0, 0], [1.0])


def test_group_checks():
    g, G = debias.check_groups(torch.tensor([0, 1, 1, 0, 2, 2]), 6, 2)
    assert G == 3 and g.tolist() == [0, 1, 1, 0, 2, 2]
    for groups, k, msg in (([0, 1, 1], 2, "exceeds the smallest group's 1 images"), ([0, 0, 0], 1, "2 <= G <= 8"), ([0, 1, 9], 1, "2 <= G <= 8"),
                           ([0, -1, 1], 1, "2 <= G <= 8"), ([0.0, 1.0], 1, "integers"), ([0, 1], 0, r"\[1, 256\]"), ([0, 1] * 300, 257, r"\[1, 256\]")):
        with pytest.raises(ValueError, match=msg):
            debias.check_groups(groups, len(groups), k)
    with pytest.raises(ValueError, match="5 group labels for 6 images"):
        debias.check_groups([0, 1, 0, 1, 0], 6, 1)


def test_host_tensors_and_bad_shapes_are_refused_before_any_launch():
    x, v = torch.zeros(4, 16), torch.zeros(1, 16)
    with pytest.raises(RuntimeError, match="no CPU path"):
        debias.remove(x, v)
    with pytest.raises(RuntimeError, match="no CPU path"):
        debias.directions(x, x)
    with pytest.raises(RuntimeError, match="no CPU path"):
        debias.evaluate(x, [0, 1, 0, 1], v, v, 1)
    for bad in (torch.zeros(4, 12), torch.zeros(4, 4104), torch.zeros(0, 16), torch.zeros(16), torch.zeros(4, 16, dtype=torch.int32)):
        with pytest.raises(ValueError):
            debias.remove(bad, v)


def test_embed_defaults_are_unchanged():
    for fn in (retrieval.embed_images, retrieval.embed_texts):
        sig = inspect.signature(fn)
        assert sig.parameters["normalize"].default is True and sig.parameters["batch_size"].default == 128
        assert list(sig.parameters)[-1] == "normalize"                 # appended: positional callers are unaffected
