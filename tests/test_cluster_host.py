"""CPU-side checks of clustered negative sampling's host side: data.ClusteredDataset (option discovery, the linear schedule, negatives from the
item's cluster, the singleton fallback, reproducible draws, collate contract, errors), NegativeSamplingDatasetFactory, init_dataloaders
(type="clusters") and utils.common.cycle calling update_iter without a distributed sampler."""
import argparse
import os
import pickle

import pytest
import torch

from clip_lite_amd import data as D
from clip_lite_amd.config import Config


def _write_maps(root, split, n, ks, fn=lambda i, k: i % k):
    os.makedirs(root, exist_ok=True)
    for k in ks:
        with open(os.path.join(root, f"img_id_cluster_map_{split}_{k}.pkl"), "wb") as fh:
            pickle.dump({i: int(fn(i, k)) for i in range(n)}, fh, protocol=pickle.HIGHEST_PROTOCOL)
    return str(root)


def _base(n=40):
    return D.RandomDataset(image_size=16, length=n, seed=3)


def test_option_discovery_and_missing_assets(tmp_path):
    root = _write_maps(tmp_path / "c", "train", 10, [10, 2, 5])
    _write_maps(root, "val", 10, [3])
    open(os.path.join(root, "img_id_caption_map_train.pkl"), "wb").close()
    open(os.path.join(root, "img_id_cluster_map_train_x.pkl"), "wb").close()
    assert D.get_cluster_options(root, "train") == [2, 5, 10]
    assert D.get_cluster_options(root, "val") == [3]
    assert D.get_cluster_options(root, "test") == []
    with pytest.raises(FileNotFoundError, match="cluster.py"):
        D.get_cluster_options(str(tmp_path / "nope"), "train")
    with pytest.raises(FileNotFoundError, match="cluster.py"):
        D.ClusteredDataset(_base(10), root, "test")


def test_schedule_follows_the_reference_formula(tmp_path):
    root = _write_maps(tmp_path / "c", "train", 40, range(2, 11))
    ds = D.ClusteredDataset(_base(), root, "train", total_iters=1100, negative_sampling_start_iter=100)
    assert ds.cluster_options == list(range(2, 11))
    assert ds.scheduled_option(100) == 2                      # pred 0: the closest option is the smallest
    assert ds.scheduled_option(600) == 5                      # pred 10 * 500 / 1000 = 5
    assert ds.scheduled_option(1100) == 10
    assert ds.scheduled_option(350) == 2                      # pred 2.5: an exact tie between 2 and 3 goes to the smaller
    assert ds.scheduled_option(351) == 3
    for it in (100, 230, 777, 1100):
        pred = 10 * (it - 100) / 1000
        assert abs(ds.scheduled_option(it) - pred) == min(abs(k - pred) for k in range(2, 11))
    ds.update_iter(600)
    ds.negative_index(0)
    assert ds.iter_num == 600 and ds.num_clusters == 5          # loaded lazily, on first use after the change


def test_negatives_share_the_cluster_and_differ_from_the_item(tmp_path):
    n = 40
    root = _write_maps(tmp_path / "c", "train", n, [4])
    ds = D.ClusteredDataset(_base(n), root, "train", total_iters=10, negative_sampling_start_iter=0, seed=7)
    first = [ds.negative_index(i) for i in range(n)]
    for i, j in enumerate(first):
        assert j != i and j % 4 == i % 4
    assert first == [ds.negative_index(i) for i in range(n)]              # the same iter_num: the same negatives
    ds.update_iter(1)
    second = [ds.negative_index(i) for i in range(n)]
    assert second != first and all(j != i and j % 4 == i % 4 for i, j in enumerate(second))
    seen = {ds.negative_index(0) for it in range(200) if ds.update_iter(it) is None}
    assert seen == set(range(4, n, 4))                                     # every other member can be drawn
    item = ds[5]
    neg = ds.base[ds.negative_index(5)]
    assert torch.equal(item["neg_image"], neg["image"]) and torch.equal(item["neg_caption_tokens"], neg["caption_tokens"])
    assert torch.equal(item["image"], ds.base[5]["image"]) and int(item["image_id"]) == 5


def test_singleton_cluster_falls_back_to_the_whole_dataset(tmp_path):
    n = 12
    root = _write_maps(tmp_path / "c", "train", n, [3], fn=lambda i, k: 2 if i == 7 else i % 2)
    ds = D.ClusteredDataset(_base(n), root, "train", total_iters=50)
    seen = set()
    for it in range(100):
        ds.update_iter(it)
        j = ds.negative_index(7)
        assert j != 7 and 0 <= j < n
        seen.add(j)
    assert len(seen) > 5


def test_missing_id_names_the_file(tmp_path):
    root = _write_maps(tmp_path / "c", "train", 10, [2])
    ds = D.ClusteredDataset(_base(12), root, "train")
    with pytest.raises(KeyError, match="img_id_cluster_map_train_2.pkl"):
        ds.negative_index(11)


def test_collate_keys_dtypes_and_independent_padding(tmp_path):
    class Captions(D.RandomDataset):
        def caption(self, idx):
            return "a cat" if idx % 2 == 0 else "a very large dog sleeping on the left side of a long couch"
    n = 8
    root = _write_maps(tmp_path / "c", "train", n, [2])
    ds = D.ClusteredDataset(Captions(image_size=16, length=n), root, "train")
    batch = ds.collate_fn([ds[0], ds[2]])                       # short positives; cluster 0 = the even rows: short negatives as well
    assert list(batch) == ["image_id", "image", "input_ids", "attention_mask", "neg_image", "neg_input_ids", "neg_attention_mask"]
    assert batch["neg_image"].shape == batch["image"].shape == (2, 3, 16, 16) and batch["neg_image"].dtype == torch.float32
    for k in ("input_ids", "attention_mask", "neg_input_ids", "neg_attention_mask"):
        assert batch[k].dtype == torch.long
    mixed = ds.collate_fn([ds[0], ds[1]])
    assert mixed["input_ids"].shape[1] > batch["input_ids"].shape[1]
    root2 = _write_maps(tmp_path / "d", "train", n, [2], fn=lambda i, k: (i // 2) % 2)      # clusters mix short and long captions
    ds2 = D.ClusteredDataset(Captions(image_size=16, length=n), root2, "train")
    items = [ds2[0], ds2[4]]                                   # positives short; negatives from {1, 4, 5} / {0, 1, 5}
    b2 = ds2.collate_fn(items)
    assert b2["input_ids"].shape[1] == batch["input_ids"].shape[1]
    assert b2["neg_input_ids"].shape[1] == max(len(i["neg_caption_tokens"]) for i in items)
    assert int(b2["neg_attention_mask"].sum()) == sum(len(i["neg_caption_tokens"]) for i in items)
    assert (b2["neg_input_ids"][b2["neg_attention_mask"] == 0] == 0).all()


def _config(tmp_path, cluster_path, extra=()):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return Config(os.path.join(root, "configs", "smoke_random_clusters.yaml"), ["DATA.CLUSTER_PATH", cluster_path, "DATA.IMAGE_CROP_SIZE", 32] + list(extra))


def test_factory_and_init_dataloaders_clusters(tmp_path):
    from clip_lite_amd import train_loop
    from clip_lite_amd.factories import NegativeSamplingDatasetFactory
    root = _write_maps(tmp_path / "c", "train", 118000, [2, 3])
    _C = _config(tmp_path, root)
    ds = NegativeSamplingDatasetFactory.from_config(_C, split="train")
    assert isinstance(ds, D.ClusteredDataset) and ds.total_iters == 8 and ds.start_iter == 3 and len(ds) == 118000
    _A = argparse.Namespace(cpu_workers=0)
    train, val = train_loop.init_dataloaders(_C, _A, type="clusters")
    assert train.batch_size == 16 and val.batch_size == 16                       # (BATCH_SIZE // world) // 2
    assert isinstance(train.dataset, D.ClusteredDataset) and not isinstance(val.dataset, D.ClusteredDataset)      # no val maps: the normal val set
    batch = next(iter(train))
    assert batch["image"].shape[0] == batch["neg_image"].shape[0] == 16 and "neg_input_ids" in batch
    _write_maps(root, "val", 5000, [2])
    _, val = train_loop.init_dataloaders(_C, _A, type="clusters")
    assert isinstance(val.dataset, D.ClusteredDataset)
    normal, _ = train_loop.init_dataloaders(_C, _A, type="normal")
    assert normal.batch_size == 32 and "neg_image" not in next(iter(normal))


def test_missing_cluster_path_fails_at_start_up_naming_cluster_py(tmp_path):
    from clip_lite_amd import train_loop
    for path in ("", str(tmp_path / "empty")):
        if path:
            os.makedirs(path)
        _C = _config(tmp_path, path, ["DATA.NEGATIVE_SAMPLING_START_ITERATION", 250000])
        with pytest.raises(FileNotFoundError, match="cluster.py"):
            train_loop.check_cluster_assets(_C)
        with pytest.raises(FileNotFoundError, match="cluster.py"):
            train_loop.init_dataloaders(_C, argparse.Namespace(cpu_workers=0), type="clusters")


def test_cycle_updates_the_iteration_without_a_distributed_sampler(tmp_path):
    from torch.utils.data import DataLoader
    from clip_lite_amd.utils.common import cycle
    n = 8
    root = _write_maps(tmp_path / "c", "train", n, [2, 4])
    ds = D.ClusteredDataset(_base(n), root, "train", total_iters=20, negative_sampling_start_iter=0)
    calls = []
    orig = ds.update_iter
    ds.update_iter = lambda it: (calls.append(it), orig(it))[1]
    loader = DataLoader(ds, batch_size=4, shuffle=False, collate_fn=ds.collate_fn)
    it = cycle(loader, torch.device("cpu"), start_iteration=5, type="clusters", prefetch=0)
    batches = [next(it) for _ in range(5)]
    assert calls[:3] == [5, 7, 9]                               # the start of every pass of two batches
    assert all("neg_image" in b for b in batches)
    calls.clear()
    it = cycle(DataLoader(ds, batch_size=4, collate_fn=ds.collate_fn), torch.device("cpu"), 0, type="normal", prefetch=0)
    next(it)
    assert calls == []
