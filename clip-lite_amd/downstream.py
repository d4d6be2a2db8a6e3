"""Command lines of the downstream evaluations: `linear_clf.py` (linear probe / fine-tune, reference linear_clf.py:25-300) and `zero_shot.py`
(reference zero_shot.py), on ImageClassifier / zero_shot_counts (classify.py); `voc_clf.py` (svm.py), `knn_clf.py` (knn.py), `logreg_clf.py`
(logreg.py), `retrieval.py` (retrieval.py) and `bias_eval.py` (debias.py). One GPU: the reference's multi-GPU launch, hipGraph capture of the classification step, and the `clip` / `imagenet`
initialisations (the `clip` package, torchvision downloads) are not available."""
import argparse
import os

import torch
from torch.utils.data import DataLoader, DistributedSampler

from .classify import ImageClassifier, TopkAccuracy, cross_entropy, zero_shot_counts
from .config import Config
from .factories import DownstreamDatasetFactory, LRSchedulerFactory, OptimizerFactory, PretrainingModelFactory
from .utils.base import Timer
from .utils.checkpointing import CheckpointManager
from .utils.common import common_parser, common_setup, cycle, logger


def build_linear_clf_parser():
    parser = common_parser(description="Do image classification with linear models and frozen feature extractor, or fine-tune the feature "
                                       "extractor end-to-end.")
    parser.set_defaults(num_gpus_per_machine=1)
    group = parser.add_argument_group("Downstream config arguments.")
    group.add_argument("--down-config", metavar="FILE", help="Path to a downstream config file.")
    group.add_argument("--down-config-override", nargs="*", default=[], help="A list of key-value pairs to modify downstream config params.")
    group = parser.add_argument_group("Checkpointing and Logging")
    group.add_argument("--weight-init", choices=["random", "imagenet", "torchvision", "vlinfo", "clip"], default="vlinfo",
                       help="'random': random weights; 'vlinfo': the backbone of a pretraining checkpoint (--checkpoint-path). 'imagenet', "
                            "'torchvision' and 'clip' are not supported (downloads, the clip package); resume a run of this script with --resume-from.")
    group.add_argument("--log-every", type=int, default=500, help="Log the training loss after every these many iterations.")
    group.add_argument("--checkpoint-path", help="Checkpoint to initialise from (vlinfo: a pretraining checkpoint).")
    group.add_argument("--checkpoint-every", type=int, default=10000, help="Validate and serialize after every these many iterations.")
    group.add_argument("--resume-from", type=str, default=None, help="Resume training from a checkpoint of this script.")
    group.add_argument("--serialization-dir", default=None, help="Where checkpoints go (default: <checkpoint-path dir>/<dataset>, or "
                                                                 "<checkpoints-dir><RUN_ID> without a checkpoint path).")
    return parser


def _check_launch(_A):
    if _A.num_gpus_per_machine > 1 or _A.num_machines > 1:
        raise SystemExit("linear_clf: runs on one GPU (--num-gpus-per-machine 1); multi-GPU data parallelism of the classification step is "
                         "not implemented")
    if _A.num_gpus_per_machine == 0:
        raise SystemExit("linear_clf: the classification kernels run on the MI355X only; there is no CPU path (--num-gpus-per-machine 1)")


def _check_init(_A):
    if _A.weight_init in ("imagenet", "torchvision", "clip"):
        need = {"imagenet": "torchvision model-zoo downloads", "torchvision": "torchvision's classification training checkpoints",
                "clip": "the clip package"}[_A.weight_init]
        raise SystemExit(f"linear_clf: --weight-init {_A.weight_init} needs {need}, which is not supported here; use random or vlinfo")
    if _A.weight_init == "vlinfo" and not _A.checkpoint_path:
        raise SystemExit(f"linear_clf: --weight-init {_A.weight_init} needs --checkpoint-path")


def build_classifier(_A, _C, _DOWNC, num_classes):
    frozen, amp = _DOWNC.MODEL.VISUAL.FROZEN, _DOWNC.AMP
    if _A.weight_init == "vlinfo":
        ckpt = torch.load(_A.checkpoint_path, map_location="cpu", weights_only=False)
        model = ImageClassifier.from_pretraining(ckpt, _C.MODEL.VISUAL.NETWORK_NAME, num_classes, frozen, amp)
    else:
        model = ImageClassifier(_DOWNC.MODEL.VISUAL.NETWORK_NAME, num_classes, frozen, amp)
    if model.out_dim != _DOWNC.MODEL.VISUAL.FEATURE_SIZE:
        raise ValueError(f"MODEL.VISUAL.FEATURE_SIZE {_DOWNC.MODEL.VISUAL.FEATURE_SIZE} != the {model.visual_name} feature size {model.out_dim}")
    return model


def linear_clf_main(_A):
    _check_launch(_A)
    _check_init(_A)
    if not torch.cuda.is_available():
        raise SystemExit("linear_clf: no GPU visible; the classification kernels run on the MI355X only")
    device = torch.device("cuda", torch.cuda.current_device())
    _DOWNC = Config(_A.down_config, _A.down_config_override)
    common_setup(_DOWNC, _A, job_type="downstream")
    _C = Config(_A.config, _A.config_override)
    DATASET = DownstreamDatasetFactory.dataset_name(_DOWNC.DATA.ROOT)

    train_dataset = DownstreamDatasetFactory.from_config(_DOWNC, split="train")
    val_dataset = DownstreamDatasetFactory.from_config(_DOWNC, split="val")
    NUM_CLASSES = train_dataset.num_classes
    bs = _DOWNC.OPTIM.BATCH_SIZE
    train_dataloader = DataLoader(train_dataset, batch_size=bs, num_workers=_A.cpu_workers,
                                  sampler=DistributedSampler(train_dataset, num_replicas=1, rank=0, shuffle=True), drop_last=False,
                                  pin_memory=True, collate_fn=train_dataset.collate_fn)
    val_dataloader = DataLoader(val_dataset, batch_size=bs, num_workers=_A.cpu_workers,
                                sampler=DistributedSampler(val_dataset, num_replicas=1, rank=0, shuffle=False), drop_last=False,
                                pin_memory=True, collate_fn=val_dataset.collate_fn)

    model = build_classifier(_A, _C, _DOWNC, NUM_CLASSES).to(device)
    frozen = _DOWNC.MODEL.VISUAL.FROZEN
    if frozen:
        model.eval()
    top1 = TopkAccuracy(top_k=1)
    optimizer = OptimizerFactory.from_config(_DOWNC, model.named_parameters())
    scheduler = LRSchedulerFactory.from_config(_DOWNC, optimizer)

    start_iteration = 0
    if _A.resume_from is not None:
        start_iteration = max(0, CheckpointManager(model=model, optimizer=optimizer, scheduler=scheduler).load(_A.resume_from))
    if _A.serialization_dir:
        serialization_dir = _A.serialization_dir
    elif _A.checkpoint_path:
        serialization_dir = os.path.join(os.path.dirname(_A.checkpoint_path), DATASET)
    else:
        serialization_dir = _A.checkpoints_dir + _DOWNC.RUN_ID
    os.makedirs(serialization_dir, exist_ok=True)
    checkpoint_manager = CheckpointManager(serialization_dir, model=model, optimizer=optimizer, scheduler=scheduler)

    timer = Timer(start_from=start_iteration, total_iterations=_DOWNC.OPTIM.NUM_ITERATIONS)
    train_iter = cycle(train_dataloader, device, start_iteration)
    for iteration in range(start_iteration + 1, _DOWNC.OPTIM.NUM_ITERATIONS + 1):
        timer.tic()
        optimizer.zero_grad()
        batch = next(train_iter)
        logits = model(batch["image"])
        loss = cross_entropy(logits, batch["label"])
        loss.backward()
        optimizer.step()
        scheduler.step()
        timer.toc()
        if iteration % _A.log_every == 0:
            logger.info(f"{timer.stats} | Loss: {loss.item():.3f}")

        if iteration % _A.checkpoint_every == 0:
            torch.set_grad_enabled(False)
            model.eval()
            total_val_loss = torch.zeros((), device=device)
            n_val = 0
            for batch in val_dataloader:
                logits = model(batch["image"].to(device, non_blocking=True))
                labels = batch["label"].to(device, non_blocking=True)
                total_val_loss += cross_entropy(logits, labels)
                top1(logits, labels)
                n_val += 1
            total_val_loss = total_val_loss / max(n_val, 1)
            acc = top1.get_metric(reset=True)
            torch.set_grad_enabled(True)
            if not frozen:                     # back to train mode only when fine-tuning end to end (reference linear_clf.py:280-282)
                model.train()
            checkpoint_manager.step(iteration)
            logger.info(f"Iter: {iteration} | Val loss: {total_val_loss.item():.4f} | Top-1 accuracy: {acc}")
    return model


def linear_clf_cli(argv=None):
    _A = build_linear_clf_parser().parse_args(argv)
    return linear_clf_main(_A)


# ------------------------------------------------------------------------------------------------ zero-shot
def build_zero_shot_parser():
    parser = argparse.ArgumentParser(description="Zero-shot image classification with a pretrained model: class prompts through the text "
                                                 "encoder, each image assigned to the prompt of highest cosine (reference zero_shot.py).")
    parser.add_argument("--config", metavar="FILE", help="Path to the pretraining config file.")
    parser.add_argument("--config-override", nargs="*", default=[], help="A list of key-value pairs to modify pretraining config params.")
    parser.add_argument("--checkpoint-path", required=True, help="Pretraining checkpoint to evaluate.")
    parser.add_argument("--data-root", required=True, help="Image folder root/val/<class>/<image>, or 'random' for the synthetic source.")
    parser.add_argument("--prompt", default="a picture of a {}.", help="Prompt template; {} is replaced by the class name (reference "
                                                                      "zero_shot.py:74-85).")
    parser.add_argument("--max-length", type=int, default=30, help="Prompt token length (padded); at most 128 with the BERT tower, 32 with MPNet.")
    parser.add_argument("--batch-size", type=int, default=128)
    parser.add_argument("--cpu-workers", type=int, default=2)
    parser.add_argument("--num-gpus-per-machine", type=int, default=1, help="Only 1 is supported.")
    return parser


def tokenize_texts(texts, max_length, vocab="", text_model="bert-base-uncased"):
    """(input_ids, attention_mask) int64 [N][max_length] of every text, padded with the pad id of the text tower `text_model` names (0 for BERT,
    1 for MPNet: data.text_framing) (padding="max_length", truncation=True: reference zero_shot.py:104-110, retrieval.py:94-100). The project's
    WordPiece tokenizer when a vocabulary file is configured, else hash_tokenize."""
    from .data import WordPieceTokenizer, hash_tokenize, normalize_caption, text_framing
    framing = text_framing(text_model)
    tok = WordPieceTokenizer(vocab, framing) if vocab else None
    pad = tok.pad_token_id if tok is not None else (0 if framing == "bert" else 1)
    ids = torch.full((len(texts), max_length), pad, dtype=torch.long)
    mask = torch.zeros(len(texts), max_length, dtype=torch.long)
    for i, text in enumerate(texts):
        t = tok(normalize_caption(text, max_length), max_length) if tok is not None else hash_tokenize(text, max_length, framing=framing)
        t = list(t)[:max_length]
        ids[i, :len(t)] = torch.tensor(t, dtype=torch.long)
        mask[i, :len(t)] = 1
    return ids, mask


def tokenize_prompts(names, template, max_length, vocab="", text_model="bert-base-uncased"):
    """(input_ids, attention_mask) int64 [C][max_length] of template.format(name) for every class (tokenize_texts)."""
    return tokenize_texts([template.format(name.replace("_", " ")) for name in names], max_length, vocab, text_model)


def zero_shot_main(_A):
    if _A.num_gpus_per_machine != 1:
        raise SystemExit("zero_shot: runs on one GPU (--num-gpus-per-machine 1)")
    if not torch.cuda.is_available():
        raise SystemExit("zero_shot: no GPU visible; the kernels run on the MI355X only")
    from . import retrieval
    from .data import ImageFolderDataset, RandomLabelledDataset
    device = torch.device("cuda", torch.cuda.current_device())
    _C = Config(_A.config, _A.config_override)
    model = PretrainingModelFactory.from_config(_C)
    CheckpointManager(model=model).load(_A.checkpoint_path)
    model = model.to(device).eval()
    size = _C.DATA.IMAGE_CROP_SIZE
    if _A.data_root == "random":
        ds = RandomLabelledDataset(image_size=size, length=500, split="val", seed=_C.RANDOM_SEED)
    else:
        ds = ImageFolderDataset(_A.data_root, "val", tuple(_C.DATA.IMAGE_TRANSFORM_VAL), size)
    ids, mask = tokenize_prompts(ds.classes, _A.prompt, _A.max_length, _C.DATA.TOKENIZER_VOCAB, _C.MODEL.TEXTUAL.NETWORK_NAME)
    text = retrieval.embed_texts(model, ids.to(device), mask.to(device), _A.batch_size)
    acc = torch.zeros(4, device=device)
    loader = DataLoader(ds, batch_size=_A.batch_size, shuffle=False, num_workers=_A.cpu_workers, collate_fn=ds.collate_fn)
    for batch in loader:
        zero_shot_counts(model, text, batch["image"], batch["label"], acc, 5, _A.batch_size)
    a = acc.tolist()
    n = max(a[3], 1e-12)
    res = {"top1": 100.0 * a[1] / n, "top5": 100.0 * a[2] / n}
    print(f"zero-shot top-1: {res['top1']:.2f} | top-5: {res['top5']:.2f} ({int(a[3])} images, {len(ds.classes)} classes)")
    return res


def zero_shot_cli(argv=None):
    return zero_shot_main(build_zero_shot_parser().parse_args(argv))


# ------------------------------------------------------------------------------------------------ VOC07 SVMs
def build_voc_clf_parser():
    parser = common_parser(description="Train SVMs for VOC2007 classification on a pretrained model.")
    parser.set_defaults(num_gpus_per_machine=1)
    group = parser.add_argument_group("Downstream config arguments.")
    group.add_argument("--down-config", metavar="FILE", help="Path to a downstream config file.")
    group.add_argument("--down-config-override", nargs="*", default=[], help="A list of key-value pairs to modify downstream config params.")
    group = parser.add_argument_group("Checkpointing")
    group.add_argument("--weight-init", choices=["random", "imagenet", "torchvision", "vlinfo"], default="vlinfo",
                       help="'random': random weights for the first evaluation; 'vlinfo': checkpoint_<start-iter>.pth of --checkpoint-dir. "
                            "'imagenet' and 'torchvision' (model-zoo downloads) are not supported.")
    group.add_argument("--loss-type", choices=["dot", "concat"], default="dot", help="Which MI estimation approach has been used?")
    group.add_argument("--checkpoint-dir", required=True, help="Path to load checkpoints from and write voc07_mAP.txt to.")
    group.add_argument("--freq", type=int, default=46200, help="Evaluate every these many iterations.")
    group.add_argument("--start-iter", type=int, default=46200, help="First iteration to evaluate.")
    return parser


def _check_voc_launch(_A):
    if _A.num_gpus_per_machine == 0:
        raise SystemExit("voc_clf: feature extraction and the SVM solver run on the MI355X only; there is no CPU path (--num-gpus-per-machine 1)")
    if _A.num_gpus_per_machine > 1 or _A.num_machines > 1:
        raise SystemExit("voc_clf: runs on one GPU (--num-gpus-per-machine 1)")
    if _A.weight_init in ("imagenet", "torchvision"):
        raise SystemExit(f"voc_clf: --weight-init {_A.weight_init} needs torchvision model-zoo downloads, which are not supported here; use random "
                         "or vlinfo")


def checkpoint_path(checkpoint_dir: str, iteration: int) -> str:
    return os.path.join(checkpoint_dir, f"checkpoint_{iteration}.pth")


def _report_map(test_map):
    """voc_clf.py's line and file entry for one evaluation: the mAP, a fraction, as a percentage."""
    print("Test mAP: " + str(test_map * 100))
    return test_map * 100


def run_checkpoint_loop(checkpoint_dir, start_iter, freq, evaluate, load, filename="voc07_mAP.txt", report=_report_map):
    """Reference voc_clf.py:218-237: evaluate (-> mAP as a fraction), print it, merge {iteration: mAP x 100} into <checkpoint_dir>/voc07_mAP.txt
    (JSON), then load checkpoint_<iteration + freq>.pth and go on until that load fails ("Completed!"). Returns the merged results. Another
    evaluation (knn_clf.py) names its own file and its own `report`, which prints evaluate()'s result and returns the JSON entry of the iteration."""
    import json
    out = os.path.join(checkpoint_dir, filename)
    results = {}
    if os.path.exists(out):
        with open(out) as f:
            results = json.load(f)
    it = int(start_iter)
    while True:
        results[str(it)] = report(evaluate())
        with open(out, "w") as f:
            json.dump(results, f)
        it += int(freq)
        try:
            load(checkpoint_path(checkpoint_dir, it))
        except Exception:
            print("Completed!")
            return results


@torch.no_grad()
def extract_features(model, loader, device):
    """(features f32 [N][F], targets int [N][K]) in dataset order: the pretraining model's image encoder in eval mode, then clite_l2_normalize
    (reference voc_clf.py:171-200: pooled features / their L2 norm). The encoder's compute dtype is the model's (AMP: bf16, else exact f32)."""
    from . import hip
    enc = model.image_encoder
    was = enc.training
    enc.eval()
    feats, tgts = [], []
    for batch in loader:
        f = enc(batch["image"].to(device)).contiguous()
        o = torch.empty_like(f)
        hip.l2_normalize(model.runtime.dt, f, o, f.shape[0], f.shape[1])
        feats.append(o.float())
        tgts.append(batch["label"])
    enc.train(was)
    return torch.cat(feats, 0), torch.cat(tgts, 0)


def voc_clf_main(_A):
    """Reference voc_clf.py main(): features of VOC07 trainval / test from every checkpoint in turn, the batched SVM evaluation
    (svm.voc07_svm_eval), Test mAP printed and merged into <checkpoint-dir>/voc07_mAP.txt."""
    _check_voc_launch(_A)
    if not torch.cuda.is_available():
        raise SystemExit("voc_clf: no GPU visible; the kernels run on the MI355X only")
    from .svm import voc07_svm_eval
    device = torch.device("cuda", torch.cuda.current_device())
    _DOWNC = Config(_A.down_config, _A.down_config_override)
    common_setup(_DOWNC, _A, job_type="downstream")
    _C = Config(_A.config, list(_A.config_override) + ["AMP", _DOWNC.AMP])       # the encoder's compute dtype follows the downstream config
    train_dataset = DownstreamDatasetFactory.from_config(_DOWNC, split="trainval")
    test_dataset = DownstreamDatasetFactory.from_config(_DOWNC, split="test")
    bs = _DOWNC.OPTIM.BATCH_SIZE
    loaders = [DataLoader(ds, batch_size=bs, shuffle=False, num_workers=_A.cpu_workers, pin_memory=True, collate_fn=ds.collate_fn)
               for ds in (train_dataset, test_dataset)]
    arch = PretrainingModelFactory.from_config(_C).to(device)

    def load(path):
        CheckpointManager(model=arch).load(path)

    if _A.weight_init == "vlinfo":
        load(checkpoint_path(_A.checkpoint_dir, _A.start_iter))

    def evaluate():
        ftr, ttr = extract_features(arch, loaders[0], device)
        fte, tte = extract_features(arch, loaders[1], device)
        res = voc07_svm_eval(ftr, ttr.numpy(), fte, tte.numpy())
        for name, cost, ap in zip(train_dataset.class_names, res["cost"], res["test_ap"]):
            logger.info(f"SVM {name}: cost {cost}, test AP {ap * 100:.2f}")
        return res["map"]

    return run_checkpoint_loop(_A.checkpoint_dir, _A.start_iter, _A.freq, evaluate, load)


def voc_clf_cli(argv=None):
    return voc_clf_main(build_voc_clf_parser().parse_args(argv))


# ------------------------------------------------------------------------------------------------ weighted k-NN
def build_knn_parser():
    parser = common_parser(description="Weighted k-nearest-neighbour classification on the frozen features of a pretrained model.")
    parser.set_defaults(num_gpus_per_machine=1)
    group = parser.add_argument_group("Downstream config arguments.")
    group.add_argument("--down-config", metavar="FILE", help="Path to a downstream config file.")
    group.add_argument("--down-config-override", nargs="*", default=[], help="A list of key-value pairs to modify downstream config params.")
    group = parser.add_argument_group("k-NN")
    group.add_argument("--k", type=int, nargs="+", default=[10, 20, 100, 200], help="Neighbour counts to evaluate (each at most 256; one larger "
                                                                                    "than the bank is dropped).")
    group.add_argument("--temperature", type=float, default=0.07, help="Temperature of the vote's weights exp(similarity / T).")
    group = parser.add_argument_group("Checkpointing")
    group.add_argument("--weight-init", choices=["random", "imagenet", "torchvision", "vlinfo"], default="vlinfo",
                       help="'random': random weights for the first evaluation; 'vlinfo': checkpoint_<start-iter>.pth of --checkpoint-dir. "
                            "'imagenet' and 'torchvision' (model-zoo downloads) are not supported.")
    group.add_argument("--checkpoint-dir", required=True, help="Path to load checkpoints from and write knn_acc.txt to.")
    group.add_argument("--freq", type=int, default=46200, help="Evaluate every these many iterations.")
    group.add_argument("--start-iter", type=int, default=46200, help="First iteration to evaluate.")
    return parser


def _check_knn_launch(_A):
    from . import hip
    if _A.num_gpus_per_machine == 0:
        raise SystemExit("knn_clf: feature extraction and the k-NN kernels run on the MI355X only; there is no CPU path (--num-gpus-per-machine 1)")
    if _A.num_gpus_per_machine > 1 or _A.num_machines > 1:
        raise SystemExit("knn_clf: runs on one GPU (--num-gpus-per-machine 1)")
    if _A.weight_init in ("imagenet", "torchvision"):
        raise SystemExit(f"knn_clf: --weight-init {_A.weight_init} needs torchvision model-zoo downloads, which are not supported here; use random "
                         "or vlinfo")
    if not _A.k or min(_A.k) < 1 or max(_A.k) > hip.KNN_MAX_K:
        raise SystemExit(f"knn_clf: every --k must be in [1, {hip.KNN_MAX_K}]")
    if len(set(_A.k)) > hip.KNN_MAX_KS:
        raise SystemExit(f"knn_clf: at most {hip.KNN_MAX_KS} different --k")
    if not _A.temperature > 0:
        raise SystemExit("knn_clf: --temperature must be positive")


def _report_knn(res):
    """One line per k, and the JSON entry {k: {"top1", "top5"}} of the iteration."""
    for k, acc in res.items():
        line = f"k-NN top-1 (k = {k}): {acc['top1']:.2f}"
        if "top5" in acc:
            line += f" | top-5: {acc['top5']:.2f}"
        print(line)
    return {str(k): acc for k, acc in res.items()}


def knn_clf_main(_A):
    """Weighted k-NN accuracy (knn.knn_eval) of every checkpoint in turn, as voc_clf.py walks them: features of the `train` split as the bank and of
    the `val` split as the queries (image folder or the synthetic source), printed per k and merged into <checkpoint-dir>/knn_acc.txt."""
    _check_knn_launch(_A)
    if not torch.cuda.is_available():
        raise SystemExit("knn_clf: no GPU visible; the kernels run on the MI355X only")
    from .knn import knn_eval
    device = torch.device("cuda", torch.cuda.current_device())
    _DOWNC = Config(_A.down_config, _A.down_config_override)
    common_setup(_DOWNC, _A, job_type="downstream")
    _C = Config(_A.config, list(_A.config_override) + ["AMP", _DOWNC.AMP])       # the encoder's compute dtype follows the downstream config
    train_dataset = DownstreamDatasetFactory.from_config(_DOWNC, split="train")
    val_dataset = DownstreamDatasetFactory.from_config(_DOWNC, split="val")
    num_classes = train_dataset.num_classes
    bs = _DOWNC.OPTIM.BATCH_SIZE
    loaders = [DataLoader(ds, batch_size=bs, shuffle=False, num_workers=_A.cpu_workers, pin_memory=True, collate_fn=ds.collate_fn)
               for ds in (train_dataset, val_dataset)]
    arch = PretrainingModelFactory.from_config(_C).to(device)

    def load(path):
        CheckpointManager(model=arch).load(path)

    if _A.weight_init == "vlinfo":
        load(checkpoint_path(_A.checkpoint_dir, _A.start_iter))

    def evaluate():
        ftr, ytr = extract_features(arch, loaders[0], device)
        fte, yte = extract_features(arch, loaders[1], device)
        return knn_eval(ftr, ytr.reshape(-1), fte, yte.reshape(-1), num_classes, _A.k, _A.temperature)

    return run_checkpoint_loop(_A.checkpoint_dir, _A.start_iter, _A.freq, evaluate, load, filename="knn_acc.txt", report=_report_knn)


def knn_clf_cli(argv=None):
    return knn_clf_main(build_knn_parser().parse_args(argv))


# ------------------------------------------------------------------------------------------------ logistic-regression probe
def build_logreg_parser():
    parser = common_parser(description="Logistic-regression probe (multinomial, fitted to convergence, cost chosen on a hold-out part of the "
                                       "train split) on the frozen features of a pretrained model.")
    parser.set_defaults(num_gpus_per_machine=1)
    group = parser.add_argument_group("Downstream config arguments.")
    group.add_argument("--down-config", metavar="FILE", help="Path to a downstream config file.")
    group.add_argument("--down-config-override", nargs="*", default=[], help="A list of key-value pairs to modify downstream config params.")
    group = parser.add_argument_group("Logistic regression")
    group.add_argument("--cost", type=float, nargs="+", default=[1.0, 10.0, 100.0, 1000.0],
                       help="Costs C of f(W) = 1/2 |W|^2 + C sum_i loss_i to choose from (the features are L2-normalised, so useful costs are large).")
    group.add_argument("--holdout", type=float, default=0.1, help="Fraction of every class's train rows (its last ones) held out to choose the cost.")
    group.add_argument("--tol", type=float, default=1e-5, help="Stop at |grad f(W)| <= tol |grad f(0)|.")
    group = parser.add_argument_group("Checkpointing")
    group.add_argument("--weight-init", choices=["random", "imagenet", "torchvision", "vlinfo"], default="vlinfo",
                       help="'random': random weights for the first evaluation; 'vlinfo': checkpoint_<start-iter>.pth of --checkpoint-dir. "
                            "'imagenet' and 'torchvision' (model-zoo downloads) are not supported.")
    group.add_argument("--checkpoint-dir", required=True, help="Path to load checkpoints from and write logreg_acc.txt to.")
    group.add_argument("--freq", type=int, default=46200, help="Evaluate every these many iterations.")
    group.add_argument("--start-iter", type=int, default=46200, help="First iteration to evaluate.")
    return parser


def _check_logreg_launch(_A):
    import math
    if _A.num_gpus_per_machine == 0:
        raise SystemExit("logreg_clf: feature extraction and the solver's kernels run on the MI355X only; there is no CPU path "
                         "(--num-gpus-per-machine 1)")
    if _A.num_gpus_per_machine > 1 or _A.num_machines > 1:
        raise SystemExit("logreg_clf: runs on one GPU (--num-gpus-per-machine 1)")
    if _A.weight_init in ("imagenet", "torchvision"):
        raise SystemExit(f"logreg_clf: --weight-init {_A.weight_init} needs torchvision model-zoo downloads, which are not supported here; use "
                         "random or vlinfo")
    if not _A.cost or any(not (c > 0 and math.isfinite(c)) for c in _A.cost):
        raise SystemExit("logreg_clf: every --cost must be positive and finite")
    if len(set(_A.cost)) != len(_A.cost):
        raise SystemExit("logreg_clf: --cost holds a value twice")
    if not 0 < _A.holdout < 1:
        raise SystemExit("logreg_clf: --holdout must be in (0, 1)")
    if not (_A.tol > 0 and math.isfinite(_A.tol)):
        raise SystemExit("logreg_clf: --tol must be positive")


def _report_logreg(res):
    """The probe's line, and the JSON entry {"cost", "top1", "top5", "holdout_top1": {cost: top-1}} of the iteration."""
    line = f"Logistic-regression probe top-1: {res['top1']:.2f}"
    if "top5" in res:
        line += f" | top-5: {res['top5']:.2f}"
    print(line + f" (cost {res['cost']:g})")
    return {"cost": res["cost"], "top1": res["top1"], "top5": res.get("top5"), "holdout_top1": {f"{c:g}": a for c, a in res["holdout_top1"].items()}}


def logreg_clf_main(_A):
    """The logistic-regression probe (logreg.logreg_eval) of every checkpoint in turn, as knn_clf.py walks them: features of the `train` split to
    fit on and of the `val` split to report on (image folder or the synthetic source), printed and merged into <checkpoint-dir>/logreg_acc.txt."""
    _check_logreg_launch(_A)
    _DOWNC = Config(_A.down_config, _A.down_config_override)
    if "voc" in DownstreamDatasetFactory.dataset_name(_DOWNC.DATA.ROOT).lower():
        raise SystemExit("logreg_clf: a VOC2007 root is multi-label, which a multinomial probe does not fit; evaluate it with voc_clf.py")
    if not torch.cuda.is_available():
        raise SystemExit("logreg_clf: no GPU visible; the kernels run on the MI355X only")
    from .logreg import logreg_eval
    device = torch.device("cuda", torch.cuda.current_device())
    common_setup(_DOWNC, _A, job_type="downstream")
    _C = Config(_A.config, list(_A.config_override) + ["AMP", _DOWNC.AMP])       # the encoder's compute dtype follows the downstream config
    train_dataset = DownstreamDatasetFactory.from_config(_DOWNC, split="train")
    val_dataset = DownstreamDatasetFactory.from_config(_DOWNC, split="val")
    num_classes = train_dataset.num_classes
    bs = _DOWNC.OPTIM.BATCH_SIZE
    loaders = [DataLoader(ds, batch_size=bs, shuffle=False, num_workers=_A.cpu_workers, pin_memory=True, collate_fn=ds.collate_fn)
               for ds in (train_dataset, val_dataset)]
    arch = PretrainingModelFactory.from_config(_C).to(device)

    def load(path):
        CheckpointManager(model=arch).load(path)

    if _A.weight_init == "vlinfo":
        load(checkpoint_path(_A.checkpoint_dir, _A.start_iter))

    def evaluate():
        ftr, ytr = extract_features(arch, loaders[0], device)
        fte, yte = extract_features(arch, loaders[1], device)
        return logreg_eval(ftr, ytr.reshape(-1), fte, yte.reshape(-1), num_classes, _A.cost, _A.holdout, tol=_A.tol)

    return run_checkpoint_loop(_A.checkpoint_dir, _A.start_iter, _A.freq, evaluate, load, filename="logreg_acc.txt", report=_report_logreg)


def logreg_clf_cli(argv=None):
    return logreg_clf_main(build_logreg_parser().parse_args(argv))


# ------------------------------------------------------------------------------------------------ image-text retrieval
def build_retrieval_parser():
    parser = common_parser(description="Image-text retrieval (recall@1/5/10 in both directions) of a pretrained model.")
    parser.set_defaults(num_gpus_per_machine=1)
    group = parser.add_argument_group("Downstream config arguments.")
    group.add_argument("--down-config", metavar="FILE", help="Path to a downstream config file.")
    group.add_argument("--down-config-override", nargs="*", default=[], help="A list of key-value pairs to modify downstream config params.")
    group = parser.add_argument_group("Checkpointing")
    group.add_argument("--weight-init", choices=["random", "imagenet", "torchvision", "vlinfo", "clip"], default="vlinfo",
                       help="'vlinfo': the pretraining checkpoint --checkpoint-path; 'random': the randomly initialised model (the checkpoint is "
                            "not read). 'imagenet', 'torchvision' (downloads) and 'clip' (the clip package) are not supported.")
    group.add_argument("--checkpoint-path", required=True, help="Path to load checkpoint and run downstream task evaluation.")
    group.add_argument("--ann-file", default=None, help="JSON list of {'image', 'caption': [...]} with image paths relative to DATA.ROOT "
                                                        "(default: by DATA.ROOT, see RetrievalDatasetFactory).")
    return parser


def _check_retrieval_launch(_A):
    if _A.weight_init == "clip":
        raise SystemExit("retrieval: --weight-init clip needs the clip package, which is not part of the reference; use vlinfo or random")
    if _A.weight_init in ("imagenet", "torchvision"):
        raise SystemExit(f"retrieval: --weight-init {_A.weight_init} needs torchvision model-zoo downloads, which are not supported here; use "
                         "vlinfo or random")
    if _A.num_gpus_per_machine > 1 or _A.num_machines > 1:
        raise SystemExit("retrieval: runs on one GPU (--num-gpus-per-machine 1)")
    if _A.num_gpus_per_machine == 0:
        raise SystemExit("retrieval: the encoders and the ranking kernels run on the MI355X only; there is no CPU path (--num-gpus-per-machine 1)")


def retrieval_main(_A):
    """Reference retrieval.py main(): image and text embeddings of the pretraining model in eval mode, the similarity matrix, ranks on the
    GPU and recall@1/5/10 (retrieval.evaluate). Prints the result dict, then its val_-prefixed form, and returns the dict."""
    _check_retrieval_launch(_A)
    if not torch.cuda.is_available():
        raise SystemExit("retrieval: no GPU visible; the encoders and the ranking kernels run on the MI355X only")
    from . import retrieval
    from .factories import RetrievalDatasetFactory
    device = torch.device("cuda", torch.cuda.current_device())
    _DOWNC = Config(_A.down_config, _A.down_config_override)
    common_setup(_DOWNC, _A, job_type="downstream")
    _C = Config(_A.config, list(_A.config_override) + ["AMP", _DOWNC.AMP])       # the compute dtype follows the downstream config
    dataset = RetrievalDatasetFactory.from_config(_DOWNC, split="val", ann_file=_A.ann_file)
    loader = DataLoader(dataset, batch_size=_DOWNC.OPTIM.BATCH_SIZE, shuffle=False, num_workers=_A.cpu_workers, pin_memory=True,
                        collate_fn=dataset.collate_fn)
    arch = PretrainingModelFactory.from_config(_C)
    if _A.weight_init == "vlinfo":
        CheckpointManager(model=arch).load(_A.checkpoint_path)
    arch = arch.to(device)
    ids, mask = tokenize_texts(dataset.text, 30, _C.DATA.TOKENIZER_VOCAB, _C.MODEL.TEXTUAL.NETWORK_NAME)
    val_result = retrieval.evaluate(arch, loader, ids, mask)
    print(val_result)
    log_stats = {**{f"val_{k}": v for k, v in val_result.items()}}
    print(log_stats)
    return val_result


def retrieval_cli(argv=None):
    return retrieval_main(build_retrieval_parser().parse_args(argv))


def build_cluster_parser():
    parser = common_parser(description="Cluster the captions of the pretraining dataset (k-means on the GPU) for clustered negative sampling.")
    parser.set_defaults(num_gpus_per_machine=1)
    group = parser.add_argument_group("Clustering (reference scripts/cluster.py:155-176)")
    group.add_argument("--cluster-root", required=True, help="Directory under which clusters_<max-clusters>/ is written.")
    group.add_argument("--coco-root", default="", help="Accepted for the reference's command line; image paths come from the dataset records.")
    group.add_argument("--min-clusters", type=int, default=2)
    group.add_argument("--max-clusters", type=int, default=10)
    group.add_argument("--split", type=str, default="train")
    group.add_argument("--seed", type=int, default=1234, help="Seed of the initial centroids (kmeans.init_rows).")
    group.add_argument("--encodings", metavar="FILE", default=None, help="A reference-format img_id_encoding_map_<split>.pkl ({id: float vector}): "
                       "cluster these vectors as they are instead of embedding the captions.")
    group.add_argument("--batch-size", type=int, default=256, help="Captions per text-encoder batch.")
    group = parser.add_argument_group("Checkpointing")
    group.add_argument("--weight-init", choices=["vlinfo", "random"], default="vlinfo",
                       help="'vlinfo': the text encoder of the pretraining checkpoint --checkpoint-path; 'random': the randomly initialised model.")
    group.add_argument("--checkpoint-path", default=None, help="Pretraining checkpoint whose text encoder embeds the captions.")
    return parser


@torch.no_grad()
def embed_captions(model, captions, max_length, vocab="", batch_size=256, text_model="bert-base-uncased"):
    """f32 [N][768] on the model's device: the text encoder's features (eval mode, no projection head) of every caption through
    clite_l2_normalize. Stands in for the reference's paraphrase-mpnet-base-v2 sentence encoder (scripts/cluster.py:115-124), which does not
    exist offline. max_length (DATA.MAX_CAPTION_LENGTH): up to 128 tokens with the BERT tower, 32 with MPNet (bert.bert_forward)."""
    from . import hip
    rt, enc = model.runtime, model.text_encoder
    device = next(model.parameters()).device
    was = enc.training
    enc.eval()
    outs = []
    for i in range(0, len(captions), batch_size):
        ids, mask = tokenize_texts(captions[i:i + batch_size], max_length, vocab, text_model)
        f = enc({"input_ids": ids.to(device), "attention_mask": mask.to(device)}).contiguous()
        o = torch.empty_like(f)
        hip.l2_normalize(rt.dt, f, o, f.shape[0], f.shape[1])
        outs.append(o.float())
    enc.train(was)
    return torch.cat(outs, 0)


def _save_pickle(obj, path):
    import pickle
    with open(path, "wb") as fh:
        pickle.dump(obj, fh, protocol=pickle.HIGHEST_PROTOCOL)


def cluster_main(_A):
    """Reference scripts/cluster.py: the first caption of every record of the split embedded once, k-means (kmeans.fit) for every K in
    [--min-clusters, --max-clusters], and the maps written into <cluster-root>/clusters_<max>/ in the reference's layouts, so that the
    directory is a valid DATA.CLUSTER_PATH here and for the reference. Returns {K: fit result}."""
    import pickle
    import numpy as np
    from . import kmeans
    from .factories import PretrainingDatasetFactory
    from .utils.common import logger
    if _A.num_gpus_per_machine > 1 or _A.num_machines > 1:
        raise SystemExit("cluster: runs on one GPU (--num-gpus-per-machine 1)")
    if _A.num_gpus_per_machine == 0 or not torch.cuda.is_available():
        raise SystemExit("cluster: the text encoder and the k-means kernels run on the MI355X only; there is no CPU path (--num-gpus-per-machine 1)")
    if not 2 <= _A.min_clusters <= _A.max_clusters:
        raise SystemExit("cluster: need 2 <= --min-clusters <= --max-clusters")
    if _A.encodings is None and _A.weight_init == "vlinfo" and not _A.checkpoint_path:
        raise SystemExit("cluster: --weight-init vlinfo needs --checkpoint-path (or pass --weight-init random, or --encodings FILE)")
    device = torch.device("cuda", torch.cuda.current_device())
    _C = Config(_A.config, _A.config_override)
    split = str(_A.split)
    out_dir = os.path.join(_A.cluster_root, f"clusters_{_A.max_clusters}")
    os.makedirs(out_dir, exist_ok=True)
    dataset = PretrainingDatasetFactory.from_config(_C, split=split)
    if dataset.mode == "sbert":
        raise SystemExit("cluster: needs captions (MODEL.TEXTUAL.NAME train_sbert), not frozen caption encodings")
    n = len(dataset)
    captions = [dataset.caption(i) for i in range(n)]
    if _A.encodings is not None:
        with open(_A.encodings, "rb") as fh:
            enc_map = pickle.load(fh)
        if sorted(int(k) for k in enc_map) != list(range(n)):
            raise SystemExit(f"cluster: {_A.encodings} must hold one vector for every dataset index 0 .. {n - 1}")
        X = torch.from_numpy(np.stack([np.asarray(enc_map[i], np.float32) for i in range(n)])).to(device)
    else:
        arch = PretrainingModelFactory.from_config(_C)
        if _A.weight_init == "vlinfo":
            CheckpointManager(model=arch).load(_A.checkpoint_path)
        arch = arch.to(device)
        X = embed_captions(arch, captions, int(_C.DATA.MAX_CAPTION_LENGTH), _C.DATA.TOKENIZER_VOCAB, _A.batch_size, _C.MODEL.TEXTUAL.NETWORK_NAME)
    X_host = X.cpu().numpy()
    _save_pickle({i: [captions[i]] for i in range(n)}, os.path.join(out_dir, f"img_id_caption_map_{split}.pkl"))
    _save_pickle({i: (dataset.image_path(i) or "") for i in range(n)}, os.path.join(out_dir, f"img_id_filename_map_{split}.pkl"))
    _save_pickle({i: X_host[i] for i in range(n)}, os.path.join(out_dir, f"img_id_encoding_map_{split}.pkl"))
    results = {}
    for K in range(_A.min_clusters, _A.max_clusters + 1):
        out = kmeans.fit(X, K, niter=200, seed=_A.seed)
        assign = out["assign"].cpu().tolist()
        _save_pickle({i: int(assign[i]) for i in range(n)}, os.path.join(out_dir, f"img_id_cluster_map_{split}_{K}.pkl"))
        counts = out["counts"].cpu()
        msg = (f"k-means K = {K}: {out['iterations']} iterations, inertia {out['inertia']:.6f}, smallest cluster {int(counts.min())}, "
               f"largest {int(counts.max())}")
        logger.info(msg)
        print(msg)
        results[K] = out
    return results


def cluster_cli(argv=None):
    return cluster_main(build_cluster_parser().parse_args(argv))


# ------------------------------------------------------------------------------------------------ bias evaluation
# Bolukbasi et al. 2016, "Man is to computer programmer as woman is to homemaker?": the ten definitional pairs (the reference's
# definitional_pairs.json)
DEFINITIONAL_PAIRS = (("woman", "man"), ("girl", "boy"), ("she", "he"), ("mother", "father"), ("daughter", "son"), ("gal", "guy"),
                      ("female", "male"), ("her", "his"), ("herself", "himself"), ("mary", "john"))


def build_bias_eval_parser():
    parser = common_parser(description="Bias evaluation of a pretrained model: a direction found in the text embeddings of definitional word "
                                       "pairs is removed from the image features; what a prompt retrieves from every group of images is "
                                       "compared before and after (reference bias_eda.py, without its prompt loop).")
    parser.set_defaults(num_gpus_per_machine=1)
    group = parser.add_argument_group("Downstream config arguments.")
    group.add_argument("--down-config", metavar="FILE", help="Path to a downstream config file.")
    group.add_argument("--down-config-override", nargs="*", default=[], help="A list of key-value pairs to modify downstream config params.")
    group = parser.add_argument_group("Checkpointing")
    group.add_argument("--weight-init", choices=["random", "imagenet", "torchvision", "vlinfo", "clip"], default="vlinfo",
                       help="'vlinfo': the pretraining checkpoint --checkpoint-path; 'random': the randomly initialised model. 'imagenet', "
                            "'torchvision' (downloads) and 'clip' (the clip package) are not supported.")
    group.add_argument("--checkpoint-path", default=None, help="Pretraining checkpoint to evaluate.")
    group = parser.add_argument_group("Evaluation")
    group.add_argument("--split", default="train", help="Which data split to use (reference: train, val or test).")
    group.add_argument("--gender-data-path", metavar="DIR", default=None, help="The reference's COCO gender annotation: DIR/<split>.data, a "
                       "pickled list of {image_id, file_name, gender}; images under <DATA.ROOT>/<split>2017/. Without it DATA.ROOT is an "
                       "image folder root/<split>/<group>/<image>, or 'random'.")
    group.add_argument("--pairs", metavar="FILE", default=None, help="JSON list of two-string lists (the reference's definitional_pairs.json); "
                                                                     "default: Bolukbasi's ten gender pairs.")
    group.add_argument("--query", nargs="+", default=[], metavar="TEXT", help="Prompt(s) to retrieve with.")
    group.add_argument("--queries", metavar="FILE", default=None, help="File with one prompt per line.")
    group.add_argument("--num-results", type=int, default=10, help="Images retrieved per prompt and group.")
    group.add_argument("--components", type=int, default=1, help="Principal directions to remove.")
    group.add_argument("--max-length", type=int, default=30, help="Token length of pair words and prompts (padded); at most 128 with the BERT "
                                                                  "tower, 32 with MPNet.")
    group.add_argument("--output", metavar="FILE", default=None, help="Write the result dict as JSON.")
    return parser


def read_pairs(path):
    """[(a, b)] from a JSON list of two-string lists (the reference's definitional_pairs.json)."""
    import json
    with open(path) as fh:
        pairs = json.load(fh)
    if not isinstance(pairs, list) or not pairs or any(not isinstance(p, (list, tuple)) or len(p) != 2 or not all(isinstance(w, str) and w.strip() for w in p)
                                                       for p in pairs):
        raise SystemExit(f"bias_eval: {path} must hold a non-empty JSON list of two-string lists, e.g. [[\"woman\", \"man\"], ...]")
    return [(p[0], p[1]) for p in pairs]


def read_queries(path):
    """The non-empty lines of a prompt file."""
    with open(path) as fh:
        return [line.strip() for line in fh if line.strip()]


def _check_bias_eval_launch(_A):
    """(pairs, prompts) after every refusal that needs no config."""
    if _A.weight_init == "clip":
        raise SystemExit("bias_eval: --weight-init clip needs the clip package, which is not part of the reference; use vlinfo or random")
    if _A.weight_init in ("imagenet", "torchvision"):
        raise SystemExit(f"bias_eval: --weight-init {_A.weight_init} needs torchvision model-zoo downloads, which are not supported here; use "
                         "vlinfo or random")
    if _A.weight_init == "vlinfo" and not _A.checkpoint_path:
        raise SystemExit("bias_eval: --weight-init vlinfo needs --checkpoint-path (or pass --weight-init random)")
    if _A.num_gpus_per_machine > 1 or _A.num_machines > 1:
        raise SystemExit("bias_eval: runs on one GPU (--num-gpus-per-machine 1)")
    if _A.num_gpus_per_machine == 0:
        raise SystemExit("bias_eval: the encoders and the debias kernels run on the MI355X only; there is no CPU path (--num-gpus-per-machine 1)")
    from . import hip
    pairs = read_pairs(_A.pairs) if _A.pairs else list(DEFINITIONAL_PAIRS)
    prompts = list(_A.query) + (read_queries(_A.queries) if _A.queries else [])
    if not prompts:
        raise SystemExit("bias_eval: at least one prompt is required (--query TEXT ... or --queries FILE)")
    if len(pairs) > hip.DEBIAS_MAX_PAIRS:
        raise SystemExit(f"bias_eval: at most {hip.DEBIAS_MAX_PAIRS} pairs, got {len(pairs)}")
    if not 1 <= _A.components <= min(len(pairs), hip.DEBIAS_MAX_COMPONENTS):
        raise SystemExit(f"bias_eval: --components must be in [1, {min(len(pairs), hip.DEBIAS_MAX_COMPONENTS)}] for {len(pairs)} pairs, got "
                         f"{_A.components}")
    if not 1 <= _A.num_results <= hip.KNN_MAX_K:
        raise SystemExit(f"bias_eval: --num-results must be in [1, {hip.KNN_MAX_K}], got {_A.num_results}")
    return pairs, prompts


def _check_bias_eval_model(_A, _C):
    from .data import text_framing
    if _C.MODEL.LOSS.TYPE not in ("dot", "dotcon"):
        raise SystemExit(f"bias_eval: MODEL.LOSS.TYPE {_C.MODEL.LOSS.TYPE} has no projection heads (loss.global_d.img_block / text_block), which "
                         "carry both towers into the space the direction lives in; the reference's --loss-type concat path never worked either")
    limit = 128 if text_framing(_C.MODEL.TEXTUAL.NETWORK_NAME) == "bert" else 32
    if _C.MODEL.TEXTUAL.NETWORK_NAME.startswith("clip_text"):          # the CLIP text tower takes what its positional embedding covers
        limit = int(_C.MODEL.TEXTUAL.CONTEXT_LENGTH)
    if not 1 <= _A.max_length <= limit:
        raise SystemExit(f"bias_eval: --max-length {_A.max_length} exceeds the {limit} tokens of the text tower {_C.MODEL.TEXTUAL.NETWORK_NAME}")


def report_bias(res, prompts, group_names):
    """The per-prompt lines bias_eval prints: mean alignment and share of every group, before and after."""
    lines = []
    for q, text in enumerate(prompts):
        lines.append(f"prompt {text!r}")
        for g, name in enumerate(group_names):
            ma, sh = res["mean_alignment"], res["share"]
            lines.append(f"  Mean Alignment | {name} | Biased: {ma['biased'][q][g]:.6f} | Debiased: {ma['debiased'][q][g]:.6f} || share of the top "
                         f"{res['k']}: {sh['biased'][q][g]:.3f} -> {sh['debiased'][q][g]:.3f} (prior {res['group_sizes'][g] / res['num_images']:.3f})")
    return lines


def bias_eval_main(_A):
    """Reference bias_eda.py as an evaluation: unnormalised projected text embeddings of the definitional pairs -> principal directions
    (debias.directions); unnormalised projected image features of the split with their groups; normalised prompt embeddings;
    debias.evaluate. Prints the per-prompt report and the result dict (also written to --output as JSON) and returns the dict."""
    import json
    import numpy as np
    pairs, prompts = _check_bias_eval_launch(_A)
    _DOWNC = Config(_A.down_config, _A.down_config_override)
    _C = Config(_A.config, list(_A.config_override) + ["AMP", _DOWNC.AMP])       # the compute dtype follows the downstream config
    _check_bias_eval_model(_A, _C)
    if not torch.cuda.is_available():
        raise SystemExit("bias_eval: no GPU visible; the encoders and the debias kernels run on the MI355X only")
    from . import debias, retrieval
    device = torch.device("cuda", torch.cuda.current_device())
    common_setup(_DOWNC, _A, job_type="downstream")
    synthetic = _DOWNC.DATA.ROOT == "random" and not _A.gender_data_path
    dataset = DownstreamDatasetFactory.from_config(_DOWNC, split=_A.split, gender_data_path=_A.gender_data_path, num_classes=2 if synthetic else None)
    groups = [dataset.label(i) for i in range(len(dataset))] if synthetic else list(dataset.targets)
    g, G = debias.check_groups(np.asarray(groups, dtype=np.int64), len(dataset), _A.num_results)
    loader = DataLoader(dataset, batch_size=_DOWNC.OPTIM.BATCH_SIZE, shuffle=False, num_workers=_A.cpu_workers, pin_memory=True,
                        collate_fn=dataset.collate_fn)
    arch = PretrainingModelFactory.from_config(_C)
    if _A.weight_init == "vlinfo":
        CheckpointManager(model=arch).load(_A.checkpoint_path)
    arch = arch.to(device)
    vocab, text_model = _C.DATA.TOKENIZER_VOCAB, _C.MODEL.TEXTUAL.NETWORK_NAME
    sides = []
    for side in (0, 1):
        ids, mask = tokenize_texts([p[side] for p in pairs], _A.max_length, vocab, text_model)
        sides.append(retrieval.embed_texts(arch, ids.to(device), mask.to(device), normalize=False))
    comps, evr = debias.directions(sides[0], sides[1], _A.components)
    ids, mask = tokenize_texts(prompts, _A.max_length, vocab, text_model)
    prompt_embeds = retrieval.embed_texts(arch, ids.to(device), mask.to(device))
    feats, labels = [], []
    for batch in loader:
        feats.append(retrieval.embed_images(arch, batch["image"].to(device, non_blocking=True), normalize=False).float())
        labels.append(batch["label"].reshape(-1))
    if not np.array_equal(torch.cat(labels).numpy(), g):
        raise ValueError("bias_eval: the loader's labels differ from the dataset's groups")
    res = debias.evaluate(torch.cat(feats, 0), g, prompt_embeds, comps, _A.num_results, evr.tolist())
    res.update({"prompts": prompts, "groups": [str(c) for c in dataset.classes], "pairs": [list(p) for p in pairs]})
    for line in report_bias(res, prompts, res["groups"]):
        print(line)
    print(json.dumps(res))
    if _A.output:
        with open(_A.output, "w") as fh:
            json.dump(res, fh)
    return res


def bias_eval_cli(argv=None):
    return bias_eval_main(build_bias_eval_parser().parse_args(argv))
