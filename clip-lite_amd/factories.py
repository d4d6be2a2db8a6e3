"""Name -> class registries with the reference's factory interface (reference factories.py:36-73 `Factory.create/from_config`,
:303-434 model factories, :437-487 OptimizerFactory, :490-531 LRSchedulerFactory, :169-238 PretrainingDatasetFactory).
Model/optimizer/scheduler products are the HIP-backed classes of this package; dataset products are the batch sources of
data.py (the albumentations / LMDB-backed datasets of the reference need dependencies and files that are not available)."""
import os
import re
from typing import Any, Callable, Dict, Iterable, List

from torch import nn

from . import data as vdata
from .config import Config
from .encoder import ImageEncoder, TextEncoder
from .loss import InfoNCELoss, JSDInfoMaxLoss, SigLIPLoss
from .model import VLInfoModel
from .optim import FusedAdamW, FusedLAMB, FusedLARS, FusedSGD, Lookahead, lr_scheduler


class Factory(object):
    PRODUCTS: Dict[str, Callable] = {}

    def __init__(self):
        raise ValueError(f"Cannot instantiate {self.__class__.__name__} object, use `create` classmethod.")

    @classmethod
    def create(cls, name: str, *args, **kwargs) -> Any:
        if name not in cls.PRODUCTS:
            raise KeyError(f"{cls.__class__.__name__} cannot create {name}.")
        return cls.PRODUCTS[name](*args, **kwargs)

    @classmethod
    def from_config(cls, config: Config) -> Any:
        raise NotImplementedError


class PretrainingDatasetFactory(Factory):
    PRODUCTS: Dict[str, Callable] = {"random": vdata.RandomDataset, "json": vdata.JsonCaptionDataset}

    @classmethod
    def from_config(cls, config: Config, split: str = "train"):
        _C = config
        kwargs = {"mode": _C.MODEL.TEXTUAL.NAME, "image_size": _C.DATA.IMAGE_CROP_SIZE, "max_caption_length": _C.DATA.MAX_CAPTION_LENGTH,
                  "tokenizer_vocab": _C.DATA.TOKENIZER_VOCAB, "text_model": _C.MODEL.TEXTUAL.NETWORK_NAME,
                  # transform names as configured; resize / crop transforms take IMAGE_CROP_SIZE (reference factories.py:213-224)
                  "image_transform": tuple(getattr(_C.DATA, f"IMAGE_TRANSFORM_{split.upper()}")),
                  "gpu_augment": _C.DATA.GPU_AUGMENT, "source_size": _C.DATA.GPU_AUGMENT_SOURCE_SIZE,
                  "visual_self_supervised": _C.MODEL.VISUAL.SELF_SUPERVISED, "textual_self_supervised": _C.MODEL.TEXTUAL.SELF_SUPERVISED}
        if _C.MODEL.NAME == "json":
            kwargs["json_files"] = list(_C.DATA.JSON_FILES_TRAIN if split == "train" else _C.DATA.JSON_FILES_VAL)
            kwargs["data_root"] = _C.DATA.ROOT
        elif _C.MODEL.NAME == "random":
            kwargs["length"] = 118000 if split == "train" else 5000
        else:
            raise KeyError(f"MODEL.NAME={_C.MODEL.NAME!r}: the LMDB-backed COCO dataset needs lmdb/albumentations and the serialized "
                           "dataset, which are not available; use MODEL.NAME random or json")
        return cls.create(_C.MODEL.NAME, **kwargs)


class NegativeSamplingDatasetFactory(Factory):
    """The clustered dataset of the second training phase (reference factories.py:248-300): the pretraining dataset of the split wrapped
    in data.ClusteredDataset. Of the reference's kwargs those that apply here: cluster_path, split, total_iters,
    negative_sampling_start_iter (data_root / tokenizer / transforms are the base dataset's; use_single_caption and coco_root belong to
    the LMDB reader)."""
    PRODUCTS: Dict[str, Callable] = {"clusters": vdata.ClusteredDataset}

    @classmethod
    def from_config(cls, config: Config, split: str = "train"):
        _C = config
        kind = "clusters" if "clusters" in _C.DATA.NEGATIVE_SAMPLING else _C.DATA.NEGATIVE_SAMPLING
        return cls.create(kind, base=PretrainingDatasetFactory.from_config(_C, split=split), cluster_path=_C.DATA.CLUSTER_PATH, split=split,
                          total_iters=_C.OPTIM.NUM_ITERATIONS, negative_sampling_start_iter=_C.DATA.NEGATIVE_SAMPLING_START_ITERATION,
                          seed=_C.RANDOM_SEED)


class DownstreamDatasetFactory(Factory):
    """Labelled image sources of the downstream evaluations (reference factories.py:534-596, linear_clf.py, voc_clf.py): DATA.ROOT "random"
    is the synthetic RandomLabelledDataset; a VOC2007 root (the last path component contains "voc") with split "trainval" or "test" is
    VOC07ClassificationDataset, the source of voc_clf.py's SVM evaluation; any other root is an image folder root/{train,val}/<class>/<image>
    (ImageFolderDataset, the layout of the reference's ImageNetDataset / INaturalist2018Dataset). A VOC root with another split (linear_clf.py's
    train / val) and VOC detection (voc_det.py: detectron2) are not supported. bias_eval.py passes `gender_data_path` (the reference's COCO
    gender annotation over a COCO root: GenderAnnotationDataset) or `num_classes` (the number of groups of the synthetic source)."""
    PRODUCTS: Dict[str, Callable] = {"random": vdata.RandomLabelledDataset, "folder": vdata.ImageFolderDataset,
                                     "voc": vdata.VOC07ClassificationDataset, "gender": vdata.GenderAnnotationDataset}
    # reference linear_clf.py:105 (the dataset name is the last path component of DATA.ROOT; "imagenet2012" means "imagenet")
    NUM_CLASSES_MAPPING = {"imagenet": 1000, "inaturalist": 8142}

    @staticmethod
    def dataset_name(root: str) -> str:
        name = root.rstrip("/").split("/")[-1]
        return "imagenet" if name == "imagenet2012" else name

    @classmethod
    def from_config(cls, config: Config, split: str = "train", gender_data_path: str = None, num_classes: int = None):
        _C = config
        root = _C.DATA.ROOT
        if gender_data_path:
            if root == "random":
                raise ValueError("the gender annotation needs the COCO images: set DATA.ROOT to the COCO root (<root>/<split>2017/<image>)")
            return cls.create("gender", data_root=root, gender_data_path=gender_data_path, split=split,
                              image_transform=tuple(_C.DATA.IMAGE_TRANSFORM_VAL), image_size=_C.DATA.IMAGE_CROP_SIZE, seed=_C.RANDOM_SEED)
        if "voc" in cls.dataset_name(root).lower():
            if split not in ("trainval", "test"):
                raise NotImplementedError(f"VOC2007 split {split!r}: VOC2007 is evaluated by voc_clf.py's SVMs on 'trainval' / 'test'; "
                                          "linear_clf.py's train / val splits of VOC and detection (voc_det.py, detectron2) are not supported")
            transform = tuple(_C.DATA.IMAGE_TRANSFORM_TRAIN if split == "trainval" else _C.DATA.IMAGE_TRANSFORM_VAL)
            return cls.create("voc", data_root=root, split=split, image_transform=transform, image_size=_C.DATA.IMAGE_CROP_SIZE,
                              seed=_C.RANDOM_SEED)
        if root == "random":
            extra = {} if num_classes is None else {"num_classes": int(num_classes)}
            return cls.create("random", image_size=_C.DATA.IMAGE_CROP_SIZE, length=50000 if split == "train" else 500, split=split,
                              seed=_C.RANDOM_SEED, **extra)
        transform = tuple(_C.DATA.IMAGE_TRANSFORM_TRAIN if "train" in split else _C.DATA.IMAGE_TRANSFORM_VAL)
        ds = cls.create("folder", data_root=root, split=split, image_transform=transform, image_size=_C.DATA.IMAGE_CROP_SIZE,
                        percentage=_C.DATA.USE_PERCENTAGE, seed=_C.RANDOM_SEED)
        want = cls.NUM_CLASSES_MAPPING.get(cls.dataset_name(root))
        if want is not None and ds.num_classes != want:
            raise ValueError(f"{root}/{split} has {ds.num_classes} class directories; {cls.dataset_name(root)} has {want}")
        return ds


class RetrievalDatasetFactory(Factory):
    """Image-text retrieval sources of retrieval.py (reference factories.py:604-616 with ReEvalDataset / re_eval_dataset): an explicit
    `ann_file` is a JSON list of {"image", "caption": [...]} with image paths relative to DATA.ROOT; otherwise a root whose last path component
    contains "flickr" reads <root>/data/flickr30k_test.json the same way, and one that contains "coco" is the COCO 2017 layout
    <root>/{split}2017/*.jpg + <root>/annotations/captions_{split}2017.json. Images go through DATA.IMAGE_TRANSFORM_VAL at IMAGE_CROP_SIZE."""
    PRODUCTS: Dict[str, Callable] = {"retrieval": vdata.RetrievalEvalDataset}

    @classmethod
    def from_config(cls, config: Config, split: str = "val", ann_file: str = None):
        _C = config
        root = _C.DATA.ROOT
        name = DownstreamDatasetFactory.dataset_name(root).lower()
        if not ann_file:
            if "flickr" in name:
                ann_file = os.path.join(root, "data", "flickr30k_test.json")
            elif "coco" not in name:
                raise ValueError(f"retrieval dataset root {root!r}: supported layouts are a JSON caption list (--ann-file), a Flickr30k root "
                                 "(last path component contains 'flickr': <root>/data/flickr30k_test.json) and a COCO 2017 root (last path "
                                 "component contains 'coco': <root>/{split}2017/*.jpg, <root>/annotations/captions_{split}2017.json)")
        return cls.create("retrieval", data_root=root, ann_file=ann_file or "", split=split,
                          image_transform=tuple(_C.DATA.IMAGE_TRANSFORM_VAL), image_size=_C.DATA.IMAGE_CROP_SIZE, seed=_C.RANDOM_SEED)


class VisualBackboneFactory(Factory):
    PRODUCTS: Dict[str, Callable] = {"captions": ImageEncoder, "random": ImageEncoder, "json": ImageEncoder}

    @classmethod
    def from_config(cls, config: Config) -> ImageEncoder:
        # like the reference (factories.py:324-327) the network name is forwarded; a ViT is also built for one image size (its position embedding)
        _C = config
        enc = cls.create(_C.MODEL.NAME, img_enc_net=_C.MODEL.VISUAL.NETWORK_NAME, image_size=_C.DATA.IMAGE_CROP_SIZE,
                         patch_dropout=_C.MODEL.VISUAL.PATCH_DROPOUT)
        if enc.out_dim != _C.MODEL.VISUAL.FEATURE_SIZE:
            raise ValueError(f"MODEL.VISUAL.FEATURE_SIZE is {_C.MODEL.VISUAL.FEATURE_SIZE}, but {_C.MODEL.VISUAL.NETWORK_NAME} produces "
                             f"{enc.out_dim} features; set MODEL.VISUAL.FEATURE_SIZE to {enc.out_dim}")
        return enc


class TextualHeadFactory(Factory):
    PRODUCTS: Dict[str, Callable] = {"glove": TextEncoder, "sbert": TextEncoder, "train_sbert": TextEncoder}

    @classmethod
    def from_config(cls, config: Config) -> nn.Module:
        _C = config
        name = _C.MODEL.TEXTUAL.NAME
        kwargs = {
            "word_dict": {}, "mode": name, "transform_embedding": _C.MODEL.TEXTUAL.TRANSFORM, "txt_enc_dim": _C.MODEL.TEXTUAL.FEATURE_SIZE,
            "load_glove": _C.MODEL.TEXTUAL.LOAD_GLOVE, "glove_path": _C.MODEL.TEXTUAL.GLOVE_PATH, "train_enc": _C.MODEL.TEXTUAL.TRAIN_EMBEDDINGS,
            "pretrained": _C.MODEL.TEXTUAL.PRETRAINED, "model_name": _C.MODEL.TEXTUAL.NETWORK_NAME,
            "num_hidden_layers": _C.MODEL.TEXTUAL.NUM_HIDDEN_LAYERS, "context_length": _C.MODEL.TEXTUAL.CONTEXT_LENGTH,
        }
        return cls.create(name, **kwargs)


class LossFactory(Factory):
    # "infonce": BASELINE config 4, "siglip": the pairwise sigmoid loss of Zhai et al. 2023 (neither is in the reference)
    PRODUCTS: Dict[str, Callable] = {"jsd": JSDInfoMaxLoss, "infonce": InfoNCELoss, "siglip": SigLIPLoss}

    @classmethod
    def from_config(cls, config: Config) -> JSDInfoMaxLoss:
        _C = config
        kwargs = {
            "image_dim": _C.MODEL.VISUAL.FEATURE_SIZE, "text_dim": _C.MODEL.TEXTUAL.FEATURE_SIZE, "type": _C.MODEL.LOSS.TYPE,
            "image_prior": _C.MODEL.LOSS.IMAGE_PRIOR, "text_prior": _C.MODEL.LOSS.TEXT_PRIOR, "prior_weight": _C.MODEL.LOSS.PRIOR_WEIGHT,
            "visual_self_supervised": _C.MODEL.VISUAL.SELF_SUPERVISED, "textual_self_supervised": _C.MODEL.TEXTUAL.SELF_SUPERVISED,
        }
        return cls.create(_C.MODEL.LOSS.NAME, **kwargs)


class PretrainingModelFactory(Factory):
    PRODUCTS: Dict[str, Callable] = {"captions": VLInfoModel, "random": VLInfoModel, "json": VLInfoModel}

    @classmethod
    def from_config(cls, config: Config) -> nn.Module:
        _C = config
        visual = VisualBackboneFactory.from_config(_C)      # construction order as in the reference (factories.py:429-431)
        textual = TextualHeadFactory.from_config(_C)
        loss = LossFactory.from_config(_C)
        return cls.create(_C.MODEL.NAME, textual, visual, loss, _C.MODEL.TEXTUAL.NAME, _C.AMP)


class OptimizerFactory(Factory):
    PRODUCTS: Dict[str, Callable] = {"sgd": FusedSGD, "adamw": FusedAdamW, "lars": FusedLARS, "lamb": FusedLAMB}

    @classmethod
    def from_config(cls, config: Config, named_parameters: Iterable[Any]):
        _C = config
        param_groups: List[Dict[str, Any]] = []
        for name, param in named_parameters:
            wd = 0.0 if re.match(_C.OPTIM.NO_DECAY, name) else _C.OPTIM.WEIGHT_DECAY
            if "image_encoder" in name:
                lr = _C.OPTIM.CNN_LR
            elif "text_encoder" in name:
                lr = _C.OPTIM.TRANS_LR
            else:
                lr = _C.OPTIM.LR
            param_groups.append({"params": [param], "lr": lr, "weight_decay": wd})
        kwargs = {"momentum": _C.OPTIM.SGD_MOMENTUM} if _C.OPTIM.OPTIMIZER_NAME in ("sgd", "lars") else {}          # (reference factories.py:478-483)
        if _C.OPTIM.OPTIMIZER_NAME == "lars":
            kwargs.update(trust_coefficient=_C.OPTIM.LARS.TRUST_COEFFICIENT, eps=_C.OPTIM.LARS.EPS)
        if _C.OPTIM.OPTIMIZER_NAME == "lamb":
            kwargs.update(betas=(_C.OPTIM.LAMB.BETA1, _C.OPTIM.LAMB.BETA2), eps=_C.OPTIM.LAMB.EPS, trust_clip=_C.OPTIM.LAMB.TRUST_CLIP)
        optimizer = cls.create(_C.OPTIM.OPTIMIZER_NAME, param_groups, **kwargs)
        if _C.OPTIM.LOOKAHEAD.USE:
            optimizer = Lookahead(optimizer, k=_C.OPTIM.LOOKAHEAD.STEPS, alpha=_C.OPTIM.LOOKAHEAD.ALPHA)
        return optimizer


class LRSchedulerFactory(Factory):
    PRODUCTS: Dict[str, Callable] = {
        "none": lr_scheduler.LinearWarmupNoDecayLR, "multistep": lr_scheduler.LinearWarmupMultiStepLR,
        "linear": lr_scheduler.LinearWarmupLinearDecayLR, "cosine": lr_scheduler.LinearWarmupCosineAnnealingLR,
    }

    @classmethod
    def from_config(cls, config: Config, optimizer):
        _C = config
        kwargs = {"total_steps": _C.OPTIM.NUM_ITERATIONS, "warmup_steps": _C.OPTIM.WARMUP_STEPS}
        if _C.OPTIM.LR_DECAY_NAME == "multistep":
            kwargs.update(gamma=_C.OPTIM.LR_GAMMA, milestones=_C.OPTIM.LR_STEPS)
        if _C.OPTIM.LR_DECAY_NAME == "cosine":
            kwargs.update(min_mult=_C.OPTIM.MIN_LR_MULT)
        return cls.create(_C.OPTIM.LR_DECAY_NAME, optimizer, **kwargs)
