"""Batch sources for the pretraining step. Only the batch-dict CONTRACT of the reference's input pipeline is in scope
(SURVEY.md §8b): `image` f32 NCHW (ImageNet-normalised), `input_ids` / `attention_mask` int64 right-padded with the pad id 0
(reference data/dataloader.py:218-236), or `caption_encodings` f32 [B][768] in the frozen-sentence-embedding mode
(reference model.py:48-50). The LMDB / albumentations stack (reference data/readers.py, data/transforms.py) is CPU-side I/O outside the accelerated path and
its dependencies are absent from the image.

`RandomDataset` is the counterpart of the reference's synthetic dataset (data/dataloader.py:36-114: random 3x224x224 images and
four fixed captions, len 118000). `JsonCaptionDataset` reads the reference's json record format ({"image": path, "caption": str},
data/mock_data.json; reference data/dataloader.py:115-236, JsonDataset).

Text source: `WordPieceTokenizer(vocab.txt)` is BERT's uncased WordPiece (the reference calls
`BertTokenizer.from_pretrained('bert-base-uncased')(caption, padding=False, truncation=True, max_length=L)`, data/dataloader.py:139-141,
196-202) built on the installed `tokenizers` package from a local vocabulary file (`DATA.TOKENIZER_VOCAB`; the HF hub is not reachable
here, so the file must be supplied). Without a vocabulary the offline default is `hash_tokenize`, a deterministic word -> id hash with the
same [CLS] ... [SEP] framing.

Image source: when a record's image file exists it is decoded with PIL and put through the reference's transforms by name
(`DATA.IMAGE_TRANSFORM_{TRAIN,VAL}`; factories.py:112-160): smallest_resize (shorter side -> 256 for DEFAULT_IMAGE_TRANSFORM, else the
crop size), center_crop, random_resized_crop (scale 0.2-1), horizontal_flip (which also swaps "left" / "right" in the caption), color_jitter,
random_gray, blur, normalize (ImageNet mean / std on [0, 1] pixels), HWC -> CHW float32
(data/dataloader.py:186-192). A record whose file is missing gets a seeded synthetic image (the mock json of the reference points at
files that exist on no machine we have).
"""
import hashlib
import json
import math
import os
import re
import unicodedata

import torch
from torch.utils.data import Dataset

CAPTIONS = ["a photo of a cat sitting on a couch", "two people riding bikes down a city street",
            "a plate of food with vegetables on a table", "a large airplane flying through a cloudy sky"]


_DROPPED = str.maketrans("", "", ",.'!?\"()*#:;~")


def normalize_caption(caption: str, max_caption_length: int = 30) -> str:
    """The reference's caption normalisation (data/transforms.py:46-90, NormalizeCaption): lower-case; delete , . ' ! ? " ( ) * # : ; ~;
    '-' and '/' become spaces; the COCO placeholder "<person>" becomes "person"; runs of two or more whitespace characters collapse
    to one space; trailing newlines and surrounding spaces go; at most `max_caption_length` space-separated words are kept; finally NFKD
    decomposition with the combining marks removed (accents stripped)."""
    c = caption.lower().translate(_DROPPED).replace("-", " ").replace("/", " ").replace("<person>", "person")
    c = re.sub(r"\s{2,}", " ", c).rstrip("\n").strip(" ")
    words = c.split(" ")
    if len(words) > max_caption_length:
        c = " ".join(words[:max_caption_length])
    c = unicodedata.normalize("NFKD", c.lower())
    return "".join(ch for ch in c if not unicodedata.combining(ch))


def text_framing(model_name: str) -> str:
    """Which tokenizer framing a text tower's name selects — the same test the reference applies to the name (encoder.py:165): "bert" in it
    means BERT ([CLS] ... [SEP], pad id 0), anything else the MPNet tower (<s> ... </s>, pad id 1). A CLIP text tower ("clip_text*", tested
    first) takes the BERT framing: WordPiece ids, pad id 0, and [SEP] — the last attended token — in the end-of-text role its pooling reads
    (CLIP's own BPE tokenizer is a download)."""
    name = model_name or "bert"
    return "bert" if name.startswith("clip_text") or "bert" in name else "mpnet"


MPNET_VOCAB_SIZE = 30527          # transformers.MPNetConfig().vocab_size


def hash_tokenize(caption: str, max_len: int, vocab: int = 30522, framing: str = "bert"):
    """normalize_caption, then map every word to a stable id in [1000, vocab); [CLS]=101 ... [SEP]=102 (the HF tokenizer files the
    reference loads, data/tokenizers.py, are not available offline). framing "mpnet": <s>=0 ... </s>=2 around word ids in
    [4, MPNET_VOCAB_SIZE), so that the specials 0 .. 3 (<s>, <pad>, </s>, <unk>) never occur inside a caption."""
    words = re.sub(r"[^a-z0-9 ]", " ", normalize_caption(caption, max_len)).split()
    if framing == "mpnet":
        return [0] + [4 + int.from_bytes(hashlib.md5(w.encode()).digest()[:4], "little") % (MPNET_VOCAB_SIZE - 4) for w in words][: max_len - 2] + [2]
    ids = [101] + [1000 + int.from_bytes(hashlib.md5(w.encode()).digest()[:4], "little") % (vocab - 1000) for w in words][: max_len - 2] + [102]
    return ids


class WordPieceTokenizer:
    """BERT uncased WordPiece over a local vocab.txt: BertNormalizer (clean text, lower-case, strip accents, CJK spacing) ->
    BertPreTokenizer (whitespace + punctuation) -> greedy longest-match WordPiece ("##" continuation, [UNK] for unmatched words, words
    over 100 characters -> [UNK]) -> "[CLS] ... [SEP]" -> truncation to max_length INCLUDING the two specials — i.e. what the reference's
    `BertTokenizer(caption, padding=False, truncation=True, max_length=L)` returns in `input_ids` (data/dataloader.py:196-202).
    framing "mpnet": the same pipeline with transformers.MPNetTokenizer's specials, read from the user's vocab.txt: "<s> ... </s>", pad
    "<pad>", and as the unknown token "[UNK]" where the vocabulary has it (the published MPNet vocabularies do, and it is MPNetTokenizer's
    default), else "<unk>"."""

    SPECIALS = {"bert": ("[PAD]", "[CLS]", "[SEP]"), "mpnet": ("<pad>", "<s>", "</s>")}

    def __init__(self, vocab_path: str, framing: str = "bert"):
        from tokenizers import Tokenizer, models, normalizers, pre_tokenizers, processors
        if not os.path.isfile(vocab_path):
            raise FileNotFoundError(f"WordPiece vocabulary {vocab_path!r} not found (DATA.TOKENIZER_VOCAB)")
        self.vocab_path = vocab_path
        vocab = {}
        with open(vocab_path, encoding="utf-8") as fh:
            for i, line in enumerate(fh):
                tok = line.rstrip("\n")
                if tok != "" and tok not in vocab:
                    vocab[tok] = i
        self.framing = framing
        pad, cls, sep = self.SPECIALS[framing]
        unk = "[UNK]" if framing == "bert" or "[UNK]" in vocab else "<unk>"
        for special in (pad, unk, cls, sep):
            if special not in vocab:
                raise ValueError(f"{vocab_path}: vocabulary lacks {special}")
        self.pad_token_id, self.cls_token_id, self.sep_token_id, self.unk_token_id = vocab[pad], vocab[cls], vocab[sep], vocab[unk]
        self.vocab_size = max(vocab.values()) + 1
        tk = Tokenizer(models.WordPiece(vocab, unk_token=unk, max_input_chars_per_word=100))
        tk.normalizer = normalizers.BertNormalizer(clean_text=True, handle_chinese_chars=True, strip_accents=None, lowercase=True)
        tk.pre_tokenizer = pre_tokenizers.BertPreTokenizer()
        tk.post_processor = processors.TemplateProcessing(single=f"{cls} $A {sep}", special_tokens=[(cls, self.cls_token_id), (sep, self.sep_token_id)])
        self._tk = tk

    def __getstate__(self):          # picklable for DataLoader workers (the reference's tokenizers do the same, data/tokenizers.py:80-92)
        return {"vocab_path": self.vocab_path, "framing": self.framing}

    def __setstate__(self, st):
        self.__init__(st["vocab_path"], st.get("framing", "bert"))

    def __call__(self, caption: str, max_length: int):
        self._tk.enable_truncation(max_length=max_length)
        return self._tk.encode(caption).ids


IMAGENET_COLOR_MEAN = (0.485, 0.456, 0.406)      # reference data/transforms.py:232-235
IMAGENET_COLOR_STD = (0.229, 0.224, 0.225)
DEFAULT_IMAGE_TRANSFORM = ("smallest_resize::256", "center_crop", "normalize")     # reference data/transforms.py:238-244


def swap_left_right(caption: str) -> str:
    """What the reference's HorizontalFlip does to the caption of a flipped image (data/transforms.py:175-181): "left" <-> "right"."""
    return caption.replace("left", "[TMP]").replace("right", "left").replace("[TMP]", "right")


def _transform_args(arg: str, crop_size: int):
    """The part after "::" of a transform name. The reference's syntax is a kwargs dict, `random_resized_crop::{'scale': (0.08, 1.0)}`
    (factories.py:112-115,163-173: eval of the text; here ast.literal_eval — literals only); a bare integer is this package's short form for
    the size. Returns (size, kwargs)."""
    if not arg:
        return crop_size, {}
    import ast
    val = ast.literal_eval(arg)
    if isinstance(val, dict):
        kw = dict(val)
        size = int(kw.pop("size", kw.pop("max_size", crop_size)))
        return size, kw
    return int(val), {}


def _color_jitter(img, rnd, brightness=0.4, contrast=0.4, saturation=0.4, hue=0.1, p=0.8):
    """The reference's `color_jitter` (factories.py:132-134: albumentations ColorJitter(0.4, 0.4, 0.4, 0.1, p = 0.8)) on a PIL image:
    with probability p, brightness / contrast / saturation factors uniform in [1 - x, 1 + x] and a hue shift uniform in [-hue, hue] (fraction of
    the colour circle), applied in a random order. Same distribution family as albumentations / torchvision; the draws come from this
    package's generator, so individual images differ from an albumentations run with the same seed."""
    from PIL import Image, ImageEnhance
    import numpy as np
    if rnd() >= p:
        return img
    fb, fc, fs = (1.0 + (2.0 * rnd() - 1.0) * x for x in (brightness, contrast, saturation))
    fh = (2.0 * rnd() - 1.0) * hue
    order = sorted(range(4), key=lambda _: rnd())
    for op in order:
        if op == 0:
            img = ImageEnhance.Brightness(img).enhance(fb)
        elif op == 1:
            img = ImageEnhance.Contrast(img).enhance(fc)
        elif op == 2:
            img = ImageEnhance.Color(img).enhance(fs)
        else:
            hsv = np.asarray(img.convert("HSV")).copy()
            hsv[..., 0] = (hsv[..., 0].astype(np.int16) + int(round(fh * 255))) % 256
            img = Image.fromarray(hsv, "HSV").convert("RGB")
    return img


def _gaussian_blur(img, weights):
    """The reference's `blur` once it fires (factories.py: albumentations GaussianBlur over cv2.GaussianBlur with sigma 0) on a PIL image, in
    NumPy: the separable 7-tap filter with the symmetric `weights` (centre outward; augment.BLUR_WEIGHTS, OpenCV's fixed kernels), border
    REFLECT_101, the horizontal pass then the vertical one in f32 (exact: the weights are dyadic), rounded back to uint8."""
    from PIL import Image
    import numpy as np
    a = np.asarray(img, dtype=np.float32)
    h, w = a.shape[:2]
    if min(h, w) < 4:
        raise ValueError(f"blur of a {h} x {w} image: the reflected border needs at least 4 pixels per side")
    taps = [weights[abs(i)] for i in range(-3, 4)]
    p = np.pad(a, ((0, 0), (3, 3), (0, 0)), mode="reflect")
    a = sum(np.float32(t) * p[:, i:i + w] for i, t in enumerate(taps))
    p = np.pad(a, ((3, 3), (0, 0), (0, 0)), mode="reflect")
    a = sum(np.float32(t) * p[i:i + h] for i, t in enumerate(taps))
    return Image.fromarray(np.clip(np.rint(a), 0, 255).astype(np.uint8), "RGB")


def load_image(path: str, transforms, crop_size: int, generator=None, return_flipped=False, decisions=None):
    """PIL decode -> RGB -> the named transforms -> f32 CHW (reference data/dataloader.py:186-192 with the transform table of
    factories.py:112-160). Names may carry arguments as "name::{kwargs dict}" (the reference's syntax, factories.py:112-115) or "name::size";
    factories.py:213-221 passes the crop size to the resize / crop transforms. Random transforms draw from `generator` (a torch.Generator) so
    that a dataset index is reproducible. return_flipped: also return whether `horizontal_flip` fired — the reference's flip swaps "left" and
    "right" in the caption of a flipped image (data/transforms.py:156-181), which the dataset applies before tokenising.
    `random_gray` (factories.py: alb.ToGray, p = 0.2) and `blur` (alb.GaussianBlur, p = 0.5, blur_limit (3, 7)) draw as augment.py's docstring
    says, the same draws as the GPU path's planner. decisions: a dict that receives what the random transforms decided ("flipped", "gray",
    "blur": the kernel size or 0)."""
    from PIL import Image
    import numpy as np
    img = Image.open(path).convert("RGB")

    def rnd():
        return float(torch.rand((), generator=generator))

    normalized, flipped, gray, blur_k = False, False, False, 0
    for spec in transforms:
        name, _, arg = spec.partition("::")
        size, kw = _transform_args(arg, crop_size)
        if name == "smallest_resize":            # albumentations SmallestMaxSize: shorter side -> size, aspect kept, bilinear
            w, h = img.size
            sc = size / min(w, h)
            img = img.resize((max(1, round(w * sc)), max(1, round(h * sc))), Image.BILINEAR)
        elif name == "global_resize":
            img = img.resize((size, size), Image.BILINEAR)
        elif name == "center_crop":              # reference data/transforms.py CenterSquareCrop
            w, h = img.size
            l, t = (w - size) // 2, (h - size) // 2
            img = img.crop((l, t, l + size, t + size))
        elif name == "random_resized_crop":      # reference factories.py:124-126: RandomResizedSquareCrop(scale=(0.2, 1.0), ratio=(0.75, 1.333)); 10 tries then centre
            s_lo, s_hi = kw.get("scale", (0.2, 1.0))
            r_lo, r_hi = kw.get("ratio", (0.75, 1.333))
            w, h = img.size
            box = None
            for _ in range(10):
                area = w * h * (s_lo + (s_hi - s_lo) * rnd())
                logr = math.log(r_lo) + (math.log(r_hi) - math.log(r_lo)) * rnd()
                ar = math.exp(logr)
                cw, ch = int(round(math.sqrt(area * ar))), int(round(math.sqrt(area / ar)))
                if 0 < cw <= w and 0 < ch <= h:
                    l, t = int(rnd() * (w - cw + 1)), int(rnd() * (h - ch + 1))
                    box = (l, t, l + cw, t + ch)
                    break
            if box is None:
                s_ = min(w, h)
                box = ((w - s_) // 2, (h - s_) // 2, (w - s_) // 2 + s_, (h - s_) // 2 + s_)
            img = img.crop(box).resize((size, size), Image.BILINEAR)
        elif name == "horizontal_flip":          # reference factories.py:141: p = 0.5; the caption side is the caller's (return_flipped)
            if rnd() < kw.get("p", 0.5):
                img = img.transpose(Image.FLIP_LEFT_RIGHT)
                flipped = not flipped
        elif name in ("color_jitter", "color_jitter8"):
            x = 0.8 if name == "color_jitter8" else 0.4
            img = _color_jitter(img, rnd, kw.get("brightness", x), kw.get("contrast", x), kw.get("saturation", x), kw.get("hue", 0.1), kw.get("p", 0.8))
        elif name == "random_gray":
            from . import augment
            if augment.draw_gray(rnd, kw):
                img = img.convert("L").convert("RGB")
                gray = True
        elif name == "blur":
            from . import augment
            k = augment.draw_blur(rnd, kw)
            if k:
                img = _gaussian_blur(img, augment.BLUR_WEIGHTS[k])
                blur_k = k
        elif name == "normalize":
            normalized = True
        else:
            raise KeyError(f"unknown image transform {spec!r}")
    if decisions is not None:
        decisions.update(flipped=flipped, gray=gray, blur=blur_k)
    x = torch.from_numpy(np.asarray(img, dtype=np.float32).copy()) / 255.0          # HWC in [0, 1]
    if normalized:                               # albumentations Normalize(mean, std, max_pixel_value=255)
        x = (x - torch.tensor(IMAGENET_COLOR_MEAN)) / torch.tensor(IMAGENET_COLOR_STD)
    x = x.permute(2, 0, 1).contiguous()
    return (x, flipped) if return_flipped else x


class _CaptionDataset(Dataset):
    """Image-caption pairs. gpu_augment: items carry a uint8 canvas and a plan row instead of the finished image (augment.py; the kernels finish it
    on the device), source_size being DATA.GPU_AUGMENT_SOURCE_SIZE. visual_self_supervised: a second view of the image - `aug_image`, a second
    load_image of the same file from the same generator, or with gpu_augment `aug_image_plan`, a second plan row over the same canvas.
    textual_self_supervised: `aug_input_ids` / `aug_attention_mask` from another caption of the same record (reference data/dataloader.py:335-339,
    390-407); a record with a single distinct caption re-uses it (the reference's `while aug_caption == caption` loops for ever there)."""

    def __init__(self, mode: str, image_size: int, max_caption_length: int, length: int, seed: int = 0, tokenizer_vocab: str = "",
                 image_transform=DEFAULT_IMAGE_TRANSFORM, gpu_augment: bool = False, source_size: int = 256, visual_self_supervised: bool = False,
                 textual_self_supervised: bool = False, text_model: str = "bert-base-uncased"):
        self.mode, self.image_size, self.max_len, self.length, self.seed = mode, image_size, max_caption_length, length, seed
        # the text tower's name (MODEL.TEXTUAL.NETWORK_NAME) picks the framing and the pad id: BERT [CLS] ... [SEP] / 0, MPNet <s> ... </s> / 1
        self.framing = text_framing(text_model)
        self.tokenizer = WordPieceTokenizer(tokenizer_vocab, self.framing) if tokenizer_vocab else None
        self.pad_token_id = self.tokenizer.pad_token_id if self.tokenizer is not None else (0 if self.framing == "bert" else 1)
        self.image_transform = tuple(image_transform)
        self.gpu_augment, self.visual_ssl, self.textual_ssl = bool(gpu_augment), bool(visual_self_supervised), bool(textual_self_supervised)
        self.textual_ssl = self.textual_ssl and mode != "sbert"          # (frozen caption encodings: there is no caption to re-tokenise)
        if self.gpu_augment:
            from . import augment
            self.canvas_side = augment.canvas_short_side(self.image_transform, image_size, source_size)
            self.canvas_cap = augment.canvas_capacity(self.canvas_side)

    def tokenize(self, caption: str):
        if self.tokenizer is not None:            # the reference's order: NormalizeCaption, then the BERT tokenizer (data/dataloader.py:194-202)
            return self.tokenizer(normalize_caption(caption, self.max_len), self.max_len)
        return hash_tokenize(caption, self.max_len, framing=self.framing)

    def image_path(self, idx):
        return None

    def __len__(self):
        return self.length

    def caption(self, idx):
        raise NotImplementedError

    def captions(self, idx):
        """Every caption of the record; `caption(idx)` is the one the pair uses."""
        return [self.caption(idx)]

    def aug_caption(self, idx, caption, generator):
        """Another caption of the record, uniform over those that differ from `caption`; `caption` itself when there is none."""
        others = [c for c in self.captions(idx) if c != caption]
        if not others:
            return caption
        return others[int(torch.randint(len(others), (), generator=generator))]

    def _gpu_item(self, path, g):
        """canvas + plan row(s) of one record (augment.py); returns (item entries, flipped)"""
        from . import augment
        if path is not None and os.path.isfile(path):
            from PIL import Image
            canvas = augment.make_canvas(Image.open(path), self.canvas_side)
        else:
            canvas = augment.synthetic_canvas(self.canvas_side, g)
        h, w = canvas.shape[:2]
        post = augment.needs_post(self.image_transform)          # random_gray / blur: a post row beside every plan row
        out = {"image_u8": torch.from_numpy(canvas)}
        for pre in ("", "aug_") if self.visual_ssl else ("",):
            rows = augment.plan_transforms(h, w, self.image_transform, self.image_size, g, return_post=post)
            out[pre + "image_plan"] = rows[0] if post else rows
            if post:
                out[pre + "image_post"] = rows[1]
        return out, bool(out["image_plan"][augment.PLAN_FLIP] != 0)

    def __getitem__(self, idx):
        g = torch.Generator().manual_seed(self.seed * 1000003 + idx)
        path = self.image_path(idx)
        flipped = False
        item = {"image_id": torch.tensor(idx, dtype=torch.long)}
        if self.gpu_augment:
            views, flipped = self._gpu_item(path, g)
            item.update(views)
        elif path is not None and os.path.isfile(path):
            item["image"], flipped = load_image(path, self.image_transform, self.image_size, g, return_flipped=True)
            if self.visual_ssl:
                item["aug_image"] = load_image(path, self.image_transform, self.image_size, g)
        else:
            item["image"] = torch.randn(3, self.image_size, self.image_size, generator=g)
            if self.visual_ssl:
                item["aug_image"] = torch.randn(3, self.image_size, self.image_size, generator=g)
        if self.mode == "sbert":
            item["caption_encodings"] = torch.randn(768, generator=g)
        else:
            caption = self.caption(idx)
            aug = self.aug_caption(idx, caption, g) if self.textual_ssl else None
            if flipped:          # the image transforms run on (image, RAW caption) pairs in the reference: a flipped image swaps left / right
                caption = swap_left_right(caption)
            item["caption_tokens"] = torch.tensor(self.tokenize(caption), dtype=torch.long)
            if aug is not None:
                item["aug_caption_tokens"] = torch.tensor(self.tokenize(aug), dtype=torch.long)
        return item

    @staticmethod
    def _pad_captions(tokens, pad_id=0):
        """ids right-padded with the tokenizer's pad id; the attention mask is 0 at the pads. (The reference pads the MASK with pad_token_id too,
        data/dataloader.py:218-236 — all ones for MPNet's pad id 1; the correct mask is emitted here, README "MPNet text encoder".)"""
        L = max(len(t) for t in tokens)
        ids = torch.full((len(tokens), L), int(pad_id), dtype=torch.long)
        mask = torch.zeros(len(tokens), L, dtype=torch.long)
        for r, t in enumerate(tokens):
            ids[r, :len(t)] = t
            mask[r, :len(t)] = 1
        return ids, mask

    def collate_fn(self, items):
        batch = {"image_id": torch.stack([i["image_id"] for i in items])}
        if "image_u8" in items[0]:          # fixed-capacity tensors: every batch has the same shapes
            from . import augment
            batch["image_u8"], batch["image_hw"] = augment.pack_canvases([i["image_u8"] for i in items], self.canvas_cap)
            for k in ("image_plan", "aug_image_plan"):
                if k in items[0]:
                    batch[k] = torch.stack([i[k] for i in items])
                    augment.check_plan(batch[k], batch["image_hw"], self.image_size)
            for k in ("image_post", "aug_image_post"):
                if k in items[0]:
                    batch[k] = torch.stack([i[k] for i in items])
                    augment.check_post(batch[k], self.image_size)
        else:
            batch["image"] = torch.stack([i["image"] for i in items])
            if "aug_image" in items[0]:
                batch["aug_image"] = torch.stack([i["aug_image"] for i in items])
        if self.mode == "sbert":
            batch["caption_encodings"] = torch.stack([i["caption_encodings"] for i in items])
        else:
            batch["input_ids"], batch["attention_mask"] = self._pad_captions([i["caption_tokens"] for i in items], self.pad_token_id)
            if "aug_caption_tokens" in items[0]:
                batch["aug_input_ids"], batch["aug_attention_mask"] = self._pad_captions([i["aug_caption_tokens"] for i in items], self.pad_token_id)
        return batch


class RandomDataset(_CaptionDataset):
    def __init__(self, mode="train_sbert", image_size=224, max_caption_length=30, length=118000, seed=0, tokenizer_vocab="",
                 image_transform=DEFAULT_IMAGE_TRANSFORM, **augment_kwargs):
        super().__init__(mode, image_size, max_caption_length, length, seed, tokenizer_vocab, image_transform, **augment_kwargs)

    def caption(self, idx):
        return CAPTIONS[idx % len(CAPTIONS)]

    def aug_caption(self, idx, caption, generator):          # the next of the fixed captions (no draw)
        return CAPTIONS[(idx + 1) % len(CAPTIONS)]


class JsonCaptionDataset(_CaptionDataset):
    def __init__(self, json_files, mode="train_sbert", image_size=224, max_caption_length=30, seed=0, tokenizer_vocab="",
                 image_transform=DEFAULT_IMAGE_TRANSFORM, data_root="", **augment_kwargs):
        self.records = []
        for f in json_files:
            with open(f) as fh:
                self.records += json.load(fh)
        self.data_root = data_root
        super().__init__(mode, image_size, max_caption_length, len(self.records), seed, tokenizer_vocab, image_transform, **augment_kwargs)

    def image_path(self, idx):
        path = self.records[idx].get("image")
        if not path:
            return None
        return path if os.path.isabs(path) or not self.data_root else os.path.join(self.data_root, path)

    def caption(self, idx):
        c = self.records[idx]["caption"]
        return c[0] if isinstance(c, list) else c

    def captions(self, idx):
        c = self.records[idx]["caption"]
        return list(c) if isinstance(c, list) else [c]


# ------------------------------------------------------------------------------------------------ clustered negative sampling
_CLUSTER_MAP_RE = re.compile(r"^img_id_cluster_map_(?P<split>[A-Za-z0-9]+)_(?P<k>\d+)\.pkl$")


def cluster_map_path(cluster_path: str, split: str, k: int) -> str:
    """The file scripts/cluster.py writes for one cluster count (reference scripts/cluster.py:146-149)."""
    return os.path.join(cluster_path, f"img_id_cluster_map_{split}_{k}.pkl")


def get_cluster_options(cluster_path: str, split: str):
    """Cluster counts for which `cluster_path` holds an img_id_cluster_map_<split>_<k>.pkl, ascending (reference data/dataloader.py:
    get_cluster_options reads them off the file names in os.listdir order, which is undefined; sorted here so that a tie of the schedule goes
    to the smaller count)."""
    if not cluster_path or not os.path.isdir(cluster_path):
        raise FileNotFoundError(f"DATA.CLUSTER_PATH {cluster_path!r} is not a directory; write the cluster maps with cluster.py first")
    ks = set()
    for name in os.listdir(cluster_path):
        m = _CLUSTER_MAP_RE.match(name)
        if m and m.group("split") == split:
            ks.add(int(m.group("k")))
    return sorted(ks)


class ClusteredDataset(Dataset):
    """Pairs with a hard negative from the same caption cluster (reference data/dataloader.py:494-797, the clustered COCO dataset of
    train.py:150-208) over any `_CaptionDataset`. An item is the base item plus `neg_image` / `neg_input_ids` / `neg_attention_mask`: another
    record of the item's cluster, put through the same transforms and tokenizer as a positive (it IS `base[neg]`, left / right swap on a flip
    included). The id of a record is its dataset index, which is what `_CaptionDataset` emits as `image_id` and cluster.py writes as keys.

    The cluster count follows the reference's linear schedule: at iteration `iter_num` (set by `update_iter`, which utils.common.cycle calls at
    the start of every pass) pred = max(options) * (iter_num - start) / (total - start), and the option closest to pred is used (ties to
    the smaller); the map is reloaded lazily when the option changes. Draws come from a generator seeded by (seed, index, iter_num):
    reproducible per index, a new negative each pass.

    Deviation: a cluster with a single member makes the reference draw forever (data/dataloader.py:705-707); here the negative then comes from
    the whole dataset (never the item itself)."""

    def __init__(self, base, cluster_path: str, split: str = "train", total_iters: int = 500000, negative_sampling_start_iter: int = 0, seed: int = 0):
        if getattr(base, "mode", None) == "sbert":
            raise ValueError("ClusteredDataset needs tokenised captions (MODEL.TEXTUAL.NAME train_sbert), not frozen caption encodings")
        if len(base) < 2:
            raise ValueError("ClusteredDataset needs at least two records")
        self.base, self.cluster_path, self.split, self.seed = base, cluster_path, split, int(seed)
        self.total_iters, self.start_iter = int(total_iters), int(negative_sampling_start_iter)
        self.cluster_options = get_cluster_options(cluster_path, split)
        if not self.cluster_options:
            raise FileNotFoundError(f"no img_id_cluster_map_{split}_<k>.pkl in {cluster_path!r}; write the cluster maps with cluster.py first")
        self.iter_num = self.start_iter
        self.num_clusters = None           # the option whose map is loaded
        self._cluster_of = self._members = None
        self.update_iter(self.iter_num)

    def scheduled_option(self, iter_num: int) -> int:
        """The reference's schedule (data/dataloader.py:update_iter): the option closest to max(options) * progress, ties to the smaller."""
        span = max(self.total_iters - self.start_iter, 1)
        pred = max(self.cluster_options) * (iter_num - self.start_iter) / span
        return min(self.cluster_options, key=lambda k: (abs(k - pred), k))

    def update_iter(self, iter_num: int):
        # Called on the parent process's dataset object. DataLoader workers see it because they are forked anew at every pass (the loaders are
        # built without persistent_workers; with it the workers would keep the iter_num of their first pass), and each of them loads the map
        # of a changed option on its first item.
        self.iter_num = int(iter_num)
        self._wanted = self.scheduled_option(self.iter_num)

    def _load(self):
        import pickle
        path = cluster_map_path(self.cluster_path, self.split, self._wanted)
        with open(path, "rb") as fh:
            cmap = pickle.load(fh)
        outside = [int(i) for i in cmap if not 0 <= int(i) < len(self.base)]
        if outside:
            raise ValueError(f"{path} holds {len(outside)} image ids outside the dataset's 0 .. {len(self.base) - 1} (first: {outside[0]}): "
                             "it was written for another dataset")
        members = {}
        for img_id, c in cmap.items():
            members.setdefault(int(c), []).append(int(img_id))
        for m in members.values():
            m.sort()
        self._cluster_of, self._members, self.num_clusters, self._path = {int(i): int(c) for i, c in cmap.items()}, members, self._wanted, path

    def negative_index(self, idx: int) -> int:
        if self.num_clusters != self._wanted:          # lazily: DataLoader workers load their own copy after the option changed
            self._load()
        if idx not in self._cluster_of:
            raise KeyError(f"image id {idx} is not in {self._path}")
        g = torch.Generator().manual_seed((self.seed * 1000003 + idx) * 1000003 + self.iter_num)
        peers = self._members[self._cluster_of[idx]]
        if len(peers) > 1:                              # uniform over the cluster's other members
            j = int(torch.randint(len(peers) - 1, (), generator=g))
            pos = peers.index(idx) if len(peers) < 64 else _bisect(peers, idx)
            return peers[j if j < pos else j + 1]
        j = int(torch.randint(len(self.base) - 1, (), generator=g))
        return j if j < idx else j + 1

    def __len__(self):
        return len(self.base)

    def __getitem__(self, idx):
        idx = int(idx)
        item = self.base[idx]
        neg = self.base[self.negative_index(idx)]
        for k in ("image", "image_u8", "image_plan", "image_post", "caption_tokens"):          # (a GPU-augmenting base: the negative's canvas and rows)
            if k in neg:
                item["neg_" + k] = neg[k]
        return item

    def collate_fn(self, items):
        batch = self.base.collate_fn(items)
        negs = [{"image_id": i["image_id"], **{k[4:]: v for k, v in i.items() if k.startswith("neg_")}} for i in items]
        nb = self.base.collate_fn(negs)               # the negatives' captions are padded to their own longest row (data/dataloader.py:778-790)
        for k in ("image", "image_u8", "image_hw", "image_plan", "image_post", "input_ids", "attention_mask"):
            if k in nb:
                batch["neg_" + k] = nb[k]
        return batch


def _bisect(sorted_list, x):
    import bisect
    return bisect.bisect_left(sorted_list, x)


# ------------------------------------------------------------------------------------------------ downstream classification
IMAGE_EXTENSIONS = (".jpg", ".jpeg", ".png", ".ppm", ".bmp", ".pgm", ".tif", ".tiff", ".webp")     # torchvision datasets.folder


def _label_collate(items):
    """reference data/dataloader.py ImageNetDataset.collate_fn: {"image": f32 [B][3][H][W], "label": int64 [B]}"""
    return {"image": torch.stack([i["image"] for i in items], 0), "label": torch.stack([i["label"] for i in items], 0)}


class ImageFolderDataset(Dataset):
    """root/{train,val}/<class>/<image>: classes sorted by directory name into indices, images sorted inside a class (torchvision ImageFolder
    order, behind the reference's ImageNetDataset / INaturalist2018Dataset). `percentage` < 100 keeps the first K % of every class on the
    train split only (reference data/dataloader.py:986-995). Images go through `load_image` with the reference's transform names; random
    transforms draw from a generator seeded by (seed, index)."""

    def __init__(self, data_root: str, split: str = "train", image_transform=DEFAULT_IMAGE_TRANSFORM, image_size: int = 224,
                 percentage: float = 100.0, seed: int = 0):
        if percentage <= 0:
            raise ValueError("Cannot load dataset with 0 percent original size.")
        self.root = os.path.join(data_root, split)
        if not os.path.isdir(self.root):
            raise FileNotFoundError(f"image folder split not found: {self.root} (expected <root>/{split}/<class>/<image>)")
        self.classes = sorted(d.name for d in os.scandir(self.root) if d.is_dir())
        if not self.classes:
            raise FileNotFoundError(f"no class directories under {self.root}")
        self.class_to_idx = {c: i for i, c in enumerate(self.classes)}
        self.samples = []
        for c in self.classes:
            files = sorted(f for f in os.listdir(os.path.join(self.root, c)) if f.lower().endswith(IMAGE_EXTENSIONS))
            if split == "train" and percentage < 100:
                files = files[:int(len(files) * (percentage / 100))]
            self.samples += [(os.path.join(self.root, c, f), self.class_to_idx[c]) for f in files]
        self.targets = [t for _, t in self.samples]
        self.image_transform, self.image_size, self.seed = tuple(image_transform), image_size, seed

    @property
    def num_classes(self):
        return len(self.classes)

    def __len__(self):
        return len(self.samples)

    def __getitem__(self, idx):
        path, label = self.samples[idx]
        g = torch.Generator().manual_seed(self.seed * 1000003 + idx)
        return {"image": load_image(path, self.image_transform, self.image_size, g), "label": torch.tensor(label, dtype=torch.long)}

    collate_fn = staticmethod(_label_collate)


class RandomLabelledDataset(Dataset):
    """Synthetic labelled images (DATA.ROOT "random"): image = N(0, 1) noise + `strength` x a fixed random pattern of its class, so a linear
    probe on a random backbone can learn it. Every index is reproducible (seeded by split, seed and index); the class patterns depend on
    `seed` only, so train and val share them."""

    def __init__(self, num_classes: int = 10, image_size: int = 224, length: int = 50000, split: str = "train", seed: int = 0, strength: float = 1.0):
        self.num_classes, self.image_size, self.length, self.strength = num_classes, image_size, length, strength
        self.seed = seed * 2 + (0 if split == "train" else 1)
        g = torch.Generator().manual_seed(seed * 7919 + 17)
        self.patterns = torch.randn(num_classes, 3, image_size, image_size, generator=g)
        self.classes = [f"class_{i}" for i in range(num_classes)]

    def __len__(self):
        return self.length

    def label(self, idx):
        return (idx * 7 + self.seed) % self.num_classes

    def __getitem__(self, idx):
        g = torch.Generator().manual_seed(self.seed * 1000003 + idx)
        y = self.label(idx)
        image = torch.randn(3, self.image_size, self.image_size, generator=g) + self.strength * self.patterns[y]
        return {"image": image, "label": torch.tensor(y, dtype=torch.long)}

    collate_fn = staticmethod(_label_collate)


class VOC07ClassificationDataset(Dataset):
    """PASCAL VOC 2007 image-label pairs (reference data/dataloader.py:800-882): classes are the sorted `ImageSets/Main/<class>_<split>.txt`
    files; each line "<image> <label>" maps VOC 1 -> 1 (present), -1 -> 0 (absent), 0 -> -1 (difficult); an image missing from a class file
    keeps -1 there. Instances come in order of first appearance while reading the sorted class files; images are JPEGImages/<name>.jpg through
    `load_image` with the reference's transform names (random ones seeded by (seed, index), like ImageFolderDataset).
    Items: {"image": f32 [3][H][W], "label": int64 [K]}."""

    def __init__(self, data_root: str, split: str = "trainval", image_transform=DEFAULT_IMAGE_TRANSFORM, image_size: int = 224, seed: int = 0):
        import glob
        ann_paths = sorted(glob.glob(os.path.join(data_root, "ImageSets", "Main", f"*_{split}.txt")))
        if not ann_paths:
            raise FileNotFoundError(f"no VOC class files {data_root}/ImageSets/Main/*_{split}.txt")
        self.split = split
        self.class_names = [os.path.basename(p).split("_")[0] for p in ann_paths]
        labels = {}
        for k, path in enumerate(ann_paths):
            with open(path) as f:
                for line in f:
                    if not line.strip():
                        continue
                    name, orig = line.split()
                    orig = int(orig)
                    lab = labels.setdefault(name, [-1] * len(ann_paths))
                    lab[k] = 0 if orig == -1 else -1 if orig == 0 else 1
        self.instances = [(os.path.join(data_root, "JPEGImages", f"{name}.jpg"), lab) for name, lab in labels.items()]
        self.image_transform, self.image_size, self.seed = tuple(image_transform), image_size, seed

    @property
    def num_classes(self):
        return len(self.class_names)

    def __len__(self):
        return len(self.instances)

    def __getitem__(self, idx):
        path, label = self.instances[idx]
        g = torch.Generator().manual_seed(self.seed * 1000003 + idx)
        return {"image": load_image(path, self.image_transform, self.image_size, g), "label": torch.tensor(label, dtype=torch.long)}

    collate_fn = staticmethod(_label_collate)


def read_gender_records(path: str):
    """The reference's COCO gender annotation `<split>.data` (bias_eda.py's GenderDataset source): a pickled list of dicts with `image_id`,
    `file_name` and a one-hot `gender` ([1, 0] man, [0, 1] woman). Returns [(image_id, file name inside <split>2017/, group)] with group 0 =
    men, 1 = women, in file order; a record without exactly one of the two set is refused."""
    import pickle
    with open(path, "rb") as fh:
        records = pickle.load(fh)
    if not isinstance(records, (list, tuple)) or not records:
        raise ValueError(f"{path}: expected a pickled non-empty list of records")
    out = []
    for i, r in enumerate(records):
        try:
            g = [int(v) for v in r["gender"]]
            name, image_id = str(r["file_name"]).split("_")[-1], int(r["image_id"])
        except (KeyError, TypeError, ValueError) as e:
            raise ValueError(f"{path}: record {i} needs image_id, file_name and gender ({e!r})")
        if g not in ([1, 0], [0, 1]):
            raise ValueError(f"{path}: record {i} has gender {g}; expected [1, 0] (man) or [0, 1] (woman)")
        out.append((image_id, name, g[1]))
    return out


class GenderAnnotationDataset(Dataset):
    """COCO images with the reference's gender annotation (reference bias_eda.py): records from <gender_data_path>/<split>.data
    (read_gender_records), images at <data_root>/<split>2017/<file_name.split("_")[-1]>. The groups are `classes` = ["men", "women"].
    Items as ImageFolderDataset's: {"image": f32 [3][H][W], "label": the group}."""
    classes = ["men", "women"]

    def __init__(self, data_root: str, gender_data_path: str, split: str = "train", image_transform=DEFAULT_IMAGE_TRANSFORM,
                 image_size: int = 224, seed: int = 0):
        records = read_gender_records(os.path.join(gender_data_path, f"{split}.data"))
        self.image_ids = [r[0] for r in records]
        self.samples = [(os.path.join(data_root, f"{split}2017", r[1]), r[2]) for r in records]
        self.targets = [t for _, t in self.samples]
        self.image_transform, self.image_size, self.seed = tuple(image_transform), image_size, seed

    @property
    def num_classes(self):
        return len(self.classes)

    def __len__(self):
        return len(self.samples)

    def __getitem__(self, idx):
        path, label = self.samples[idx]
        g = torch.Generator().manual_seed(self.seed * 1000003 + idx)
        return {"image": load_image(path, self.image_transform, self.image_size, g), "label": torch.tensor(label, dtype=torch.long)}

    collate_fn = staticmethod(_label_collate)


# ------------------------------------------------------------------------------------------------ image-text retrieval
def pre_caption(caption: str, max_words: int = 30) -> str:
    """The reference's retrieval caption cleanup (data/dataloader.py:1027-1052): lower-case; delete , . ' ! ? " ( ) * # : ; ~; '-' and '/'
    become spaces; "<person>" becomes "person"; runs of two or more whitespace characters collapse to one space; trailing newlines and
    surrounding spaces go; at most `max_words` space-separated words are kept. Unlike normalize_caption, accents are kept."""
    c = re.sub(r"([,.'!?\"()*#:;~])", "", caption.lower()).replace("-", " ").replace("/", " ").replace("<person>", "person")
    c = re.sub(r"\s{2,}", " ", c).rstrip("\n").strip(" ")
    words = c.split(" ")
    if len(words) > max_words:
        c = " ".join(words[:max_words])
    return c


def _retrieval_collate(items):
    return {"image": torch.stack([i["image"] for i in items], 0), "index": torch.tensor([i["index"] for i in items], dtype=torch.long)}


class RetrievalEvalDataset(Dataset):
    """Images and captions of an image-text retrieval evaluation, in the reference's two layouts:

    - a JSON list of {"image": path relative to data_root, "caption": [str, ...]} (reference re_eval_dataset, data/dataloader.py:1130-1166:
      Flickr30k's flickr30k_test.json, ALBEF's COCO Karpathy files) when `ann_file` is given; captions are numbered in file order;
    - COCO 2017 (reference ReEvalDataset, data/dataloader.py:1055-1127): images data_root/{split}2017/*.jpg, the image id being the integer
      file stem, captions from data_root/annotations/captions_{split}2017.json grouped by image_id in annotation order. An image without
      captions stays a row that misses at every k. Deliberate deviation: rows are in sorted file-name order; the reference's glob order
      is not defined.

    Fields as the reference's: `text` (pre_caption of every caption), `image` (paths, one per row), `img2txt` (row -> caption indices) and
    `txt2img` (caption index -> row); both maps are keyed by row, and `image_ids` holds the reference's id of every row (the COCO id, or the
    row itself for the JSON layout). Items: {"image": f32 CHW through load_image(image_transform, image_size), "index": row}."""

    def __init__(self, data_root: str, ann_file: str = "", split: str = "val", image_transform=DEFAULT_IMAGE_TRANSFORM, image_size: int = 224,
                 max_words: int = 30, seed: int = 0):
        self.data_root, self.max_words = data_root, max_words
        self.text, self.image, self.image_ids = [], [], []
        self.img2txt, self.txt2img = {}, {}
        if ann_file:
            with open(ann_file) as f:
                ann = json.load(f)
            rows = []
            for k, a in enumerate(ann):
                if not isinstance(a.get("caption"), list):
                    raise ValueError(f"{ann_file}: record {k} has a 'caption' that is not a list (the retrieval layout lists every caption "
                                     "of an image)")
                rows.append((k, os.path.join(data_root, a["image"]), a["caption"]))
        else:
            image_dir = os.path.join(data_root, f"{split}2017")
            cap_file = os.path.join(data_root, "annotations", f"captions_{split}2017.json")
            if not os.path.isdir(image_dir) or not os.path.isfile(cap_file):
                raise FileNotFoundError(f"COCO 2017 layout not found: need {image_dir}/*.jpg and {cap_file}")
            with open(cap_file) as f:
                annotations = json.load(f)["annotations"]
            by_id = {}
            for a in annotations:
                by_id.setdefault(int(a["image_id"]), []).append(a["caption"])
            names = sorted(n for n in os.listdir(image_dir) if n.endswith(".jpg"))
            rows = [(int(n[:-4]), os.path.join(image_dir, n), by_id.get(int(n[:-4]), [])) for n in names]
        for row, (img_id, path, captions) in enumerate(rows):
            self.image.append(path)
            self.image_ids.append(img_id)
            self.img2txt[row] = []
            for caption in captions:
                self.img2txt[row].append(len(self.text))
                self.txt2img[len(self.text)] = row
                self.text.append(pre_caption(caption, max_words))
        self.image_transform, self.image_size, self.seed = tuple(image_transform), image_size, seed

    def __len__(self):
        return len(self.image)

    def __getitem__(self, idx):
        g = torch.Generator().manual_seed(self.seed * 1000003 + idx)
        return {"image": load_image(self.image[idx], self.image_transform, self.image_size, g), "index": idx}

    collate_fn = staticmethod(_retrieval_collate)
