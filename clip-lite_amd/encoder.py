"""Image and text encoders with the reference's call surface (reference encoder.py:13-65 ImageEncoder, :115-205 TextEncoder),
running on the HIP executors in resnet.py / vit.py / bert.py. Attribute names (`img_encoder`, `strans`, `fc1`/`fc2`) and state_dict keys
match the reference so checkpoints interchange."""
from typing import Any, Dict

import torch
import torch.nn as nn

from . import hip
from .bert import BertModel, LinearParams, bert_backward, bert_forward
from .cliptext import SPECS as CLIP_TEXT_SPECS, ClipTextModel, cliptext_backward, cliptext_forward
from .resnet import ResNet, resnet_backward, resnet_forward
from .vit import VisionTransformer, vit_backward, vit_forward


def _runtime_of(module):
    rt = getattr(module, "_clite_rt", None)
    if rt is None:
        raise RuntimeError("clip_lite_amd: module is not attached to a device runtime; build it through VLInfoModel (or "
                           "clip_lite_amd.model.attach_runtime) and move it to the GPU — there is no CPU path")
    return rt


class _ResNetFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, image, anchor, enc, rt, training):
        feat, saved = resnet_forward(rt, enc.img_encoder, image.to(torch.float32).contiguous(), training)
        if training:
            rt.bump_counters("image_encoder", 1)
        ctx.enc, ctx.rt, ctx.saved = enc, rt, saved
        return feat

    @staticmethod
    def backward(ctx, dfeat):
        resnet_backward(ctx.rt, ctx.enc.img_encoder, ctx.saved, dfeat.contiguous())
        ctx.rt.arena.note_stream_work()
        return None, None, None, None, None


class _ViTFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, image, anchor, enc, rt, training):
        feat, saved = vit_forward(rt, enc.img_encoder, image.to(torch.float32).contiguous(), training)
        ctx.enc, ctx.rt, ctx.saved = enc, rt, saved
        return feat

    @staticmethod
    def backward(ctx, dfeat):
        vit_backward(ctx.rt, ctx.enc.img_encoder, ctx.saved, dfeat.contiguous())
        ctx.rt.arena.note_stream_work()
        return None, None, None, None, None


class ImageEncoder(nn.Module):
    r"""torchvision-topology ResNet with ``fc = Identity`` (reference encoder.py:28-65), or — a name starting with ``vit_`` — torchvision's
    ViT-B/32 / ViT-B/16 with ``heads = Identity`` (vit.py; built for ``image_size`` pixels, DATA.IMAGE_CROP_SIZE). ``pretrained`` weights cannot
    be downloaded here (no network) and raise; ``frozen`` keeps all weights fixed and the encoder in eval mode. ``patch_dropout`` (a ViT option,
    MODEL.VISUAL.PATCH_DROPOUT) is the share of patches each image drops in training (FLIP); evaluation and a frozen encoder see every token."""

    def __init__(self, img_enc_net: str = "resnet50", pretrained: bool = False, frozen: bool = False, image_size=224, patch_dropout: float = 0.0,
                 **vit_kwargs):
        """vit_kwargs: VisionTransformer's num_layers / hidden / heads / mlp_dim (small models for tests); a ResNet takes none."""
        super().__init__()
        if pretrained:
            raise RuntimeError("pretrained torchvision weights are not available offline; load a state_dict instead")
        self.is_vit = img_enc_net.startswith("vit_")
        if patch_dropout != 0.0:
            if not self.is_vit:
                raise ValueError(f"clip_lite_amd: patch_dropout (MODEL.VISUAL.PATCH_DROPOUT) is a ViT option: {img_enc_net!r} has no patch tokens "
                                 f"to drop; got {patch_dropout}")
            vit_kwargs["patch_dropout"] = patch_dropout
        if vit_kwargs and not self.is_vit:
            raise TypeError(f"ImageEncoder({img_enc_net!r}): unexpected arguments {sorted(vit_kwargs)}")
        self.img_encoder = VisionTransformer(img_enc_net, image_size=image_size, **vit_kwargs) if self.is_vit else ResNet(img_enc_net)
        self.out_dim = self.img_encoder.out_dim
        self.frozen = frozen
        if frozen:
            for param in self.img_encoder.parameters():
                param.requires_grad = False
            self.img_encoder.eval()

    def forward(self, image: torch.Tensor) -> torch.Tensor:
        rt = _runtime_of(self)
        training = self.img_encoder.training and not self.frozen
        grad = torch.is_grad_enabled() and any(p.requires_grad for p in self.img_encoder.parameters())
        if self.is_vit:          # (no BatchNorm, no counters to bump: training and eval differ by the patch dropout alone, where it is on)
            if grad:
                x = _ViTFn.apply(image, rt.anchor, self, rt, training)
            else:
                x, _ = vit_forward(rt, self.img_encoder, image.to(torch.float32).contiguous(), training)
        elif grad:
            x = _ResNetFn.apply(image, rt.anchor, self, rt, training)
        else:
            x, _ = resnet_forward(rt, self.img_encoder, image.to(torch.float32).contiguous(), training)
            if training:
                rt.bump_counters("image_encoder", 1)
        return x.view(x.size(0), x.size(1))

    def detectron2_backbone_state_dict(self) -> Dict[str, Any]:
        """Same renaming as reference encoder.py:67-112 (torchvision names -> Detectron2 names)."""
        if self.is_vit:
            raise NotImplementedError("detectron2_backbone_state_dict: the Detectron2 export renames a ResNet's stages (res2 .. res5); a ViT image "
                                      "encoder has none")
        mapping = {"layer1": "res2", "layer2": "res3", "layer3": "res4", "layer4": "res5", "bn1": "conv1.norm", "bn2": "conv2.norm",
                   "bn3": "conv3.norm", "downsample.0": "shortcut", "downsample.1": "shortcut.norm"}
        out = {}
        for name, param in self.img_encoder.state_dict().items():
            for old, new in mapping.items():
                name = name.replace(old, new)
            if not name.startswith("res"):
                name = f"stem.{name}"
            out[name] = param
        return {"model": out, "__author__": "VLInfo", "matching_heuristics": True}


class _BertFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, anchor, enc, rt, input_ids, attention_mask, step):
        out, saved = bert_forward(rt, enc.strans, input_ids, attention_mask, step)
        ctx.enc, ctx.rt, ctx.saved = enc, rt, saved
        return out

    @staticmethod
    def backward(ctx, dout):
        bert_backward(ctx.rt, ctx.enc.strans, ctx.saved, dout.contiguous())
        rt = ctx.rt
        ev = rt.arena.note_stream_work()     # gradients were written on this node's stream: consumers of the arena join it
        # ... and so does everything the caller enqueues after backward() on the stream forward was called on (reading .grad,
        # a hand-written update): this node runs after the image encoder's (it was created first), so the join does not
        # serialise the two backward passes.
        main = getattr(rt, "main_stream", None)
        if ev is not None and main is not None and main != torch.cuda.current_stream(rt.device):
            main.wait_event(ev)
        return None, None, None, None, None, None


class _ClipTextFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, anchor, enc, rt, input_ids, attention_mask):
        out, saved = cliptext_forward(rt, enc.strans, input_ids, attention_mask)
        ctx.enc, ctx.rt, ctx.saved = enc, rt, saved
        return out

    @staticmethod
    def backward(ctx, dout):
        cliptext_backward(ctx.rt, ctx.enc.strans, ctx.saved, dout.contiguous())
        rt = ctx.rt
        ev = rt.arena.note_stream_work()     # as _BertFn.backward: consumers of the arena, and the caller's stream, join this node's stream
        main = getattr(rt, "main_stream", None)
        if ev is not None and main is not None and main != torch.cuda.current_stream(rt.device):
            main.wait_event(ev)
        return None, None, None, None, None


class _TransformFn(torch.autograd.Function):
    """optional fc1 -> ReLU -> fc2 head (reference encoder.py:182-185,200-203; TRANSFORM is false in every shipped YAML)"""

    @staticmethod
    def forward(ctx, x, enc, rt):
        B, D = x.shape
        E = enc.txt_enc_dim
        x = x.to(rt.tdtype).contiguous()
        h = torch.empty(B, E, device=rt.device, dtype=rt.tdtype)
        hip.gemm_nt(rt.dt, x, rt.arena.w(enc.fc1.weight), B, E, D, hip.epilogue(h, E, bias=enc.fc1.bias, act=hip.ACT_RELU))
        y = torch.empty(B, E, device=rt.device, dtype=rt.tdtype)
        hip.gemm_nt(rt.dt, h, rt.arena.w(enc.fc2.weight), B, E, E, hip.epilogue(y, E, bias=enc.fc2.bias))
        ctx.enc, ctx.rt, ctx.saved = enc, rt, (x, h)
        return y

    @staticmethod
    def backward(ctx, dy):
        from .bert import _linear_grads
        enc, rt = ctx.enc, ctx.rt
        x, h = ctx.saved
        B, D = x.shape
        E = enc.txt_enc_dim
        dy = dy.contiguous()
        _linear_grads(rt, enc.fc2, dy, h, B)
        dh = torch.empty(B, E, device=rt.device, dtype=rt.tdtype)
        hip.gemm_nn(rt.dt, dy, rt.arena.w(enc.fc2.weight), B, E, E, hip.epilogue(dh, E, dact_aux=h, dact=hip.DACT_RELU))
        _linear_grads(rt, enc.fc1, dh, x, B)
        dx = torch.empty(B, D, device=rt.device, dtype=rt.tdtype)
        hip.gemm_nn(rt.dt, dh, rt.arena.w(enc.fc1.weight), B, D, E, hip.epilogue(dx, D))
        return dx, None, None


class TextEncoder(nn.Module):
    r"""Reference encoder.py:122-205. Modes on the HIP path: ``"sbert"`` (frozen sentence embeddings passed through, 0 parameters)
    and ``"train_sbert"`` with ``pretrained=False``: a ``model_name`` containing "bert" builds the random-init BertModel and returns
    ``pooler_output``; any other name (the reference's "sentence-transformers/paraphrase-mpnet-base-v2") builds the random-init MPNetModel
    (mpnet.py) and returns the masked mean over the token states (reference encoder.py:171-175, 197-198). One deviation on that branch:
    the reference ignores ``num_hidden_layers`` there and always builds MPNetConfig()'s 12 layers; here it is honoured (default 12).
    A ``model_name`` beginning with "clip_text" (tested first; not in the reference) builds the CLIP text transformer (cliptext.py; "clip_text_b" is
    the one named size: 77 tokens, 512 wide, 8 heads, 512 output features) and returns the projected end-of-text state; ``txt_enc_dim`` must then
    be the tower's output width, and ``context_length`` (MODEL.TEXTUAL.CONTEXT_LENGTH) sizes its positional embedding.
    GloVe and pretrained weights need assets or a download that are unavailable and raise."""

    def __init__(self, word_dict=None, mode="train_sbert", transform_embedding=False, txt_enc_dim=512, glove_path=None, train_enc=False,
                 load_glove=True, model_name="bert-base-uncased", pretrained=False, num_hidden_layers=12, context_length=None):
        super().__init__()
        self.transform_embedding = transform_embedding
        self.txt_enc_dim = txt_enc_dim
        self.mode = mode
        self.model_name = model_name
        self.num_hidden_layers = num_hidden_layers
        if mode == "sbert":
            in_dim = 768
        elif mode == "train_sbert":
            if pretrained:
                raise RuntimeError(f"pretrained weights of {model_name!r} are a download, which is not available; build the randomly initialised "
                                   "encoder (MODEL.TEXTUAL.PRETRAINED false) and load a state_dict instead")
            in_dim = 768
            if model_name.startswith("clip_text"):
                if model_name not in CLIP_TEXT_SPECS:
                    raise ValueError(f"unsupported CLIP text tower {model_name!r}; supported: {sorted(CLIP_TEXT_SPECS)}")
                ctxlen, width, heads, _, embed = CLIP_TEXT_SPECS[model_name]
                if txt_enc_dim != embed:
                    raise ValueError(f"MODEL.TEXTUAL.FEATURE_SIZE is {txt_enc_dim}, but {model_name} produces {embed} features; set "
                                     f"MODEL.TEXTUAL.FEATURE_SIZE to {embed}")
                print("Using clip text model with layers: " + str(self.num_hidden_layers))
                self.strans = ClipTextModel(context_length=ctxlen if context_length is None else context_length, width=width, heads=heads,
                                            num_hidden_layers=self.num_hidden_layers, embed_dim=embed)
                in_dim = self.strans.out_dim
            elif "bert" in model_name:
                print("Using bert model with layers: " + str(self.num_hidden_layers))
                self.strans = BertModel(num_hidden_layers=self.num_hidden_layers)
            else:
                from .mpnet import MPNetModel
                print("Using mpnet model with layers: " + str(self.num_hidden_layers))
                self.strans = MPNetModel(num_hidden_layers=self.num_hidden_layers)
        else:
            raise NotImplementedError(f"text encoder mode {mode!r} needs assets that are not available (GloVe vectors / HF hub)")
        if transform_embedding:
            self.fc1 = LinearParams(in_dim, self.txt_enc_dim)
            self.fc2 = LinearParams(self.txt_enc_dim, self.txt_enc_dim)

    def forward(self, x):
        rt = _runtime_of(self)
        if self.mode == "train_sbert" and self.strans.kind == "clip":          # (no dropout: no seed is drawn)
            grad = torch.is_grad_enabled() and any(p.requires_grad for p in self.strans.parameters())
            if grad:
                x = _ClipTextFn.apply(rt.anchor, self, rt, x["input_ids"], x["attention_mask"])
            else:
                x, _ = cliptext_forward(rt, self.strans, x["input_ids"], x["attention_mask"])
        elif self.mode == "train_sbert":
            step = rt.next_step(self.training)
            grad = torch.is_grad_enabled() and any(p.requires_grad for p in self.strans.parameters())
            if grad:
                x = _BertFn.apply(rt.anchor, self, rt, x["input_ids"], x["attention_mask"], step)
            else:
                x, _ = bert_forward(rt, self.strans, x["input_ids"], x["attention_mask"], step)
        if self.transform_embedding:
            x = _TransformFn.apply(x, self, rt)
        return x

    def train_enc(self):
        for param in self.strans.parameters():
            param.requires_grad = True
        if hasattr(self.strans, "freeze_unused"):
            self.strans.freeze_unused()          # MPNet's pooler never takes part in the step (mpnet.py)

    def dont_train_enc(self):
        for param in self.strans.parameters():
            param.requires_grad = False
