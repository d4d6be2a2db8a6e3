"""Downstream classification on the HIP kernels: the linear probe / end-to-end fine-tune of reference linear_clf.py and the zero-shot
evaluation of reference zero_shot.py.

`ImageClassifier` is the torchvision ResNet with a real `fc` (reference linear_clf.py:150-186): parameter names and state_dict keys are
torchvision's (`conv1.weight` ... `layer4.*`, `fc.weight`, `fc.bias`), so the reference's classifier checkpoints interchange. Moving it to a
GPU builds its own parameter arena (runtime.DeviceRuntime): bf16 kernels when `is_amp`, exact f32 otherwise, as VLInfoModel does.
The logits are f32 out of one `clite_gemm_nt` with a bias epilogue; the loss, the top-k counters and the logit gradient are
`clite_xent_fwd` / `clite_xent_bwd` (csrc/cls_ops.hip). The GEMMs want N % 8 == 0 and K % 8 == 0 (include/clite.h), so the class count is
padded to Cp = ceil8(C) and the batch to a multiple of 8 for the weight gradient; state_dict shapes stay [C][D] / [C].
"""
from typing import Dict

import torch
from torch import nn

from . import hip
from .bert import LinearParams
from .resnet import ResNet, resnet_backward, resnet_forward
from .runtime import DeviceRuntime


def _ceil8(n):
    return (n + 7) // 8 * 8


class _ClassifierFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, image, anchor, model, rt, train_bn, backbone_grad):
        logits, feat, saved, wpad = model._forward_impl(rt, image, train_bn, keep=backbone_grad)
        ctx.model, ctx.rt, ctx.feat, ctx.saved, ctx.wpad = model, rt, feat, saved, wpad
        ctx.B = image.shape[0]
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        model, rt = ctx.model, ctx.rt
        B, Bp, Cp = ctx.B, _ceil8(ctx.B), _ceil8(model.num_classes)
        C, D = model.num_classes, model.out_dim
        # autograd's gradient w.r.t. the logits (whatever produced it: cross_entropy, several losses summed, a hook) as the GEMMs read it:
        # [Bp][Cp] in the compute dtype, zero in the padding
        dpad = torch.zeros(Bp, Cp, device=rt.device, dtype=rt.tdtype)
        dpad[:B, :C].copy_(dlogits)
        fc = model.fc
        A = rt.arena
        if fc.weight.requires_grad:
            if C % 8 == 0:
                hip.gemm_tn(rt.dt, dpad, ctx.feat, C, D, Bp, hip.epilogue(A.g(fc.weight), D, atomic=True, out_f32=True), lda=Cp, ldb=D)
            else:
                # clite_gemm_tn wants M % 8 == 0: the Cp-row product is stored (not accumulated) into the model's workspace, and its first C rows
                # are added into the gradient
                ws = model._dw_workspace(rt)
                hip.gemm_tn(rt.dt, dpad, ctx.feat, Cp, D, Bp, hip.epilogue(ws, D, out_f32=True), lda=Cp, ldb=D)
                g = A.g(fc.weight)
                hip.add(hip.F32, g, ws[:C], g)
        if fc.bias.requires_grad:
            # the arena pads every tensor to 64 elements (>= Cp - C); the padding columns of dpad are zero
            o, _ = A.index[fc.bias._clite[1]]
            hip.colsum(rt.dt, dpad, A.flat_g[o:o + Cp], Bp, Cp)
        if ctx.saved is not None:
            dfeat = torch.empty(B, D, device=rt.device, dtype=rt.tdtype)
            hip.gemm_nn(rt.dt, dpad, ctx.wpad, B, D, Cp, hip.epilogue(dfeat, D), lda=Cp, ldb=D)
            resnet_backward(rt, model, ctx.saved, dfeat)
        A.note_stream_work()
        ctx.saved = ctx.feat = ctx.wpad = None
        return None, None, None, None, None, None


class ImageClassifier(ResNet):
    r"""ResNet backbone + ``fc`` (reference linear_clf.py:150-186). ``fc`` starts at N(0, 0.01) / 0 (linear_clf.py:159-160). ``frozen``: the
    backbone is fixed — ``requires_grad=False`` and BatchNorm on running statistics whatever ``train()`` says (linear_clf.py:168-178).
    Only ``fc`` learns (a linear probe). Otherwise the whole network is fine-tuned."""

    def __init__(self, visual_name: str = "resnet50", num_classes: int = 1000, frozen: bool = False, is_amp: bool = True):
        if str(visual_name).startswith("vit_"):
            raise ValueError(f"linear_clf: the classifier (linear probe / fine-tune) is built on a ResNet backbone; {visual_name!r} is a ViT image "
                             "encoder: evaluate its features with logreg_clf.py or knn_clf.py instead")
        super().__init__(visual_name)
        if num_classes < 2:
            raise ValueError(f"num_classes must be >= 2, got {num_classes}")
        self.visual_name, self.num_classes, self.frozen, self.is_amp = visual_name, int(num_classes), bool(frozen), bool(is_amp)
        self.fc = LinearParams(self.out_dim, self.num_classes, std=0.01)        # weight N(0, 0.01), bias 0
        self._rt = None
        self._pad_bufs = {}
        if self.frozen:
            for name, param in self.named_parameters():
                if not name.startswith("fc."):
                    param.requires_grad = False
            self.eval()

    @classmethod
    def from_pretraining(cls, state_dict_or_model, visual_name: str = "resnet50", num_classes: int = 1000, frozen: bool = False,
                         is_amp: bool = True, prefix: str = "image_encoder.img_encoder."):
        """The backbone weights and BatchNorm buffers of a pretraining checkpoint (reference linear_clf.py:143-156): a VLInfoModel, its
        state_dict, or a CheckpointManager file's dict (weights under "model"). Built and loaded on the CPU; call .to(device) after."""
        sd = state_dict_or_model
        if isinstance(sd, nn.Module):
            sd = sd.state_dict()
        if "model" in sd and isinstance(sd["model"], dict):
            sd = sd["model"]
        model = cls(visual_name, num_classes, frozen, is_amp)
        want = [k for k in model.state_dict() if not k.startswith("fc.")]
        picked = {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}
        missing = [k for k in want if k not in picked]
        unexpected = [k for k in picked if k not in want]
        if missing or unexpected:
            raise KeyError(f"pretraining checkpoint does not hold a {visual_name} backbone under {prefix!r}: missing {missing[:4]}, "
                           f"unexpected {unexpected[:4]}")
        model.load_state_dict(picked, strict=False)
        return model

    # -- device placement builds the arena (as VLInfoModel._apply) ---------------------------------------------------------------
    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        p = next(self.parameters(), None)
        dev = p.device if p is not None else None
        if dev is not None and (dev.type == "cuda" or hip._allow_host_tensors):
            if self._rt is None or self._rt.device != dev:
                self._rt = self._attach(dev)
        return out

    def _attach(self, dev):
        rt = DeviceRuntime(self, dev, self.is_amp, (), seed=torch.initial_seed() % (2 ** 31))
        rt.anchor = torch.zeros(1, device=rt.device, requires_grad=True)
        if self.is_amp and not self.frozen:
            # DeviceRuntime registers the transposed dgrad copies for the modules under image_encoder / text_encoder; here the backbone is the
            # model itself (torchvision names)
            convs = [m.weight for m in self.modules() if hasattr(m, "in_channels") and hasattr(m.weight, "_clite")]
            rt.arena.register_transposed(convs)
        return rt

    @property
    def runtime(self):
        if self._rt is None:
            raise RuntimeError("clip_lite_amd: move the classifier to a GPU first (model.to(device)); there is no CPU path")
        return self._rt

    def state_dict(self, *args, **kw):
        if self._rt is not None:
            self._rt.arena.flush_pending()
        return super().state_dict(*args, **kw)

    def load_state_dict(self, state_dict, strict=True, **kw):
        if self._rt is not None:
            self._rt.arena.flush_pending()
        out = super().load_state_dict(state_dict, strict=strict, **kw)
        if self._rt is not None:
            self._rt.arena.refresh_lowp()
        return out

    def train(self, mode: bool = True):
        super().train(mode)
        if self.frozen:              # the backbone's BatchNorms stay on running statistics (reference linear_clf.py:171-174)
            for m in self.children():
                m.train(False)
        return self

    # -- forward ---------------------------------------------------------------------------------------------------------------
    def _pad_buf(self, rt, key, dtype):
        """A [Cp][D] buffer of the model, allocated (zeroed) once per runtime: C % 8 != 0 only."""
        buf = self._pad_bufs.get(key)
        if buf is None or buf.device != rt.device or buf.dtype != dtype:
            buf = self._pad_bufs[key] = torch.zeros(_ceil8(self.num_classes), self.out_dim, device=rt.device, dtype=dtype)
        return buf

    def _dw_workspace(self, rt):
        return self._pad_buf(rt, "dw", torch.float32)

    def _padded_fc(self, rt):
        """(weight [Cp][D] in the compute dtype, bias [Cp] f32) as the logit GEMM reads them: the arena's own storage when C % 8 == 0, else the
        current weight copied into the model's zero-padded buffer (rows >= C stay zero; the bias reads its arena padding, which stays zero).
        Two forwards before one backward write the same values there, since the weights only change in the optimizer step."""
        C, D, Cp = self.num_classes, self.out_dim, _ceil8(self.num_classes)
        w = rt.arena.w(self.fc.weight)
        if Cp != C:
            wp = self._pad_buf(rt, "w", rt.tdtype)
            wp[:C].copy_(w)
            w = wp
        o, _ = rt.arena.index[self.fc.bias._clite[1]]
        return w, rt.arena.flat_p[o:o + Cp]

    def _forward_impl(self, rt, image, train_bn, keep):
        B = image.shape[0]
        C, D, Cp, Bp = self.num_classes, self.out_dim, _ceil8(self.num_classes), _ceil8(image.shape[0])
        feat, saved = resnet_forward(rt, self, image.to(device=rt.device, dtype=torch.float32).contiguous(), train_bn)
        if train_bn:
            for owner in rt.counters:            # num_batches_tracked of every BatchNorm (one counter tensor per top-level child)
                rt.bump_counters(owner, 1)
        if Bp != B:                              # zero rows up to Bp: the weight gradient's K dimension
            fp = torch.zeros(Bp, D, device=rt.device, dtype=rt.tdtype)
            fp[:B].copy_(feat)
            feat = fp
        w, bias = self._padded_fc(rt)
        out = torch.empty(B, Cp, device=rt.device, dtype=torch.float32)
        hip.gemm_nt(rt.dt, feat, w, B, Cp, D, hip.epilogue(out, Cp, bias=bias, out_f32=True))
        return out[:, :C], feat, (saved if keep else None), w

    def forward(self, images: torch.Tensor) -> torch.Tensor:
        """images f32 [B][3][H][W] -> logits f32 [B][C] (a view of a [B][Cp] buffer)."""
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("ImageClassifier: hipGraph capture of the classification step is not supported (it allocates per-step "
                               "tensors); run it eagerly")
        rt = self.runtime
        train_bn = self.training and not self.frozen
        grad = torch.is_grad_enabled()
        backbone_grad = grad and any(p.requires_grad for n, p in self.named_parameters() if not n.startswith("fc."))
        if backbone_grad and not train_bn:
            raise RuntimeError("ImageClassifier: a backbone gradient needs train mode (batch statistics); call model.train(), or freeze the "
                               "backbone, or evaluate under torch.no_grad()")
        if grad and (backbone_grad or self.fc.weight.requires_grad or self.fc.bias.requires_grad):
            return _ClassifierFn.apply(images, rt.anchor, self, rt, train_bn, backbone_grad)
        return self._forward_impl(rt, images, train_bn, keep=False)[0]


# ------------------------------------------------------------------------------------------------ loss and metrics
def _row_major(logits):
    """(tensor, ld) that clite_xent_* can read: f32, unit column stride, ld % 4 == 0, 16-byte aligned base; a copy only when needed."""
    B, C = logits.shape
    if logits.dtype == torch.float32 and logits.stride(1) == 1 and logits.stride(0) % 4 == 0 and logits.stride(0) >= C and logits.data_ptr() % 16 == 0:
        return logits, logits.stride(0)
    ld = (C + 3) // 4 * 4
    z = torch.zeros(B, ld, device=logits.device, dtype=torch.float32)
    z[:, :C].copy_(logits)
    return z, ld


def _labels(labels, device):
    return labels.to(device=device, dtype=torch.int64).contiguous()


class _CrossEntropyFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels):
        B, C = logits.shape
        z, ld = _row_major(logits)
        y = _labels(labels, logits.device)
        lse = torch.empty(B, device=logits.device, dtype=torch.float32)
        acc = torch.zeros(4, device=logits.device, dtype=torch.float32)
        hip.xent_fwd(z, ld, B, C, y, 1, lse, acc)
        ctx.z, ctx.ld, ctx.y, ctx.lse, ctx.acc, ctx.B, ctx.C = z, ld, y, lse, acc, B, C
        return acc[0] / acc[3]

    @staticmethod
    def backward(ctx, gout):
        B, C = ctx.B, ctx.C
        gout = gout.to(torch.float32).reshape(1).contiguous()
        Cp = _ceil8(C)
        d = torch.empty(B, Cp, device=gout.device, dtype=torch.float32)
        hip.xent_bwd(hip.F32, ctx.z, ctx.ld, B, B, C, ctx.lse, ctx.y, ctx.acc, gout, d, Cp)
        return d[:, :C], None


def cross_entropy(logits: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """nn.CrossEntropyLoss()(logits, labels) (reference linear_clf.py:188): the mean over the rows whose label is not -100, as a 0-d device
    tensor, differentiable w.r.t. the logits. logits f32 [B][C] on the device; labels int64 [B].
    Unlike torch, a label outside [0, C) other than -100 does not raise (that would need a host synchronisation per call): the kernel
    skips such rows like ignored ones, so the mean is over fewer rows. Check the labels against num_classes when building the dataset
    (DownstreamDatasetFactory does so for the classes it derives from the directories)."""
    if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
        raise RuntimeError("cross_entropy: hipGraph capture of the classification step is not supported; run it eagerly")
    if logits.dim() != 2:
        raise ValueError(f"logits must be [B][C], got {tuple(logits.shape)}")
    return _CrossEntropyFn.apply(logits, labels)


class TopkAccuracy(object):
    """Reference utils/metrics.py:20-73: accumulates top-k accuracy over batches and returns it as a fraction. The counters stay on the
    device (clite_xent_fwd's acc); only get_metric synchronises. Rows labelled -100 are not counted, nor are rows whose label lies
    outside [0, C) (the reference would count those as misses)."""

    def __init__(self, top_k: int = 1):
        self._top_k = top_k
        self.reset()

    def reset(self):
        self._acc = None

    def __call__(self, predictions: torch.Tensor, ground_truth: torch.Tensor):
        B, C = predictions.shape
        z, ld = _row_major(predictions.detach())
        if self._acc is None:
            self._acc = torch.zeros(4, device=z.device, dtype=torch.float32)
        lse = torch.empty(B, device=z.device, dtype=torch.float32)
        hip.xent_fwd(z, ld, B, C, _labels(ground_truth, z.device), self._top_k, lse, self._acc)

    def get_metric(self, reset: bool = False):
        acc = [0.0] * 4 if self._acc is None else self._acc.tolist()
        correct = acc[1] if self._top_k == 1 else acc[2]
        accuracy = correct / acc[3] if acc[3] > 1e-12 else 0.0
        if reset:
            self.reset()
        return accuracy


# ------------------------------------------------------------------------------------------------ zero-shot
@torch.no_grad()
def zero_shot_counts(model, text_embeds: torch.Tensor, images: torch.Tensor, labels: torch.Tensor, acc: torch.Tensor, topk: int = 5,
                     batch_size: int = 128):
    """acc (f32 [4] on the device) += {-, #top-1, #top-k, #images} of the images against L2-normalised prompt embeddings [C][2048]
    (retrieval.embed_texts): each image goes to the prompt of highest cosine (reference zero_shot.py:150-157), ties to the lower class."""
    from . import retrieval
    C = text_embeds.shape[0]
    rt = model.runtime
    for i in range(0, images.shape[0], batch_size):
        img = retrieval.embed_images(model, images[i:i + batch_size].to(rt.device), batch_size)
        sims = retrieval.similarity(model, img, text_embeds)            # f32 [n][C], row stride ceil8(C)
        n = sims.shape[0]
        lse = torch.empty(n, device=rt.device, dtype=torch.float32)
        hip.xent_fwd(sims, sims.stride(0), n, C, _labels(labels[i:i + batch_size], rt.device), topk, lse, acc)


@torch.no_grad()
def zero_shot_accuracy(model, images: torch.Tensor, labels: torch.Tensor, prompt_ids: torch.Tensor, prompt_mask: torch.Tensor, topk: int = 5,
                       batch_size: int = 128) -> Dict[str, float]:
    """Zero-shot classification with a pretrained VLInfoModel (reference zero_shot.py): class prompts through the text encoder and its
    projector, images through the image encoder and its projector, both L2-normalised; top-1 / top-k in percent."""
    from . import retrieval
    rt = model.runtime
    text = retrieval.embed_texts(model, prompt_ids.to(rt.device), prompt_mask.to(rt.device), batch_size)
    acc = torch.zeros(4, device=rt.device, dtype=torch.float32)
    zero_shot_counts(model, text, images, labels, acc, topk, batch_size)
    a = acc.tolist()
    n = max(a[3], 1e-12)
    return {"top1": 100.0 * a[1] / n, f"top{topk}": 100.0 * a[2] / n}
