"""Image augmentation on the GPU: the semantics, written once.

The CPU recipe (data.load_image: PIL decode, crop, antialiased resize, flip, colour jitter, f32 normalise, HWC -> CHW) costs a loader worker
most of its time and ships 602 KB of f32 per 224 x 224 sample. With `DATA.GPU_AUGMENT` a worker only decodes and pre-sizes the image to a
bounded uint8 CANVAS and draws a PLAN row; the kernels of csrc/augment_ops.hip do the rest on the device and write either the f32 NCHW
`image` of the batch-dict contract or the padded NHWC4 tensor the stem reads (train_loop.TrainStep). A second view of the same image
(`MODEL.VISUAL.SELF_SUPERVISED`) is a second plan row over the same bytes.

Canvas (worker side, `make_canvas`): PIL decode to RGB; if the transform list holds `smallest_resize` it is applied as configured, otherwise the
shorter side is resized to `DATA.GPU_AUGMENT_SOURCE_SIZE` with the same PIL call; the longer side is then centre-trimmed to at most
floor(1.5 x shorter side). The result is HWC uint8 with its own (h, w); a batch packs the canvases into uint8 [N][cap], cap = s * floor(1.5 s) * 3
for the shorter side s, sample n at the front of its slot with pitch 3 w. A record without an image file gets a seeded synthetic uint8 canvas.

Plan (`plan_transforms`): one f32 row of PLAN_W columns per view -
    PLAN_X0, PLAN_Y0, PLAN_CW, PLAN_CH   crop box in canvas pixels (floats)
    PLAN_FLIP                            1: mirror the view left-right (the caption swaps "left" and "right", as on the CPU path)
    PLAN_JITTER                          1: apply the four colour ops
    PLAN_FB, PLAN_FC, PLAN_FS, PLAN_FH   brightness, contrast, saturation factors and the hue shift (fraction of the circle)
    PLAN_ORDER .. +3                     the order of the ops: 0 brightness, 1 contrast, 2 saturation, 3 hue
    PLAN_NORMALIZE                       1: ImageNet mean / std
    PLAN_VIEW_SIZE                       S, the side of the view (the kernels ignore this column; the host reads the size of a batch's views here)
with the distributions and the draw order of data.load_image (crop scale and log-ratio ranges, 10 tries then the centred square, uniform offsets;
flip with p = 0.5; jitter with p = 0.8, factors uniform in 1 +- x, hue in +-0.1, random order; the `::{kwargs}` syntax), drawn from the
per-index generator `seed * 1000003 + idx`. `center_crop` yields the integer centred box at scale 1.

Post (`plan_transforms(..., return_post=True)`): a second f32 row of POST_W columns per view, for the two transforms that follow the jitter -
    POST_GRAY                            1: `random_gray` fired (reference factories.py: alb.ToGray, p = 0.2)
    POST_BLUR                            1: `blur` fired (reference factories.py: alb.GaussianBlur, p = 0.5)
    POST_W0 .. +3                        the blur's weights, centre outward (zeros without blur); two reserved zero columns follow
Draws, in list order from the same generator, on both paths (data.load_image makes the same ones): `random_gray` one draw, applied if
rnd() < p (default 0.2); `blur` one draw, applied if rnd() < p (default 0.5), and if applied one more, k = lo + int(rnd() (hi - lo + 1)) for
blur_limit = (lo, hi) (default (3, 7)), an even k going up by one - so the default gives 3, 5, 7 with probabilities 1/5, 2/5, 2/5. lo and hi must
be odd and lie in 3..7, and a `sigma_limit` other than 0 is refused (ValueError): the kernel is OpenCV's fixed one for sigma <= 0, k <= 7,
    k = 3: 0.5, 0.25, 0, 0      k = 5: 0.375, 0.25, 0.0625, 0      k = 7: 0.28125, 0.21875, 0.109375, 0.03125      (centre outward)
all dyadic, so exact in f32 and of sum 1. The host writes the weights, not k, into the row. Both names take `::{kwargs}` for p, `blur` also for
blur_limit. Same distribution family as albumentations 1.0.0 over OpenCV 4.5; the draws come from this package's generator, so an individual
image differs from an albumentations run with the same seed.

Pixel function, for output pixel (oy, ox) of an S x S view (f32 throughout, no intermediate rounding, no fused multiply-add):
  1. ox <- S - 1 - ox if the flip flag is set.
  2. The crop box is resampled to S x S with PIL's antialiased triangle filter (Image.BILINEAR with reducing support), per axis: scale = c / S,
     centre = x0 + (o + 0.5) scale, support = max(scale, 1), taps [int(centre - support + 0.5), int(centre + support + 0.5)) clipped to the canvas,
     weights max(0, 1 - |(i - centre + 0.5) / max(scale, 1)|) divided by their sum; value = sum_y wy (sum_x wx pixel), both in ascending order.
     A plan whose scale exceeds MAX_SCALE = 4 on an axis is refused on the host (`check_plan`): the kernels read at most 9 taps per axis.
  3. With jitter on, the four ops in the plan's order on values in [0, 255], clamped to [0, 255] after each: brightness v fb; contrast
     m + fc (v - m) with m the mean of gray = 0.299 R + 0.587 G + 0.114 B over the view as it stands in front of the contrast op; saturation
     g + fs (v - g) with the pixel's own gray g; hue RGB -> HSV (colorsys), h + fh mod 1, HSV -> RGB.
  3b. Gray, when POST_GRAY is set: g = 0.299 R + 0.587 G + 0.114 B on the unrounded values of step 3, v = (g, g, g).
  3c. Blur, when POST_BLUR is set: a separable 7-tap filter with the symmetric weights w[|i|] = POST_W0 + |i| on the S x S view as it stands
     after 3 / 3b, the horizontal pass first, then the vertical one, each adding its taps in ascending offset -3 .. +3 from zero. A coordinate
     outside the view takes OpenCV's default border REFLECT_101 (-1 -> 1, S -> S - 2; numpy.pad(mode="reflect")). A blurred view needs S >= 4.
  4. (v / 255 - mean) / std with the normalise flag, else v / 255.
The device path has this one order - crop, flip, jitter, gray, blur, normalise - whatever the list says: the planner refuses a list that names
`random_gray` or `blur` ahead of a colour jitter or of the box transform (the colour ops are not linear); gray and blur commute up to rounding
and may come in either order. The CPU path applies the list in its own order.
tests/augment_ref.py restates this in NumPy float64 (tests/augment_post_ref.py adds 3b / 3c) and is the yardstick of the kernels. Deliberate
differences from the CPU path: PIL rounds to uint8 after each of its two resize passes and after every colour op, ImageEnhance.Contrast rounds
its mean to an integer, gray is PIL's integer `L` conversion and the blur rounds its result to uint8 (measured differences: DESIGN.md section 7
and 3.3f); random_resized_crop cuts from the canvas, not from the full-resolution file.

The evaluation command lines (retrieval.py, voc_clf.py, linear_clf.py, zero_shot.py, cluster.py) keep the CPU path: their datasets do not emit
canvases.
"""
import math

import torch

from . import hip
from .hip import AUGMENT_MAX_SCALE as MAX_SCALE
from .hip import AUGMENT_PLAN_W as PLAN_W
from .hip import AUGMENT_POST_W as POST_W

PLAN_X0, PLAN_Y0, PLAN_CW, PLAN_CH, PLAN_FLIP, PLAN_JITTER, PLAN_FB, PLAN_FC, PLAN_FS, PLAN_FH, PLAN_ORDER, PLAN_NORMALIZE, PLAN_VIEW_SIZE = 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 14, 15
OP_BRIGHTNESS, OP_CONTRAST, OP_SATURATION, OP_HUE = 0, 1, 2, 3
POST_GRAY, POST_BLUR, POST_W0 = 0, 1, 2
POST_NAMES = ("random_gray", "blur")
BLUR_WEIGHTS = {3: (0.5, 0.25, 0.0, 0.0), 5: (0.375, 0.25, 0.0625, 0.0), 7: (0.28125, 0.21875, 0.109375, 0.03125)}      # centre outward
BLUR_MIN_VIEW = 4     # REFLECT_101 of a 3-pixel reach
TRIM = 1.5            # longer side of a canvas <= floor(TRIM * shorter side)


def canvas_short_side(transforms, crop_size: int, source_size: int) -> int:
    """Shorter side of every canvas of a dataset: the size of the `smallest_resize` in the transform list, else `source_size`."""
    from .data import _transform_args
    for spec in transforms:
        name, _, arg = spec.partition("::")
        if name == "smallest_resize":
            return _transform_args(arg, crop_size)[0]
    return int(source_size)


def canvas_capacity(short_side: int) -> int:
    """Bytes of one canvas slot."""
    return short_side * int(TRIM * short_side) * 3


def make_canvas(img, short_side: int):
    """PIL image -> HWC uint8 ndarray: shorter side -> short_side (the PIL call of load_image's smallest_resize), longer side centre-trimmed to
    floor(1.5 x short_side)."""
    from PIL import Image
    import numpy as np
    img = img.convert("RGB")
    w, h = img.size
    sc = short_side / min(w, h)
    img = img.resize((max(1, round(w * sc)), max(1, round(h * sc))), Image.BILINEAR)
    w, h = img.size
    lim = int(TRIM * min(w, h))
    if w > lim:
        l = (w - lim) // 2
        img = img.crop((l, 0, l + lim, h))
    elif h > lim:
        t = (h - lim) // 2
        img = img.crop((0, t, w, t + lim))
    return np.asarray(img, dtype=np.uint8).copy()


def synthetic_canvas(short_side: int, generator):
    """The uint8 counterpart of the CPU path's seeded `randn` image for a record without an image file: a square canvas of uniform bytes."""
    return torch.randint(0, 256, (short_side, short_side, 3), generator=generator, dtype=torch.uint8).numpy()


def needs_post(transforms) -> bool:
    """The list names `random_gray` or `blur`: its views need a post row beside the plan row."""
    return any(spec.partition("::")[0] in POST_NAMES for spec in transforms)


def draw_gray(rnd, kw) -> bool:
    """The draw of `random_gray` (one), shared by both paths."""
    return rnd() < kw.get("p", 0.2)


def draw_blur(rnd, kw) -> int:
    """The draws of `blur` (one, and one more when it fires), shared by both paths: the kernel size 3, 5 or 7, or 0 when it does not fire."""
    if kw.get("sigma_limit", 0) not in (0, (0, 0), [0, 0]):
        raise ValueError(f"blur: sigma_limit {kw['sigma_limit']!r} is not supported (only 0: OpenCV's fixed kernels)")
    lim = kw.get("blur_limit", (3, 7))
    if not isinstance(lim, (tuple, list)) or len(lim) != 2:
        raise ValueError(f"blur: blur_limit {lim!r} must be a pair (lo, hi)")
    lo, hi = lim
    if not all(isinstance(x, int) and x % 2 == 1 and 3 <= x <= 7 for x in (lo, hi)) or lo > hi:
        raise ValueError(f"blur: blur_limit {lim!r} must be odd sizes in 3..7, (lo, hi) with lo <= hi")
    if rnd() >= kw.get("p", 0.5):
        return 0
    k = lo + int(rnd() * (hi - lo + 1))
    return k + 1 if k % 2 == 0 else k


def plan_transforms(h: int, w: int, transforms, crop_size: int, generator=None, return_post=False):
    """One plan row (f32 [PLAN_W]) for a view of an h x w canvas through the named transforms, with load_image's distributions and draw order.
    `smallest_resize` is the worker's (make_canvas) and draws nothing; `global_resize` takes the whole canvas; at most one of the box
    transforms (center_crop, random_resized_crop, global_resize) may appear. Raises ValueError for a plan the kernels refuse (check_plan).
    return_post: return (row, post row [POST_W]) - required for a list that names `random_gray` or `blur` (ValueError otherwise: neither is
    dropped silently), which must name them behind its box transform and its colour jitter."""
    from .data import _transform_args
    if not return_post and needs_post(transforms):
        raise ValueError("the transform list names random_gray / blur: its views need a post row (plan_transforms(..., return_post=True))")
    post = torch.zeros(POST_W, dtype=torch.float32)
    post_seen = None

    def rnd():
        return float(torch.rand((), generator=generator))

    row = torch.zeros(PLAN_W, dtype=torch.float32)
    box = None
    row[PLAN_FB] = row[PLAN_FC] = row[PLAN_FS] = 1.0
    order = [0, 1, 2, 3]
    for spec in transforms:
        name, _, arg = spec.partition("::")
        size, kw = _transform_args(arg, crop_size)
        if name == "smallest_resize":
            continue
        if post_seen and name in ("global_resize", "center_crop", "random_resized_crop", "color_jitter", "color_jitter8"):
            raise ValueError(f"GPU augmentation applies gray and blur after the crop and the colour jitter; {post_seen!r} stands ahead of {spec!r}")
        if name in ("global_resize", "center_crop", "random_resized_crop"):
            if box is not None:
                raise ValueError(f"GPU augmentation takes one crop / resize transform per view; {spec!r} is a second one")
            if size != crop_size:
                raise ValueError(f"GPU augmentation writes IMAGE_CROP_SIZE ({crop_size}) views; {spec!r} asks for {size}")
        if name == "global_resize":
            box = (0.0, 0.0, float(w), float(h))
        elif name == "center_crop":
            if size > w or size > h:
                raise ValueError(f"center_crop of {size} from a {h} x {w} canvas")
            box = (float((w - size) // 2), float((h - size) // 2), float(size), float(size))
        elif name == "random_resized_crop":
            s_lo, s_hi = kw.get("scale", (0.2, 1.0))
            r_lo, r_hi = kw.get("ratio", (0.75, 1.333))
            for _ in range(10):
                area = w * h * (s_lo + (s_hi - s_lo) * rnd())
                logr = math.log(r_lo) + (math.log(r_hi) - math.log(r_lo)) * rnd()
                ar = math.exp(logr)
                cw, ch = int(round(math.sqrt(area * ar))), int(round(math.sqrt(area / ar)))
                if 0 < cw <= w and 0 < ch <= h:
                    l, t = int(rnd() * (w - cw + 1)), int(rnd() * (h - ch + 1))
                    box = (float(l), float(t), float(cw), float(ch))
                    break
            if box is None:
                s_ = min(w, h)
                box = (float((w - s_) // 2), float((h - s_) // 2), float(s_), float(s_))
        elif name == "horizontal_flip":
            if rnd() < kw.get("p", 0.5):
                row[PLAN_FLIP] = 1.0 - row[PLAN_FLIP]
        elif name in ("color_jitter", "color_jitter8"):
            if row[PLAN_JITTER] != 0:
                raise ValueError("GPU augmentation takes one color_jitter per view")
            x = 0.8 if name == "color_jitter8" else 0.4
            if rnd() < kw.get("p", 0.8):          # the draws of data._color_jitter, in its order
                fb, fc, fs = (1.0 + (2.0 * rnd() - 1.0) * kw.get(k, x) for k in ("brightness", "contrast", "saturation"))
                fh = (2.0 * rnd() - 1.0) * kw.get("hue", 0.1)
                order = sorted(range(4), key=lambda _: rnd())
                row[PLAN_JITTER] = 1.0
                row[PLAN_FB], row[PLAN_FC], row[PLAN_FS], row[PLAN_FH] = fb, fc, fs, fh
        elif name == "random_gray":
            post_seen = post_seen or spec
            if draw_gray(rnd, kw):
                post[POST_GRAY] = 1.0
        elif name == "blur":
            post_seen = post_seen or spec
            if post[POST_BLUR] != 0:
                raise ValueError("GPU augmentation takes one blur per view")
            k = draw_blur(rnd, kw)
            if k:
                if crop_size < BLUR_MIN_VIEW:
                    raise ValueError(f"a blurred view needs IMAGE_CROP_SIZE >= {BLUR_MIN_VIEW}")
                post[POST_BLUR] = 1.0
                post[POST_W0:POST_W0 + 4] = torch.tensor(BLUR_WEIGHTS[k])
        elif name == "normalize":
            row[PLAN_NORMALIZE] = 1.0
        else:
            raise KeyError(f"unknown image transform {spec!r}")
    if box is None:
        if (h, w) != (crop_size, crop_size):
            raise ValueError(f"no crop / resize transform and the canvas is {h} x {w}, not {crop_size} x {crop_size}")
        box = (0.0, 0.0, float(w), float(h))
    row[PLAN_X0], row[PLAN_Y0], row[PLAN_CW], row[PLAN_CH] = box
    row[PLAN_ORDER:PLAN_ORDER + 4] = torch.tensor(order, dtype=torch.float32)
    row[PLAN_VIEW_SIZE] = float(crop_size)
    check_plan(row[None], torch.tensor([[h, w]]), crop_size)
    if return_post:
        check_post(post[None], crop_size)
        return row, post
    return row


def check_plan(plan, hw, S: int):
    """Host-side refusal of plan rows the kernels do not take: a box that is empty, not finite or outside its canvas, a scale above MAX_SCALE on
    an axis (more than 9 taps), an order that is no permutation."""
    plan, hw = torch.as_tensor(plan, dtype=torch.float32), torch.as_tensor(hw)
    if plan.dim() != 2 or plan.shape[1] != PLAN_W or tuple(hw.shape) != (plan.shape[0], 2):
        raise ValueError(f"plan must be [N][{PLAN_W}] with an [N][2] table of canvas extents")
    if not bool(torch.isfinite(plan).all()):
        raise ValueError("plan rows must be finite")
    x0, y0, cw, ch = (plan[:, k] for k in (PLAN_X0, PLAN_Y0, PLAN_CW, PLAN_CH))
    h, w = hw[:, 0].to(torch.float32), hw[:, 1].to(torch.float32)
    if bool(((cw <= 0) | (ch <= 0) | (x0 < 0) | (y0 < 0) | (x0 + cw > w) | (y0 + ch > h)).any()):
        raise ValueError("a crop box is empty or lies outside its canvas")
    if bool(((cw > MAX_SCALE * S) | (ch > MAX_SCALE * S)).any()):
        raise ValueError(f"a crop box is more than {MAX_SCALE} x the view size {S} on an axis: the resampling kernels read at most "
                         f"{2 * MAX_SCALE + 1} taps per axis (use a smaller DATA.GPU_AUGMENT_SOURCE_SIZE)")
    if bool((plan[:, PLAN_ORDER:PLAN_ORDER + 4].sort(dim=1).values != torch.arange(4.0)).any()):
        raise ValueError("the colour-op order of a plan row is not a permutation of 0..3")


def check_post(post, S: int):
    """Host-side refusal of post rows the kernel does not take: a flag that is not 0 or 1, a weight that is not finite or is negative, and
    on a blurred row weights that do not sum to 1 or a view smaller than BLUR_MIN_VIEW."""
    post = torch.as_tensor(post, dtype=torch.float32)
    if post.dim() != 2 or post.shape[1] != POST_W:
        raise ValueError(f"post must be [N][{POST_W}]")
    flags, wt = post[:, [POST_GRAY, POST_BLUR]], post[:, POST_W0:POST_W0 + 4]
    if bool(((flags != 0) & (flags != 1)).any()):
        raise ValueError("a gray / blur flag of a post row is not 0 or 1")
    if not bool(torch.isfinite(wt).all()) or bool((wt < 0).any()):
        raise ValueError("the blur weights of a post row must be finite and not negative")
    blurred = post[:, POST_BLUR] != 0
    if bool(blurred.any()):
        if S < BLUR_MIN_VIEW:
            raise ValueError(f"a blurred view needs S >= {BLUR_MIN_VIEW}")
        total = wt[:, 0] + 2.0 * (wt[:, 1] + wt[:, 2] + wt[:, 3])
        if bool(((total - 1.0).abs() > 1e-3)[blurred].any()):
            raise ValueError("the blur weights of a post row do not sum to 1")


def view_size(plan) -> int:
    """S of a batch's plan rows, from a host copy of the first row (one small read; a device plan costs a synchronisation, so callers that
    know S pass it instead)."""
    return int(plan[0, PLAN_VIEW_SIZE])


def pack_canvases(canvases, cap: int):
    """[HWC uint8 ndarray / tensor, ...] -> (uint8 [N][cap], int32 [N][2]): each canvas at the front of its slot, the rest zero."""
    out = torch.zeros(len(canvases), cap, dtype=torch.uint8)
    hw = torch.zeros(len(canvases), 2, dtype=torch.int32)
    for n, c in enumerate(canvases):
        c = torch.as_tensor(c)
        if c.dtype != torch.uint8 or c.dim() != 3 or c.shape[2] != 3 or c.numel() > cap:
            raise ValueError(f"canvas {n}: expected HWC uint8 of at most {cap} bytes, got {tuple(c.shape)} {c.dtype}")
        out[n, :c.numel()] = c.reshape(-1)
        hw[n, 0], hw[n, 1] = c.shape[0], c.shape[1]
    return out, hw


# ------------------------------------------------------------------------------------------------ device side
def gray_means(image_u8, image_hw, plan, S: int, plan_host=None, hw_host=None):
    """f32 [N]: every jittered view's mean gray in front of its contrast op (first pass of `views`)."""
    N = image_u8.shape[0]
    mean = torch.empty(N, device=image_u8.device, dtype=torch.float32)
    work = torch.empty(N * hip.augment_gray_blocks(S), device=image_u8.device, dtype=torch.float32)
    hip.augment_gray_mean(image_u8, image_hw, plan, S, mean, work, plan_host, hw_host)
    return mean


def views(image_u8, image_hw, plan, S: int, plan_host=None, hw_host=None, post=None, post_host=None):
    """The batch-dict form: f32 NCHW [N][3][S][S] views of device canvases. post: the views' gray / blur rows (None: neither, the plain
    entry point)."""
    image_u8, image_hw, plan = image_u8.contiguous(), image_hw.contiguous(), plan.contiguous()
    mean = gray_means(image_u8, image_hw, plan, S, plan_host, hw_host)
    out = torch.empty(image_u8.shape[0], 3, S, S, device=image_u8.device, dtype=torch.float32)
    if post is None:
        hip.augment_apply(hip.AUGMENT_NCHW, hip.F32, image_u8, image_hw, plan, mean, S, out, plan_host=plan_host, hw_host=hw_host)
    else:
        hip.augment_apply_post(hip.AUGMENT_NCHW, hip.F32, image_u8, image_hw, plan, post.contiguous(), mean, S, out, plan_host=plan_host,
                               hw_host=hw_host, post_host=post_host)
    return out


def stage_views(rt, image_u8, image_hw, plan, S: int, out=None, post=None):
    """The stem form, what resnet.stage_image makes of `views(...)`: padded NHWC4 in the compute dtype. `out` re-uses an earlier result's
    storage (the captured train step stages every batch into the buffer its graphs read). post: as in `views`."""
    from .resnet import _alloc
    image_u8, image_hw, plan = image_u8.contiguous(), image_hw.contiguous(), plan.contiguous()
    N = image_u8.shape[0]
    Hp, Wp = S + 6, S + 6 + 2
    Wp += Wp % 2
    xpad = _alloc(rt, N, Hp, Wp, 4) if out is None else out
    assert tuple(xpad.shape) == (N, Hp, Wp, 4) and xpad.dtype == rt.tdtype
    mean = gray_means(image_u8, image_hw, plan, S)
    if post is None:
        hip.augment_apply(hip.AUGMENT_NHWC4, rt.dt, image_u8, image_hw, plan, mean, S, xpad, 3, Hp, Wp)
    else:
        hip.augment_apply_post(hip.AUGMENT_NHWC4, rt.dt, image_u8, image_hw, plan, post.contiguous(), mean, S, xpad, 3, Hp, Wp)
    return xpad
