"""GPU augmentation beside what it replaces (README.md "Augmenting on the GPU"): at N = 128, S = 224 and 256 x 341 canvases the gray pass, the
apply in the stem form and image_to_nhwc4 (the staging kernel of the f32 path), timed with device events in one process; and loader samples/s
per worker for the CPU recipe (data.load_image) and the canvas recipe (augment.make_canvas + plan_transforms) on a generated 640 x 480 JPEG.
--post adds `apply_post_stem_us`: clite_augment_apply_post on the same tables in the same stem form with every view gray and blurred at k = 7 (the
tiled LDS kernel's worst case), next to `apply_stem_us` from the same process. Prints one JSON line. python tools/bench_augment.py [--reps 50] [--post]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clip_lite_amd import augment, data, hip      # noqa: E402

TRAIN = ("random_resized_crop", "horizontal_flip", "color_jitter", "normalize")


def timed(fn, reps):
    for _ in range(5):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3          # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--loader-samples", type=int, default=40)
    ap.add_argument("--post", action="store_true", help="also time clite_augment_apply_post with every view gray and blurred at k = 7")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("bench_augment.py times kernels on the GPU; there is none")
    N, S, h, w = 128, 224, 256, 341
    rng = np.random.default_rng(0)
    canv = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(N)]
    u8, hw = augment.pack_canvases(canv, augment.canvas_capacity(256))
    plan = torch.stack([augment.plan_transforms(h, w, ("random_resized_crop", "horizontal_flip", "color_jitter::{'p': 1.0}", "normalize"), S,
                                                torch.Generator().manual_seed(n)) for n in range(N)])
    u8, hw, plan = u8.cuda(), hw.cuda(), plan.cuda()
    Hp, Wp = S + 6, S + 8
    mean = torch.empty(N, device="cuda")
    work = torch.empty(N * hip.augment_gray_blocks(S), device="cuda")
    xpad = torch.empty(N, Hp, Wp, 4, device="cuda", dtype=torch.bfloat16)
    f32 = augment.views(u8, hw, plan, S)
    out = {"N": N, "S": S, "canvas": [h, w],
           "gray_us": timed(lambda: hip.augment_gray_mean(u8, hw, plan, S, mean, work), a.reps),
           "apply_stem_us": timed(lambda: hip.augment_apply(hip.AUGMENT_NHWC4, hip.BF16, u8, hw, plan, mean, S, xpad, 3, Hp, Wp), a.reps),
           "apply_nchw_us": timed(lambda: hip.augment_apply(hip.AUGMENT_NCHW, hip.F32, u8, hw, plan, mean, S, f32), a.reps),
           "image_to_nhwc4_us": timed(lambda: hip.image_to_nhwc4(hip.BF16, f32, xpad, N, S, S, 3, Hp, Wp), a.reps),
           "bytes_in": int(N * h * w * 3), "bytes_out_stem": int(xpad.numel() * 2)}
    if a.post:
        post = torch.zeros(N, augment.POST_W)
        post[:, augment.POST_GRAY] = post[:, augment.POST_BLUR] = 1.0
        post[:, augment.POST_W0:augment.POST_W0 + 4] = torch.tensor(augment.BLUR_WEIGHTS[7])
        post = post.cuda()
        out["apply_post_stem_us"] = timed(lambda: hip.augment_apply_post(hip.AUGMENT_NHWC4, hip.BF16, u8, hw, plan, post, mean, S, xpad, 3, Hp, Wp),
                                          a.reps)
        out["post_over_plain"] = out["apply_post_stem_us"] / out["apply_stem_us"]
    from PIL import Image
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "img.jpg")
        yy, xx = np.mgrid[0:480, 0:640]
        Image.fromarray(np.stack([xx * 255 // 640, yy * 255 // 480, rng.integers(0, 256, (480, 640))], -1).astype(np.uint8)).save(path, quality=90)
        t0 = time.perf_counter()
        for i in range(a.loader_samples):
            data.load_image(path, TRAIN, S, torch.Generator().manual_seed(i))
        t1 = time.perf_counter()
        for i in range(a.loader_samples):
            c = augment.make_canvas(Image.open(path), 256)
            augment.plan_transforms(c.shape[0], c.shape[1], TRAIN, S, torch.Generator().manual_seed(i))
        t2 = time.perf_counter()
    out["loader_cpu_samples_per_s"] = a.loader_samples / (t1 - t0)
    out["loader_canvas_samples_per_s"] = a.loader_samples / (t2 - t1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
