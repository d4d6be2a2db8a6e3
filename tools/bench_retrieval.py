"""Time the retrieval ranking at COCO-5k scale (5000 images x 25014 captions) on one GPU and print one JSON line: the GPU time of gpu_ranks (both
rank kernels, the t2i chunk sum and the copy of the Ni + Nt ranks to the host), each kernel launch on its own between stream events with the
bandwidth of its pass over the similarity matrix, whether the ranks equal the host's, and, unless --no-host, the time of the host itm_eval on
the same matrix. The matrix comes out of similarity() on seeded unit-norm embeddings (2048 wide, captions correlated with their image), so its
row stride is the padded text count.

    python tools/bench_retrieval.py [--repeats 5] [--no-host]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def coco_scale_sims(model, Ni=5000, Nt=25014, D=2048, seed=0):
    """similarity() of seeded embeddings: caption t belongs to image t % Ni (5 or 6 captions per image) and sits near it."""
    from clip_lite_amd import retrieval
    g = torch.Generator().manual_seed(seed)
    img = torch.randn(Ni, D, generator=g)
    txt = img[torch.arange(Nt) % Ni] + 1.5 * torch.randn(Nt, D, generator=g)
    img, txt = (torch.nn.functional.normalize(x, dim=1).cuda() for x in (img, txt))
    img2txt = [list(range(i, Nt, Ni)) for i in range(Ni)]
    txt2img = [t % Ni for t in range(Nt)]
    return retrieval.similarity(model, img, txt), img2txt, txt2img


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-host", action="store_true", help="skip the host itm_eval timing (about half a minute at this size)")
    a = ap.parse_args()
    from clip_lite_amd import retrieval
    from clip_lite_amd.encoder import ImageEncoder, TextEncoder
    from clip_lite_amd.loss import JSDInfoMaxLoss
    from clip_lite_amd.model import VLInfoModel
    model = VLInfoModel(TextEncoder(mode="train_sbert", num_hidden_layers=1), ImageEncoder("resnet18"),
                        JSDInfoMaxLoss(512, 768, "dot", 0.1, True, True), "train_sbert", is_amp=False).cuda()
    sims, img2txt, txt2img = coco_scale_sims(model)
    Ni, Nt = sims.shape
    retrieval.gpu_ranks(sims, img2txt, txt2img)                       # warm-up: first launches
    torch.cuda.synchronize()
    times, ranks = [], None
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        ranks = retrieval.gpu_ranks(sims, img2txt, txt2img)
        times.append(time.perf_counter() - t0)
    # the kernels alone, between events on the stream
    off, idx, t2i = retrieval._index_tables(Ni, Nt, img2txt, txt2img)
    off, idx, t2i = (torch.from_numpy(x).cuda() for x in (off, idx, t2i))
    r_i = torch.empty(Ni, dtype=torch.int32, device="cuda")
    r_t = torch.empty(Nt, dtype=torch.int32, device="cuda")
    from clip_lite_amd import hip
    work = torch.empty((Ni + hip.RETRIEVAL_T2I_ROWS - 1) // hip.RETRIEVAL_T2I_ROWS, Nt, dtype=torch.int32, device="cuda")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    k_i, k_t = [], []
    for _ in range(a.repeats):
        ev[0].record()
        hip.retrieval_rank_i2t(sims, sims.stride(0), Ni, Nt, off, idx, r_i)
        ev[1].record()
        hip.retrieval_rank_t2i(sims, sims.stride(0), Ni, Nt, t2i, r_t, work)
        ev[2].record()
        torch.cuda.synchronize()
        k_i.append(ev[0].elapsed_time(ev[1]) * 1e-3)
        k_t.append(ev[1].elapsed_time(ev[2]) * 1e-3)
    pass_bytes = Ni * Nt * 4
    host = sims.cpu().numpy()
    want = retrieval.host_ranks(host, img2txt, txt2img)
    equal = bool(np.array_equal(ranks[0], want[0]) and np.array_equal(ranks[1], want[1])
                 and np.array_equal(r_i.cpu().numpy(), want[0]) and np.array_equal(r_t.cpu().numpy(), want[1]))
    out = {"metric": "retrieval_rank", "Ni": Ni, "Nt": Nt, "ld": int(sims.stride(0)), "gpu_ranks_s": min(times), "gpu_ranks_s_all": times,
           "i2t_kernel_s": min(k_i), "t2i_kernel_s": min(k_t), "i2t_GBps": pass_bytes / min(k_i) / 1e9, "t2i_GBps": pass_bytes / min(k_t) / 1e9,
           "gpu_ranks_GBps": 2 * pass_bytes / min(times) / 1e9, "ranks_equal_host": equal,
           "recalls": retrieval.recalls(*ranks)}
    if not a.no_host:
        t0 = time.perf_counter()
        res = retrieval.itm_eval(host, host.T, txt2img, {i: c for i, c in enumerate(img2txt)}, list(range(Ni)))
        out["host_itm_eval_s"] = time.perf_counter() - t0
        out["host_recalls_equal"] = res == out["recalls"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
