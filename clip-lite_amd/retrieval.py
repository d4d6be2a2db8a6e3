"""Embedding extraction and image-text retrieval on the trained model (reference retrieval.py:66-210), on the HIP kernels.

The reference puts the two encoders and the two mutual-information projection heads in eval mode, L2-normalises the projected
features and scores every image against every caption with one matrix product (`image_embeds @ text_embeds.t()`,
retrieval.py:143), then reports recall@1/5/10 in both directions (`itm_eval`, retrieval.py:150-207). Here the encoders and the heads
are the same executors as in training (BatchNorm on running statistics, no dropout), the normalisation is `clite_l2_normalize` and the
N x M similarity is one `clite_gemm_nt` on the MFMA engine. The ranking that recall@k needs is two counting kernels
(`clite_retrieval_rank_i2t` / `_t2i`, `gpu_ranks`) instead of the reference's full argsort of every row on the host; `evaluate` runs the
whole evaluation over a `data.RetrievalEvalDataset` loader.
"""
from typing import Dict, Sequence, Tuple

import numpy as np
import torch

from . import hip


@torch.no_grad()
def embed_images(model, images: torch.Tensor, batch_size: int = 128, normalize: bool = True) -> torch.Tensor:
    """images: f32 NCHW on the model's device -> L2-normalised projected embeddings [N][2048] (compute dtype).
    Reference retrieval.py:122-127: image_projector(image_encoder(image)) then F.normalize. normalize=False returns the projected features
    as they are (reference bias_eda.py drops the direction from the unnormalised features)."""
    rt = model.runtime
    enc, proj = model.image_encoder, model.loss.global_d.img_block
    was = (enc.training, proj.training)
    enc.eval(), proj.eval()
    outs = []
    for i in range(0, images.shape[0], batch_size):
        f = proj(enc(images[i:i + batch_size]))
        if normalize:
            o = torch.empty_like(f)
            hip.l2_normalize(rt.dt, f.contiguous(), o, f.shape[0], f.shape[1])
            f = o
        outs.append(f)
    enc.train(was[0]), proj.train(was[1])
    return torch.cat(outs, 0)


@torch.no_grad()
def embed_texts(model, input_ids: torch.Tensor, attention_mask: torch.Tensor, batch_size: int = 128, normalize: bool = True) -> torch.Tensor:
    """input_ids / attention_mask: int64 [N][L <= 128] (BERT; 32 for MPNet) -> L2-normalised projected embeddings [N][2048].
    Reference retrieval.py:90-108: text_projector(text_encoder({...})) then F.normalize. normalize=False: the projected features as they are."""
    rt = model.runtime
    enc, proj = model.text_encoder, model.loss.global_d.text_block
    was = (enc.training, proj.training)
    enc.eval(), proj.eval()
    outs = []
    for i in range(0, input_ids.shape[0], batch_size):
        f = proj(enc({"input_ids": input_ids[i:i + batch_size], "attention_mask": attention_mask[i:i + batch_size]}))
        if normalize:
            o = torch.empty_like(f)
            hip.l2_normalize(rt.dt, f.contiguous(), o, f.shape[0], f.shape[1])
            f = o
        outs.append(f)
    enc.train(was[0]), proj.train(was[1])
    return torch.cat(outs, 0)


@torch.no_grad()
def similarity(model, image_embeds: torch.Tensor, text_embeds: torch.Tensor) -> torch.Tensor:
    """sims[i][t] = <image_embeds[i], text_embeds[t]> as f32 [Ni][Nt] (reference retrieval.py:143). The text count is padded to a
    multiple of 8 internally (GEMM column granularity)."""
    rt = model.runtime
    Ni, D = image_embeds.shape
    Nt = text_embeds.shape[0]
    Np = (Nt + 7) // 8 * 8
    te = text_embeds.contiguous()
    if Np != Nt:
        te = torch.cat([te, torch.zeros(Np - Nt, D, device=te.device, dtype=te.dtype)], 0)
    out = torch.empty(Ni, Np, device=image_embeds.device, dtype=torch.float32)
    hip.gemm_nt(rt.dt, image_embeds.contiguous(), te, Ni, Np, D, hip.epilogue(out, Np, out_f32=True))
    return out[:, :Nt]


def _stable_positions(scores: np.ndarray) -> np.ndarray:
    """pos[i][t] = 0-based position of t in row i sorted by score, highest first, ties to the lower index (np.argsort(-s, kind="stable"))."""
    order = np.argsort(-scores, axis=1, kind="stable")
    pos = np.empty_like(order)
    rows = np.arange(order.shape[0])[:, None]
    pos[rows, order] = np.arange(order.shape[1])[None, :]
    return pos


def recalls(rank_i2t, rank_t2i) -> Dict[str, float]:
    """Recall@1/5/10 in both directions from the ranks (an image's rank is the best rank among its captions, a caption's rank is the rank of
    its image); the result keys and formulas of reference retrieval.py:180-207."""
    ranks, ranks_t = np.asarray(rank_i2t), np.asarray(rank_t2i)
    tr1, tr5, tr10 = (100.0 * float(np.mean(ranks < k)) for k in (1, 5, 10))
    ir1, ir5, ir10 = (100.0 * float(np.mean(ranks_t < k)) for k in (1, 5, 10))
    tr_mean, ir_mean = (tr1 + tr5 + tr10) / 3, (ir1 + ir5 + ir10) / 3
    return {"txt_r1": tr1, "txt_r5": tr5, "txt_r10": tr10, "txt_r_mean": tr_mean, "img_r1": ir1, "img_r5": ir5, "img_r10": ir10,
            "img_r_mean": ir_mean, "r_mean": (tr_mean + ir_mean) / 2}


def itm_eval(scores_i2t: np.ndarray, scores_t2i: np.ndarray, txt2img: Sequence[int], img2txt: Dict[int, Sequence[int]],
             image_ids: Sequence[int]) -> Dict[str, float]:
    """Recall@1/5/10 for image->text and text->image retrieval; same definitions and result keys as reference retrieval.py:150-207
    (an image's rank is the best rank among its own captions; a caption's rank is the rank of its image). Ranks on the host by a full
    stable argsort of every row; `gpu_ranks` + `recalls` compute the same ranks on the GPU."""
    image_ids = [int(i) for i in image_ids]
    img2idx = {img_id: idx for idx, img_id in enumerate(image_ids)}
    pos = _stable_positions(scores_i2t)                                # pos[i][t] = rank of caption t for image i
    ranks = np.array([min(pos[index, t] for t in img2txt[image_ids[index]]) for index in range(scores_i2t.shape[0])])
    pos_t = _stable_positions(scores_t2i)
    ranks_t = np.array([pos_t[index, img2idx[int(txt2img[index])]] for index in range(scores_t2i.shape[0])])
    return recalls(ranks, ranks_t)


def host_ranks(scores: np.ndarray, img2txt_rows: Sequence[Sequence[int]], txt2img_rows: Sequence[int]) -> Tuple[np.ndarray, np.ndarray]:
    """(rank_i2t, rank_t2i) of scores [Ni][Nt] by itm_eval's stable argsorts on the host; Nt for an image without captions. What gpu_ranks
    returns, for tests and tools/bench_retrieval.py."""
    Ni, Nt = scores.shape
    pos = _stable_positions(scores)
    r_i = np.array([min((pos[i, t] for t in img2txt_rows[i]), default=Nt) for i in range(Ni)], dtype=np.int32)
    pos_t = _stable_positions(np.ascontiguousarray(scores.T))
    r_t = np.array([pos_t[t, int(txt2img_rows[t])] for t in range(Nt)], dtype=np.int32)
    return r_i, r_t


def _index_tables(Ni: int, Nt: int, img2txt_rows, txt2img_rows):
    """int32 CSR (offsets [Ni + 1], caption indices) and txt2img [Nt], every index checked against the matrix shape (ValueError)."""
    if len(img2txt_rows) != Ni:
        raise ValueError(f"gpu_ranks: {len(img2txt_rows)} caption lists for {Ni} image rows")
    if len(txt2img_rows) != Nt:
        raise ValueError(f"gpu_ranks: {len(txt2img_rows)} txt2img entries for {Nt} caption columns")
    lens = np.array([len(c) for c in img2txt_rows], dtype=np.int64)
    off = np.zeros(Ni + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    if off[-1] > np.iinfo(np.int32).max:
        raise ValueError("gpu_ranks: too many caption indices")
    idx = np.zeros(max(int(off[-1]), 1), np.int64)
    if off[-1]:
        idx[:off[-1]] = np.concatenate([np.asarray(c, dtype=np.int64).reshape(-1) for c in img2txt_rows if len(c)])
    if off[-1] and (idx[:off[-1]].min() < 0 or idx[:off[-1]].max() >= Nt):
        raise ValueError(f"gpu_ranks: caption index outside [0, {Nt})")
    t2i = np.asarray(txt2img_rows, dtype=np.int64).reshape(-1)
    if t2i.size != Nt or (Nt and (t2i.min() < 0 or t2i.max() >= Ni)):
        raise ValueError(f"gpu_ranks: txt2img entry outside [0, {Ni})")
    return off.astype(np.int32), idx.astype(np.int32), t2i.astype(np.int32)


@torch.no_grad()
def gpu_ranks(sims: torch.Tensor, img2txt_rows: Sequence[Sequence[int]], txt2img_rows: Sequence[int]) -> Tuple[np.ndarray, np.ndarray]:
    """(rank_i2t int32 [Ni], rank_t2i int32 [Nt]) of a similarity matrix f32 [Ni][Nt] on the GPU (a strided view such as similarity()'s,
    whose row stride is the padded text count, is read in place): rank_i2t[i] = rank of image i's best caption in its row (Nt without
    captions), rank_t2i[t] = rank of image txt2img_rows[t] in column t; ranks as in itm_eval (stable, highest first). img2txt_rows: caption
    index lists in row order; txt2img_rows: an image row per caption. Every index is checked on the host before any launch (ValueError);
    only the Ni + Nt ranks come back to the host."""
    if sims.dim() != 2 or sims.dtype != torch.float32:
        raise ValueError(f"gpu_ranks: sims must be f32 [Ni][Nt], got {sims.dtype} {tuple(sims.shape)}")
    Ni, Nt = sims.shape
    if Ni == 0 or Nt == 0:
        raise ValueError("gpu_ranks: empty similarity matrix")
    off, idx, t2i = _index_tables(Ni, Nt, img2txt_rows, txt2img_rows)
    if not sims.is_cuda:
        raise RuntimeError("gpu_ranks: sims must be a GPU tensor; the ranking kernels run on the MI355X only")
    ld = sims.stride(0)
    if sims.stride(1) != 1 or ld < Nt or (sims.storage_offset() + Ni * ld) * 4 > sims.untyped_storage().nbytes():
        sims = sims.contiguous()                    # every row must be whole in memory up to ld (the kernels load 16-byte vectors)
        ld = Nt
    dev = sims.device
    off_d, idx_d, t2i_d = (torch.from_numpy(a).to(dev) for a in (off, idx, t2i))
    r_i = torch.empty(Ni, dtype=torch.int32, device=dev)
    r_t = torch.empty(Nt, dtype=torch.int32, device=dev)
    work = torch.empty((Ni + hip.RETRIEVAL_T2I_ROWS - 1) // hip.RETRIEVAL_T2I_ROWS, Nt, dtype=torch.int32, device=dev)
    hip.retrieval_rank_i2t(sims, ld, Ni, Nt, off_d, idx_d, r_i)
    hip.retrieval_rank_t2i(sims, ld, Ni, Nt, t2i_d, r_t, work)
    return r_i.cpu().numpy(), r_t.cpu().numpy()


@torch.no_grad()
def evaluate(model, loader, input_ids: torch.Tensor, attention_mask: torch.Tensor, text_batch_size: int = 128) -> Dict[str, float]:
    """Image-text retrieval of a pretraining model (reference retrieval.py:66-207): image embeddings one loader batch at a time, text
    embeddings of the tokenised captions, the similarity matrix, the ranks (gpu_ranks) and recall@1/5/10 (recalls). loader iterates a
    dataset with `img2txt` (row -> caption indices) and `txt2img` (caption -> row) whose items carry "image" and their row "index", in row
    order (shuffle=False). Returns the itm_eval dict."""
    ds = loader.dataset
    device = next(model.parameters()).device
    embeds, rows = [], []
    for batch in loader:
        embeds.append(embed_images(model, batch["image"].to(device, non_blocking=True)))
        rows.append(torch.as_tensor(batch["index"]).reshape(-1))
    image_embeds = torch.cat(embeds, 0)
    rows = torch.cat(rows, 0)
    if not torch.equal(rows, torch.arange(len(ds))):
        raise ValueError("retrieval.evaluate: the loader must visit every dataset row once, in order (shuffle=False, no sampler)")
    text_embeds = embed_texts(model, input_ids.to(device), attention_mask.to(device), text_batch_size)
    sims = similarity(model, image_embeds, text_embeds)
    Ni = len(ds)
    r_i, r_t = gpu_ranks(sims, [ds.img2txt[i] for i in range(Ni)], [ds.txt2img[t] for t in range(len(ds.text))])
    return recalls(r_i, r_t)
