"""Weighted k-nearest-neighbour classification on frozen features (Wu et al. 2018, "Unsupervised feature learning via non-parametric instance
discrimination"; the protocol DINO and others report as "k-NN top-1"), on the HIP kernels. It needs no training, no hyper-parameter search and
no text: a labelled bank of features, and queries.

    scores = Xq Xb^T            one [query block] x [bank chunk] tile at a time: clite_gemm_nt in its exact-f32 form into a reused scratch (the
                                chunk padded to the GEMM's column granularity, as retrieval.similarity and kmeans do); the whole matrix
                                (50 000 x 1 281 167 f32 = 256 GB at ImageNet scale) never exists
    merge                       clite_knn_topk_merge after every tile: each query's running list of its k best bank rows, score descending, bank
                                index ascending among equal scores (the first k of a stable argsort of the whole row)
    vote                        clite_knn_vote: class score = sum over the k neighbours of that class of exp((s - s_best) / T); the five best
                                classes by (score descending, class ascending), for several k at once

Subtracting the best similarity inside the exponential scales every class score of a query by the same positive factor, so no ranking changes
and nothing can overflow. No float atomics take part: the lists and the predictions are bitwise reproducible. There is no CPU path.
"""
from typing import Dict, Sequence, Tuple

import torch

from . import hip
from .utils.common import logger


def _check_features(name: str, x: torch.Tensor) -> torch.Tensor:
    if x.dim() != 2 or x.dtype != torch.float32:
        raise ValueError(f"knn: {name} must be f32 [rows][D], got {x.dtype} {tuple(x.shape)}")
    if x.shape[0] == 0 or x.shape[1] == 0 or x.shape[1] % 8:
        raise ValueError(f"knn: {name} needs at least one row and D a positive multiple of 8, got {tuple(x.shape)}")
    if not x.is_cuda:
        raise RuntimeError(f"knn: {name} must be a GPU tensor; the k-NN kernels run on the MI355X only, there is no CPU path")
    if not bool(torch.isfinite(x).all()):
        raise ValueError(f"knn: {name} holds non-finite values (a NaN similarity has no rank)")
    return x.contiguous()


@torch.no_grad()
def topk(queries: torch.Tensor, bank: torch.Tensor, k: int, query_rows: int = 1024, bank_rows: int = 65536) -> Tuple[torch.Tensor, torch.Tensor]:
    """(scores f32 [Q][k], indices int32 [Q][k]): for every query row its k most similar bank rows by inner product, score descending, bank
    index ascending among equal scores. queries [Q][D], bank [N][D]: f32 on the GPU, D % 8 == 0, finite; 1 <= k <= min(256, N). The bank is
    visited in chunks of `bank_rows` rows (rounded up to a multiple of 8) for every block of `query_rows` queries; one scratch tile of
    query_rows x bank_rows scores is reused."""
    k, query_rows, bank_rows = int(k), int(query_rows), int(bank_rows)
    if query_rows < 1 or bank_rows < 1:
        raise ValueError("knn.topk: query_rows and bank_rows must be positive")
    if queries.dim() == 2 and bank.dim() == 2 and queries.shape[1] != bank.shape[1]:
        raise ValueError(f"knn.topk: queries have {queries.shape[1]} features, the bank {bank.shape[1]}")
    if k < 1 or k > hip.KNN_MAX_K:
        raise ValueError(f"knn.topk: k must be in [1, {hip.KNN_MAX_K}] (the running list lives in LDS), got {k}")
    if bank.dim() == 2 and k > bank.shape[0]:
        raise ValueError(f"knn.topk: k = {k} exceeds the bank's {bank.shape[0]} rows")
    queries, bank = _check_features("queries", queries), _check_features("bank", bank)
    if queries.device != bank.device:
        raise ValueError("knn.topk: queries and bank must be on the same device")
    Q, D = queries.shape
    N = bank.shape[0]
    if N > 0x7fffffff:
        raise ValueError("knn.topk: the bank has more rows than an int32 index can name")
    dev = queries.device
    chunk = min((bank_rows + 7) // 8 * 8, (N + 7) // 8 * 8)
    qb = min(query_rows, Q)
    scratch = torch.empty(qb, chunk, device=dev, dtype=torch.float32)
    top_s = torch.empty(Q, k, device=dev, dtype=torch.float32)
    top_i = torch.empty(Q, k, device=dev, dtype=torch.int32)
    tail = None
    if N % 8:                              # the last chunk, padded with zero rows: its padding columns are computed, never selected
        t0 = N // chunk * chunk            # chunk % 8 == 0, so the ragged chunk is the last one
        tail = torch.zeros((N - t0 + 7) // 8 * 8, D, device=dev, dtype=torch.float32)
        tail[:N - t0].copy_(bank[t0:])
    split = hip.is_f32_split()
    if split:
        hip.set_f32_split(False)           # exact f32 products only: a neighbour decided by a bf16 product is not the neighbour of the input
    try:
        for q0 in range(0, Q, qb):
            nq = min(qb, Q - q0)
            xq = queries[q0:q0 + nq]
            ts, ti = top_s[q0:q0 + nq], top_i[q0:q0 + nq]
            for base in range(0, N, chunk):
                nc = min(chunk, N - base)
                np8 = (nc + 7) // 8 * 8
                rows = bank[base:base + nc] if np8 == nc else tail
                hip.gemm_nt(hip.F32, xq, rows, nq, np8, D, hip.epilogue(scratch, np8, out_f32=True))
                hip.knn_topk_merge(scratch, np8, nq, nc, base, k, min(k, base), ts, ti)
    finally:
        if split:
            hip.set_f32_split(True)
    return top_s, top_i


@torch.no_grad()
def classify(scores: torch.Tensor, indices: torch.Tensor, bank_labels: torch.Tensor, num_classes: int, ks: Sequence[int], temperature: float = 0.07,
             return_scores: bool = False):
    """pred int32 [len(ks)][Q][5] (and, with return_scores, the class scores f32 [len(ks)][Q][num_classes]) of the weighted vote over topk()'s
    lists: for every k in ks (strictly ascending, 1 <= k <= the lists' width, at most 8 of them) the five best classes by (score descending,
    class ascending), -1 beyond num_classes. bank_labels: integers [N] in [0, num_classes), num_classes <= 16384. Labels and indices are checked
    here, before the launch."""
    if scores.dim() != 2 or scores.shape != indices.shape or scores.dtype != torch.float32 or indices.dtype != torch.int32:
        raise ValueError("knn.classify: scores f32 [Q][K] and indices int32 [Q][K] as topk() returns them")
    if not scores.is_cuda or not indices.is_cuda:
        raise RuntimeError("knn.classify: the lists must be GPU tensors; the k-NN kernels run on the MI355X only, there is no CPU path")
    Q, K = scores.shape
    ks = [int(k) for k in ks]
    num_classes = int(num_classes)
    if not 1 <= K <= hip.KNN_MAX_K or Q < 1:
        raise ValueError(f"knn.classify: lists of width 1 .. {hip.KNN_MAX_K} for at least one query, got {tuple(scores.shape)}")
    if not 1 <= len(ks) <= hip.KNN_MAX_KS or any(not 1 <= k <= K for k in ks) or any(a >= b for a, b in zip(ks, ks[1:])):
        raise ValueError(f"knn.classify: ks must be 1 .. {hip.KNN_MAX_KS} strictly ascending values in [1, {K}], got {ks}")
    if not 1 <= num_classes <= hip.KNN_MAX_CLASSES:
        raise ValueError(f"knn.classify: num_classes must be in [1, {hip.KNN_MAX_CLASSES}] (the class bins live in LDS), got {num_classes}")
    if not temperature > 0:
        raise ValueError(f"knn.classify: temperature must be positive, got {temperature}")
    labels = torch.as_tensor(bank_labels).reshape(-1)
    if labels.is_floating_point() or labels.numel() == 0:
        raise ValueError("knn.classify: bank_labels must be a non-empty integer vector")
    N = labels.numel()
    if int(labels.min()) < 0 or int(labels.max()) >= num_classes:
        raise ValueError(f"knn.classify: bank label outside [0, {num_classes})")
    if int(indices.min()) < 0 or int(indices.max()) >= N:
        raise ValueError(f"knn.classify: neighbour index outside the bank's {N} rows")
    dev = scores.device
    labels = labels.to(device=dev, dtype=torch.int32).contiguous()
    pred = torch.empty(len(ks), Q, hip.KNN_PRED, device=dev, dtype=torch.int32)
    cs = torch.empty(len(ks), Q, num_classes, device=dev, dtype=torch.float32) if return_scores else None
    hip.knn_vote(scores.contiguous(), indices.contiguous(), labels, Q, K, N, num_classes, ks, 1.0 / float(temperature), cs, pred)
    return (pred, cs) if return_scores else pred


def accuracies(pred: torch.Tensor, labels: torch.Tensor, ks: Sequence[int], num_classes: int) -> Dict[int, Dict[str, float]]:
    """{k: {"top1", "top5"}} in percent from classify()'s predictions; top5 only when there are at least five classes."""
    pred = pred.cpu()
    y = torch.as_tensor(labels).reshape(-1).cpu().to(torch.int32)
    if y.numel() != pred.shape[1]:
        raise ValueError(f"knn: {y.numel()} query labels for {pred.shape[1]} queries")
    out, n = {}, y.numel()
    for j, k in enumerate(ks):
        hit = pred[j] == y[:, None]
        out[int(k)] = {"top1": 100.0 * (int(hit[:, 0].sum()) / n)}
        if num_classes >= hip.KNN_PRED:
            out[int(k)]["top5"] = 100.0 * (int(hit.any(1).sum()) / n)
    return out


@torch.no_grad()
def knn_eval(train_feats: torch.Tensor, train_labels, test_feats: torch.Tensor, test_labels, num_classes: int,
             ks: Sequence[int] = (10, 20, 100, 200), temperature: float = 0.07, query_rows: int = 1024, bank_rows: int = 65536,
             return_pred: bool = False):
    """Weighted k-NN accuracy of test_feats against the labelled bank train_feats: {k: {"top1": ..., "top5": ...}} in percent (top5 only with at
    least five classes). A k larger than the bank is dropped with a logged line; the remaining ks are evaluated from one selection of max(ks)
    neighbours. With return_pred also the predictions int32 [len(ks)][Q][5] (on the GPU) and the ks that were kept."""
    N = train_feats.shape[0]
    keep = sorted({int(k) for k in ks})
    for k in keep:
        if k > N:
            logger.info(f"k-NN: k = {k} exceeds the bank's {N} rows, dropped")
    keep = [k for k in keep if k <= N]
    if not keep:
        raise ValueError(f"knn_eval: no k in {list(ks)} fits the bank's {N} rows")
    if keep[0] < 1 or keep[-1] > hip.KNN_MAX_K:
        raise ValueError(f"knn_eval: every k must be in [1, {hip.KNN_MAX_K}], got {keep}")
    top_s, top_i = topk(test_feats, train_feats, keep[-1], query_rows, bank_rows)
    pred = classify(top_s, top_i, train_labels, num_classes, keep, temperature)
    res = accuracies(pred, test_labels, keep, int(num_classes))
    return (res, pred, keep) if return_pred else res
