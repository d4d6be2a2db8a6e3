"""Bias evaluation: a direction found in the text embedding space is removed from image features (reference bias_eda.py, utils/we.py), on
the HIP kernels.

The reference embeds Bolukbasi's definitional word pairs with the text tower and its projection head, takes the first principal component
of the pair-centred embeddings (`we.doPCA`), projects it out of every projected image feature (`we.drop`) and compares what a prompt
retrieves from the "men" and "women" image sets before and after. Here:

    directions   clite_debias_pca: the principal directions of the pair differences e(a_i) - e(b_i). doPCA's 2 P rows +-d_i / 2 have a zero
                 column mean, so its components are the right singular vectors of the differences; they come from the P x P Gram matrix
                 (f32, fixed summation order), diagonalised by a Jacobi iteration in LDS
    remove       clite_debias_rows: one streaming pass over the image bank: xn = x / |x|, xd = the row with the directions projected out,
                 normalised (F.normalize's rule, |y| taken from y itself), coef = <x, v_j>
    evaluate     per prompt and mode (biased: xn, debiased: xd) the k best images of every group by cosine (knn.topk on the group's rows) and
                 the share of every group among the k best of the whole bank

No float atomics take part: every figure is bitwise reproducible. There is no CPU path.
"""
from typing import Dict, Tuple

import numpy as np
import torch

from . import hip, knn

MODES = ("biased", "debiased")
MIN_EIGEN_RATIO = 1e-4      # the f32 Gram matrix's noise floor is about P eps lambda_1 (4e-6 lambda_1 at P = 64): a direction below this is noise
MAX_GROUPS = 8


def _check_rows(where: str, name: str, x: torch.Tensor) -> torch.Tensor:
    if not isinstance(x, torch.Tensor) or x.dim() != 2 or not x.is_floating_point():
        raise ValueError(f"{where}: {name} must be a floating-point tensor [rows][D]")
    if x.shape[0] == 0 or x.shape[1] == 0 or x.shape[1] % 8 or x.shape[1] > hip.DEBIAS_MAX_DIM:
        raise ValueError(f"{where}: {name} needs at least one row and D a positive multiple of 8, at most {hip.DEBIAS_MAX_DIM}, "
                         f"got {tuple(x.shape)}")
    if not x.is_cuda:
        raise RuntimeError(f"{where}: {name} must be a GPU tensor; the debias kernels run on the MI355X only, there is no CPU path")
    x = x.float().contiguous()
    if not bool(torch.isfinite(x).all()):
        raise ValueError(f"{where}: {name} holds non-finite values")
    return x


def _check_components(where: str, components: torch.Tensor, D: int) -> torch.Tensor:
    v = _check_rows(where, "components", components)
    if v.shape[0] > hip.DEBIAS_MAX_COMPONENTS:
        raise ValueError(f"{where}: at most {hip.DEBIAS_MAX_COMPONENTS} components (they live in LDS), got {v.shape[0]}")
    if v.shape[1] != D:
        raise ValueError(f"{where}: the components have {v.shape[1]} features, the rows {D}")
    return v


@torch.no_grad()
def directions(text_embeds_a: torch.Tensor, text_embeds_b: torch.Tensor, components: int = 1) -> Tuple[torch.Tensor, torch.Tensor]:
    """(components f32 [R][D] on the GPU, explained_variance_ratio f32 [R] on the host) of the pairs (a_i, b_i): what
    we.doPCA(pairs, E, R).components_ / .explained_variance_ratio_ hold, up to the sign of each row (here: the entry of largest magnitude is
    positive). text_embeds_a / _b: [P][D] on the GPU, 1 <= P <= 64, cast to f32. Refuses (ValueError) a direction whose eigenvalue is below
    1e-4 of the first: it is rounding noise of the f32 Gram matrix (fewer independent pairs than components)."""
    R = int(components)
    a, b = _check_rows("debias.directions", "text_embeds_a", text_embeds_a), _check_rows("debias.directions", "text_embeds_b", text_embeds_b)
    if a.shape != b.shape or a.device != b.device:
        raise ValueError(f"debias.directions: the two sides of the pairs differ: {tuple(a.shape)} and {tuple(b.shape)}")
    P, D = a.shape
    if P > hip.DEBIAS_MAX_PAIRS:
        raise ValueError(f"debias.directions: at most {hip.DEBIAS_MAX_PAIRS} pairs (their Gram matrix lives in LDS), got {P}")
    if not 1 <= R <= min(P, hip.DEBIAS_MAX_COMPONENTS):
        raise ValueError(f"debias.directions: components must be in [1, {min(P, hip.DEBIAS_MAX_COMPONENTS)}] for {P} pairs, got {R}")
    dev = a.device
    diffs = (a - b).contiguous()
    eig = torch.empty(P, device=dev, dtype=torch.float32)
    comps = torch.empty(R, D, device=dev, dtype=torch.float32)
    work = torch.empty(P * P, device=dev, dtype=torch.float32)
    info = torch.zeros(2, device=dev, dtype=torch.int32)
    hip.debias_pca(diffs, P, D, R, eig, comps, work, info)
    code, sweeps = (int(v) for v in info.cpu())
    if code:
        raise RuntimeError(f"debias.directions: the Jacobi iteration did not converge in {sweeps} sweeps (code {code})")
    lam = eig.cpu().numpy().astype(np.float64)
    if not np.all(np.isfinite(lam)):
        raise ValueError("debias.directions: the Gram matrix of the pair differences is not finite in f32 (differences of magnitude 1e19 "
                         "or more overflow their squares); scale the embeddings down")
    if lam[0] <= 0 or lam[R - 1] < MIN_EIGEN_RATIO * lam[0]:
        raise ValueError(f"debias.directions: component {R} has eigenvalue {lam[R - 1]:.3e} against {lam[0]:.3e} of the first, below "
                         f"{MIN_EIGEN_RATIO:g}: the pairs span fewer than {R} directions")
    return comps, torch.from_numpy((lam[:R] / lam.sum()).astype(np.float32))


@torch.no_grad()
def remove(x: torch.Tensor, components: torch.Tensor):
    """(xn, xd, coef) of the rows x [N][D] (cast to f32) and the orthonormal components [R][D]: xn = x / max(|x|, 1e-12), xd = y / max(|y|,
    1e-12) with y = x - sum_j <x, v_j> v_j, coef [N][R] = <x, v_j>."""
    x = _check_rows("debias.remove", "x", x)
    v = _check_components("debias.remove", components, x.shape[1])
    if v.device != x.device:
        raise ValueError("debias.remove: x and components must be on the same device")
    N, D = x.shape
    R = v.shape[0]
    xn, xd = torch.empty_like(x), torch.empty_like(x)
    coef = torch.empty(N, R, device=x.device, dtype=torch.float32)
    hip.debias_rows(x, v, N, D, R, xn, xd, coef)
    return xn, xd, coef


def check_groups(groups, N: int, k: int) -> Tuple[np.ndarray, int]:
    """(groups int64 [N] on the host, G): integers in [0, G), 2 <= G <= 8, every group with at least k rows."""
    g = np.asarray(torch.as_tensor(groups).cpu() if isinstance(groups, torch.Tensor) else groups).reshape(-1)
    if g.size != N:
        raise ValueError(f"debias.evaluate: {g.size} group labels for {N} images")
    if not np.issubdtype(g.dtype, np.integer):
        raise ValueError("debias.evaluate: groups must be integers")
    g = g.astype(np.int64)
    G = int(g.max()) + 1
    if g.min() < 0 or not 2 <= G <= MAX_GROUPS:
        raise ValueError(f"debias.evaluate: groups must be integers in [0, G) with 2 <= G <= {MAX_GROUPS}, got [{int(g.min())}, {G - 1}]")
    sizes = np.bincount(g, minlength=G)
    if not 1 <= k <= hip.KNN_MAX_K:
        raise ValueError(f"debias.evaluate: k must be in [1, {hip.KNN_MAX_K}], got {k}")
    if k > sizes.min():
        raise ValueError(f"debias.evaluate: k = {k} exceeds the smallest group's {int(sizes.min())} images (group sizes {sizes.tolist()})")
    return g, G


def assemble(groups: np.ndarray, G: int, k: int, lists: Dict[str, tuple], prior, explained_variance_ratio) -> Dict:
    """The result dict from the top-k lists. lists[mode] = (group_scores [Q][G][k], group_indices [Q][G][k] (bank rows), bank_indices [Q][k]):
    mean_alignment[mode][prompt][group] = mean of the group's k cosines (the reference's "Mean Alignment", correctly labelled),
    share[mode][prompt][group] = fraction of the group among the k best of the whole bank."""
    groups = np.asarray(groups)
    out = {"k": int(k), "num_groups": int(G), "num_images": int(groups.size), "group_sizes": np.bincount(groups, minlength=G).tolist(),
           "prior": [float(p) for p in prior], "explained_variance_ratio": [float(r) for r in explained_variance_ratio],
           "mean_alignment": {}, "share": {}, "top_scores": {}, "top_indices": {}}
    for mode in MODES:
        gs, gi, bi = (np.asarray(a) for a in lists[mode])
        if gs.shape != gi.shape or gs.shape[1:] != (G, k) or bi.shape != (gs.shape[0], k):
            raise ValueError(f"debias.assemble: lists of mode {mode} have shapes {gs.shape}, {gi.shape}, {bi.shape}")
        out["mean_alignment"][mode] = gs.astype(np.float64).mean(-1).tolist()
        out["share"][mode] = [[float(np.mean(groups[row] == g)) for g in range(G)] for row in bi]
        out["top_scores"][mode] = gs.astype(np.float64).tolist()
        out["top_indices"][mode] = gi.astype(np.int64).tolist()
    return out


@torch.no_grad()
def evaluate(image_feats: torch.Tensor, groups, prompt_embeds: torch.Tensor, components: torch.Tensor, k: int = 10,
             explained_variance_ratio=()) -> Dict:
    """The bias evaluation of the projected image features image_feats [N][D] (unnormalised, as the reference drops the direction from them)
    with group labels groups [N] in [0, G), for the L2-normalised prompt embeddings prompt_embeds [Q][D]: the dict of assemble(), with
    prior[g] = mean over group g of the first component's coefficient. Every argument is checked before any launch."""
    k = int(k)
    x = _check_rows("debias.evaluate", "image_feats", image_feats)
    q = _check_rows("debias.evaluate", "prompt_embeds", prompt_embeds)
    v = _check_components("debias.evaluate", components, x.shape[1])
    if q.shape[1] != x.shape[1]:
        raise ValueError(f"debias.evaluate: the prompts have {q.shape[1]} features, the images {x.shape[1]}")
    if not (x.device == q.device == v.device):
        raise ValueError("debias.evaluate: image_feats, prompt_embeds and components must be on the same device")
    g, G = check_groups(groups, x.shape[0], k)
    xn, xd, coef = remove(x, v)
    rows = [torch.from_numpy(np.flatnonzero(g == c)).to(x.device) for c in range(G)]
    lists = {}
    for mode, bank in zip(MODES, (xn, xd)):
        gs, gi = [], []
        for idx in rows:
            s, i = knn.topk(q, bank[idx], k)
            gs.append(s.cpu().numpy())
            gi.append(idx.cpu().numpy()[i.cpu().numpy()])
        lists[mode] = (np.stack(gs, 1), np.stack(gi, 1), knn.topk(q, bank, k)[1].cpu().numpy())
    c0 = coef[:, 0].cpu().numpy().astype(np.float64)
    return assemble(g, G, k, lists, [c0[g == c].mean() for c in range(G)], explained_variance_ratio)
