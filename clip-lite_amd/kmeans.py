"""k-means of caption embeddings on the GPU, the clustering behind clustered negative sampling (reference scripts/cluster.py:131-150:
`faiss.Kmeans(d, k, niter=200, gpu=n).train(x)` followed by `kmeans.index.search(x, 1)`).

Lloyd's algorithm, everything on the device. One iteration is

    scores = X C^T              clite_gemm_nt in its exact-f32 form (K padded to the GEMM's column granularity, as retrieval.similarity does);
                                an assignment decided by a bf16 product would not be k-means of the input
    assign                      clite_kmeans_assign: argmin_k 0.5 |c_k|^2 - score, ties to the lower k; squared distance; changed-row count
    accumulate, update          clite_kmeans_accumulate / _update: rows grouped by cluster, summed in a fixed order, c_k = sum_k / count_k

with one host synchronisation (the changed-row count and the cluster sizes). No float atomics take part, so two runs give bit-identical
centroids, in both settings of `hip.set_deterministic`.

Empty clusters follow scikit-learn's relocation rule, which has no random component: after an assignment the empty clusters are served in
ascending k, and each takes the not-yet-taken row with the largest squared distance to its assigned centroid (ties to the lower row); that
row leaves its old cluster. The rule runs on the host from the distance vector (it is rare). A cluster that the departure of a relocated row
leaves empty keeps its centroid for that iteration.

Deliberate deviations from `faiss.Kmeans`:
  * all points take part in training (faiss subsamples to 256 K points: 2 560 of 118 k at K = 10);
  * no random perturbation: an empty cluster is refilled by the rule above, not by splitting a large cluster with a perturbed copy;
  * the iteration stops early when no assignment changed: a fixed point, identical to running all `niter` iterations;
  * the initial centroids are K distinct rows chosen by a seeded torch permutation, not faiss's own generator.
"""
from typing import Dict, Optional

import numpy as np
import torch

from . import hip


def init_rows(N: int, K: int, seed: int = 1234) -> torch.Tensor:
    """Row indices of the K initial centroids: the head of a `torch.Generator(seed)` permutation of N (host)."""
    return torch.randperm(N, generator=torch.Generator().manual_seed(int(seed)))[:K]


def relocate(assign: np.ndarray, dist: np.ndarray, counts: np.ndarray) -> np.ndarray:
    """The empty-cluster rule on the host: the i-th empty cluster (ascending k) takes the row with the i-th largest dist (ties to the lower
    row). Returns the new assignment; `assign` is not modified."""
    empty = np.flatnonzero(np.asarray(counts) == 0)
    out = np.array(assign, copy=True)
    if empty.size:
        far = np.argsort(-np.asarray(dist), kind="stable")[:empty.size]
        out[far] = empty.astype(out.dtype)
    return out


class _State:
    """Device buffers of one fit: allocated once, reused by every iteration."""

    def __init__(self, X: torch.Tensor, K: int):
        N, D = X.shape
        dev = X.device
        self.N, self.D, self.K, self.Kp, self.ld = N, D, K, (K + 7) // 8 * 8, X.stride(0)
        self.X = X
        self.C = torch.zeros(self.Kp, D, device=dev, dtype=torch.float32)        # rows >= K stay zero: padding columns of the scores
        self.hc = torch.empty(K, device=dev, dtype=torch.float32)
        self.xnorm = torch.empty(N, device=dev, dtype=torch.float32)
        self.scores = torch.empty(N, self.Kp, device=dev, dtype=torch.float32)
        self.assign = torch.full((N,), -1, device=dev, dtype=torch.int32)
        self.dist = torch.empty(N, device=dev, dtype=torch.float32)
        # what the host reads once per iteration, in one buffer: counts [K], the changed-row counter, (padding to 8 bytes,) the inertia (a double)
        self._ioff = (K + 2) // 2 * 2
        self.stat = torch.zeros(self._ioff + 2, device=dev, dtype=torch.int32)
        self.inertia = self.stat[self._ioff:].view(torch.float64)
        self.work = torch.empty(hip.kmeans_work_bytes(N, D, K), device=dev, dtype=torch.uint8)
        hip.kmeans_row_norms(X, self.ld, N, D, 1.0, self.xnorm)

    def set_centroids(self, C0: torch.Tensor):
        self.C[:self.K].copy_(C0)
        hip.kmeans_row_norms(self.C, self.D, self.K, self.D, 0.5, self.hc)

    def assign_step(self):
        self.stat[self.K:self.K + 1].zero_()
        hip.gemm_nt(hip.F32, self.X, self.C, self.N, self.Kp, self.D, hip.epilogue(self.scores, self.Kp, out_f32=True), lda=self.ld)
        hip.kmeans_assign(self.scores, self.Kp, self.hc, self.xnorm, self.N, self.K, self.assign, self.dist, self.stat[self.K:self.K + 1])

    def accumulate(self):
        hip.kmeans_accumulate(self.X, self.ld, self.assign, self.dist, self.N, self.D, self.K, self.stat, self.inertia, self.work)

    def read(self):
        """(counts int32 [K], changed rows, inertia) on the host: one device-to-host copy, the iteration's one synchronisation."""
        host = self.stat.cpu()
        return host[:self.K], int(host[self.K]), float(host[self._ioff:].view(torch.float64))

    def update(self):
        hip.kmeans_update(self.work, self.stat, self.N, self.D, self.K, self.C, self.D, self.hc)


@torch.no_grad()
def fit(X: torch.Tensor, K: int, niter: int = 200, seed: int = 1234, init: Optional[torch.Tensor] = None) -> Dict[str, object]:
    """Lloyd's k-means of the rows of X (f32 [N][D] on the GPU, D % 8 == 0, unit row stride; a row stride > D is read in place), 2 <= K <= 1024.

    init: f32 [K][D] initial centroids, or None for the rows `init_rows(N, K, seed)`. At most `niter` iterations (assignment + update); the loop
    ends early at a fixed point. Returns centroids f32 [K][D], assign int32 [N], counts int32 [K] (all on X's device), inertia (sum of squared
    distances of that assignment to those centroids), iterations (assignment steps of the loop) and history (inertia after every assignment
    step of the loop, before any relocation)."""
    if X.dim() != 2 or X.dtype != torch.float32:
        raise ValueError(f"kmeans.fit: X must be f32 [N][D], got {X.dtype} {tuple(X.shape)}")
    N, D = X.shape
    K, niter = int(K), int(niter)
    if D % 8 or D == 0:
        raise ValueError(f"kmeans.fit: D must be a positive multiple of 8, got {D}")
    if not 2 <= K <= hip.KMEANS_MAX_K or N < K:
        raise ValueError(f"kmeans.fit: need 2 <= K <= {hip.KMEANS_MAX_K} and N >= K, got K = {K}, N = {N}")
    if niter < 1:
        raise ValueError("kmeans.fit: niter must be at least 1")
    if not X.is_cuda:
        raise RuntimeError("kmeans.fit: X must be a GPU tensor; the k-means kernels run on the MI355X only")
    if X.stride(1) != 1 or X.stride(0) < D:
        X = X.contiguous()
    if init is None:
        C0 = X[init_rows(N, K, seed).to(X.device)]
    else:
        if tuple(init.shape) != (K, D):
            raise ValueError(f"kmeans.fit: init must be [{K}][{D}], got {tuple(init.shape)}")
        C0 = init.to(device=X.device, dtype=torch.float32)
    split = hip.is_f32_split()
    if split:
        hip.set_f32_split(False)         # exact f32 products only
    try:
        st = _State(X, K)
        st.set_centroids(C0)
        history = []
        converged = False
        for _ in range(niter):
            st.assign_step()
            st.accumulate()
            st.update()                  # speculative: at a fixed point it rewrites the same bits, and a relocation below redoes it
            counts, changed, inertia = st.read()         # the iteration's one synchronisation
            history.append(inertia)
            if changed == 0:
                converged = True
                break
            if bool((counts == 0).any()):
                new = relocate(st.assign.cpu().numpy(), st.dist.cpu().numpy(), counts.numpy())
                st.assign.copy_(torch.from_numpy(new))
                st.accumulate()
                st.update()
        if not converged:                # the reference's index.search against the final centroids
            st.assign_step()
            st.accumulate()
        counts, _, inertia = st.read()
    finally:
        if split:
            hip.set_f32_split(True)
    return {"centroids": st.C[:K].clone(), "assign": st.assign, "counts": st.stat[:K].clone(), "inertia": inertia,
            "iterations": len(history), "history": history}
