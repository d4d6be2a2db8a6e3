"""VOC2007 one-vs-all linear-SVM evaluation (reference voc_clf.py:75-121, `train_test_single_svm`) on the HIP kernels.

The reference fits 20 classes x 4 costs x (3 cross-validation folds + 1 full fit) = 320 sklearn LinearSVC problems in a CPU pool. They share one
feature matrix and differ only in labels and per-row weights, so here they are ONE batched problem: every Newton-CG iteration is a few f32
GEMMs over all problems at once (clite_gemm_nt / clite_gemm_tn) plus the per-problem kernels of csrc/svm_ops.hip.

Objective of problem p (LinearSVC penalty="l2", loss="squared_hinge", intercept_scaling=1: the bias is the last weight and is regularised):
    f_p(w) = 1/2 |w|^2 + sum_i c_ip max(0, 1 - y_ip w.x~_i)^2,     x~_i = (x_i, 1, 0...) of length Dp = ceil8(D + 1)
It is strictly convex; the solver targets its optimum (not sklearn's iterate at max_iter). Stopping rule: |grad f_p(w)| <= tol |grad f_p(0)|.
"""
from typing import Dict, Sequence

import numpy as np
import torch

from . import hip, newton_cg

SVM_COSTS = (0.01, 0.1, 1.0, 10.0)                  # reference voc_clf.py:83
CLASS_WEIGHT = {1: 2.0, -1: 1.0}                    # reference voc_clf.py:97 class_weight={1: 2, -1: 1}


def _ceil8(n: int) -> int:
    return (n + 7) // 8 * 8


def augment(X: torch.Tensor) -> torch.Tensor:
    """f32 [N][D] -> X~ f32 [N][Dp]: the features, a constant 1 (the bias column), zeros up to Dp = ceil8(D + 1)."""
    N, D = X.shape
    Xt = torch.zeros(N, _ceil8(D + 1), device=X.device, dtype=torch.float32)
    Xt[:, :D] = X
    Xt[:, D] = 1.0
    return Xt


def _nt(A, B, M, N, K, out):
    hip.gemm_nt(hip.F32, A, B, M, N, K, hip.epilogue(out, out.shape[1], out_f32=True))


def _tn(A, B, M, N, K, out, residual):
    """out [M][N] = 2 A^T B + residual with A [K][M], B [K][N] (f32)."""
    hip.gemm_tn(hip.F32, A, B, M, N, K, hip.epilogue(out, out.shape[1], out_f32=True, alpha=2.0, residual=residual))


@torch.no_grad()
def fit_squared_hinge(X: torch.Tensor, Y: torch.Tensor, Cw: torch.Tensor, tol: float = 1e-5, max_newton: int = 30, max_cg: int = 100,
                      eta_max: float = 0.1) -> Dict[str, torch.Tensor]:
    """Solve P problems over one feature matrix. X: f32 [N][D] on the device; Y: +-1 [N][P]; Cw: f32 [N][P] per-row weights c_ip >= 0 (0 holds
    a row out). Returns {"W": [P][D], "b": [P], "newton": int [P] Newton iterations, "rel_grad": [P] final |grad f| / |grad f(0)|,
    "cg": int [P] CG iterations, "cg_launched": total CG iterations enqueued (all problems advance together)}.

    Each Newton iteration recomputes z = X~ w (one GEMM), the gradient (one GEMM), then runs a truncated CG solve on all still-active problems
    with no host synchronisation (2 GEMMs per CG iteration), then one GEMM for delta = X~ d and an exact line search. The CG loop length of a
    Newton iteration is min(max_cg, max(10, 2 x the most CG iterations any problem used in the previous one)); a solve that hits it still
    gives a descent direction. One read-back of the per-problem state per Newton iteration decides whether to go on."""
    if X.dim() != 2 or not X.is_cuda or X.dtype != torch.float32:
        raise ValueError("fit_squared_hinge: X must be an f32 [N][D] device tensor")
    N, D = X.shape
    P = Y.shape[1]
    if Y.shape != (N, P) or Cw.shape != (N, P):
        raise ValueError(f"fit_squared_hinge: Y and Cw must be [N][P] = [{N}][{P}]")
    dev = X.device
    Dp, ldp = _ceil8(D + 1), _ceil8(P)
    Xt = augment(X.contiguous())

    def cols(t):
        o = torch.zeros(N, ldp, device=dev, dtype=torch.float32)
        o[:, :P] = t.to(device=dev, dtype=torch.float32)
        return o

    Yp, Cp = cols(Y), cols(Cw)
    rows = lambda: torch.zeros(ldp, Dp, device=dev, dtype=torch.float32)      # noqa: E731
    W, G, Xd, R, Dc, HD = rows(), rows(), rows(), rows(), rows(), rows()
    Z, S, H, Q = (torch.zeros(N, ldp, device=dev, dtype=torch.float32) for _ in range(4))
    loss = torch.zeros(P, device=dev, dtype=torch.float32)
    work = torch.zeros((N + 511) // 512, ldp, device=dev, dtype=torch.float32)
    state = torch.zeros(P, hip.SVM_STATE, device=dev, dtype=torch.float32)
    state[:, hip.NCG_ACTIVE] = 1.0

    def grad():
        _nt(Xt, W, N, ldp, Dp, Z)                                   # z = X~ w
        hip.svm_margin(Z, Yp, Cp, N, P, ldp, S, H, loss, work)
        _tn(S, Xt, ldp, Dp, N, G, W)                                # g = w + 2 X~^T (c 1_I (z - y))

    def hess_vec():
        _nt(Xt, Dc, N, ldp, Dp, Q)                                  # q = X~ d
        hip.svm_hess_scale(H, Q)                                    # q *= c 1_I
        _tn(Q, Xt, ldp, Dp, N, HD, Dc)                              # Hd = d + 2 X~^T q

    def line_search():
        _nt(Xt, Xd, N, ldp, Dp, Q)                                  # delta = X~ x
        hip.svm_line_search(Z, Q, Yp, Cp, N, P, ldp, W, Xd, Dp, Dp, state)

    launched = newton_cg.solve(state, lambda: hip.svm_newton_begin(G, Dp, Dp, P, Xd, R, Dc, state, tol, max_newton, eta_max),
                               lambda: hip.svm_cg_update(HD, Dp, Dp, P, Xd, R, Dc, state), grad, hess_vec, line_search,
                               max_newton, max_cg, first_cap=max_cg)
    st = state.cpu()
    return {"W": W[:P, :D].clone(), "b": W[:P, D].clone(), "newton": st[:, hip.NCG_NEWTON].to(torch.int64),
            "rel_grad": st[:, hip.NCG_REL].clone(), "cg": st[:, hip.NCG_CGTOT].to(torch.int64), "cg_launched": launched}


@torch.no_grad()
def decision_function(X: torch.Tensor, W: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """scores f32 [N][P] = X W^T + b (LinearSVC.decision_function), as one f32 clite_gemm_nt over the augmented features."""
    N, D = X.shape
    P = W.shape[0]
    Dp, ldp = _ceil8(D + 1), _ceil8(P)
    Wt = torch.zeros(ldp, Dp, device=X.device, dtype=torch.float32)
    Wt[:P, :D] = W
    Wt[:P, D] = b
    out = torch.empty(N, ldp, device=X.device, dtype=torch.float32)
    _nt(augment(X.float().contiguous()), Wt, N, ldp, Dp, out)
    return out[:, :P]


@torch.no_grad()
def average_precision(scores: torch.Tensor, targets: torch.Tensor) -> torch.Tensor:
    """Per-column sklearn average_precision_score: scores f32 [N][P] (or [N]), targets [N][P]: > 0 positive, 0 negative, < 0 ignored.
    Returns f32 [P] (0 for a column without positives)."""
    one = scores.dim() == 1
    s = scores.reshape(scores.shape[0], -1).float().contiguous()
    t = targets.reshape(s.shape).to(device=s.device, dtype=torch.float32).contiguous()
    N, P = s.shape
    ap = torch.empty(P, device=s.device, dtype=torch.float32)
    hip.average_precision(s, P, t, P, N, P, ap)
    return ap[0] if one else ap


def stratified_kfold_masks(y, n_splits: int = 3) -> np.ndarray:
    """Test-fold masks bool [n_splits][N] identical to sklearn's StratifiedKFold(n_splits) without shuffling (the folds cross_val_score(cv=3)
    uses for a classifier): classes in order of first appearance, each class's rows (in row order) dealt to folds by the per-fold allocation
    of the label-sorted sequence taken with stride n_splits."""
    y = np.asarray(y).ravel()
    _, y_idx, y_inv = np.unique(y, return_index=True, return_inverse=True)
    _, class_perm = np.unique(y_idx, return_inverse=True)
    y_enc = class_perm[y_inv]
    n_classes = len(y_idx)
    counts = np.bincount(y_enc)
    if n_splits > counts.max():
        raise ValueError(f"n_splits={n_splits} cannot be greater than the number of members in each class")
    y_order = np.sort(y_enc)
    alloc = np.asarray([np.bincount(y_order[i::n_splits], minlength=n_classes) for i in range(n_splits)])
    folds = np.empty(len(y), dtype=np.int64)
    for k in range(n_classes):
        folds[y_enc == k] = np.arange(n_splits).repeat(alloc[:, k])
    return np.stack([folds == i for i in range(n_splits)])


def svm_labels(targets: np.ndarray) -> np.ndarray:
    """VOC targets {1 present, 0 absent, -1 difficult} -> SVM labels: 0 -> -1, and difficult stays -1, i.e. trains as a negative
    (reference voc_clf.py:78-82)."""
    y = np.asarray(targets).copy()
    y[y == 0] = -1
    return y


def voc07_problems(train_targets: np.ndarray, costs: Sequence[float] = SVM_COSTS, n_splits: int = 3):
    """The reference protocol as one problem set. Problem p = (k * n_costs + j) * (n_splits + 1) + f for class k, cost j and f = fold
    (f < n_splits: trained without test fold f) or f = n_splits (the fit on all rows). Returns (Y +-1 [N][P], Cw [N][P], folds [K][n_splits][N])."""
    T = np.asarray(train_targets)
    N, K = T.shape
    F = n_splits + 1
    Y = np.empty((N, K * len(costs) * F), np.float32)
    Cw = np.empty_like(Y)
    folds = np.empty((K, n_splits, N), bool)
    for k in range(K):
        y = svm_labels(T[:, k])
        folds[k] = stratified_kfold_masks(y, n_splits)
        cw = np.where(y > 0, CLASS_WEIGHT[1], CLASS_WEIGHT[-1]).astype(np.float32)
        for j, cost in enumerate(costs):
            for f in range(F):
                p = (k * len(costs) + j) * F + f
                Y[:, p] = y
                Cw[:, p] = np.float32(cost) * cw * (1.0 if f == n_splits else (~folds[k, f]).astype(np.float32))
    return Y, Cw, folds


def select_cost(cv_ap: np.ndarray, costs: Sequence[float] = SVM_COSTS):
    """Reference voc_clf.py:108-113: the first cost whose mean CV AP is strictly greater than the best so far, starting from 0.0.
    cv_ap: [n_costs][n_splits]. Returns (index, mean CV AP); raises when no cost beats 0.0 (where the reference would crash)."""
    best, idx = 0.0, -1
    for j in range(len(costs)):
        m = float(np.mean(np.asarray(cv_ap[j], dtype=np.float64)))
        if m > best:
            best, idx = m, j
    if idx < 0:
        raise RuntimeError("voc07_svm_eval: no SVM cost reached a mean cross-validation AP above 0 (the reference would fail here: it "
                           "keeps no classifier)")
    return idx, best


@torch.no_grad()
def voc07_svm_eval(train_feats: torch.Tensor, train_targets, test_feats: torch.Tensor, test_targets, costs: Sequence[float] = SVM_COSTS,
                   tol: float = 1e-5, max_newton: int = 30) -> Dict[str, object]:
    """Reference `train_test_single_svm` for every class in one batched solve. feats: f32 [N][D] on the device (L2-normalised);
    targets: int [N][K] in {1, 0, -1 (difficult)}. Returns {"cv_ap": [K][n_costs][3], "cv_ap_mean": [K][n_costs], "cost": [K] chosen costs,
    "cost_index": [K], "test_ap": [K], "map": mean test AP (a fraction), "newton": [P], "cg": [P], "rel_grad": [P], "cg_launched": int}."""
    Ttr = np.asarray(train_targets if not torch.is_tensor(train_targets) else train_targets.cpu().numpy()).astype(np.int64)
    Tte = np.asarray(test_targets if not torch.is_tensor(test_targets) else test_targets.cpu().numpy()).astype(np.int64)
    K, nc, F = Ttr.shape[1], len(costs), 4
    dev = train_feats.device
    Y, Cw, folds = voc07_problems(Ttr, costs, F - 1)
    P = Y.shape[1]
    sol = fit_squared_hinge(train_feats.float(), torch.from_numpy(Y).to(dev), torch.from_numpy(Cw).to(dev), tol=tol, max_newton=max_newton)
    # cross-validation AP: each fold problem scored on its held-out rows, AP targets = (label == 1) (cross_val_score, voc_clf.py:101-103)
    tgt = np.full(Y.shape, -1.0, np.float32)
    for k in range(K):
        pos = (svm_labels(Ttr[:, k]) > 0).astype(np.float32)
        for j in range(nc):
            for f in range(F - 1):
                p = (k * nc + j) * F + f
                tgt[folds[k, f], p] = pos[folds[k, f]]
    cv = average_precision(decision_function(train_feats.float(), sol["W"], sol["b"]), torch.from_numpy(tgt).to(dev)).cpu().numpy()
    # test AP of every full fit: difficult rows excluded, targets label > 0 (voc_clf.py:117-127)
    full = [(k * nc + j) * F + F - 1 for k in range(K) for j in range(nc)]
    tt = np.repeat(np.where(Tte == -1, -1.0, (Tte > 0).astype(np.float32)), nc, axis=1).astype(np.float32)
    fi = torch.tensor(full, device=dev)
    test_ap_all = average_precision(decision_function(test_feats.float(), sol["W"][fi], sol["b"][fi]), torch.from_numpy(tt).to(dev)).cpu().numpy()
    cv_ap = np.array([[[cv[(k * nc + j) * F + f] for f in range(F - 1)] for j in range(nc)] for k in range(K)], np.float64)
    choice = [select_cost(cv_ap[k], costs) for k in range(K)]
    idx = np.array([c[0] for c in choice])
    test_ap = np.array([test_ap_all[k * nc + idx[k]] for k in range(K)], np.float64)
    return {"cv_ap": cv_ap, "cv_ap_mean": cv_ap.mean(axis=2), "cost": np.array([costs[i] for i in idx]), "cost_index": idx, "test_ap": test_ap,
            "map": float(torch.tensor(test_ap, dtype=torch.float32).mean().item()), "newton": sol["newton"].numpy(), "cg": sol["cg"].numpy(),
            "rel_grad": sol["rel_grad"].numpy(), "cg_launched": sol["cg_launched"], "problems": P}
