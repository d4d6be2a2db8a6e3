"""Logistic-regression probe on frozen features: the linear-probe number as CLIP and most later work report it, a multinomial logistic
regression fitted to convergence on cached features with its L2 strength chosen on a held-out part of the training split, on the HIP kernels.

P problems (costs, folds) share one feature matrix and are ONE batched Newton-CG solve, as svm.fit_squared_hinge: every CG iteration is two
exact-f32 GEMMs over all problems at once (clite_gemm_nt / clite_gemm_tn) plus the row kernels of csrc/logreg_ops.hip. Objective of problem p:
    f_p(W) = 1/2 |W|_F^2 + c_p sum_i w_ip (logsumexp(W x~_i) - (W x~_i)[y_i]),   W in R^{C x Dp},  x~_i = (x_i, 1, 0...), Dp = ceil8(D + 1)
This is sklearn's LogisticRegression(C=c_p, penalty="l2", fit_intercept=False) on the augmented features (svm.augment) with sample_weight =
w[:, p]: the bias is the last weight and IS regularised, as in svm.py. sklearn's default (fit_intercept=True) leaves the intercept unpenalised;
that objective is not solved here. w_ip >= 0 is a per-row, per-problem weight; 0 holds a row out, which is how folds are expressed.
f_p is 1-strongly convex: its optimum is unique and |W - W*|_F <= |grad f_p(W)|. Stopping rule: |grad f_p(W)| <= tol |grad f_p(0)|.
There is no CPU path.
"""
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import hip, newton_cg
from .svm import _ceil8, augment
from .utils.common import logger

DEFAULT_COSTS = (1.0, 10.0, 100.0, 1000.0)
_ROW_OPERANDS = 3                                   # Z, Pr and one scratch shared by S, Q and delta
_LS_EVALS = 8                                       # line-search evaluations enqueued per Newton iteration (a finished search skips the rest)


def _check_shape(name: str, x) -> None:
    if not torch.is_tensor(x) or x.dim() != 2 or x.dtype != torch.float32:
        raise ValueError(f"logreg: {name} must be f32 [rows][D], got {getattr(x, 'dtype', type(x))} {tuple(getattr(x, 'shape', ()))}")
    if x.shape[0] == 0 or x.shape[1] == 0:
        raise ValueError(f"logreg: {name} needs at least one row and one feature, got {tuple(x.shape)}")


def _check_features(name: str, x: torch.Tensor) -> torch.Tensor:
    _check_shape(name, x)
    if not x.is_cuda:
        raise RuntimeError(f"logreg: {name} must be a GPU tensor; the solver's kernels run on the MI355X only, there is no CPU path")
    if not bool(torch.isfinite(x).all()):
        raise ValueError(f"logreg: {name} holds non-finite values")
    return x.contiguous()


def _check_labels(y, N: int, num_classes: int) -> torch.Tensor:
    labels = torch.as_tensor(y).reshape(-1).cpu()
    if labels.is_floating_point() or labels.dtype == torch.bool or labels.numel() == 0:
        raise ValueError("logreg: labels must be a non-empty integer vector")
    if labels.numel() != N:
        raise ValueError(f"logreg: {labels.numel()} labels for {N} rows")
    if int(labels.min()) < 0 or int(labels.max()) >= num_classes:
        raise ValueError(f"logreg: label outside [0, {num_classes})")
    return labels.to(torch.int64)


def _check_costs(costs) -> np.ndarray:
    c = np.asarray(list(costs), np.float64).reshape(-1)
    if c.size == 0 or not np.all(np.isfinite(c)) or np.any(c <= 0):
        raise ValueError(f"logreg: costs must be positive and finite, got {c.tolist()}")
    return c


def _check_weights(weights, N: int, P: int) -> Optional[np.ndarray]:
    """float32 [N][P] on the host (None stays None: every row weighs 1)."""
    if weights is None:
        return None
    w = torch.as_tensor(weights).detach().cpu().to(torch.float32).numpy()
    if w.shape != (N, P):
        raise ValueError(f"logreg: weights must be [N][P] = [{N}][{P}], got {list(w.shape)}")
    if not np.all(np.isfinite(w)) or np.any(w < 0):
        raise ValueError("logreg: weights must be non-negative and finite")
    return np.ascontiguousarray(w)


def _check_classes_present(labels: np.ndarray, w: Optional[np.ndarray], num_classes: int, P: int) -> None:
    for p in range(P):
        rows = labels if w is None else labels[w[:, p] > 0]
        missing = np.flatnonzero(np.bincount(rows, minlength=num_classes) == 0)
        if missing.size:
            raise ValueError(f"logreg: class {int(missing[0])} has no weighted row in problem {p}")


def problem_groups(N: int, num_classes: int, P: int, max_workspace_bytes: Optional[int]):
    """Consecutive groups [(first, count)] of problems whose row operands (Z, Pr and one scratch, f32 [N][count * Cp] each) fit the bound;
    one group when there is none. At ImageNet scale one [N][P * Cp] array with 8 problems is 41 GB."""
    if max_workspace_bytes is None:
        return [(0, P)]
    per = _ROW_OPERANDS * 4 * N * _ceil8(num_classes)
    g = int(max_workspace_bytes) // per
    if g < 1:
        raise ValueError(f"logreg: max_workspace_bytes = {max_workspace_bytes} is below the {per} bytes the row operands of one problem need")
    return [(p0, min(g, P - p0)) for p0 in range(0, P, g)]


GEMM_OPERAND_BYTES = 0xF0000000 - 1                 # clite_gemm_*: every operand stays below this many bytes (32-bit buffer offsets)


def _row_chunk(rows: int, ld: int) -> int:
    """Rows per GEMM call so that an operand of row length ld floats stays inside GEMM_OPERAND_BYTES: all rows, or a multiple of 8."""
    fit = GEMM_OPERAND_BYTES // (4 * ld) // 8 * 8
    if fit < 8:
        raise ValueError(f"logreg: a row of {ld} floats does not fit a GEMM operand")
    return min(rows, fit)


def _nt(A, B, M, N, K, out):
    """out [M][N] = A B^T with A [M][K], B [N][K] (f32), the rows of A and out in chunks that fit a GEMM operand (at ImageNet scale the
    features are 10.5 GB and one row operand 20.5 GB)."""
    step = _row_chunk(M, max(K, out.shape[1]))
    for r in range(0, M, step):
        m = min(step, M - r)
        hip.gemm_nt(hip.F32, A[r:r + m], B, m, N, K, hip.epilogue(out[r:r + m], out.shape[1], out_f32=True))


def _tn(A, B, M, N, K, out, residual):
    """out [M][N] = A^T B + residual with A [K][M], B [K][N] (f32). The K rows go in chunks that fit a GEMM operand, each chunk's product added
    to the sum so far through the residual epilogue, in chunk order (one fixed order of summation); two buffers alternate so that no call reads
    the tensor it writes, and the last chunk lands in out."""
    step = _row_chunk(K, max(A.shape[1], B.shape[1]))
    starts = list(range(0, K, step))
    spare = torch.empty_like(out) if len(starts) > 1 else None
    for i, r in enumerate(starts):
        k = min(step, K - r)
        dst = out if (len(starts) - 1 - i) % 2 == 0 else spare
        hip.gemm_tn(hip.F32, A[r:r + k], B[r:r + k], M, N, k, hip.epilogue(dst, dst.shape[1], out_f32=True, residual=residual))
        residual = dst


def _solve_group(Xt, y32, costs, w, C, W, tol, max_newton, max_cg, eta_max, warm):
    """Newton-CG on the problems of one group. Xt [N][Dp]; costs f32 [P]; w f32 [N][P]; W f32 [P * Cp][Dp], the start and the result."""
    N, Dp = Xt.shape
    P = costs.numel()
    Cp = _ceil8(C)
    ldz, n = P * Cp, Cp * Dp
    dev = Xt.device
    vec = lambda: torch.zeros(P * Cp, Dp, device=dev, dtype=torch.float32)      # noqa: E731
    G, Xd, R, Dc, HD = vec(), vec(), vec(), vec(), vec()
    Z, Pr, T = (torch.zeros(N, ldz, device=dev, dtype=torch.float32) for _ in range(_ROW_OPERANDS))     # T: S, then Q, then delta
    loss = torch.zeros(P, device=dev, dtype=torch.float32)
    work = torch.zeros(2 * hip.logreg_blocks(N) * P, device=dev, dtype=torch.float32)
    state = torch.zeros(P, hip.LOGREG_STATE, device=dev, dtype=torch.float32)
    state[:, hip.NCG_ACTIVE] = 1.0

    def grad(Wc):
        _nt(Xt, Wc, N, ldz, Dp, Z)                                      # z = X~ W^T
        hip.logreg_softmax(Z, y32, costs, w, N, P, C, ldz, Pr, T, loss, work)
        _tn(T, Xt, ldz, Dp, N, G, Wc)                                   # g = W + S^T X~

    def hess_vec():
        _nt(Xt, Dc, N, ldz, Dp, T)                                      # q = X~ d^T
        hip.logreg_hess_apply(Pr, costs, w, N, P, C, ldz, T)
        _tn(T, Xt, ldz, Dp, N, HD, Dc)                                  # Hd = d + Q^T X~

    def line_search():
        _nt(Xt, Xd, N, ldz, Dp, T)                                      # delta = X~ x^T
        hip.logreg_line_search(Z, T, y32, costs, w, N, P, C, ldz, G, W, Xd, n, n, state, work, _LS_EVALS)

    if warm:                                                            # |grad f(0)| of the stopping rule, which a warm start does not pass through
        grad(HD)                                                        # HD is still zero
        hip.logreg_newton_begin(G, n, n, P, Xd, R, Dc, state, tol, max_newton, eta_max, g0_only=True)
    launched = newton_cg.solve(state, lambda: hip.logreg_newton_begin(G, n, n, P, Xd, R, Dc, state, tol, max_newton, eta_max),
                               lambda: hip.logreg_cg_update(HD, n, n, P, Xd, R, Dc, state), lambda: grad(W), hess_vec, line_search,
                               max_newton, max_cg, first_cap=min(max_cg, 10))      # eta = 0.1 in the first solve: ten iterations, or a descent direction anyway
    return state.cpu(), loss.cpu(), launched


@torch.no_grad()
def fit(X: torch.Tensor, y, num_classes: int, costs: Sequence[float], weights=None, W0=None, tol: float = 1e-5, max_newton: int = 50,
        max_cg: int = 100, max_workspace_bytes: Optional[int] = None, eta_max: float = 0.1) -> Dict[str, object]:
    """Solve P = len(costs) problems over one feature matrix. X: f32 [N][D] on the device; y: int [N] in [0, num_classes); weights: [N][P] per-row
    weights w_ip >= 0 (0 holds a row out; None: all 1). Returns {"W": f32 [P][C][D], "b": f32 [P][C], "newton": int [P] Newton iterations,
    "cg": int [P] CG iterations, "rel_grad": [P] final |grad f| / |grad f(0)|, "loss": [P] the data term of f_p at the last gradient evaluation,
    "cg_launched": CG iterations enqueued}.

    Each Newton iteration recomputes Z = X~ W^T (one GEMM), the softmax operand and the gradient (one GEMM), then runs a truncated CG solve on all
    still-active problems with no host synchronisation (2 GEMMs per CG iteration), then one GEMM for delta = X~ D^T and the line search. The CG
    loop length of a Newton iteration is min(max_cg, max(10, 2 x the most CG iterations any problem used in the previous one)), 10 in the first
    (every enqueued iteration pays its two GEMMs, used or not). One read-back of
    the state table per Newton iteration decides whether to go on. A problem whose line search ends at step 0 (no descent direction, or no point
    left of the minimiser within the evaluations) stops there, with its rel_grad above tol, instead of repeating the iteration. W0 = (W [P][C][D], b [P][C]) warm-starts the solve: a solution handed back in
    returns unchanged with 0 Newton iterations. max_workspace_bytes bounds the three [N][P' * Cp] row operands: consecutive groups of P' problems
    that fit are solved one after another. A class without a weighted row in some problem is refused (its weights would only shrink to zero)."""
    num_classes = int(num_classes)
    if not 2 <= num_classes <= hip.LOGREG_MAX_CLASSES:
        raise ValueError(f"logreg.fit: num_classes must be in [2, {hip.LOGREG_MAX_CLASSES}] (a softmax group lives in registers), got {num_classes}")
    _check_shape("X", X)
    c = _check_costs(costs)
    P, N = c.size, X.shape[0]
    labels = _check_labels(y, N, num_classes)
    wh = _check_weights(weights, N, P)
    if not tol > 0 or max_newton < 0 or max_cg < 1:
        raise ValueError("logreg.fit: tol must be positive, max_newton >= 0, max_cg >= 1")
    _check_classes_present(labels.numpy(), wh, num_classes, P)
    D = X.shape[1]
    Dp, Cp = _ceil8(D + 1), _ceil8(num_classes)
    if Cp * Dp >= 2 ** 31:
        raise ValueError("logreg.fit: a problem's weight vector exceeds an int32 index")
    groups = problem_groups(N, num_classes, P, max_workspace_bytes)
    X = _check_features("X", X)
    dev = X.device
    Wall = torch.zeros(P, Cp, Dp, device=dev, dtype=torch.float32)
    if W0 is not None:
        w0, b0 = W0
        if tuple(w0.shape) != (P, num_classes, D) or tuple(b0.shape) != (P, num_classes):
            raise ValueError(f"logreg.fit: W0 must be (W [{P}][{num_classes}][{D}], b [{P}][{num_classes}])")
        Wall[:, :num_classes, :D] = w0.to(device=dev, dtype=torch.float32)
        Wall[:, :num_classes, D] = b0.to(device=dev, dtype=torch.float32)
    Xt = augment(X)
    y32 = labels.to(device=dev, dtype=torch.int32)
    wd = torch.ones(N, P, device=dev, dtype=torch.float32) if wh is None else torch.from_numpy(wh).to(dev)
    cd = torch.from_numpy(c.astype(np.float32)).to(dev)
    newton, cg, rel, loss = (torch.zeros(P, dtype=t) for t in (torch.int64, torch.int64, torch.float32, torch.float32))
    launched = 0
    split = hip.is_f32_split()
    if split:
        hip.set_f32_split(False)           # exact f32 products only: the certificate |grad| <= tol |grad(0)| is about the f32 gradient
    try:
        for p0, g in groups:
            Wg = Wall[p0:p0 + g].reshape(g * Cp, Dp)                    # a view: the group's result lands in Wall
            st, ls, la = _solve_group(Xt, y32, cd[p0:p0 + g].contiguous(), wd[:, p0:p0 + g].contiguous(), num_classes, Wg, float(tol),
                                      int(max_newton), int(max_cg), float(eta_max), W0 is not None)
            newton[p0:p0 + g] = st[:, hip.NCG_NEWTON].to(torch.int64)
            cg[p0:p0 + g] = st[:, hip.NCG_CGTOT].to(torch.int64)
            rel[p0:p0 + g] = st[:, hip.NCG_REL]
            loss[p0:p0 + g] = ls
            launched += la
    finally:
        if split:
            hip.set_f32_split(True)
    return {"W": Wall[:, :num_classes, :D].clone(), "b": Wall[:, :num_classes, D].clone(), "newton": newton, "cg": cg, "rel_grad": rel,
            "loss": loss, "cg_launched": launched}


@torch.no_grad()
def predict_logits(X: torch.Tensor, W: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """logits f32 [N][C] = X W^T + b for one problem (W [C][D], b [C]), as one exact-f32 clite_gemm_nt over the augmented features. The result
    is a view of a [N][ceil8(C)] buffer (what clite_xent_fwd wants)."""
    X = _check_features("X", X)
    if W.dim() != 2 or W.shape[1] != X.shape[1] or tuple(b.shape) != (W.shape[0],):
        raise ValueError(f"logreg.predict_logits: W [C][{X.shape[1]}] and b [C], got {tuple(W.shape)} and {tuple(b.shape)}")
    N, D = X.shape
    C = W.shape[0]
    Dp, Cp = _ceil8(D + 1), _ceil8(C)
    Wt = torch.zeros(Cp, Dp, device=X.device, dtype=torch.float32)
    Wt[:C, :D] = W
    Wt[:C, D] = b
    out = torch.empty(N, Cp, device=X.device, dtype=torch.float32)
    split = hip.is_f32_split()
    if split:
        hip.set_f32_split(False)
    try:
        _nt(augment(X), Wt, N, Cp, Dp, out)
    finally:
        if split:
            hip.set_f32_split(True)
    return out[:, :C]


@torch.no_grad()
def accuracy(logits: torch.Tensor, labels, topk: int = 5) -> Dict[str, float]:
    """{"top1", "top<topk>"} in percent from clite_xent_fwd's counters (rank = #{j: z_j > z_y} + #{j < y: z_j == z_y}: ties go to the lower
    class); the top-k entry only when there are at least topk classes."""
    if logits.dim() != 2 or logits.dtype != torch.float32 or not logits.is_cuda:
        raise ValueError("logreg.accuracy: logits must be f32 [N][C] on the GPU")
    N, C = logits.shape
    y = _check_labels(labels, N, C).to(logits.device)
    Cp = _ceil8(C)
    z = logits
    if z.stride(1) != 1 or z.stride(0) % 4 or z.data_ptr() % 16:
        z = torch.zeros(N, Cp, device=logits.device, dtype=torch.float32)
        z[:, :C] = logits
    lse = torch.empty(N, device=z.device, dtype=torch.float32)
    acc = torch.zeros(4, device=z.device, dtype=torch.float32)
    hip.xent_fwd(z, z.stride(0), N, C, y, int(topk), lse, acc)
    a = acc.tolist()
    out = {"top1": 100.0 * a[1] / N}
    if C >= topk:
        out[f"top{int(topk)}"] = 100.0 * a[2] / N
    return out


def holdout_weights(y, fraction: float) -> Tuple[np.ndarray, np.ndarray]:
    """(weights f32 [N], held-out mask bool [N]): the last `fraction` of every class's rows, in dataset order and at least one row per class, get
    weight 0; the others 1. A class of one row is held out whole (fit then refuses it by name)."""
    y = np.asarray(torch.as_tensor(y).cpu().numpy() if torch.is_tensor(y) else y).reshape(-1)
    if not 0 < fraction < 1:
        raise ValueError(f"logreg.holdout_weights: fraction must be in (0, 1), got {fraction}")
    held = np.zeros(len(y), bool)
    for k in np.unique(y):
        rows = np.flatnonzero(y == k)
        n = max(1, int(np.floor(len(rows) * fraction + 1e-9)))        # 100 * 0.29 is 28.999999999999996 in binary: the count of exact arithmetic
        held[rows[len(rows) - n:]] = True
    return (~held).astype(np.float32), held


def select_cost(holdout_top1: Sequence[float], costs: Sequence[float]) -> int:
    """Index of the cost with the best hold-out top-1; among equal accuracies the smaller cost (the stronger regularisation)."""
    best = -1
    for j in range(len(costs)):
        if best < 0 or holdout_top1[j] > holdout_top1[best] or (holdout_top1[j] == holdout_top1[best] and costs[j] < costs[best]):
            best = j
    return best


@torch.no_grad()
def logreg_eval(train_feats: torch.Tensor, train_labels, val_feats: torch.Tensor, val_labels, num_classes: int,
                costs: Sequence[float] = DEFAULT_COSTS, holdout: float = 0.1, tol: float = 1e-5, max_newton: int = 50,
                max_workspace_bytes: Optional[int] = None) -> Dict[str, object]:
    """The probe protocol: (1) every cost solved in one batched fit with the hold-out rows (holdout_weights) weighted 0, the cost with the best
    hold-out top-1 chosen (select_cost); (2) that cost refitted on all rows, warm-started from its selection fit, and its top-1 / top-5 on the
    validation features reported. Returns {"cost", "cost_index", "top1", "top5" (with at least five classes), "holdout_top1": {cost: top-1},
    "newton": selection and refit Newton iterations, "rel_grad"}."""
    c = _check_costs(costs)
    P = c.size
    ytr = _check_labels(train_labels, train_feats.shape[0], int(num_classes))
    w1, held = holdout_weights(ytr.numpy(), holdout)
    sel = fit(train_feats, ytr, num_classes, c, np.repeat(w1[:, None], P, axis=1), tol=tol, max_newton=max_newton,
              max_workspace_bytes=max_workspace_bytes)
    hf = train_feats[torch.from_numpy(np.flatnonzero(held)).to(train_feats.device)]
    hy = ytr[torch.from_numpy(held)]
    hold = [accuracy(predict_logits(hf, sel["W"][p], sel["b"][p]), hy)["top1"] for p in range(P)]
    j = select_cost(hold, c.tolist())
    logger.info(f"logistic-regression probe: hold-out top-1 {dict(zip(c.tolist(), hold))}, cost {c[j]}")
    full = fit(train_feats, ytr, num_classes, [c[j]], None, W0=(sel["W"][j:j + 1], sel["b"][j:j + 1]), tol=tol, max_newton=max_newton,
               max_workspace_bytes=max_workspace_bytes)
    acc = accuracy(predict_logits(val_feats, full["W"][0], full["b"][0]), val_labels, 5)
    res = {"cost": float(c[j]), "cost_index": j, "top1": acc["top1"], "holdout_top1": {float(k): v for k, v in zip(c.tolist(), hold)},
           "newton": (sel["newton"].tolist(), full["newton"].tolist()), "rel_grad": (sel["rel_grad"].tolist(), full["rel_grad"].tolist())}
    if "top5" in acc:
        res["top5"] = acc["top5"]
    return res
