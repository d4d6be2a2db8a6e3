"""float64 NumPy reference of the VOC07 SVM stage (clip-lite_amd/svm.py), so GPU tests need no sklearn. CPU tests pin it to sklearn
(tests/test_svm_host.py).

`solve_primal` is a dense generalised Newton method with an exact line search (Keerthi & DeCoste 2005) on
    f(w) = 1/2 |w|^2 + sum_i c_i max(0, 1 - y_i w.x~_i)^2,  x~_i = (x_i, 1),
i.e. LinearSVC(penalty="l2", loss="squared_hinge", intercept_scaling=1) with per-row weights c_i = C * class_weight(y_i) * [row in the fit].
"""
import numpy as np


def augment64(X):
    X = np.asarray(X, np.float64)
    return np.concatenate([X, np.ones((X.shape[0], 1))], 1)


def objective(X, y, c, w, b):
    """f(w, b) in float64."""
    z = np.asarray(X, np.float64) @ np.asarray(w, np.float64) + float(b)
    m = np.maximum(0.0, 1.0 - y * z)
    return 0.5 * (np.dot(w, w) + b * b) + float(np.sum(c * m * m))


def gradient(X, y, c, w, b):
    """grad f as one vector (w, b) in float64."""
    Xt = augment64(X)
    wt = np.append(np.asarray(w, np.float64), float(b))
    z = Xt @ wt
    act = (y * z < 1.0) & (c > 0)
    return wt + 2.0 * Xt.T @ np.where(act, c * (z - y), 0.0)


def _line_search(z, delta, y, c, wd, dd):
    """argmin_t >= 0 of 1/2 |w + t d|^2 + sum c max(0, 1 - y (z + t delta))^2: Newton on the piecewise linear derivative, bracketed."""
    lo, hi, t = 0.0, np.inf, 1.0
    for _ in range(100):
        zt = z + t * delta
        act = (y * zt < 1.0) & (c > 0)
        g = wd + t * dd + 2.0 * np.sum(np.where(act, c * (zt - y) * delta, 0.0))
        h = dd + 2.0 * np.sum(np.where(act, c * delta * delta, 0.0))
        if g == 0.0:
            return t
        if g < 0:
            lo = t
        else:
            hi = t
        tn = t - g / h
        if not (lo < tn < hi):
            tn = 0.5 * (lo + hi) if np.isfinite(hi) else 2.0 * t
        if abs(tn - t) <= 1e-15 * max(1.0, t):
            return tn
        t = tn
    return t


def solve_primal(X, y, c, tol=1e-12, max_iter=200):
    """(w [D], b, iterations) at |grad f| <= tol |grad f(0)|, float64."""
    Xt = augment64(X)
    y = np.asarray(y, np.float64)
    c = np.asarray(c, np.float64)
    w = np.zeros(Xt.shape[1])
    g0 = None
    for it in range(max_iter):
        z = Xt @ w
        act = (y * z < 1.0) & (c > 0)
        g = w + 2.0 * Xt.T @ np.where(act, c * (z - y), 0.0)
        gn = np.linalg.norm(g)
        g0 = gn if g0 is None else g0
        if gn <= tol * g0 or gn == 0.0:
            break
        Xa = Xt[act]
        H = np.eye(Xt.shape[1]) + 2.0 * (Xa.T * c[act]) @ Xa
        d = np.linalg.solve(H, -g)
        t = _line_search(z, Xt @ d, y, c, float(w @ d), float(d @ d))
        w = w + t * d
    return w[:-1], float(w[-1]), it


def average_precision(targets, scores):
    """sklearn.metrics.average_precision_score(targets > 0, scores) over rows with targets >= 0 (targets < 0 ignored); 0 without positives."""
    t = np.asarray(targets).ravel()
    s = np.asarray(scores, np.float64).ravel()
    keep = t >= 0
    t, s = t[keep] > 0, s[keep]
    npos = int(t.sum())
    if npos == 0:
        return 0.0
    order = np.argsort(-s, kind="stable")
    s, t = s[order], t[order]
    tp = np.cumsum(t)
    ends = np.r_[np.nonzero(np.diff(s))[0], len(s) - 1]
    tpe = tp[ends]
    prev = np.r_[0, tpe[:-1]]
    return float(np.sum((tpe - prev) / npos * tpe / (ends + 1)))


def voc07_protocol(train_feats, train_targets, test_feats, test_targets, costs=(0.01, 0.1, 1.0, 10.0), tol=1e-12):
    """The reference train_test_single_svm for every class with the float64 optimum of every problem. Returns the same keys as
    svm.voc07_svm_eval (cv_ap, cost_index, cost, test_ap, map) plus the solutions {"W": [P][D], "b": [P]} in svm.voc07_problems order."""
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from clip_lite_amd.svm import select_cost, svm_labels, voc07_problems
    Ttr, Tte = np.asarray(train_targets), np.asarray(test_targets)
    Xtr, Xte = np.asarray(train_feats, np.float64), np.asarray(test_feats, np.float64)
    K, nc, F = Ttr.shape[1], len(costs), 4
    Y, Cw, folds = voc07_problems(Ttr, costs, F - 1)
    W = np.zeros((Y.shape[1], Xtr.shape[1]))
    b = np.zeros(Y.shape[1])
    for p in range(Y.shape[1]):
        W[p], b[p], _ = solve_primal(Xtr, Y[:, p].astype(np.float64), Cw[:, p].astype(np.float64), tol=tol)
    cv_ap = np.zeros((K, nc, F - 1))
    test_all = np.zeros((K, nc))
    for k in range(K):
        pos = (svm_labels(Ttr[:, k]) > 0).astype(np.int64)
        for j in range(nc):
            for f in range(F - 1):
                p = (k * nc + j) * F + f
                m = folds[k, f]
                cv_ap[k, j, f] = average_precision(pos[m], Xtr[m] @ W[p] + b[p])
            p = (k * nc + j) * F + F - 1
            tt = np.where(Tte[:, k] == -1, -1, (Tte[:, k] > 0).astype(np.int64))
            test_all[k, j] = average_precision(tt, Xte @ W[p] + b[p])
    idx = np.array([select_cost(cv_ap[k], costs)[0] for k in range(K)])
    test_ap = np.array([test_all[k, idx[k]] for k in range(K)])
    return {"cv_ap": cv_ap, "cost_index": idx, "cost": np.array([costs[i] for i in idx]), "test_ap": test_ap, "map": float(test_ap.mean()),
            "W": W, "b": b}
