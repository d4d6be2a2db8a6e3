"""Generate tests/golden/svm_voc_small.npz: a small VOC07-like SVM problem and what sklearn makes of it.

Run on a CPU machine with scikit-learn (the tests themselves need neither sklearn nor this script):
    python tests/golden/make_svm_golden.py

Contents
  x_train f16 [750][100], x_test f16 [500][100]: L2-normalised synthetic features (float16, so every consumer sees identical values)
  t_train, t_test int8 [N][6]: VOC targets {1 present, 0 absent, -1 difficult}
  costs f64 [4]
  w_opt f32 [P][100], b_opt f32 [P]: the tight optimum of every problem of svm.voc07_problems (LinearSVC(dual=False, tol=1e-12,
      max_iter=1e5) in float64), P = 6 classes x 4 costs x (3 folds + full)
  folds bool [6][3][750]: StratifiedKFold(3) test masks per class
  cv_ap f64 [6][4][3], cost_index i64 [6], test_ap f64 [6], map f64: the reference protocol (voc_clf.py train_test_single_svm) run through
      cross_val_score(LinearSVC(C, class_weight={1: 2, -1: 1}, max_iter=2000), cv=3, scoring="average_precision") and
      average_precision_score exactly as the reference calls them
  cv_margin f64 [6]: per class, best minus second-best mean CV AP
"""
import os
import sys
import warnings

import numpy as np
from sklearn.exceptions import ConvergenceWarning
from sklearn.metrics import average_precision_score
from sklearn.model_selection import StratifiedKFold, cross_val_score
from sklearn.svm import LinearSVC

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from clip_lite_amd.svm import voc07_problems  # noqa: E402

COSTS = (0.01, 0.1, 1.0, 10.0)


def make_data(seed=0, n_train=750, n_test=500, d=100, k=6):
    rng = np.random.default_rng(seed)
    protos = rng.standard_normal((k, d)) * 0.25
    base = rng.standard_normal(d) * 0.3

    def draw(n):
        present = rng.random((n, k)) < np.linspace(0.12, 0.35, k)
        t = present.astype(np.int8)
        difficult = (~present) & (rng.random((n, k)) < 0.04)
        t[difficult] = -1
        f = base + rng.standard_normal((n, d)) + present @ protos + 0.5 * difficult @ protos
        f = np.maximum(f, 0.0)                                   # pooled post-ReLU features are non-negative
        f /= np.linalg.norm(f, axis=1, keepdims=True)
        return f.astype(np.float16), t

    xtr, ttr = draw(n_train)
    xte, tte = draw(n_test)
    return xtr, ttr, xte, tte


def reference_protocol(xtr, ttr, xte, tte):
    """voc_clf.py train_test_single_svm, verbatim in what it calls."""
    K = ttr.shape[1]
    cv_ap = np.zeros((K, len(COSTS), 3))
    idx, test_ap, margin = [], [], []
    for c in range(K):
        labels = ttr[:, c].astype(np.int32).copy()
        labels[np.where(labels == 0)] = -1
        best, best_clf, best_j = 0.0, None, -1
        means = []
        for j, cost in enumerate(COSTS):
            clf = LinearSVC(C=cost, class_weight={1: 2, -1: 1}, penalty="l2", loss="squared_hinge", max_iter=2000)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", ConvergenceWarning)
                ap = cross_val_score(clf, xtr, labels, cv=3, scoring="average_precision")
                clf.fit(xtr, labels)
            cv_ap[c, j] = ap
            means.append(ap.mean())
            if ap.mean() > best:
                best, best_clf, best_j = ap.mean(), clf, j
        s = sorted(means, reverse=True)
        margin.append(s[0] - s[1])
        idx.append(best_j)
        pred = best_clf.decision_function(xte)
        keep = tte[:, c] != -1
        lab = tte[:, c][keep].astype(np.int32).copy()
        lab[np.where(lab == 0)] = -1
        test_ap.append(average_precision_score(lab > 0, pred[keep]))
    return cv_ap, np.array(idx), np.array(test_ap), np.array(margin)


def main():
    xtr, ttr, xte, tte = make_data()
    X = xtr.astype(np.float64)
    Y, Cw, folds = voc07_problems(ttr, COSTS, 3)
    for k in range(ttr.shape[1]):
        y = np.where(ttr[:, k] == 1, 1, -1)
        for f, (_, test) in enumerate(StratifiedKFold(3).split(X, y)):
            m = np.zeros(len(y), bool)
            m[test] = True
            assert np.array_equal(m, folds[k, f])
    P = Y.shape[1]
    W = np.zeros((P, X.shape[1]), np.float32)
    b = np.zeros(P, np.float32)
    for p in range(P):
        rows = Cw[:, p] > 0
        y = Y[rows, p].astype(np.int64)
        cost = float(Cw[rows, p][y < 0][0])                       # C * class weight of a negative = C
        clf = LinearSVC(C=cost, class_weight={1: 2, -1: 1}, penalty="l2", loss="squared_hinge", dual=False, tol=1e-12, max_iter=100000)
        clf.fit(X[rows], y)
        W[p], b[p] = clf.coef_[0], clf.intercept_[0]
    cv_ap, idx, test_ap, margin = reference_protocol(xtr, ttr, xte, tte)
    out = os.path.join(HERE, "svm_voc_small.npz")
    np.savez_compressed(out, x_train=xtr, x_test=xte, t_train=ttr, t_test=tte, costs=np.array(COSTS), w_opt=W, b_opt=b, folds=folds,
                        cv_ap=cv_ap, cost_index=idx, test_ap=test_ap, map=np.float64(test_ap.mean()), cv_margin=margin)
    print(f"wrote {out}: {os.path.getsize(out)} bytes; mAP {100 * test_ap.mean():.3f}, costs {idx.tolist()}, margins {np.round(margin, 4).tolist()}")


if __name__ == "__main__":
    main()
