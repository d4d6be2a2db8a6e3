"""Generate tests/golden/logreg_small.npz: three small multinomial logistic-regression problems and what sklearn makes of them.

Run by hand on a CPU machine with scikit-learn (the tests themselves need neither sklearn nor this script):
    python tests/golden/make_logreg_golden.py

Contents, for each problem k = 0, 1, 2 with (N, D, C) = (96, 12, 3), (300, 24, 7), (1000, 40, 33)
  x{k} f32 [N][D]: seeded Gaussian class clusters, rows L2-normalised; y{k} i64 [N]: labels, every class present
  w{k} f32 [N]: sample weights, 1 with every third row 0 (held out)
  coef{k} f64 [3][C][D + 1]: per cost, LogisticRegression(C=cost, penalty="l2", fit_intercept=False, solver="lbfgs", tol=1e-12,
      max_iter=20000).fit(x~, y, sample_weight=w).coef_ on the augmented rows x~ = (x, 1): the bias is the last column and is regularised
  r_sk{k} f64 [3]: |grad64(coef)| / |grad64(0)|, how far sklearn stopped from the optimum (tests/logreg_ref.py)
  costs f64 [3] = 0.1, 10, 1000
"""
import os
import sys
import warnings

import numpy as np
from sklearn.linear_model import LogisticRegression

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import logreg_ref as R  # noqa: E402

SHAPES = ((96, 12, 3), (300, 24, 7), (1000, 40, 33))
COSTS = (0.1, 10.0, 1000.0)


def make_problem(seed, N, D, C):
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((C, D))
    y = np.concatenate([np.arange(C), rng.integers(0, C, N - C)])       # every class present
    y = y[rng.permutation(N)]
    x = centres[y] + 1.5 * rng.standard_normal((N, D))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    w = np.ones(N, np.float32)
    w[2::3] = 0.0
    return x.astype(np.float32), y.astype(np.int64), w


def main():
    out = {"costs": np.array(COSTS)}
    for k, (N, D, C) in enumerate(SHAPES):
        x, y, w = make_problem(100 + k, N, D, C)
        assert len(np.unique(y[w > 0])) == C
        Xa = R.augment(x)
        coef, r = np.zeros((len(COSTS), C, D + 1)), np.zeros(len(COSTS))
        for j, cost in enumerate(COSTS):
            clf = LogisticRegression(C=cost, penalty="l2", fit_intercept=False, solver="lbfgs", tol=1e-12, max_iter=20000)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                clf.fit(Xa, y, sample_weight=w.astype(np.float64))
            coef[j] = clf.coef_
            r[j], _ = R.rel_grad(coef[j], x, y, cost, w)
            print(f"problem {k} cost {cost}: r_sk = {r[j]:.3e}, |W| = {np.linalg.norm(coef[j]):.3f}, max |logit| = {np.abs(Xa @ coef[j].T).max():.2f}")
        out.update({f"x{k}": x, f"y{k}": y, f"w{k}": w, f"coef{k}": coef, f"r_sk{k}": r})
    path = os.path.join(HERE, "logreg_small.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
