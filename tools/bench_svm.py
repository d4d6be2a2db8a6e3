"""Time the VOC07 SVM stage at VOC scale (5011 trainval x 2048 features, 4952 test rows, 20 classes: 320 problems) on one GPU and print one
JSON line: the GPU time of the whole stage (all fits, the CV AP and the test AP; svm.voc07_svm_eval), its Newton / CG iteration counts and, when
sklearn is importable, the reference protocol's CPU time (voc_clf.py train_test_single_svm over all classes) on the same features with
--cpu-workers processes.

    python tools/bench_svm.py [--repeats 3] [--cpu-workers 0]     (--cpu-workers 0: skip the CPU baseline)
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


def voc_scale_features(seed=0, N=5011, Nt=4952, D=2048, K=20):
    """Seeded synthetic stand-in for pooled, L2-normalised ResNet-50 features with VOC-like class frequencies and difficult flags."""
    g = torch.Generator().manual_seed(seed)
    protos = torch.randn(K, D, generator=g) * 0.04

    def draw(n):
        present = torch.rand(n, K, generator=g) < torch.linspace(0.03, 0.3, K)
        f = torch.relu(0.3 + torch.randn(n, D, generator=g) * 0.5 + present.float() @ protos)
        t = present.to(torch.int64)
        t[(~present) & (torch.rand(n, K, generator=g) < 0.03)] = -1
        return f / f.norm(dim=1, keepdim=True), t.numpy()

    ftr, ttr = draw(N)
    fte, tte = draw(Nt)
    return ftr, ttr, fte, tte


def _reference_one(args):
    import warnings
    from sklearn.exceptions import ConvergenceWarning
    from sklearn.metrics import average_precision_score
    from sklearn.model_selection import cross_val_score
    from sklearn.svm import LinearSVC
    feats_train, tgts_train, feats_test, tgts_test = args
    labels = np.copy(tgts_train)
    labels[np.where(labels == 0)] = -1
    best, best_clf = 0.0, None
    for cost in (0.01, 0.1, 1.0, 10.0):
        clf = LinearSVC(C=cost, class_weight={1: 2, -1: 1}, penalty="l2", loss="squared_hinge", max_iter=2000)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", ConvergenceWarning)
            ap = cross_val_score(clf, feats_train, labels, cv=3, scoring="average_precision")
            clf.fit(feats_train, labels)
        if ap.mean() > best:
            best, best_clf = ap.mean(), clf
    keep = tgts_test != -1
    return average_precision_score(tgts_test[keep] > 0, best_clf.decision_function(feats_test)[keep])


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cpu-workers", type=int, default=0, help="processes for the sklearn baseline; 0 skips it")
    a = ap.parse_args()
    from clip_lite_amd import svm
    ftr, ttr, fte, tte = voc_scale_features()
    Xtr, Xte = ftr.cuda(), fte.cuda()
    svm.voc07_svm_eval(Xtr[:1024], ttr[:1024], Xte[:512], tte[:512])          # warm-up: first launches
    torch.cuda.synchronize()
    times, res = [], None
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        res = svm.voc07_svm_eval(Xtr, ttr, Xte, tte)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    out = {"metric": "voc07_svm_stage", "problems": res["problems"], "N": int(Xtr.shape[0]), "D": int(Xtr.shape[1]),
           "gpu_s": min(times), "gpu_s_all": times, "newton_max": int(res["newton"].max()), "newton_mean": float(res["newton"].mean()),
           "cg_launched": int(res["cg_launched"]), "cg_max": int(res["cg"].max()), "max_rel_grad": float(res["rel_grad"].max()),
           "map": 100 * res["map"]}
    if a.cpu_workers > 0:
        try:
            import sklearn  # noqa: F401
        except ImportError:
            out["cpu_baseline"] = "sklearn not importable"
        else:
            import multiprocessing as mp
            args = [(ftr.numpy(), ttr[:, k], fte.numpy(), tte[:, k]) for k in range(ttr.shape[1])]
            t0 = time.perf_counter()
            with mp.Pool(a.cpu_workers) as pool:
                aps = pool.map(_reference_one, args)
            out["cpu_s"] = time.perf_counter() - t0
            out["cpu_workers"] = a.cpu_workers
            out["cpu_map"] = 100 * float(np.mean(aps))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
