"""CPU-side checks of the logistic-regression probe: the float64 reference (tests/logreg_ref.py) against central finite differences and against
the sklearn fixture, holdout_weights, the cost selection and its tie rule, problem grouping under a workspace bound, the logreg_clf command
line (every default and refusal), logreg_acc.txt merging, and the argument validation of logreg.fit that needs no device."""
import json
import os

import numpy as np
import pytest
import torch

import logreg_ref as R
from clip_lite_amd import logreg
from clip_lite_amd.downstream import _report_logreg, build_logreg_parser, logreg_clf_main, run_checkpoint_loop

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "logreg_small.npz")
SHAPES = ((96, 12, 3), (300, 24, 7), (1000, 40, 33))


def _small(seed=0, N=40, D=5, Cn=4):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, D))
    y = np.concatenate([np.arange(Cn), rng.integers(0, Cn, N - Cn)])
    w = rng.choice([0.0, 1.0, 2.5], size=N)
    return R.augment(X), y, w, rng.standard_normal((Cn, D + 1)) * 0.7, rng.standard_normal((Cn, D + 1))


def test_reference_derivatives_match_central_differences():
    Xa, y, w, W, V = _small()
    cost, h = 3.0, 1e-5
    f = lambda M: R.objective(M, Xa, y, cost, w)                         # noqa: E731
    g = R.gradient(W, Xa, y, cost, w)
    num = np.zeros_like(W)
    for idx in np.ndindex(*W.shape):
        E = np.zeros_like(W)
        E[idx] = h
        num[idx] = (f(W + E) - f(W - E)) / (2 * h)
    np.testing.assert_allclose(g, num, rtol=1e-6, atol=1e-7)
    hv = R.hessvec(W, V, Xa, cost, w)
    np.testing.assert_allclose(hv, (R.gradient(W + h * V, Xa, y, cost, w) - R.gradient(W - h * V, Xa, y, cost, w)) / (2 * h), rtol=1e-6, atol=1e-7)
    for t in (0.0, 0.4, 1.0, 2.5):
        d1 = R.phi_d1(W, V, t, Xa, y, cost, w)
        assert abs(d1 - (f(W + (t + h) * V) - f(W + (t - h) * V)) / (2 * h)) <= 1e-6 * max(1.0, abs(d1))
        d2 = R.phi_d2(W, V, t, Xa, cost, w)
        assert abs(d2 - (R.phi_d1(W, V, t + h, Xa, y, cost, w) - R.phi_d1(W, V, t - h, Xa, y, cost, w)) / (2 * h)) <= 1e-6 * max(1.0, abs(d2))
        assert d2 >= np.sum(V * V)                                         # f is 1-strongly convex
    assert abs(R.phi_d1(W, V, 0.0, Xa, y, cost, w) - np.sum(g * V)) <= 1e-9 * np.abs(g * V).sum()
    assert abs(R.phi_d2(W, V, 0.0, Xa, cost, w) - np.sum(hv * V)) <= 1e-9 * np.abs(hv * V).sum()


def test_reference_row_operands_compose_to_the_gradient_and_hessian():
    Xa, y, w, W, V = _small(1)
    cost = 0.7
    Z = Xa @ W.T
    Pr, S, loss = R.softmax_operand(Z, y, cost, w)
    np.testing.assert_allclose(W + S.T @ Xa, R.gradient(W, Xa, y, cost, w), rtol=1e-12, atol=1e-12)
    assert abs(0.5 * np.sum(W * W) + loss - R.objective(W, Xa, y, cost, w)) < 1e-10
    np.testing.assert_allclose(V + R.hess_operand(Pr, Xa @ V.T, cost, w).T @ Xa, R.hessvec(W, V, Xa, cost, w), rtol=1e-12, atol=1e-12)
    a, b = R.ray_sums(Z, Xa @ V.T, y, cost, w, 0.6)
    assert abs(np.sum((W + 0.6 * V) * V) + a - R.phi_d1(W, V, 0.6, Xa, y, cost, w)) < 1e-10
    assert abs(np.sum(V * V) + b - R.phi_d2(W, V, 0.6, Xa, cost, w)) < 1e-10
    big = R.softmax(np.array([[900.0, -900.0, 899.0]]))                    # stable far beyond exp's range
    assert np.isfinite(big).all() and abs(big.sum() - 1) < 1e-12


def test_fixture_shapes_and_sklearn_certificates():
    G = np.load(GOLD)
    assert list(G["costs"]) == [0.1, 10.0, 1000.0]
    for k, (N, D, Cn) in enumerate(SHAPES):
        x, y, w, coef, r_sk = G[f"x{k}"], G[f"y{k}"], G[f"w{k}"], G[f"coef{k}"], G[f"r_sk{k}"]
        assert x.shape == (N, D) and x.dtype == np.float32 and y.shape == (N,) and coef.shape == (3, Cn, D + 1)
        np.testing.assert_allclose(np.linalg.norm(x.astype(np.float64), axis=1), 1.0, atol=1e-6)
        assert np.array_equal(w, np.where(np.arange(N) % 3 == 2, 0.0, 1.0)) and len(np.unique(y[w > 0])) == Cn
        for j, cost in enumerate(G["costs"]):
            r, _ = R.rel_grad(coef[j], x, y, float(cost), w)
            assert abs(r - r_sk[j]) <= 1e-3 * r_sk[j] + 1e-12 and r <= 1.4e-7, (k, j, r, r_sk[j])


def test_holdout_weights_on_ragged_classes():
    y = np.array([0, 1, 0, 2, 0, 0, 1, 0, 0, 0, 0, 0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1])
    w, held = logreg.holdout_weights(y, 0.1)
    assert w.dtype == np.float32 and held.dtype == bool and np.array_equal(w, (~held).astype(np.float32))
    for k in range(4):
        rows = np.flatnonzero(y == k)
        n = max(1, int(len(rows) * 0.1))
        assert np.array_equal(np.flatnonzero(held & (y == k)), rows[-n:])    # the last rows of the class, in dataset order
    assert held[3] and held[12]                                              # classes 2 and 3 have one row: held out whole
    assert held.sum() == 1 + 2 + 1 + 1                                       # classes of 9, 22, 1 and 1 rows
    w2, held2 = logreg.holdout_weights(torch.from_numpy(y), 0.5)
    assert held2.sum() == 4 + 11 + 1 + 1
    for bad in (0.0, 1.0, -0.1):
        with pytest.raises(ValueError, match="fraction"):
            logreg.holdout_weights(y, bad)
    with pytest.raises(ValueError, match="class 2 has no weighted row in problem 0"):
        logreg.fit(torch.zeros(len(y), 4), y, 4, [1.0], w[:, None])


def test_holdout_counts_are_those_of_exact_arithmetic():
    """100 * 0.29 is 28.999999999999996 and 100 * 0.57 is 56.99999999999999 in binary floating point; the split holds out 29 and 57 rows."""
    y = np.zeros(100, np.int64)
    for fraction, n in ((0.29, 29), (0.57, 57), (0.1, 10), (0.3, 30), (0.999, 99), (0.001, 1)):
        w, held = logreg.holdout_weights(y, fraction)
        assert held.sum() == n and held[100 - n:].all(), (fraction, held.sum())
    assert logreg.holdout_weights(np.zeros(7, np.int64), 0.29)[1].sum() == 2            # 2.03: still rounded down


def test_cost_selection_and_its_tie_rule():
    assert logreg.select_cost([50.0, 70.0, 60.0], [1, 10, 100]) == 1
    assert logreg.select_cost([70.0, 70.0, 60.0], [1, 10, 100]) == 0         # a tie goes to the smaller cost
    assert logreg.select_cost([60.0, 70.0, 70.0], [100, 10, 1]) == 2         # whatever the order of the list
    assert logreg.select_cost([70.0, 70.0, 70.0], [10, 1, 100]) == 1
    assert logreg.select_cost([0.0], [5.0]) == 0


def test_problem_groups_under_a_workspace_bound():
    per = 3 * 4 * 1000 * 40                                                  # three f32 [N][Cp] operands of one problem
    assert logreg.problem_groups(1000, 33, 5, None) == [(0, 5)]
    assert logreg.problem_groups(1000, 33, 5, per) == [(0, 1), (1, 1), (2, 1), (3, 1), (4, 1)]
    assert logreg.problem_groups(1000, 33, 5, 2 * per + 7) == [(0, 2), (2, 2), (4, 1)]
    assert logreg.problem_groups(1000, 33, 5, 100 * per) == [(0, 5)]
    with pytest.raises(ValueError, match="max_workspace_bytes"):
        logreg.problem_groups(1000, 33, 5, per - 1)
    assert 4 * 1281167 * 8 * 1000 > 40e9                                     # one [N][P * Cp] array, 8 problems, ImageNet: 41 GB


def test_gemm_row_chunks_fit_the_operand_limit():
    assert logreg._row_chunk(5011, 2056) == 5011                             # everything in one call while it fits
    rows = logreg._row_chunk(1281167, 4000)                                  # ImageNet, 4 problems of 1000 classes
    assert rows % 8 == 0 and rows * 4000 * 4 < 0xF0000000 <= (rows + 8) * 4000 * 4
    assert logreg._row_chunk(1281167, 2056) % 8 == 0 and logreg._row_chunk(1281167, 2056) * 2056 * 4 < 0xF0000000


def test_fit_validates_arguments_before_touching_a_device():
    X, y = torch.zeros(6, 4), np.array([0, 1, 2, 0, 1, 2])
    for kw, msg in ((dict(X=X.double()), "f32"), (dict(X=torch.zeros(6)), "f32"), (dict(X=torch.zeros(0, 4), y=[]), "at least one row"),
                    (dict(y=y[:5]), "5 labels for 6 rows"), (dict(y=y.astype(np.float32)), "integer"), (dict(y=y - 1), r"outside \[0, 3\)"),
                    (dict(y=y + 1), r"outside \[0, 3\)"), (dict(costs=[]), "positive and finite"), (dict(costs=[1.0, 0.0]), "positive and finite"),
                    (dict(costs=[float("inf")]), "positive and finite"), (dict(costs=[-1.0]), "positive and finite"),
                    (dict(weights=np.ones((6, 2))), r"\[6\]\[1\]"), (dict(weights=-np.ones((6, 1))), "non-negative and finite"),
                    (dict(weights=np.full((6, 1), np.nan)), "non-negative and finite"), (dict(num_classes=1), "num_classes"),
                    (dict(num_classes=5000), "num_classes"), (dict(num_classes=4), "class 3 has no weighted row in problem 0"),
                    (dict(tol=0.0), "tol"), (dict(max_workspace_bytes=10), "max_workspace_bytes")):
        args = dict(X=X, y=y, num_classes=3, costs=[1.0])
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            logreg.fit(**args)
    w = np.ones((6, 2), np.float32)
    w[[1, 4], 1] = 0.0
    with pytest.raises(ValueError, match="class 1 has no weighted row in problem 1"):
        logreg.fit(X, y, 3, [1.0, 2.0], w)
    with pytest.raises(RuntimeError, match="no CPU path"):
        logreg.fit(X, y, 3, [1.0])
    with pytest.raises(RuntimeError, match="no CPU path"):
        logreg.predict_logits(X, torch.zeros(3, 4), torch.zeros(3))
    with pytest.raises(ValueError, match="GPU"):
        logreg.accuracy(torch.zeros(6, 3), y)


def test_logreg_clf_arguments_and_errors(tmp_path):
    p = build_logreg_parser()
    a = p.parse_args(["--checkpoint-dir", "d"])
    assert (a.freq, a.start_iter, a.weight_init, a.num_gpus_per_machine, a.cost, a.holdout, a.tol) == \
        (46200, 46200, "vlinfo", 1, [1.0, 10.0, 100.0, 1000.0], 0.1, 1e-5)
    a = p.parse_args(["--config", "c.yaml", "--down-config", "d.yaml", "--down-config-override", "OPTIM.BATCH_SIZE", "8", "--weight-init", "random",
                      "--checkpoint-dir", "x", "--freq", "10", "--start-iter", "20", "--cpu-workers", "0", "--cost", "3", "0.5", "--holdout", "0.25",
                      "--tol", "1e-4"])
    assert a.down_config_override == ["OPTIM.BATCH_SIZE", "8"] and (a.freq, a.start_iter, a.cost, a.holdout, a.tol) == (10, 20, [3.0, 0.5], 0.25, 1e-4)
    with pytest.raises(SystemExit):
        p.parse_args([])                                # --checkpoint-dir is required
    with pytest.raises(SystemExit):
        p.parse_args(["--checkpoint-dir", "x", "--weight-init", "clip"])
    for args, msg in ((["--num-gpus-per-machine", "0"], "no CPU path"), (["--num-gpus-per-machine", "2"], "one GPU"),
                      (["--num-machines", "2"], "one GPU"), (["--weight-init", "imagenet"], "not supported"),
                      (["--weight-init", "torchvision"], "not supported"), (["--cost", "0"], "positive and finite"),
                      (["--cost", "1", "-2"], "positive and finite"), (["--cost", "inf"], "positive and finite"), (["--cost", "5", "5"], "twice"),
                      (["--holdout", "0"], r"\(0, 1\)"), (["--holdout", "1"], r"\(0, 1\)"), (["--tol", "0"], "positive")):
        with pytest.raises(SystemExit, match=msg):
            logreg_clf_main(p.parse_args(["--checkpoint-dir", "x"] + args))
    down = os.path.join(ROOT, "configs", "downstream_knn.yaml")
    with pytest.raises(SystemExit, match="voc_clf.py"):
        logreg_clf_main(p.parse_args(["--checkpoint-dir", "x", "--weight-init", "random", "--down-config", down, "--down-config-override", "DATA.ROOT",
                                      str(tmp_path / "VOC2007")]))


def test_logreg_clf_needs_a_gpu(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    down = os.path.join(ROOT, "configs", "downstream_knn.yaml")
    with pytest.raises(SystemExit, match="no GPU visible"):
        logreg_clf_main(build_logreg_parser().parse_args(["--checkpoint-dir", "x", "--weight-init", "random", "--down-config", down]))


def test_logreg_acc_file_merges_over_checkpoints(tmp_path, capsys):
    d = str(tmp_path)
    with open(os.path.join(d, "logreg_acc.txt"), "w") as f:
        json.dump({"10": {"cost": 1.0, "top1": 1.5}}, f)
    open(os.path.join(d, "checkpoint_30.pth"), "w").close()
    loaded = []

    def load(path):
        if not os.path.exists(path):
            raise FileNotFoundError(path)
        loaded.append(os.path.basename(path))

    evals = iter([{"cost": 10.0, "cost_index": 1, "top1": 25.0, "top5": 50.0, "holdout_top1": {1.0: 20.0, 10.0: 30.0}, "newton": ([3], [1])},
                  {"cost": 0.5, "cost_index": 0, "top1": 40.125, "holdout_top1": {0.5: 41.0}}])
    res = run_checkpoint_loop(d, 20, 10, lambda: next(evals), load, filename="logreg_acc.txt", report=_report_logreg)
    assert loaded == ["checkpoint_30.pth"]
    with open(os.path.join(d, "logreg_acc.txt")) as f:
        got = json.load(f)
    assert got == res == {"10": {"cost": 1.0, "top1": 1.5},
                          "20": {"cost": 10.0, "top1": 25.0, "top5": 50.0, "holdout_top1": {"1": 20.0, "10": 30.0}},
                          "30": {"cost": 0.5, "top1": 40.125, "top5": None, "holdout_top1": {"0.5": 41.0}}}
    out = capsys.readouterr().out
    assert "Logistic-regression probe top-1: 25.00 | top-5: 50.00 (cost 10)\n" in out
    assert "Logistic-regression probe top-1: 40.12 (cost 0.5)\n" in out and out.rstrip().endswith("Completed!")


def test_entry_script_and_config():
    src = open(os.path.join(ROOT, "logreg_clf.py")).read()
    assert "logreg_clf_cli" in src
    from clip_lite_amd.config import Config
    assert Config(os.path.join(ROOT, "configs", "downstream_knn.yaml"), []).DATA.ROOT == "random"


def test_hip_wrappers_on_the_simulator_build(monkeypatch):
    """hip.logreg_* (their asserts and argument order) on host tensors through the wave-simulator build of the same sources: one gradient
    operand, one Hessian apply and one whole line search along a descent direction against float64."""
    import ctypes as C
    import simlib
    from clip_lite_amd import hip
    simlib.build_sim()
    monkeypatch.setattr(hip, "_lib", hip._bind(C.CDLL(simlib.SIM_SO)))
    monkeypatch.setattr(hip, "_allow_host_tensors", True)
    rng = np.random.default_rng(4)
    N, D, Cn, P = 50, 6, 5, 2
    Dp, Cp = 8, 8
    ldz, n = P * Cp, Cp * Dp
    Xt = np.zeros((N, Dp), np.float32)
    Xt[:, :D], Xt[:, D] = rng.standard_normal((N, D)), 1.0
    y = rng.integers(0, Cn, N)
    wts = rng.choice([0.0, 1.0], size=(N, P)).astype(np.float32)
    costs = np.array([0.5, 4.0], np.float32)
    W = np.zeros((P * Cp, Dp), np.float32)
    for p in range(P):
        W[p * Cp:p * Cp + Cn, :D + 1] = rng.standard_normal((Cn, D + 1)) * 0.5
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))              # noqa: E731
    Z, Pr, S = t(Xt @ W.T), torch.zeros(N, ldz), torch.zeros(N, ldz)
    loss, work = torch.zeros(P), torch.zeros(2 * hip.logreg_blocks(N) * P)
    y32 = t(y.astype(np.int32))
    hip.logreg_softmax(Z, y32, t(costs), t(wts), N, P, Cn, ldz, Pr, S, loss, work)
    G = S.numpy().T @ Xt + W
    Xa = Xt[:, :D + 1].astype(np.float64)
    for p in range(P):
        Wp = W[p * Cp:p * Cp + Cn, :D + 1].astype(np.float64)
        np.testing.assert_allclose(G[p * Cp:p * Cp + Cn, :D + 1], R.gradient(Wp, Xa, y, float(costs[p]), wts[:, p].astype(np.float64)), rtol=1e-4, atol=1e-5)
    with pytest.raises(AssertionError):
        hip.logreg_softmax(Z, t(y), t(costs), t(wts), N, P, Cn, ldz, Pr, S, loss, work)              # int64 labels
    Dv = (-G).astype(np.float32)
    Q = t(Xt @ Dv.T)
    delta = Q.clone()
    hip.logreg_hess_apply(Pr, t(costs), t(wts), N, P, Cn, ldz, Q)
    state = torch.zeros(P, hip.LOGREG_STATE)
    state[:, 9] = 1.0
    Wt, W0 = t(W.copy()), W.copy()
    hip.logreg_line_search(Z, delta, y32, t(costs), t(wts), N, P, Cn, ldz, t(G), Wt, t(Dv), n, n, state, work, evals=8)
    for p in range(P):
        Wp, Dp_ = (a[p * Cp:p * Cp + Cn, :D + 1].astype(np.float64) for a in (W0, Dv))
        wp = wts[:, p].astype(np.float64)
        hv = Dp_ + R.hess_operand(Pr.numpy()[:, p * Cp:p * Cp + Cn], Xa @ Dp_.T, float(costs[p]), wp).T @ Xa
        np.testing.assert_allclose(Dv[p * Cp:p * Cp + Cn, :D + 1] + (Q.numpy().T @ Xt)[p * Cp:p * Cp + Cn, :D + 1], hv, rtol=1e-4, atol=1e-4)
        step = float(state[p, 5])
        assert step > 0 and abs(R.phi_d1(Wp, Dp_, step, Xa, y, float(costs[p]), wp)) <= 1e-3 * abs(R.phi_d1(Wp, Dp_, 0.0, Xa, y, float(costs[p]), wp))
        np.testing.assert_allclose(Wt.numpy()[p * Cp:(p + 1) * Cp], W0[p * Cp:(p + 1) * Cp] + np.float32(step) * Dv[p * Cp:(p + 1) * Cp], rtol=1e-6, atol=1e-6)
