"""Logistic-regression probe on the MI355X (logreg.py, csrc/logreg_ops.hip): the row kernels on the real build against float64 and the
one-workgroup line-search and Newton / CG state kernels on hand-made problems (the checks of tests/test_wavesim_logreg.py; the latter are the
shared ones of logreg_ref.py, here on real LDS barriers), logreg.fit on the sklearn fixture against its float64 certificate
|g64(W)| <= 1.1 tol |g64(0)|, bit-equal reruns in both deterministic modes, warm starts, problem groups under a workspace bound, predict_logits / accuracy, logreg_eval on a separable problem, and logreg_clf.py end to end.

Measured on the MI355X (tol = 1e-5; r64 = |g64(W)| / |g64(0)| in float64 on the CPU at the returned W, to stay below 1.1e-5;
dW = |W - W_sk|_F against its bound (1.1 tol + r_sk) |g64(0)|):
  (N, D, C)       cost   newton  cg    r64       dW        bound
  (96, 12, 3)     0.1    4       11    1.06e-07  2.00e-07  2.34e-05
  (96, 12, 3)     10     4       22    4.08e-06  2.39e-04  2.34e-03
  (96, 12, 3)     1000   6       66    3.21e-07  1.26e-03  2.34e-01
  (300, 24, 7)    0.1    3       9     7.24e-06  1.67e-05  4.84e-05
  (300, 24, 7)    10     5       39    1.67e-06  1.85e-04  4.85e-03
  (300, 24, 7)    1000   7       116   6.93e-08  1.15e-03  4.83e-01
  (1000, 40, 33)  0.1    4       12    4.81e-07  2.68e-06  8.18e-05
  (1000, 40, 33)  10     6       64    8.45e-08  2.41e-05  8.17e-03
  (1000, 40, 33)  1000   8       160   7.13e-08  9.47e-04  8.14e-01
Row kernels against float64, error over max |ref|: at most 2.5e-07 (Pr, S) and 4.7e-07 (Q); loss sums within 1.2e-07 relative."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import logreg_ref as R
from logreg_ref import KERNEL_SHAPES, S_LSDONE, S_T, SENT, ceil8, kernel_problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "logreg_small.npz")
TOL = 1e-5                      # the solver's stopping rule, and the f32 bound of the kernel checks (error over max |ref|)

pytestmark = pytest.mark.gpu


def _relerr(got, want):
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("N,P,Cn", KERNEL_SHAPES)
def test_row_kernels_match_float64(N, P, Cn):
    from clip_lite_amd import hip
    Z, Dl, y, w, costs, Cp, ldz = kernel_problem(N, P, Cn)
    nb = hip.logreg_blocks(N)
    Zd, Dld, yd, wd, cd = _dev(Z), _dev(Dl), _dev(y), _dev(w), _dev(costs)
    runs = []
    for _ in range(2):
        Pr, S = torch.full((N + 1, ldz), SENT, device="cuda"), torch.full((N + 1, ldz), SENT, device="cuda")
        loss, work = torch.full((P + 1,), SENT, device="cuda"), torch.zeros(2 * nb * P + 1, device="cuda")
        hip.logreg_softmax(Zd, yd, cd, wd, N, P, Cn, ldz, Pr, S, loss, work)
        Q = Dld.clone()
        for p in range(P):
            Q[:N, p * Cp + Cn:(p + 1) * Cp] = 3.0                         # garbage in the padding must come out as zero
        hip.logreg_hess_apply(Pr, cd, wd, N, P, Cn, ldz, Q)
        st = torch.zeros(P, hip.LOGREG_STATE, device="cuda")
        ts = np.linspace(0.25, 1.5, P).astype(np.float32)
        st[:, S_T] = _dev(ts)
        if P > 1:
            st[P - 1, S_LSDONE] = 1.0
        work.fill_(SENT)
        hip.check(hip.lib().clite_logreg_ray_eval(hip.p(Zd), hip.p(Dld), hip.p(yd), hip.p(cd), hip.p(wd), N, P, Cn, ldz, hip.p(st), hip.p(work),
                                                  hip.stream_ptr(Zd)), "logreg_ray_eval")
        runs.append([t.cpu().numpy() for t in (Pr, S, loss, Q, work)])
    for a, b in zip(*runs):
        assert a.tobytes() == b.tobytes()                                  # two runs are bit-equal
    Pr, S, loss, Q, work = runs[0]
    for A in (Pr, S, Q):
        assert (A[N:] == SENT).all() and (A[:, P * Cp:] == SENT).all()    # untouched outside [N][P * Cp]
    assert loss[P] == SENT and work[-1] == SENT
    p1, p2 = work[:nb * P].reshape(nb, P), work[nb * P:2 * nb * P].reshape(nb, P)
    for p in range(P):
        g, pad = slice(p * Cp, p * Cp + Cn), slice(p * Cp + Cn, (p + 1) * Cp)
        pr, s, ls = R.softmax_operand(Z[:N, g], y, float(costs[p]), w[:, p])
        e = (_relerr(Pr[:N, g], pr), _relerr(S[:N, g], s), _relerr(Q[:N, g], R.hess_operand(pr, Dl[:N, g], float(costs[p]), w[:, p])))
        print(f"(N, P, C) = {(N, P, Cn)} problem {p}: Pr {e[0]:.2e}, S {e[1]:.2e}, Q {e[2]:.2e}, loss {abs(loss[p] - ls) / abs(ls):.2e}")
        assert max(e) < TOL, (p, e)
        assert not Pr[:N, pad].any() and not S[:N, pad].any() and not Q[:N, pad].any()
        assert abs(loss[p] - ls) <= 1e-6 * abs(ls), (p, loss[p], ls)
        if P > 1 and p == P - 1:
            assert (p1[:, p] == SENT).all() and (p2[:, p] == SENT).all()
            continue
        a, b = R.ray_sums(Z[:N, g], Dl[:N, g], y, float(costs[p]), w[:, p], float(ts[p]))
        cw = float(costs[p]) * w[:, p].astype(np.float64)
        scale = float(np.sum(cw * np.abs(Dl[:N, g]).max(axis=1))) + 1e-300
        assert abs(p1[:, p].astype(np.float64).sum() - a) <= TOL * scale and abs(p2[:, p].astype(np.float64).sum() - b) <= TOL * abs(b)


def test_row_kernels_refuse_bad_arguments():
    from clip_lite_amd import hip
    L = hip.lib()
    z = torch.full((4, 16), SENT, device="cuda")
    y, c, w = torch.zeros(4, dtype=torch.int32, device="cuda"), torch.ones(2, device="cuda"), torch.ones(4, 2, device="cuda")
    out, loss, work = torch.full((4, 16), SENT, device="cuda"), torch.full((2,), SENT, device="cuda"), torch.full((8,), SENT, device="cuda")
    p, s = hip.p, hip.stream_ptr(z)
    assert L.clite_logreg_softmax(p(z), p(y), p(c), p(w), 4, 2, 9, 16, p(out), p(out), p(loss), p(work), s) == -1         # 2 x 16 columns do not fit
    assert L.clite_logreg_softmax(p(z), p(y), p(c), p(w), 4, 2, 5000, 16, p(out), p(out), p(loss), p(work), s) == -2
    assert L.clite_logreg_softmax(p(z), p(y), p(c), p(w), 0, 2, 5, 16, p(out), p(out), p(loss), p(work), s) == -1
    assert L.clite_logreg_hess_apply(p(z), p(c), p(w), 4, 2, 5, 12, p(out), s) == -1
    assert L.clite_logreg_hess_apply(p(z), p(c), p(w), 4, 2, 5, 16, hip.p(out) + 4, s) == -1                              # misaligned
    torch.cuda.synchronize()
    assert bool((out == SENT).all()) and bool((loss == SENT).all()) and bool((work == SENT).all())


def _call(name, *args):
    """clite_logreg_<name> on NumPy arrays (copied to the device and, after the kernel, back in place) and scalars, on the current stream: what
    the shared checks of logreg_ref.py drive."""
    from clip_lite_amd import hip
    dev = [_dev(a) if isinstance(a, np.ndarray) else a for a in args]
    first = next(d for d in dev if torch.is_tensor(d))
    rc = getattr(hip.lib(), "clite_logreg_" + name)(*[hip.p(d) if torch.is_tensor(d) else d for d in dev], hip.stream_ptr(first))
    torch.cuda.synchronize()
    for a, d in zip(args, dev):
        if isinstance(a, np.ndarray):
            a[...] = d.cpu().numpy()
    return rc


def test_ray_step_finds_the_minimiser_of_a_convex_phi():
    R.check_ray_step_finds_the_minimiser_of_a_convex_phi(_call)


def test_ray_step_out_of_evaluations_takes_the_left_end_of_the_bracket():
    R.check_ray_step_out_of_evaluations(_call)


def test_ray_begin_refuses_a_non_descent_direction_and_finish_updates():
    R.check_ray_begin_refuses_a_non_descent_direction_and_finish_updates(_call)


def test_newton_begin_g0_and_cg_on_explicit_systems():
    R.check_newton_begin_g0_and_cg_on_explicit_systems(_call)


def test_newton_begin_stops_a_problem_after_a_zero_step():
    R.check_newton_begin_stops_a_problem_after_a_zero_step(_call)


@pytest.fixture(scope="module")
def fixture_fits():
    """logreg.fit on the three fixture problems, all three costs in one call each; computed once and left unchanged."""
    from clip_lite_amd import logreg
    G = np.load(GOLD)
    fits = []
    for k in range(3):
        x, y, w = G[f"x{k}"], G[f"y{k}"], G[f"w{k}"]
        W3 = np.repeat(w[:, None], 3, axis=1)
        sol = logreg.fit(_dev(x), y, int(G[f"coef{k}"].shape[1]), G["costs"], W3, tol=TOL)
        fits.append((x, y, w, W3, sol))
    return G, fits


def _certificate(G, k, x, y, w, sol, label):
    """Assert |g64(W)| <= 1.1 tol |g64(0)| and the distance to sklearn's optimum that strong convexity then gives, for every cost."""
    for j, cost in enumerate(G["costs"]):
        Wp = np.concatenate([sol["W"][j].cpu().double().numpy(), sol["b"][j].cpu().double().numpy()[:, None]], axis=1)
        r, g0 = R.rel_grad(Wp, x, y, float(cost), w)
        dW = float(np.linalg.norm(Wp - G[f"coef{k}"][j]))
        bound = (1.1 * TOL + G[f"r_sk{k}"][j]) * g0
        print(f"{label} {x.shape} C={Wp.shape[0]} cost {cost}: newton {int(sol['newton'][j])}, cg {int(sol['cg'][j])}, f32 rel {float(sol['rel_grad'][j]):.3e}, "
              f"r64 {r:.3e}, |W - W_sk| {dW:.3e} (bound {bound:.3e})")
        assert r <= 1.1 * TOL, (k, j, r)
        assert dW <= bound, (k, j, dW, bound)
        assert float(sol["rel_grad"][j]) <= TOL and 0 < int(sol["newton"][j]) < 50


def test_fit_meets_the_float64_certificate_on_the_fixture(fixture_fits):
    G, fits = fixture_fits
    for k, (x, y, w, _, sol) in enumerate(fits):
        assert sol["W"].shape == (3, G[f"coef{k}"].shape[1], x.shape[1]) and sol["b"].shape == sol["W"].shape[:2]
        _certificate(G, k, x, y, w, sol, "fit")
        for j, cost in enumerate(G["costs"]):                             # the reported loss is the data term of f at the returned W
            Wp = np.concatenate([sol["W"][j].cpu().double().numpy(), sol["b"][j].cpu().double().numpy()[:, None]], axis=1)
            want = R.objective(Wp, R.augment(x), y, float(cost), w.astype(np.float64)) - 0.5 * np.sum(Wp * Wp)
            assert abs(float(sol["loss"][j]) - want) <= 1e-5 * abs(want)


def test_fit_is_bitwise_reproducible_and_a_solution_warm_starts_unchanged(fixture_fits):
    from clip_lite_amd import hip, logreg
    G, fits = fixture_fits
    mode = hip.is_deterministic()
    for k in range(3):
        x, y, w, W3, sol = fits[k]
        Cn = G[f"coef{k}"].shape[1]
        try:                                                               # a rerun gives the same bits, in the fixture's deterministic mode and in the other
            for det in (mode, not mode):
                hip.set_deterministic(det)
                first = sol if det == mode else logreg.fit(_dev(x), y, Cn, G["costs"], W3, tol=TOL)
                again = logreg.fit(_dev(x), y, Cn, G["costs"], W3, tol=TOL)
                for key in ("W", "b", "newton", "cg", "rel_grad", "loss"):
                    assert torch.equal(again[key], first[key]), (k, det, key)
        finally:
            hip.set_deterministic(mode)
        warm = logreg.fit(_dev(x), y, Cn, G["costs"], W3, W0=(sol["W"], sol["b"]), tol=TOL)
        assert warm["newton"].tolist() == [0, 0, 0] and warm["cg"].tolist() == [0, 0, 0]
        assert torch.equal(warm["W"], sol["W"]) and torch.equal(warm["b"], sol["b"])
        assert float(warm["rel_grad"].max()) <= TOL
    # a warm start that is no solution is solved on: from a perturbed optimum back to the certificate
    x, y, w, W3, sol = fits[1]
    off = logreg.fit(_dev(x), y, 7, G["costs"], W3, W0=(sol["W"] * 0.9, sol["b"] + 0.05), tol=TOL)
    assert min(off["newton"].tolist()) >= 1
    _certificate(G, 1, x, y, w, off, "warm")


def test_one_problem_per_group_under_a_workspace_bound(fixture_fits):
    from clip_lite_amd import logreg
    G, fits = fixture_fits
    for k in range(3):
        x, y, w, W3, sol = fits[k]
        Cn = G[f"coef{k}"].shape[1]
        bound = 3 * 4 * x.shape[0] * ceil8(Cn)                             # the row operands of exactly one problem
        assert logreg.problem_groups(x.shape[0], Cn, 3, bound) == [(0, 1), (1, 1), (2, 1)]
        one = logreg.fit(_dev(x), y, Cn, G["costs"], W3, tol=TOL, max_workspace_bytes=bound)
        _certificate(G, k, x, y, w, one, "grouped")
    x, y = G["x2"], G["y2"]
    xv, yv = _dev(x[::3]), y[::3]
    a = logreg.logreg_eval(_dev(x), y, xv, yv, 33, G["costs"], 0.2)
    b = logreg.logreg_eval(_dev(x), y, xv, yv, 33, G["costs"], 0.2, max_workspace_bytes=3 * 4 * x.shape[0] * ceil8(33))
    assert a["cost"] == b["cost"] and a["holdout_top1"] == b["holdout_top1"] and a["top1"] == b["top1"]


def test_gemm_rows_in_chunks_meet_the_certificate(fixture_fits, monkeypatch):
    """The solver's GEMMs take their rows in chunks that fit a GEMM operand (below 4 GiB: every 251 000 rows at ImageNet shape). With the limit
    lowered to 304 and to 336 rows of the largest operand (four chunks, and three with a ragged last one), the gradient sums over the chunks in
    order and every problem still meets the certificate."""
    from clip_lite_amd import logreg
    G, fits = fixture_fits
    x, y, w, W3, sol = fits[2]
    for rows in (304, 336):
        monkeypatch.setattr(logreg, "GEMM_OPERAND_BYTES", 4 * 120 * rows)  # ldz = 3 x 40 floats is the longest row
        assert logreg._row_chunk(1000, 120) == rows and logreg._row_chunk(1000, 48) >= rows
        one = logreg.fit(_dev(x), y, 33, G["costs"], W3, tol=TOL)
        _certificate(G, 2, x, y, w, one, f"chunks of {rows}")
        z = logreg.predict_logits(_dev(x), one["W"][1], one["b"][1])
        want = R.augment(x) @ np.concatenate([one["W"][1].cpu().double().numpy(), one["b"][1].cpu().double().numpy()[:, None]], axis=1).T
        assert np.abs(z.cpu().numpy() - want).max() <= 1e-5 * np.abs(want).max()
    with pytest.raises(ValueError, match="does not fit"):
        logreg._row_chunk(1000, 2 ** 30)


def test_predict_logits_and_accuracy(fixture_fits):
    from clip_lite_amd import logreg
    G, fits = fixture_fits
    x, y, w, _, sol = fits[2]
    for j in (0, 2):
        Wj, bj = sol["W"][j], sol["b"][j]
        z = logreg.predict_logits(_dev(x), Wj, bj)
        assert z.shape == (1000, 33) and z.dtype == torch.float32
        zh = z.cpu().numpy()
        want = R.augment(x) @ np.concatenate([Wj.cpu().double().numpy(), bj.cpu().double().numpy()[:, None]], axis=1).T
        assert np.abs(zh - want).max() <= 1e-5 * np.abs(want).max()
        # integer counts with numpy on those same logits, ties to the lower class
        zt = z.clone()
        zt[::7, 5] = zt[::7, 20]                                           # exact ties between a lower and a higher class
        zq = zt.cpu().numpy()
        zy = zq[np.arange(len(y)), y][:, None]
        rank = (zq > zy).sum(1) + ((zq == zy) & (np.arange(33)[None, :] < y[:, None])).sum(1)
        acc = logreg.accuracy(zt, y, 5)
        assert acc["top1"] == 100.0 * int((rank == 0).sum()) / len(y) and acc["top5"] == 100.0 * int((rank < 5).sum()) / len(y)
    small = logreg.accuracy(_dev(np.array([[0.5, 0.5, 0.1], [0.1, 0.2, 0.2]], np.float32)), [1, 1], 5)
    assert small == {"top1": 50.0}                                         # fewer than five classes: no top-5; row 0's tie goes to class 0


def test_logreg_eval_on_a_separable_problem():
    from clip_lite_amd import logreg
    rng = np.random.default_rng(0)
    Cn, per, D = 10, 40, 16
    centres = np.eye(Cn, D) * 4.0
    y = np.tile(np.arange(Cn), per)
    x = centres[y] + 0.1 * rng.standard_normal((Cn * per, D))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    yv = np.tile(np.arange(Cn), 8)
    xv = centres[yv] + 0.1 * rng.standard_normal((Cn * 8, D))
    xv /= np.linalg.norm(xv, axis=1, keepdims=True)
    res = logreg.logreg_eval(_dev(x.astype(np.float32)), y, _dev(xv.astype(np.float32)), yv, Cn, (1.0, 10.0, 100.0), 0.1)
    print(res)
    assert res["top1"] == 100.0 and res["top5"] == 100.0 and all(v == 100.0 for v in res["holdout_top1"].values())
    assert res["cost"] == 1.0 and res["cost_index"] == 0                  # all tie at 100: the smaller cost


def test_logreg_clf_end_to_end(tmp_path):
    """logreg_clf.py on configs/downstream_knn.yaml with the synthetic source, ResNet-18 at crop 32 with random weights, two costs, in a fresh
    child process: one evaluation, a well-formed logreg_acc.txt, and `Completed!` when the next checkpoint is missing."""
    ck = os.path.join(str(tmp_path), "ck")
    os.makedirs(ck)
    over = ["MODEL.VISUAL.NETWORK_NAME", "resnet18", "MODEL.VISUAL.FEATURE_SIZE", 512, "MODEL.TEXTUAL.NUM_HIDDEN_LAYERS", 1]
    cmd = [sys.executable, os.path.join(ROOT, "logreg_clf.py"), "--config", os.path.join(ROOT, "configs", "smoke_random.yaml"), "--config-override",
           *[str(v) for v in over], "--down-config", os.path.join(ROOT, "configs", "downstream_knn.yaml"), "--weight-init", "random",
           "--checkpoint-dir", ck, "--start-iter", "100", "--freq", "50", "--cost", "10", "1000", "--cpu-workers", "0", "--checkpoints-dir",
           os.path.join(str(tmp_path), "logs") + "/"]
    r = subprocess.run(cmd, cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    print(r.stdout[-2000:], r.stderr[-3000:])
    assert r.returncode == 0
    assert r.stdout.count("Logistic-regression probe top-1: ") == 1 and " | top-5: " in r.stdout and r.stdout.rstrip().endswith("Completed!")
    with open(os.path.join(ck, "logreg_acc.txt")) as f:
        got = json.load(f)
    assert sorted(got) == ["100"] and set(got["100"]) == {"cost", "top1", "top5", "holdout_top1"}
    e = got["100"]
    assert e["cost"] in (10.0, 1000.0) and sorted(e["holdout_top1"]) == ["10", "1000"]
    assert all(0.0 <= v <= 100.0 for v in (e["top1"], e["top5"], *e["holdout_top1"].values())) and e["top5"] >= e["top1"]
