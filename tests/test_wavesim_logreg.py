"""CPU-side (wave simulator) checks of the logistic-regression kernels (csrc/logreg_ops.hip) through the C ABI against the float64 reference
tests/logreg_ref.py: the softmax / gradient operand, the Hessian apply and the line-search evaluation at logits up to +-90 with zero weights,
padding and sentinels; the line-search step kernel on a hand-made convex phi and the Newton / CG state kernels (checks shared with the GPU
tests, in logreg_ref.py); argument refusals. A last test
drives the whole batched Newton-CG loop of logreg.fit with NumPy standing in for the two GEMMs. Runs without a GPU."""
import ctypes as C

import numpy as np
import pytest

import logreg_ref as R
from logreg_ref import KERNEL_SHAPES as SHAPES
from logreg_ref import S_ACTIVE, S_CGACT, S_CGTOT, S_LSDONE, S_NEWTON, S_REL, S_T, SENT, ST, aligned, ceil8, f32, nblocks
from logreg_ref import kernel_problem as _problem
from simlib import lib, ptr

_P, _I, _F = C.c_void_p, C.c_int, C.c_float
TOL = 1e-5                      # error over max |ref|: the f32 bound of the project's exact-f32 kernels


def _bind():
    L = lib()
    L.clite_logreg_softmax.argtypes = [_P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P]
    L.clite_logreg_hess_apply.argtypes = [_P, _P, _P, _I, _I, _I, _I, _P, _P]
    L.clite_logreg_newton_begin.argtypes = [_P, _I, _I, _I, _P, _P, _P, _P, _F, _I, _F, _I, _P]
    L.clite_logreg_cg_update.argtypes = [_P, _I, _I, _I, _P, _P, _P, _P, _P]
    L.clite_logreg_ray_begin.argtypes = [_P, _P, _P, _I, _I, _I, _P, _P]
    L.clite_logreg_ray_eval.argtypes = [_P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _P]
    L.clite_logreg_ray_step.argtypes = [_P, _I, _I, _P, _I, _P]
    L.clite_logreg_ray_finish.argtypes = [_P, _P, _I, _I, _I, _P, _P]
    return L


def _relerr(got, want):
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))


def _outside_untouched(A, N, P, Cp):
    return bool((A[N:] == SENT).all() and (A[:, P * Cp:] == SENT).all())


@pytest.mark.parametrize("N,P,Cn", SHAPES)
def test_softmax_operand_matches_float64(N, P, Cn):
    L = _bind()
    Z, _, y, w, costs, Cp, ldz = _problem(N, P, Cn)
    nb = nblocks(N)
    out = []
    for _ in range(2):
        Pr, S = aligned((N + 1, ldz), SENT), aligned((N + 1, ldz), SENT)
        loss, work = np.full(P + 1, SENT, np.float32), np.zeros(nb * P, np.float32)
        assert L.clite_logreg_softmax(ptr(Z), ptr(y), ptr(costs), ptr(w), N, P, Cn, ldz, ptr(Pr), ptr(S), ptr(loss), ptr(work), None) == 0
        out.append((Pr, S, loss))
    (Pr, S, loss), (Pr2, S2, loss2) = out
    assert Pr.tobytes() == Pr2.tobytes() and S.tobytes() == S2.tobytes() and loss.tobytes() == loss2.tobytes()
    assert _outside_untouched(Pr, N, P, Cp) and _outside_untouched(S, N, P, Cp) and loss[P] == SENT
    for p in range(P):
        g = slice(p * Cp, p * Cp + Cn)
        pr, s, ls = R.softmax_operand(Z[:N, g], y, float(costs[p]), w[:, p])
        assert _relerr(Pr[:N, g], pr) < TOL and _relerr(S[:N, g], s) < TOL, (p, _relerr(Pr[:N, g], pr), _relerr(S[:N, g], s))
        assert not Pr[:N, p * Cp + Cn:(p + 1) * Cp].any() and not S[:N, p * Cp + Cn:(p + 1) * Cp].any()
        assert abs(loss[p] - ls) <= 1e-6 * abs(ls), (p, loss[p], ls)
        assert not S[:N, g][w[:, p] == 0].any()


@pytest.mark.parametrize("N,P,Cn", SHAPES)
def test_hess_apply_matches_float64(N, P, Cn):
    L = _bind()
    Z, Dl, y, w, costs, Cp, ldz = _problem(N, P, Cn)
    Pr = aligned((N + 1, ldz), SENT)
    for p in range(P):
        Pr[:N, p * Cp:(p + 1) * Cp] = 0.0
        Pr[:N, p * Cp:p * Cp + Cn] = R.softmax(Z[:N, p * Cp:p * Cp + Cn])
    out = []
    for _ in range(2):
        Q = aligned(Dl.shape)
        Q[...] = Dl
        for p in range(P):
            Q[:N, p * Cp + Cn:(p + 1) * Cp] = 3.0                         # garbage in the padding must come out as zero
        assert L.clite_logreg_hess_apply(ptr(Pr), ptr(costs), ptr(w), N, P, Cn, ldz, ptr(Q), None) == 0
        out.append(Q)
    Q = out[0]
    assert Q.tobytes() == out[1].tobytes() and _outside_untouched(Q, N, P, Cp)
    for p in range(P):
        g = slice(p * Cp, p * Cp + Cn)
        want = R.hess_operand(Pr[:N, g], Dl[:N, g], float(costs[p]), w[:, p])
        assert _relerr(Q[:N, g], want) < TOL, (p, _relerr(Q[:N, g], want))
        assert not Q[:N, p * Cp + Cn:(p + 1) * Cp].any()


@pytest.mark.parametrize("N,P,Cn", SHAPES)
def test_ray_eval_matches_float64(N, P, Cn):
    L = _bind()
    Z, Dl, y, w, costs, Cp, ldz = _problem(N, P, Cn)
    nb = nblocks(N)
    st = f32(np.zeros((P, ST)))
    ts = np.linspace(0.25, 1.5, P).astype(np.float32)
    st[:, S_T] = ts
    if P > 1:
        st[P - 1, S_LSDONE] = 1.0                                         # a finished search: its partials are not written
    out = []
    for _ in range(2):
        work = np.full(2 * nb * P + 1, SENT, np.float32)
        assert L.clite_logreg_ray_eval(ptr(Z), ptr(Dl), ptr(y), ptr(costs), ptr(w), N, P, Cn, ldz, ptr(st), ptr(work), None) == 0
        out.append(work)
    work = out[0]
    assert work.tobytes() == out[1].tobytes() and work[-1] == SENT
    p1, p2 = work[:nb * P].reshape(nb, P), work[nb * P:2 * nb * P].reshape(nb, P)
    for p in range(P):
        if P > 1 and p == P - 1:
            assert (p1[:, p] == SENT).all() and (p2[:, p] == SENT).all()
            continue
        g = slice(p * Cp, p * Cp + Cn)
        a, b = R.ray_sums(Z[:N, g], Dl[:N, g], y, float(costs[p]), w[:, p], float(ts[p]))
        # scale of the sums: what the terms add up to in magnitude (the sum itself may cancel)
        cw = float(costs[p]) * w[:, p].astype(np.float64)
        scale = float(np.sum(cw * np.abs(Dl[:N, g]).max(axis=1))) + 1e-300
        assert abs(p1[:, p].astype(np.float64).sum() - a) <= TOL * scale, (p, p1[:, p].sum(), a)
        assert abs(p2[:, p].astype(np.float64).sum() - b) <= TOL * max(abs(b), 1e-300), (p, p2[:, p].sum(), b)


def _call(name, *args):
    """clite_logreg_<name> on NumPy arrays and scalars, on the null stream (what the shared checks of logreg_ref.py drive)."""
    return getattr(_bind(), "clite_logreg_" + name)(*[ptr(a) if isinstance(a, np.ndarray) else a for a in args], None)


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


def test_bad_arguments_return_an_error_and_write_nothing():
    L = _bind()
    N, P, Cn = 9, 2, 5
    Z, Dl, y, w, costs, Cp, ldz = _problem(N, P, Cn)
    nb = nblocks(N)
    Pr, S = aligned((N + 1, ldz), SENT), aligned((N + 1, ldz), SENT)
    loss, work = np.full(P, SENT, np.float32), np.full(2 * nb * P, SENT, np.float32)
    st = f32(np.zeros((P, ST)))

    def soft(Zp=Z, N_=N, P_=P, C_=Cn, ld_=ldz, Prp=Pr):
        return L.clite_logreg_softmax(ptr(Zp) if Zp is not None else None, ptr(y), ptr(costs), ptr(w), N_, P_, C_, ld_, ptr(Prp), ptr(S), ptr(loss),
                                      ptr(work), None)

    assert soft(N_=0) == -1 and soft(P_=0) == -1 and soft(C_=0) == -1 and soft(Zp=None) == -1
    assert soft(ld_=P * Cp - 4) == -1 and soft(ld_=ldz + 1) == -1 and soft(C_=4097, ld_=2 * 4104) == -2
    assert soft(Prp=Pr.reshape(-1)[1:]) == -1                             # misaligned
    assert L.clite_logreg_hess_apply(ptr(Pr), ptr(costs), ptr(w), N, P, Cn, P * Cp - 8, ptr(S), None) == -1
    assert L.clite_logreg_hess_apply(ptr(Pr), None, ptr(w), N, P, Cn, ldz, ptr(S), None) == -1
    assert L.clite_logreg_ray_eval(ptr(Z), ptr(Dl), ptr(y), ptr(costs), ptr(w), N, P, 5000, ldz, ptr(st), ptr(work), None) == -2
    assert L.clite_logreg_ray_eval(ptr(Z), None, ptr(y), ptr(costs), ptr(w), N, P, Cn, ldz, ptr(st), ptr(work), None) == -1
    assert L.clite_logreg_ray_step(ptr(work), 0, P, ptr(st), 0, None) == -1 and L.clite_logreg_ray_step(None, N, P, ptr(st), 0, None) == -1
    v = f32(np.full((P, 16), SENT))
    assert L.clite_logreg_newton_begin(ptr(v), 8, 16, P, ptr(v), ptr(v), ptr(v), ptr(st), 1e-5, 30, 0.1, 0, None) == -1       # ld < n
    assert L.clite_logreg_newton_begin(ptr(v), 16, 16, P, ptr(v), ptr(v), ptr(v), ptr(st), 1e-5, -1, 0.1, 0, None) == -1
    assert L.clite_logreg_cg_update(ptr(v), 16, 0, P, ptr(v), ptr(v), ptr(v), ptr(st), None) == -1
    assert L.clite_logreg_ray_begin(ptr(v), ptr(v), ptr(v), 16, 16, 0, ptr(st), None) == -1
    assert L.clite_logreg_ray_finish(ptr(v), ptr(v), 8, 16, P, ptr(st), None) == -1
    assert (Pr == SENT).all() and (S == SENT).all() and (loss == SENT).all() and (work == SENT).all() and (v == SENT).all() and not st.any()


def test_batched_newton_cg_reaches_the_float64_optimum():
    """The loop of logreg.fit with NumPy for the two GEMMs, on the smallest fixture problem with all three costs: the float64 gradient at the
    result satisfies the solver's certificate, and by strong convexity W is that close to sklearn's."""
    import os
    L = _bind()
    G_ = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "logreg_small.npz"))
    Xf, y, w1, costs64 = G_["x0"], G_["y0"].astype(np.int32), G_["w0"], G_["costs"]
    N, D = Xf.shape
    Cn, P = 3, len(costs64)
    Dp, Cp = ceil8(D + 1), ceil8(Cn)
    ldz, n = P * Cp, Cp * Dp
    Xt = f32(np.zeros((N, Dp)))
    Xt[:, :D], Xt[:, D] = Xf, 1.0
    costs, w = f32(costs64), f32(np.repeat(w1[:, None], P, axis=1))
    W, G, Xd, Rr, Dc, HD = (f32(np.zeros((P * Cp, Dp))) for _ in range(6))
    Z, Pr, T = (aligned((N, ldz)) for _ in range(3))
    loss, work = np.zeros(P, np.float32), np.zeros(2 * nblocks(N) * P, np.float32)
    st = f32(np.zeros((P, ST)))
    st[:, S_ACTIVE] = 1.0
    tol = 1e-5
    for _ in range(51):
        Z[:] = Xt @ W.T
        assert L.clite_logreg_softmax(ptr(Z), ptr(y), ptr(costs), ptr(w), N, P, Cn, ldz, ptr(Pr), ptr(T), ptr(loss), ptr(work), None) == 0
        G[:] = T.T @ Xt + W
        assert L.clite_logreg_newton_begin(ptr(G), n, n, P, ptr(Xd), ptr(Rr), ptr(Dc), ptr(st), tol, 50, 0.1, 0, None) == 0
        if not st[:, S_ACTIVE].any():
            break
        for _ in range(40):
            if not st[:, S_CGACT].any():
                break
            T[:] = Xt @ Dc.T
            assert L.clite_logreg_hess_apply(ptr(Pr), ptr(costs), ptr(w), N, P, Cn, ldz, ptr(T), None) == 0
            HD[:] = T.T @ Xt + Dc
            assert L.clite_logreg_cg_update(ptr(HD), n, n, P, ptr(Xd), ptr(Rr), ptr(Dc), ptr(st), None) == 0
        T[:] = Xt @ Xd.T
        assert L.clite_logreg_ray_begin(ptr(G), ptr(W), ptr(Xd), n, n, P, ptr(st), None) == 0
        for e in range(8):
            assert L.clite_logreg_ray_eval(ptr(Z), ptr(T), ptr(y), ptr(costs), ptr(w), N, P, Cn, ldz, ptr(st), ptr(work), None) == 0
            assert L.clite_logreg_ray_step(ptr(work), N, P, ptr(st), int(e == 7), None) == 0
        assert L.clite_logreg_ray_finish(ptr(W), ptr(Xd), n, n, P, ptr(st), None) == 0
    assert not st[:, S_ACTIVE].any() and (st[:, S_REL] <= tol).all() and (st[:, S_NEWTON] < 50).all()
    Wr = W.reshape(P, Cp, Dp)
    assert not Wr[:, Cn:].any() and not Wr[:, :, D + 1:].any()
    for p in range(P):
        Wp = Wr[p, :Cn, :D + 1].astype(np.float64)
        r, g0 = R.rel_grad(Wp, Xf, y, float(costs64[p]), w1)
        print(f"cost {costs64[p]}: newton {int(st[p, S_NEWTON])}, cg {int(st[p, S_CGTOT])}, r64 {r:.3e}, |W - W_sk| {np.linalg.norm(Wp - G_['coef0'][p]):.3e}")
        assert r <= 1.1 * tol
        assert np.linalg.norm(Wp - G_["coef0"][p]) <= (1.1 * tol + G_["r_sk0"][p]) * g0
