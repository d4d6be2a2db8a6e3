"""CPU-side (wave simulator) checks of the SVM kernels (csrc/svm_ops.hip) against float64 NumPy: the margin / residual kernel, the Newton
start and CG update with some problems already frozen, the line search, and average precision against sklearn. A last test drives the whole
batched Newton-CG loop of svm.fit_squared_hinge with NumPy standing in for the two GEMMs and checks the float64 optimum. Runs without a GPU."""
import ctypes as C

import numpy as np
import pytest

from simlib import lib, ptr
from svm_ref import average_precision as ap_ref
from svm_ref import solve_primal

ST = 16
S_G0, S_GN, S_REL, S_RR, S_CGTOL2, S_STEP, S_NEWTON, S_CGIT, S_CGTOT, S_ACTIVE, S_CGACT = range(11)
_P, _I, _F, _U64 = C.c_void_p, C.c_int, C.c_float, C.c_uint64


def _bind():
    L = lib()
    L.clite_svm_margin.argtypes = [_P, _P, _P, _I, _I, _I, _P, _P, _P, _P, _P]
    L.clite_svm_hess_scale.argtypes = [_P, _P, _U64, _P]
    L.clite_svm_newton_begin.argtypes = [_P, _I, _I, _I, _P, _P, _P, _P, _F, _I, _F, _P]
    L.clite_svm_cg_update.argtypes = [_P, _I, _I, _I, _P, _P, _P, _P, _P]
    L.clite_svm_line_search.argtypes = [_P, _P, _P, _P, _I, _I, _I, _P, _P, _I, _I, _P, _P]
    L.clite_average_precision.argtypes = [_P, _I, _P, _I, _I, _I, _P, _P]
    return L


def f32(a):
    return np.ascontiguousarray(a, np.float32)


def _problem(rng, N, P, ldp):
    Z = f32(np.zeros((N, ldp)))
    Z[:, :P] = rng.standard_normal((N, P)) * 1.5
    Y = f32(np.zeros((N, ldp)))
    Y[:, :P] = np.where(rng.random((N, P)) < 0.3, 1.0, -1.0)
    Cw = f32(np.zeros((N, ldp)))
    Cw[:, :P] = rng.choice([0.0, 0.5, 1.0, 2.0], size=(N, P))
    Z[:, P:] = Y[:, P:] = Cw[:, P:] = 7.0          # padding columns must not leak into S / H
    return Z, Y, Cw


@pytest.mark.parametrize("N,P,ldp", [(37, 3, 8), (1100, 13, 24)])
def test_margin_matches_float64(N, P, ldp):
    L = _bind()
    Z, Y, Cw = _problem(np.random.default_rng(N), N, P, ldp)
    S = np.full((N, ldp), 9.0, np.float32)
    H = np.full((N, ldp), 9.0, np.float32)
    loss = np.zeros(P, np.float32)
    work = np.zeros(((N + 511) // 512, ldp), np.float32)
    assert L.clite_svm_margin(ptr(Z), ptr(Y), ptr(Cw), N, P, ldp, ptr(S), ptr(H), ptr(loss), ptr(work), None) == 0
    z, y, c = (a[:, :P].astype(np.float64) for a in (Z, Y, Cw))
    act = (y * z < 1) & (c > 0)
    np.testing.assert_allclose(S[:, :P], np.where(act, c * (z - y), 0.0), rtol=1e-6, atol=1e-6)
    np.testing.assert_array_equal(H[:, :P], np.where(act, c, 0.0))
    assert not S[:, P:].any() and not H[:, P:].any()
    np.testing.assert_allclose(loss, (c * np.maximum(0, 1 - y * z) ** 2).sum(0), rtol=2e-5)
    Q = f32(np.random.default_rng(1).standard_normal((N, ldp)))
    want = Q * H
    assert L.clite_svm_hess_scale(ptr(H), ptr(Q), Q.size, None) == 0
    np.testing.assert_array_equal(Q, want)


def test_newton_begin_and_cg_with_frozen_problems():
    """Run CG on explicit SPD systems H_p = I + A_p^T A_p. Problem 1 starts frozen, problem 2 converges before the others (gradient small
    relative to its recorded g0), problem 3 has a zero gradient: none of them may move."""
    L = _bind()
    rng = np.random.default_rng(3)
    P, Dp, ld = 5, 40, 48
    A = rng.standard_normal((P, 12, Dp)) * 0.7
    Hm = np.eye(Dp)[None] + np.einsum("pki,pkj->pij", A, A)
    G = f32(np.zeros((P, ld)))
    G[:, :Dp] = rng.standard_normal((P, Dp))
    G[3] = 0.0
    st = f32(np.zeros((P, ST)))
    st[:, S_ACTIVE] = 1.0
    st[1, S_ACTIVE] = 0.0
    st[2, S_NEWTON], st[2, S_G0] = 3.0, 1e9           # |g| / g0 far below tol: converged
    X, R, D = (f32(np.full((P, ld), 5.0)) for _ in range(3))
    assert L.clite_svm_newton_begin(ptr(G), ld, Dp, P, ptr(X), ptr(R), ptr(D), ptr(st), 1e-5, 30, 0.1, None) == 0
    gn = np.linalg.norm(G[:, :Dp].astype(np.float64), axis=1)
    assert list(st[:, S_ACTIVE]) == [1, 0, 0, 0, 1] and list(st[:, S_CGACT]) == [1, 0, 0, 0, 1]
    np.testing.assert_allclose(st[[0, 4], S_G0], gn[[0, 4]], rtol=1e-6)
    assert st[0, S_NEWTON] == 1 and st[2, S_NEWTON] == 3 and st[3, S_REL] == 0
    np.testing.assert_allclose(st[[0, 4], S_CGTOL2], (0.1 * gn[[0, 4]]) ** 2, rtol=1e-5)
    for p in (0, 4):
        assert not X[p, :Dp].any() and np.array_equal(R[p, :Dp], -G[p, :Dp]) and np.array_equal(D[p, :Dp], -G[p, :Dp])
    frozen = [X[q].copy() for q in (1, 2, 3)]
    st[4, S_CGTOL2] = 0.0                               # problem 4 runs every iteration; problem 0 stops at eta = 0.1
    # float64 CG from the same start for comparison
    x64, r64 = np.zeros((P, Dp)), -G[:, :Dp].astype(np.float64)
    d64, rr64 = r64.copy(), (r64 * r64).sum(1)
    done = np.zeros(P, bool)
    for it in range(15):
        HD = f32(np.zeros((P, ld)))
        HD[:, :Dp] = np.einsum("pij,pj->pi", Hm, D[:, :Dp].astype(np.float64))
        assert L.clite_svm_cg_update(ptr(HD), ld, Dp, P, ptr(X), ptr(R), ptr(D), ptr(st), None) == 0
        for p in (0, 4):
            if done[p]:
                continue
            hd = Hm[p] @ d64[p]
            a = rr64[p] / (d64[p] @ hd)
            x64[p] += a * d64[p]
            r64[p] -= a * hd
            rn = r64[p] @ r64[p]
            if p == 0 and rn <= (0.1 * gn[0]) ** 2:
                done[p] = True
                continue
            d64[p] = r64[p] + rn / rr64[p] * d64[p]
            rr64[p] = rn
    assert done[0] and st[0, S_CGACT] == 0 and st[4, S_CGACT] == 1 and st[4, S_CGIT] == 15
    assert st[0, S_CGIT] == st[0, S_CGTOT] < 15
    for p in (0, 4):
        np.testing.assert_allclose(X[p, :Dp], x64[p], rtol=2e-3, atol=2e-4 * np.abs(x64[p]).max())
    for q, x in zip((1, 2, 3), frozen):
        assert np.array_equal(X[q], x)


def test_line_search_exact_minimiser_and_update():
    L = _bind()
    rng = np.random.default_rng(5)
    N, P, ldp, Dp, ld = 700, 11, 16, 24, 24
    Z, Y, Cw = _problem(rng, N, P, ldp)
    Dl = f32(np.zeros((N, ldp)))
    Dl[:, :P] = rng.standard_normal((N, P))
    W = f32(rng.standard_normal((ldp, ld)) * 0.3)
    X = f32(rng.standard_normal((ldp, ld)) * 0.3)
    z, y, c, dl = (a[:, :P].astype(np.float64) for a in (Z, Y, Cw, Dl))
    # make every x a descent direction: flip the sign where phi'(0) > 0
    wx = (W[:P, :Dp] * X[:P, :Dp]).astype(np.float64).sum(1)
    act0 = (y * z < 1) & (c > 0)
    d0 = wx + 2 * (np.where(act0, c * (z - y), 0) * dl).sum(0)
    flip = d0 > 0
    X[:P][flip] *= -1
    Dl[:, :P][:, flip] *= -1
    dl = Dl[:, :P].astype(np.float64)
    st = f32(np.zeros((P, ST)))
    st[:, S_ACTIVE] = 1.0
    st[6, S_ACTIVE] = 0.0                               # frozen: no step
    W0 = W.copy()
    assert L.clite_svm_line_search(ptr(Z), ptr(Dl), ptr(Y), ptr(Cw), N, P, ldp, ptr(W), ptr(X), ld, Dp, ptr(st), None) == 0
    for p in range(P):
        w, x = W0[p, :Dp].astype(np.float64), X[p, :Dp].astype(np.float64)
        ts = np.linspace(0, 3, 30001)
        phi = [0.5 * np.sum((w + t * x) ** 2) + np.sum(c[:, p] * np.maximum(0, 1 - y[:, p] * (z[:, p] + t * dl[:, p])) ** 2) for t in ts]
        t_best = ts[int(np.argmin(phi))]
        t = st[p, S_STEP]
        if p == 6:
            assert t == 0 and np.array_equal(W[p], W0[p])
            continue
        assert abs(t - t_best) <= 2e-4 + 1e-3 * t_best, (p, t, t_best)
        np.testing.assert_allclose(W[p, :Dp], W0[p, :Dp] + t * X[p, :Dp], rtol=1e-6, atol=1e-6)
    assert np.array_equal(W[P:], W0[P:])


def _ap_case(rng, N, P, ties):
    S = rng.standard_normal((N, P)).astype(np.float32)
    if ties:
        S = np.round(S * ties) / ties                 # heavy ties: few distinct thresholds
    T = (rng.random((N, P)) < 0.3).astype(np.float32)
    T[rng.random((N, P)) < 0.1] = -1.0                # ignored rows
    return f32(S), f32(T)


@pytest.mark.parametrize("N,P,ties", [(1, 2, 0), (7, 3, 0), (300, 4, 2), (1000, 3, 0), (4952, 2, 8), (8192, 1, 1)])
def test_average_precision_matches_sklearn(N, P, ties):
    from sklearn.metrics import average_precision_score
    L = _bind()
    rng = np.random.default_rng(N + P)
    S, T = _ap_case(rng, N, P, ties)
    if N > 1:
        T[0, 0], T[1, 0] = 1.0, 0.0                   # at least one positive and one negative in column 0
    ap = np.zeros(P, np.float32)
    assert L.clite_average_precision(ptr(S), P, ptr(T), P, N, P, ptr(ap), None) == 0
    for p in range(P):
        keep = T[:, p] >= 0
        want = ap_ref(T[:, p], S[:, p])
        if (T[keep, p] > 0).any():
            assert abs(want - average_precision_score(T[keep, p] > 0, S[keep, p])) < 1e-12
        assert abs(ap[p] - want) < 1e-6, (p, ap[p], want)


def test_average_precision_row_limit():
    L = _bind()
    N = 8193
    S, T, ap = f32(np.zeros((N, 1))), f32(np.zeros((N, 1))), np.zeros(1, np.float32)
    assert L.clite_average_precision(ptr(S), 1, ptr(T), 1, N, 1, ptr(ap), None) == -2


def test_batched_newton_cg_reaches_the_optimum():
    """The loop of svm.fit_squared_hinge with NumPy for the two GEMMs: the float64 optimum of every problem, frozen ones included."""
    L = _bind()
    rng = np.random.default_rng(11)
    N, D, P = 300, 13, 6
    Dp, ldp = 16, 8
    Xf = np.abs(rng.standard_normal((N, D)))
    Xf /= np.linalg.norm(Xf, axis=1, keepdims=True)
    Xf = Xf.astype(np.float32)
    Xt = f32(np.zeros((N, Dp)))
    Xt[:, :D], Xt[:, D] = Xf, 1.0
    lab = np.where(Xf[:, 0] + 0.3 * rng.standard_normal(N) > 0.3, 1.0, -1.0)
    Y = f32(np.zeros((N, ldp)))
    Cw = f32(np.zeros((N, ldp)))
    for p, C0 in enumerate([0.01, 0.1, 1.0, 10.0, 1.0, 10.0]):
        Y[:, p] = lab if p < 4 else -lab
        Cw[:, p] = C0 * np.where(Y[:, p] > 0, 2.0, 1.0) * (rng.random(N) > 0.33 if p >= 4 else 1.0)
    W, G, Xd, R, Dc, HD = (f32(np.zeros((ldp, Dp))) for _ in range(6))
    Z, S, H, Q = (f32(np.zeros((N, ldp))) for _ in range(4))
    loss, work = np.zeros(P, np.float32), np.zeros((1, ldp), np.float32)
    st = f32(np.zeros((P, ST)))
    st[:, S_ACTIVE] = 1.0
    for _ in range(31):
        Z[:] = Xt @ W.T
        assert L.clite_svm_margin(ptr(Z), ptr(Y), ptr(Cw), N, P, ldp, ptr(S), ptr(H), ptr(loss), ptr(work), None) == 0
        G[:] = 2 * S.T @ Xt + W
        assert L.clite_svm_newton_begin(ptr(G), Dp, Dp, P, ptr(Xd), ptr(R), ptr(Dc), ptr(st), 1e-5, 30, 0.1, None) == 0
        if not st[:, S_ACTIVE].any():
            break
        for _ in range(Dp):
            Q[:] = Xt @ Dc.T
            assert L.clite_svm_hess_scale(ptr(H), ptr(Q), Q.size, None) == 0
            HD[:] = 2 * Q.T @ Xt + Dc
            assert L.clite_svm_cg_update(ptr(HD), Dp, Dp, P, ptr(Xd), ptr(R), ptr(Dc), ptr(st), None) == 0
        Q[:] = Xt @ Xd.T
        assert L.clite_svm_line_search(ptr(Z), ptr(Q), ptr(Y), ptr(Cw), N, P, ldp, ptr(W), ptr(Xd), Dp, Dp, ptr(st), None) == 0
    assert not st[:, S_ACTIVE].any() and (st[:, S_REL] <= 1e-5).all()
    for p in range(P):
        w, b, _ = solve_primal(Xf, Y[:, p], Cw[:, p])
        np.testing.assert_allclose(W[p, :D], w, rtol=2e-3, atol=2e-4 * np.abs(w).max())
        assert abs(W[p, D] - b) <= 2e-3 * max(1.0, abs(b))
