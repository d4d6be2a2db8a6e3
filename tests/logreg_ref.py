"""Float64 NumPy reference of the logistic-regression probe (clip-lite_amd/logreg.py, csrc/logreg_ops.hip): the objective
    f(W) = 1/2 |W|_F^2 + c sum_i w_i (logsumexp(W x~_i) - (W x~_i)[y_i]),   W [C][D + 1], x~_i = (x_i, 1)
(the bias is the last column of W and is regularised), its gradient, Hessian-vector product, the line-search derivatives phi' and phi'', and the
per-group quantities the row kernels write; and the checks of the one-workgroup vector kernels (line-search begin / step / finish, Newton / CG state)
that the simulator and the GPU tests share. Test infrastructure only."""
import numpy as np


def augment(X):
    """[N][D] -> float64 [N][D + 1]: the features and a constant 1."""
    X = np.asarray(X, np.float64)
    return np.concatenate([X, np.ones((X.shape[0], 1))], axis=1)


def log_softmax(Z):
    Z = np.asarray(Z, np.float64)
    m = Z.max(axis=-1, keepdims=True)
    lse = m + np.log(np.exp(Z - m).sum(axis=-1, keepdims=True))
    return Z - lse, lse[..., 0]


def softmax(Z):
    return np.exp(log_softmax(Z)[0])


def onehot(y, C):
    o = np.zeros((len(y), C))
    o[np.arange(len(y)), np.asarray(y)] = 1.0
    return o


def objective(W, Xa, y, cost, w):
    Z = Xa @ W.T
    _, lse = log_softmax(Z)
    return 0.5 * np.sum(W * W) + cost * np.sum(w * (lse - Z[np.arange(len(y)), y]))


def gradient(W, Xa, y, cost, w):
    Pr = softmax(Xa @ W.T)
    S = cost * w[:, None] * (Pr - onehot(y, W.shape[0]))
    return W + S.T @ Xa


def hessvec(W, V, Xa, cost, w):
    Pr = softmax(Xa @ W.T)
    Q = Xa @ V.T
    Q = cost * w[:, None] * (Pr * Q - Pr * np.sum(Pr * Q, axis=1, keepdims=True))
    return V + Q.T @ Xa


def phi_d1(W, D, t, Xa, y, cost, w):
    """d/dt f(W + t D)."""
    Z, dl = Xa @ W.T, Xa @ D.T
    Pr = softmax(Z + t * dl)
    return np.sum((W + t * D) * D) + cost * np.sum(w * (np.sum(Pr * dl, axis=1) - dl[np.arange(len(y)), y]))


def phi_d2(W, D, t, Xa, cost, w):
    """d2/dt2 f(W + t D)."""
    Z, dl = Xa @ W.T, Xa @ D.T
    Pr = softmax(Z + t * dl)
    m1 = np.sum(Pr * dl, axis=1, keepdims=True)
    return np.sum(D * D) + cost * np.sum(w * np.sum(Pr * (dl - m1) ** 2, axis=1))


# ------------------------------------------------------------------------------------------------ what the row kernels write, per problem
def softmax_operand(Z, y, cost, w):
    """(Pr, S, loss) of one problem: Z float [N][C], w [N]."""
    Z = np.asarray(Z, np.float64)
    ls, lse = log_softmax(Z)
    Pr = np.exp(ls)
    cw = cost * np.asarray(w, np.float64)
    S = cw[:, None] * (Pr - onehot(y, Z.shape[1]))
    return Pr, S, float(np.sum(cw * (lse - Z[np.arange(len(y)), y])))


def hess_operand(Pr, Q, cost, w):
    Pr, Q = np.asarray(Pr, np.float64), np.asarray(Q, np.float64)
    cw = cost * np.asarray(w, np.float64)
    return cw[:, None] * (Pr * Q - Pr * np.sum(Pr * Q, axis=1, keepdims=True))


def ray_sums(Z, dl, y, cost, w, t):
    """(sum_i c w (<pi, d> - d_y), sum_i c w Var_pi(d)) with pi = softmax(z + t d)."""
    Z, dl = np.asarray(Z, np.float64), np.asarray(dl, np.float64)
    Pr = softmax(Z + t * dl)
    cw = cost * np.asarray(w, np.float64)
    m1 = np.sum(Pr * dl, axis=1)
    var = np.sum(Pr * (dl - m1[:, None]) ** 2, axis=1)
    return float(np.sum(cw * (m1 - dl[np.arange(len(y)), y]))), float(np.sum(cw * var))


def rel_grad(W, X, y, cost, w):
    """|grad f(W)| / |grad f(0)| in float64, W [C][D + 1]."""
    Xa = augment(X)
    w = np.asarray(w, np.float64)
    g = gradient(np.asarray(W, np.float64), Xa, y, cost, w)
    g0 = gradient(np.zeros_like(g), Xa, y, cost, w)
    return float(np.linalg.norm(g) / np.linalg.norm(g0)), float(np.linalg.norm(g0))


# ------------------------------------------------------------------------------------------------ inputs of the row-kernel tests (simulator and GPU)
KERNEL_SHAPES = [(5, 1, 3), (70, 3, 7), (130, 2, 33), (600, 5, 130)]      # (N, P, C)
SENT = 777.0


def ceil8(n):
    return (n + 7) // 8 * 8


def aligned(shape, fill=0.0):
    """A float32 array of `shape` whose data starts on a 16-byte boundary."""
    n = int(np.prod(shape))
    raw = np.empty(n + 4, np.float32)
    off = (-raw.ctypes.data // 4) % 4
    a = raw[off:off + n].reshape(shape)
    a[...] = fill
    assert a.ctypes.data % 16 == 0
    return a


def kernel_problem(N, P, Cn, extra=8):
    """Row operands [N + 1][ldz] with ldz = P * Cp + extra, sentinel-filled outside [N][P * Cp]; logits up to +-90; weights with zeros."""
    rng = np.random.default_rng(N * 31 + P * 7 + Cn)
    Cp = ceil8(Cn)
    ldz = P * Cp + extra
    Z = aligned((N + 1, ldz), SENT)
    Dl = aligned((N + 1, ldz), SENT)
    for p in range(P):
        scale = rng.choice([0.5, 5.0, 90.0], size=(N, 1))               # small to large rows
        Z[:N, p * Cp:p * Cp + Cn] = rng.uniform(-1, 1, (N, Cn)) * scale
        Dl[:N, p * Cp:p * Cp + Cn] = rng.standard_normal((N, Cn)) * rng.choice([0.1, 2.0], size=(N, 1))
        Z[:N, p * Cp + Cn:(p + 1) * Cp] = 55.0                            # padding columns must not leak into a softmax
        Dl[:N, p * Cp + Cn:(p + 1) * Cp] = np.nan                         # nor may whatever the padding of delta holds
    y = rng.integers(0, Cn, N).astype(np.int32)
    w = np.ascontiguousarray(rng.choice([0.0, 0.5, 1.0, 2.0], size=(N, P)), np.float32)
    costs = np.ascontiguousarray(rng.choice([0.1, 1.0, 30.0], size=P), np.float32)
    return Z, Dl, y, w, costs, Cp, ldz


# ------------------------------------------------------------------------------------------------ checks of the vector kernels (simulator and GPU)
# Each takes call(name, *args) -> return code, which runs clite_logreg_<name> on float32 NumPy arrays (updated in place) and plain scalars, the
# stream argument left to it: through ctypes on the simulator, through device copies on the GPU.
ST = 24                                                                    # include/clite.h CLITE_LOGREG_STATE and the columns of the table
S_G0, S_GN, S_REL, S_STEP, S_NEWTON, S_CGIT, S_CGTOT, S_ACTIVE, S_CGACT, S_DPHI0 = 0, 1, 2, 5, 6, 7, 8, 9, 10, 12
S_T, S_LO, S_HI, S_WD, S_DD, S_LSDONE, S_EVALS = 13, 14, 15, 16, 17, 18, 21
ROWS = 32


def f32(a):
    return np.ascontiguousarray(a, np.float32)


def nblocks(N):
    return (N + ROWS - 1) // ROWS


def run_steps(call, N, P, st, dphi, d2phi, evals):
    """Drive ray_step with exact partials of the given phi'(t) - (wd + t dd) and phi''(t) - dd, spread over the row blocks."""
    nb = nblocks(N)
    for e in range(evals):
        work = np.zeros(2 * nb * P, np.float32)
        for p in range(P):
            t = float(st[p, S_T])
            a = dphi[p](t) - (float(st[p, S_WD]) + t * float(st[p, S_DD]))
            b = d2phi[p](t) - float(st[p, S_DD])
            work[np.arange(nb) * P + p] = a / nb
            work[nb * P + np.arange(nb) * P + p] = b / nb
        assert call("ray_step", work, N, P, st, int(e == evals - 1)) == 0


def _convex_phis(cases):
    """phi_p(t) = 1/2 dd t^2 + wd t + a (exp(k t) - k t) for (wd, dd, a, k): convex, phi'(0) = wd < 0. Returns (phi', phi'', the state table)."""
    dphi = [lambda t, c=c: c[0] + c[1] * t + c[2] * c[3] * (np.exp(c[3] * t) - 1) for c in cases]
    d2phi = [lambda t, c=c: c[1] + c[2] * c[3] ** 2 * np.exp(c[3] * t) for c in cases]
    st = f32(np.zeros((len(cases), ST)))
    for p, c in enumerate(cases):
        st[p, [S_ACTIVE, S_T, S_LO, S_HI, S_WD, S_DD, S_DPHI0]] = [1.0, 1.0, 0.0, np.inf, c[0], c[1], c[0]]
    return dphi, d2phi, st


def check_ray_step_finds_the_minimiser_of_a_convex_phi(call):
    """Minimisers right of 1, far right of 1 and left of 1; 100 rows are 4 row blocks."""
    cases = [(-1.0, 2.0, 0.5, 1.5), (-3.0, 0.5, 0.05, 0.8), (-40.0, 1.0, 1.0, 0.1), (-2.0, 1.0, 3.0, 2.5)]
    dphi, d2phi, st = _convex_phis(cases)
    run_steps(call, 100, len(cases), st, dphi, d2phi, 12)
    for p in range(len(cases)):
        lo, hi = 0.0, 64.0
        for _ in range(200):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if dphi[p](mid) < 0 else (lo, mid)
        t = float(st[p, S_STEP])
        assert st[p, S_LSDONE] == 1 and abs(dphi[p](t)) <= 2e-4 * abs(cases[p][0]), (p, t, lo, dphi[p](t))
        assert abs(t - lo) <= 1e-3 * lo, (p, t, lo)
        assert st[p, S_EVALS] <= 12


def check_ray_step_out_of_evaluations(call):
    """Two evaluations are too few for both problems. Problem 0 (minimiser at 3.4): phi'(1) < 0, the Newton step lands right of the minimiser,
    so the bracket is [1, 5.3] and the step its left end, t = 1. Problem 1 (minimiser at 0.1): phi' > 0 at t = 1 and at the Newton point 0.64,
    where phi is 9.0 against phi(0) = 3; no point left of the minimiser was found and the step is 0, not an ascent."""
    cases = [(-3.0, 0.5, 0.05, 0.8), (-2.0, 1.0, 3.0, 2.5)]
    dphi, d2phi, st = _convex_phis(cases)
    run_steps(call, 100, 2, st, dphi, d2phi, 2)
    assert list(st[:, S_LSDONE]) == [1, 1] and list(st[:, S_EVALS]) == [2, 2]
    assert st[0, S_STEP] == 1.0 and st[0, S_LO] == 1.0 and 5.0 < st[0, S_HI] < 5.6 and dphi[0](1.0) < 0 < dphi[0](float(st[0, S_HI]))
    assert st[1, S_STEP] == 0.0 and st[1, S_LO] == 0.0 and 0.6 < st[1, S_HI] < 0.68 and dphi[1](float(st[1, S_HI])) > 0
    # a finished search is left alone by further steps
    before = st.copy()
    run_steps(call, 100, 2, st, dphi, d2phi, 1)
    assert np.array_equal(st, before)


def check_ray_begin_refuses_a_non_descent_direction_and_finish_updates(call):
    rng = np.random.default_rng(2)
    P, n, ld = 4, 200, 208
    G, W, D = (f32(rng.standard_normal((P, ld))) for _ in range(3))
    D[0, :n] = -G[0, :n]                                                  # descent
    D[1, :n] = G[1, :n]                                                   # ascent: t = 0
    D[2, :n] = -G[2, :n]                                                  # descent but frozen: t = 0
    D[3, :n] = -0.5 * G[3, :n]
    st = f32(np.zeros((P, ST)))
    st[:, S_ACTIVE] = [1, 1, 0, 1]
    assert call("ray_begin", G, W, D, ld, n, P, st) == 0
    assert list(st[:, S_LSDONE]) == [0, 1, 1, 0] and list(st[:, S_T]) == [1, 0, 0, 1] and not st[:, S_STEP].any()
    for p in range(P):
        g, w, d = (a[p, :n].astype(np.float64) for a in (G, W, D))
        np.testing.assert_allclose(st[p, [S_DPHI0, S_WD, S_DD]], [g @ d, w @ d, d @ d], rtol=1e-6, atol=1e-6)
    # a quadratic phi: phi'(t) = d0 + t h, so that the first Newton step from t = 1 lands on t* = -d0 / h
    d0, dd = (st[:, k].astype(np.float64) for k in (S_DPHI0, S_DD))
    h = dd + 3.0
    dphi = [lambda t, p=p: d0[p] + t * h[p] for p in range(P)]
    d2phi = [lambda t, p=p: h[p] for p in range(P)]
    run_steps(call, 40, P, st, dphi, d2phi, 4)
    W0 = W.copy()
    assert call("ray_finish", W, D, ld, n, P, st) == 0
    for p in range(P):
        t = float(st[p, S_STEP])
        if p in (1, 2):
            assert t == 0 and np.array_equal(W[p], W0[p])
        else:
            assert abs(t + d0[p] / h[p]) <= 1e-3 * abs(d0[p] / h[p])
            np.testing.assert_allclose(W[p, :n], W0[p, :n] + np.float32(t) * D[p, :n], rtol=1e-6, atol=1e-6)
            assert np.array_equal(W[p, n:], W0[p, n:])


def check_newton_begin_g0_and_cg_on_explicit_systems(call):
    """g0_only records |G| and writes nothing else; the normal call uses it for the stopping test. CG on H_p = I + A_p^T A_p against float64:
    problem 1 is frozen, problem 2 converged (gradient small against its g0), problem 3 has a zero gradient."""
    rng = np.random.default_rng(3)
    P, n, ld = 5, 300, 304                                               # n > 256: more than one element per thread
    A = rng.standard_normal((P, 12, n)) * 0.3
    G = f32(np.zeros((P, ld)))
    G[:, :n] = rng.standard_normal((P, n))
    G[3] = 0.0
    st = f32(np.zeros((P, ST)))
    st[:, S_ACTIVE] = [1, 0, 1, 1, 1]
    X, Rr, D = (f32(np.full((P, ld), 5.0)) for _ in range(3))
    G0 = G.copy()
    G0[2] *= 1e7
    assert call("newton_begin", G0, ld, n, P, X, Rr, D, st, 1e-5, 30, 0.1, 1) == 0
    gn = np.linalg.norm(G[:, :n].astype(np.float64), axis=1)
    np.testing.assert_allclose(st[:, S_G0], np.linalg.norm(G0[:, :n].astype(np.float64), axis=1), rtol=1e-6)
    assert (X == 5).all() and (Rr == 5).all() and (D == 5).all() and not st[:, S_NEWTON].any() and list(st[:, S_ACTIVE]) == [1, 0, 1, 1, 1]
    assert call("newton_begin", G, ld, n, P, X, Rr, D, st, 1e-5, 30, 0.1, 0) == 0
    assert list(st[:, S_ACTIVE]) == [1, 0, 0, 0, 1] and list(st[:, S_CGACT]) == [1, 0, 0, 0, 1]
    assert st[0, S_NEWTON] == 1 and st[2, S_NEWTON] == 0 and st[3, S_REL] == 0 and abs(st[0, S_REL] - 1) < 1e-6
    for p in (0, 4):
        assert not X[p, :n].any() and np.array_equal(Rr[p, :n], -G[p, :n]) and np.array_equal(D[p, :n], -G[p, :n])
        assert (X[p, n:] == 5).all()
    frozen = [X[q].copy() for q in (1, 2, 3)]
    Hm = np.eye(n)[None] + np.einsum("pki,pkj->pij", A, A)
    x64, r64 = np.zeros((P, n)), -G[:, :n].astype(np.float64)
    d64, rr64 = r64.copy(), (r64 * r64).sum(1)
    done = np.zeros(P, bool)
    for it in range(14):
        HD = f32(np.zeros((P, ld)))
        HD[:, :n] = np.einsum("pij,pj->pi", Hm, D[:, :n].astype(np.float64))
        assert call("cg_update", HD, ld, n, P, X, Rr, D, st) == 0
        for p in (0, 4):
            if done[p]:
                continue
            hd = Hm[p] @ d64[p]
            a = rr64[p] / (d64[p] @ hd)
            x64[p] += a * d64[p]
            r64[p] -= a * hd
            rn = r64[p] @ r64[p]
            if rn <= (0.1 * gn[p]) ** 2:
                done[p] = True
                continue
            d64[p] = r64[p] + rn / rr64[p] * d64[p]
            rr64[p] = rn
    assert done.sum() == 2 and st[0, S_CGACT] == 0 and st[4, S_CGACT] == 0 and 0 < st[0, S_CGIT] == st[0, S_CGTOT] < 14
    for p in (0, 4):
        np.testing.assert_allclose(X[p, :n], x64[p], rtol=2e-3, atol=2e-4 * np.abs(x64[p]).max())
    for q, x in zip((1, 2, 3), frozen):
        assert np.array_equal(X[q], x)


def check_newton_begin_stops_a_problem_after_a_zero_step(call):
    """A line search that ended at step 0 left W where it was, so the next Newton iteration would repeat the last one: newton_begin freezes such
    a problem (problem 0, its ratio still above tol) and goes on with one whose last step moved (problem 1) or that has taken no step yet (2)."""
    rng = np.random.default_rng(4)
    P, n = 3, 40
    G = f32(rng.standard_normal((P, n)))
    st = f32(np.zeros((P, ST)))
    st[:, S_ACTIVE] = 1.0
    st[:, S_G0] = np.linalg.norm(G.astype(np.float64), axis=1) * 2
    st[:, S_NEWTON] = [2, 2, 0]
    st[:, S_STEP] = [0.0, 0.5, 0.0]
    X, Rr, D = (f32(np.full((P, n), 5.0)) for _ in range(3))
    assert call("newton_begin", G, n, n, P, X, Rr, D, st, 1e-5, 30, 0.1, 0) == 0
    assert list(st[:, S_ACTIVE]) == [0, 1, 1] and list(st[:, S_CGACT]) == [0, 1, 1] and list(st[:, S_NEWTON]) == [2, 3, 1]
    np.testing.assert_allclose(st[:, S_REL], 0.5, rtol=1e-6)
    assert (X[0] == 5).all() and (D[0] == 5).all() and not X[1:].any() and np.array_equal(D[1:], -G[1:])
