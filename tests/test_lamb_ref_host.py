"""tests/lamb_ref.py (the float64 definition the LAMB kernels are held to) against something independent of it: torch.optim.AdamW when nothing is
adapted, LAMB's defining property |p_new - p| = lr |p|, a few-line restatement of Algorithm 2 (You et al. 2020) per tensor with numpy norms, and
the zero-norm conventions. CPU only."""
import numpy as np
import torch

import lamb_ref as L
import loss_ref as R

SIZES = [(12, True), (7, False), (40, True), (3, False)]          # (elements, adapted); a gap of 5 elements follows every tensor
B1, B2, EPS = 0.9, 0.999, 1e-6


def _layout():
    tensors, start = [], 3
    for n, ad in SIZES:
        tensors.append(L.Tensor(start, n, ad))
        start += n + 5
    return tensors, start


def _problem(seed):
    tensors, n = _layout()
    rng = np.random.default_rng(seed)
    p, slow = (rng.standard_normal(n).astype(np.float32) for _ in range(2))
    lr, wd = np.zeros(n), np.zeros(n)
    inside = np.zeros(n, bool)
    for i, t in enumerate(tensors):
        lr[t.start:t.start + t.n] = L.f32((3e-3, 1e-3)[i % 2])
        wd[t.start:t.start + t.n] = L.f32((1e-2, 0.0, 5e-2, 1e-2)[i])
        inside[t.start:t.start + t.n] = True
    return tensors, n, rng, p, slow, lr, wd, inside


def _step(p, g, m, v2, slow, lr, wd, max_norm, sync, gs, step, sumsq, trust_clip, tensors):
    return L.lamb_step_ref(p, g, m, v2, slow, lr, wd, max_norm, sync, 0.5, gs, B2, EPS, 1 - B1 ** step, 1 - B2 ** step, 1 - B1, 1 - B2, sumsq, trust_clip,
                           tensors)


def test_nothing_adapted_is_torch_adamw_over_four_steps():
    """torch.optim.AdamW in float64, one parameter and one group per tensor, clip_grad_norm_ for the clip (max_norm 0.05: active on steps 0 and 2)."""
    tensors, n, rng, p0, _, lr, wd, inside = _problem(0)
    plain = [L.Tensor(t.start, t.n, False) for t in tensors]
    params = [torch.nn.Parameter(torch.tensor(p0[t.start:t.start + t.n], dtype=torch.float64)) for t in tensors]
    opt = torch.optim.AdamW([{"params": [q], "lr": float(lr[t.start]), "weight_decay": float(wd[t.start])} for q, t in zip(params, tensors)],
                            betas=(B1, B2), eps=EPS)
    p, m, v2, slow = p0.astype(np.float64), np.zeros(n), np.zeros(n), np.zeros(n)
    max_norm = 0.05
    for step in range(4):
        g = (rng.standard_normal(n) * (0.03, 0.003)[step % 2]).astype(np.float32)
        for q, t in zip(params, tensors):
            q.grad = torch.tensor(g[t.start:t.start + t.n], dtype=torch.float64)
        total = float(torch.nn.utils.clip_grad_norm_(params, max_norm))
        assert (total > max_norm) == (step % 2 == 0)
        opt.step()
        sumsq = (g[inside].astype(np.float64) ** 2).sum()
        st = _step(p, g, m, v2, slow, lr, wd, max_norm, False, 1.0, step + 1, sumsq, step % 2 == 1, plain)
        p, m, v2 = st.p, st.m, st.v2
        assert (st.q == 1.0).all()
        for q, t in zip(params, tensors):
            s = slice(t.start, t.start + t.n)
            for got, want in ((p[s], q.detach().numpy()), (m[s], opt.state[q]["exp_avg"].numpy()), (v2[s], opt.state[q]["exp_avg_sq"].numpy())):
                assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), (step, t)
    assert np.array_equal(p[~inside], p0.astype(np.float64)[~inside]) and not m[~inside].any() and not v2[~inside].any()


def test_nothing_adapted_is_the_adamw_reference():
    tensors, n, rng, p, slow, lr, wd, inside = _problem(1)
    g = (rng.standard_normal(n) * 0.01).astype(np.float32)
    m = (rng.standard_normal(n) * 0.01).astype(np.float32)
    v2 = (m.astype(np.float64) ** 2 * 1.5).astype(np.float32)
    plain = [L.Tensor(t.start, t.n, False) for t in tensors]
    sumsq = (g.astype(np.float64) ** 2).sum()
    for sync, max_norm in ((False, 0.0), (True, 0.02)):
        st = _step(p, g, m, v2, slow, lr, wd, max_norm, sync, L.f32(0.25), 7, sumsq, False, plain)
        rp, rm, rv2, rs = R.adamw_step_ref(p, g, m, v2, slow, lr, wd, max_norm, sync, 0.5, L.f32(0.25), B2, EPS, 1 - B1 ** 7, 1 - B2 ** 7, 1 - B1, 1 - B2, sumsq)
        for got, want in ((st.p, rp), (st.m, rm), (st.v2, rv2), (st.slow, rs)):          # p (1 - lr wd) - lr u against p - lr (u + wd p): float64 rounding
            assert np.abs(got - want)[inside].max() <= 1e-14 * max(1.0, np.abs(want[inside]).max())


def _algorithm_2(p, g, m, v, lr, wd, t, phi_clip):
    """Algorithm 2 of the paper for one tensor, phi the identity (or min(., 1))."""
    m = B1 * m + (1 - B1) * g
    v = B2 * v + (1 - B2) * g * g
    r = (m / (1 - B1 ** t)) / (np.sqrt(v / (1 - B2 ** t)) + EPS)
    upd = r + wd * p
    wn, un = np.linalg.norm(p), np.linalg.norm(upd)
    ratio = wn / un if wn > 0 and un > 0 else 1.0
    return p - lr * (min(ratio, 1.0) if phi_clip else ratio) * upd, m, v


def test_adapted_tensors_move_by_lr_times_their_norm_and_follow_algorithm_2():
    tensors, n, rng, p0, slow, lr, wd, inside = _problem(2)
    p0[tensors[2].start:tensors[2].start + tensors[2].n] *= np.float32(0.1)          # |u| is of order one per element: this tensor's ratio is below 1
    for trust_clip in (False, True):
        p, m, v2 = p0.astype(np.float64), np.zeros(n), np.zeros(n)
        ps = [p[t.start:t.start + t.n].copy() for t in tensors]
        ms, vs = [np.zeros(t.n) for t in tensors], [np.zeros(t.n) for t in tensors]
        clipped = []
        for step in range(1, 4):
            g = (rng.standard_normal(n) * 0.01).astype(np.float32)
            st = _step(p, g, m, v2, slow, lr, wd, 0.0, False, 1.0, step, float("nan"), trust_clip, tensors)
            free = _step(p, g, m, v2, slow, lr, wd, 0.0, False, 1.0, step, float("nan"), False, tensors)
            for i, t in enumerate(tensors):
                s = slice(t.start, t.start + t.n)
                q, rn, pn = st.q[t.start], np.linalg.norm(st.r[s]), np.linalg.norm(p[s])
                moved = np.linalg.norm(st.p[s] - p[s])
                assert abs(moved - lr[t.start] * q * rn) <= 1e-12 * moved
                if t.adapted:
                    assert st.q[t.start] <= free.q[t.start] and (trust_clip or st.q[t.start] == free.q[t.start])          # TRUST_CLIP only ever shrinks q
                    if trust_clip:
                        assert q == min(free.q[t.start], 1.0)
                        clipped.append(free.q[t.start] > 1.0)
                    else:
                        assert abs(moved - lr[t.start] * pn) <= 1e-12 * moved, "LAMB's defining property: the step's length is lr |p|"
                else:
                    assert q == 1.0
                ps[i], ms[i], vs[i] = _algorithm_2(ps[i], g[s].astype(np.float64), ms[i], vs[i], lr[t.start], wd[t.start], step, trust_clip) if t.adapted \
                    else (st.p[s], st.m[s], st.v2[s])
                assert np.abs(st.p[s] - ps[i]).max() <= 1e-12 * max(1.0, np.abs(ps[i]).max()), (step, i)
                assert np.abs(st.m[s] - ms[i]).max() <= 1e-15 and np.abs(st.v2[s] - vs[i]).max() <= 1e-15
            p, m, v2 = st.p, st.m, st.v2
        assert not trust_clip or (any(clipped) and not all(clipped))
    assert L.trust_ratio(3.0, 2.0) == 1.5 and L.trust_ratio(3.0, 2.0, True) == 1.0 and L.trust_ratio(1.0, 2.0, True) == 0.5


def test_zero_norms_give_a_ratio_of_one_and_no_nan():
    tensors, n, rng, p, slow, lr, wd, inside = _problem(3)
    g = (rng.standard_normal(n) * 0.01).astype(np.float32)
    m, v2 = np.zeros(n), np.zeros(n)
    t0, t2 = tensors[0], tensors[2]
    g[t0.start:t0.start + t0.n] = 0.0          # with zero moments and wd = 0: r = 0
    wd[t0.start:t0.start + t0.n] = 0.0
    p[t2.start:t2.start + t2.n] = 0.0          # |p| = 0
    st = _step(p, g, m, v2, slow, lr, wd, 0.0, False, 1.0, 1, float("nan"), False, tensors)
    for t in (t0, t2):
        assert (st.q[t.start:t.start + t.n] == 1.0).all()
    assert all(np.isfinite(a).all() for a in st)
    s0, s2 = slice(t0.start, t0.start + t0.n), slice(t2.start, t2.start + t2.n)
    assert np.array_equal(st.p[s0], p[s0].astype(np.float64)) and not st.r[s0].any()
    u = (st.m[s2] / (1 - B1)) / (np.sqrt(st.v2[s2] / (1 - B2)) + EPS)
    assert np.abs(st.p[s2] + lr[s2] * u).max() <= 1e-18 and np.abs(st.p[s2]).min() > 0          # the p = 0 tensor still moves, by lr u
    assert L.trust_ratio(0.0, 3.0) == 1.0 and L.trust_ratio(2.0, 0.0) == 1.0
