"""tests/lars_ref.py (the float64 definition the LARS kernels are held to) against something independent of it: torch.optim.SGD fed the LARS
gradients with trust ratios from torch.linalg.norm, loss_ref.sgd_step_ref when nothing is adapted, and the zero-norm cases. CPU only."""
import numpy as np
import torch

import lars_ref as L
import loss_ref as R

SIZES = [(12, True), (7, False), (40, True), (3, False)]          # (elements, adapted); a gap of 5 elements follows every tensor


def _layout():
    tensors, start = [], 3
    for n, ad in SIZES:
        tensors.append(L.Tensor(start, n, ad))
        start += n + 5
    return tensors, start


def _problem(seed):
    tensors, n = _layout()
    rng = np.random.default_rng(seed)
    p, v, slow = (rng.standard_normal(n).astype(np.float32) for _ in range(3))
    lr, wd = np.zeros(n), np.zeros(n)
    for i, t in enumerate(tensors):
        lr[t.start:t.start + t.n] = L.f32((0.2, 1e-3)[i % 2])
        wd[t.start:t.start + t.n] = L.f32((1e-4, 0.0, 5e-2, 1e-2)[i])
    return tensors, n, rng, p, v, slow, lr, wd


def test_three_momentum_steps_equal_torch_sgd_on_lars_gradients():
    """torch.optim.SGD(momentum, weight_decay = 0) in float64, one parameter per tensor, its .grad set to q (g' + wd p) with q from plain
    torch.linalg.norm — the way LARS wrappers around torch.optim.SGD work. Clipping (max_norm 2) is active on the first step only."""
    tensors, n, rng, p0, v0, _, lr, wd = _problem(0)
    mu, gs, eta, eps, max_norm = L.f32(0.9), L.f32(0.25), L.f32(0.02), L.f32(1e-8), L.f32(2.0)
    params = [torch.nn.Parameter(torch.tensor(p0[t.start:t.start + t.n], dtype=torch.float64)) for t in tensors]
    opt = torch.optim.SGD([{"params": [q], "lr": float(lr[t.start])} for q, t in zip(params, tensors)], lr=1.0, momentum=mu, weight_decay=0.0)
    p, v, slow = p0.astype(np.float64), np.zeros(n), np.zeros(n)          # torch starts its momentum buffer as the first gradient: v = 0 here
    for step in range(3):
        g = (rng.standard_normal(n) * (30.0, 0.3, 0.5)[step]).astype(np.float32)
        inside = np.zeros(n, bool)
        for t in tensors:
            inside[t.start:t.start + t.n] = True
        sumsq = L.f32((g[inside].astype(np.float64) ** 2).sum())
        total = torch.sqrt(torch.tensor(sumsq, dtype=torch.float64)) * gs
        clip = min(max_norm / (float(total) + 1e-6), 1.0)
        assert (clip < 1.0) == (step == 0)
        for q, t in zip(params, tensors):
            gt = torch.tensor(g[t.start:t.start + t.n], dtype=torch.float64) * gs * clip
            w = float(wd[t.start])
            ratio = 1.0
            if t.adapted:
                pn, gn = torch.linalg.norm(q.detach()), torch.linalg.norm(gt)
                ratio = float(eta * pn / (gn + w * pn + eps))
            q.grad = ratio * (gt + w * q.detach())
        opt.step()
        st = L.lars_step_ref(p, g, v, slow, lr, wd, mu, max_norm, False, 1.0, gs, sumsq, eta, eps, tensors)
        p, v = st.p, st.v
        for q, t in zip(params, tensors):
            got, want = p[t.start:t.start + t.n], q.detach().numpy()
            assert np.abs(got - want).max() <= 1e-13 * max(1.0, np.abs(want).max()), (step, t)
            buf = opt.state[q]["momentum_buffer"].numpy()
            assert np.abs(v[t.start:t.start + t.n] - buf).max() <= 1e-13 * max(1.0, np.abs(buf).max()), (step, t)
            assert t.adapted == bool((st.q[t.start:t.start + t.n] != 1.0).all())
    gaps = ~inside
    assert np.array_equal(p[gaps], p0.astype(np.float64)[gaps]) and not v[gaps].any()


def test_nothing_adapted_is_the_sgd_reference():
    tensors, n, rng, p, v, slow, lr, wd = _problem(1)
    g = rng.standard_normal(n).astype(np.float32)
    plain = [L.Tensor(t.start, t.n, False) for t in tensors]
    inside = np.zeros(n, bool)
    for t in tensors:
        inside[t.start:t.start + t.n] = True
    for sync, max_norm in ((False, 0.0), (True, 1.5)):
        sumsq = L.f32((g.astype(np.float64) ** 2).sum())
        st = L.lars_step_ref(p, g, v, slow, lr, wd, L.f32(0.9), max_norm, sync, 0.5, L.f32(0.25), sumsq, L.f32(0.001), L.f32(1e-8), plain)
        rp, rv, rs = R.sgd_step_ref(p, g, v, slow, lr, wd, L.f32(0.9), max_norm, sync, 0.5, L.f32(0.25), sumsq)
        for got, want in ((st.p, rp), (st.v, rv), (st.slow, rs)):
            assert np.array_equal(got[inside], want[inside])
        assert (st.q == 1.0).all()


def test_zero_norms_give_a_ratio_of_one_and_no_nan():
    tensors, n, rng, p, v, slow, lr, wd = _problem(2)
    g = rng.standard_normal(n).astype(np.float32)
    t0, t2 = tensors[0], tensors[2]
    g[t0.start:t0.start + t0.n] = 0.0          # gn = 0
    p[t2.start:t2.start + t2.n] = 0.0          # pn = 0
    st = L.lars_step_ref(p, g, v, slow, lr, wd, L.f32(0.9), 0.0, True, 0.5, 1.0, float("nan"), L.f32(0.001), 0.0, tensors)
    for t in (t0, t2):
        assert (st.q[t.start:t.start + t.n] == 1.0).all()
    assert all(np.isfinite(a).all() for a in (st.p, st.v, st.slow, st.q, st.u))
    rp, rv, rs = R.sgd_step_ref(p, g, v, slow, lr, wd, L.f32(0.9), 0.0, True, 0.5, 1.0, float("nan"))
    for t in (t0, t2):          # with q = 1 the tensor moves as under SGD
        s = slice(t.start, t.start + t.n)
        assert np.array_equal(st.p[s], rp[s]) and np.array_equal(st.v[s], rv[s]) and np.array_equal(st.slow[s], rs[s])
    assert L.trust_ratio(0.0, 3.0, 0.1, 0.001, 0.0) == 1.0 and L.trust_ratio(2.0, 0.0, 0.1, 0.001, 0.0) == 1.0
    assert abs(L.trust_ratio(2.0, 3.0, 0.5, 0.1, 0.0) - 0.1 * 2.0 / 4.0) < 1e-15
