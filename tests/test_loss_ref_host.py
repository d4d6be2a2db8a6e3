"""Host-side checks of tests/loss_ref.py (no GPU).

(a) Every gradient the references return is compared with central finite differences in float64: step 1e-6 on six entries per tensor plus the
temperature, bound relative 1e-6 (truncation ~1e-10, rounding ~1e-9 at that step: only a wrong formula fails). The fixture
tests/golden/loss_b8_rn18.npz holds the encoders' features (img [8][512], txt [8][768]), the prior noise and the total / cross losses, but neither
the critic's projected inputs f1 / f2 nor the prior's hidden layer h1 (both come out of head weights the fixture does not store), so the critic
and prior values cannot be tied to it here; tests/test_oracle_golden.py ties the whole loss to that fixture.

(b) The shared checks of loss_ref.py on the wave simulator, at the shapes whose paths no other simulator test executes: the masked-class
cross-entropy, the prior tail's atomic branch (K = 520) with one and with two rows per wave, the critic's second to fourth chunk slots with both
negative pairings, InfoNCE's second lane trip. tests/test_gpu_loss_ops.py and tests/test_gpu_cls_ops.py run the same checks on the device."""
import numpy as np
import pytest
import torch

import loss_ref as R
from loss_backends import BF16, F32, SimBackend

H = 1e-6


def _fd_check(what, f, x, grad, picks):
    """f: float64 ndarray -> float; grad: the reference's gradient at x."""
    for idx in picks:
        xp, xm = x.copy(), x.copy()
        xp[idx] += H
        xm[idx] -= H
        fd = (f(xp) - f(xm)) / (2 * H)
        assert abs(grad[idx] - fd) <= 1e-6 * max(abs(fd), np.abs(grad).max()), (what, idx, grad[idx], fd)


def _picks(rng, shape, n=6):
    return [tuple(int(rng.integers(0, s)) for s in shape) for _ in range(n)]


def _tt(a):
    return torch.tensor(a, dtype=torch.float64)


@pytest.mark.parametrize("pairing", [None, "cluster", "random"])
def test_critic_gradients_match_finite_differences(pairing):
    rng = np.random.default_rng(1)
    B, D = 8, 24
    neg, _ = R.negative_pairing(pairing, B, rng)
    f1 = rng.standard_normal((B, D))
    f2 = rng.standard_normal((B, D)) + 0.5 * f1
    t, g = 1.3, 1.53
    ref = R.critic_ref(f1, f2, t, neg, gout=g)

    def loss(a, b, tt):
        sp, sn, _ = R.critic_loss(_tt(a), _tt(b), _tt(tt), neg)
        return g * (sp + sn).item()

    _fd_check("df1", lambda a: loss(a, f2, t), f1, ref.df1, _picks(rng, f1.shape))
    _fd_check("df2", lambda b: loss(f1, b, t), f2, ref.df2, _picks(rng, f2.shape))
    fd = (loss(f1, f2, t + H) - loss(f1, f2, t - H)) / (2 * H)
    assert abs(ref.dtemp - fd) <= 1e-6 * abs(fd)
    assert abs(ref.dtemp_terms.sum() - ref.dtemp) <= 1e-12 * np.abs(ref.dtemp_terms).sum()
    # the work row against torch.nn.functional, an independent formulation
    a, b = torch.nn.functional.normalize(_tt(f1), dim=-1), torch.nn.functional.normalize(_tt(f2), dim=-1)
    n1 = R.roll_by_one(B) if neg is None else neg
    assert np.allclose(ref.work[:, 3], (a * b).sum(1).numpy(), rtol=0, atol=1e-14)
    assert np.allclose(ref.work[:, 6], ((a * b[torch.as_tensor(n1, dtype=torch.long)]).sum(1) * np.exp(t)).numpy(), rtol=0, atol=1e-13)
    assert abs(ref.sum_pos - torch.nn.functional.softplus(-_tt(ref.work[:, 5])).mean().item()) < 1e-9          # F.softplus: threshold 20


def test_l2_normalize_backward_matches_finite_differences_and_autograd():
    rng = np.random.default_rng(2)
    x, dy = rng.standard_normal((5, 16)) * 3, rng.standard_normal((5, 16))
    y = R.l2_normalize_ref(x)
    assert np.allclose(y, torch.nn.functional.normalize(_tt(x), dim=-1).numpy(), rtol=0, atol=1e-15)
    dx = R.l2_normalize_bwd_ref(x, y, dy)
    assert np.abs(dx - R.l2_normalize_bwd_autograd(x, dy)).max() <= 1e-13
    _fd_check("dx", lambda a: float((R.l2_normalize_ref(a) * dy).sum()), x, dx, _picks(rng, x.shape))
    z = np.zeros((2, 8))
    z[1] = 1e-20
    assert not R.l2_normalize_ref(z)[0].any() and np.allclose(R.l2_normalize_ref(z)[1], 1e-8, rtol=1e-12)


@pytest.mark.parametrize("t", [R.T_CLIP, float(np.log(100.0))])
def test_infonce_gradients_match_finite_differences(t):
    rng = np.random.default_rng(3)
    B, g = 9, 1.17
    Cm = np.clip(rng.standard_normal((B, B)) * 0.3 + 0.5 * np.eye(B), -1, 1)
    ref = R.infonce_ref(Cm, t, gout=g)

    def loss(c, tt):
        sr, sc, _ = R.infonce_loss(_tt(c), _tt(tt))
        return g * (sr + sc).item()

    _fd_check("dC", lambda c: loss(c, t), Cm, ref.dC, _picks(rng, Cm.shape) + [(4, 4)])
    fd = (loss(Cm, t + H) - loss(Cm, t - H)) / (2 * H)
    assert abs(ref.dtemp - fd) <= 1e-6 * abs(fd)
    assert abs(ref.dtemp_terms.sum() - ref.dtemp) <= 1e-10 * np.abs(ref.dtemp_terms).sum()
    S = _tt(Cm) * np.exp(t)
    ce = torch.nn.functional.cross_entropy
    lab = torch.arange(B)
    assert abs(ref.sum_r + ref.sum_c - 0.5 * (ce(S, lab) + ce(S.T, lab)).item()) < 1e-12


@pytest.mark.parametrize("use_softplus", [False, True])
def test_prior_gradients_match_finite_differences(use_softplus):
    rng = np.random.default_rng(4)
    B, K, g = 4, 16, 0.2
    pre = rng.standard_normal((2 * B, K))
    pre[np.abs(pre) < 1e-3] = 0.5          # keep the finite-difference step away from the ReLU kink
    w2, b2 = rng.standard_normal(K) * 0.4, np.array([0.05])
    ref = R.prior_ref(np.maximum(pre, 0), w2, b2, use_softplus, gout=g)

    def loss(p, w, b):
        return g * R.prior_loss(torch.relu(_tt(p)), _tt(w), _tt(b), use_softplus)[0].item()

    # dh1 is the gradient w.r.t. the pre-activation: at negative pre-activations (h1 = 0) it is zero, which the differences confirm
    _fd_check("dh1", lambda p: loss(p, w2, b2), pre, ref.dh1, _picks(rng, pre.shape, 8))
    assert not ref.dh1[pre < 0].any() and ref.dh1[pre > 0].all()
    _fd_check("dw2", lambda w: loss(pre, w, b2), w2, ref.dw2, _picks(rng, w2.shape))
    _fd_check("db2", lambda b: loss(pre, w2, b), b2, np.array([ref.db2]), [(0,)])
    assert abs(ref.gl.sum() - ref.db2) < 1e-15
    other = R.prior_ref(np.maximum(pre, 0), w2, b2, not use_softplus, gout=g)
    assert abs(other.sum - ref.sum) < 1e-12          # the two forms are the same function


def test_xent_reference_matches_torch_and_finite_differences():
    rng = np.random.default_rng(5)
    B, Cc = 7, 11
    z = rng.standard_normal((B, Cc)) * 3
    y = rng.integers(0, Cc, B)
    y[3] = -100
    z[0, (y[0] + 1) % Cc] = z[2, (y[2] + 3) % Cc] = z[2, (y[2] + 4) % Cc] = -np.inf
    ref = R.xent_ref(z, y, 3)
    ce = torch.nn.functional.cross_entropy(_tt(z), torch.as_tensor(y), ignore_index=-100, reduction="sum").item()
    assert abs(ref.loss - ce) < 1e-12 and ref.count == 6 and np.isfinite(ref.lse).all()
    assert not ref.dlogits[np.isneginf(z)].any()

    def loss(a):
        return R.xent_ref(a, y, 3).loss / 6

    picks = [p for p in _picks(rng, z.shape, 12) if np.isfinite(z[p])]
    _fd_check("dlogits", loss, z, ref.dlogits, picks)
    want_lse = R.MASKED_ROW[2]
    assert abs(R.xent_ref(*R.MASKED_ROW[:2], 1).lse[0] - want_lse) < 1e-6


def test_update_references_match_torch_optimizers():
    rng = np.random.default_rng(6)
    n = 64
    p, g, v = rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(n)
    tp = torch.nn.Parameter(_tt(p))
    opt = torch.optim.SGD([tp], lr=0.1, momentum=0.9, weight_decay=1e-2)
    opt.state[tp]["momentum_buffer"] = _tt(v).clone()
    tp.grad = _tt(g) * 0.25
    total = torch.nn.utils.clip_grad_norm_([tp], 0.5).item()
    opt.step()
    sumsq = (g ** 2).sum()
    assert abs(total - np.sqrt(sumsq) * 0.25) < 1e-12
    rp, rv, _ = R.sgd_step_ref(p, g, v, p, 0.1, 1e-2, 0.9, 0.5, False, 0.5, 0.25, sumsq)
    assert np.abs(rp - tp.detach().numpy()).max() < 1e-12 and np.abs(rv - opt.state[tp]["momentum_buffer"].numpy()).max() < 1e-12
    sp, _, ss = R.sgd_step_ref(p, g, v, 2 * p, 0.1, 1e-2, 0.9, 0.0, True, 0.25, 1.0, float("nan"))          # max_norm 0: sumsq is not read
    up = R.sgd_step_ref(p, g, v, p, 0.1, 1e-2, 0.9, 0.0, False, 0.25, 1.0, 0.0)[0]
    assert np.allclose(sp, 0.25 * up + 0.75 * 2 * p, rtol=0, atol=1e-14) and ss is sp
    # AdamW: three steps of torch.optim.AdamW in float64
    tp = torch.nn.Parameter(_tt(p))
    opt = torch.optim.AdamW([tp], lr=1e-2, weight_decay=1e-2)
    m, v2, q = np.zeros(n), np.zeros(n), p.copy()
    for step in range(1, 4):
        gs = rng.standard_normal(n)
        tp.grad = _tt(gs)
        opt.step()
        q, m, v2, _ = R.adamw_step_ref(q, gs, m, v2, q, 1e-2, 1e-2, 0.0, False, 1.0, 1.0, 0.999, 1e-8, 1 - 0.9 ** step, 1 - 0.999 ** step,
                                       1 - 0.9, 1 - 0.999, 0.0)
        assert np.abs(q - tp.detach().numpy()).max() < 1e-12
    bits = R.to_bf16_bits(np.array([1.0, 1.00390625, 1.01171875, -0.0], np.float32))          # 0x3F808000 ties to even (down), 0x3F818000 ties up
    assert list(bits) == [0x3F80, 0x3F80, 0x3F82, 0x8000]
    t = torch.tensor(rng.standard_normal(1000), dtype=torch.float32)
    assert np.array_equal(R.to_bf16_bits(t.numpy()), t.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16))


# ------------------------------------------------------------------------------------------------ (b) never-run paths, on the simulator
@pytest.fixture(scope="module")
def sim():
    return SimBackend()


DTS = [BF16, F32]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("Cc,B", [(10, 7), (1030, 9)])
def test_sim_xent_masked_classes(sim, dt, Cc, B):
    R.check_xent(sim, dt, Cc, B, 5, masked=True)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("use_softplus", [False, True])
@pytest.mark.parametrize("B,K", [(5, 520), (37, 520)])
def test_sim_prior_tail_wide_k(sim, dt, B, K, use_softplus):
    """K = 520: 65 chunks, one_chunk is false and dw2 takes the per-element atomic branch; 2B = 74 rows on the capped grid of 64 waves."""
    R.check_prior_tail(sim, dt, B, K, use_softplus)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("pairing", [None, "cluster"])
@pytest.mark.parametrize("B,D", [(7, 520), (130, 2048)])
def test_sim_critic_chunk_slots(sim, dt, B, D, pairing):
    R.check_critic(sim, dt, B, D, pairing if B % 2 == 0 else (pairing and "random"))


@pytest.mark.parametrize("dt", DTS)
def test_sim_infonce_second_lane_trip(sim, dt):
    R.check_infonce(sim, dt, 72, 80, 72, R.T_CLIP)
    R.check_infonce(sim, dt, 72, 80, 72, float(np.log(100.0)), with_dtemp=False)


def test_sim_rejects_and_small_ops(sim):
    for dt in DTS:
        R.check_critic_rejects(sim, dt)
        R.check_l2_normalize(sim, dt, 7, 520)
        R.check_add(sim, dt, 4104)
    R.check_loss_finalize(sim)
