"""float64 references of the loss, cross-entropy and parameter-update kernels (csrc/loss_ops.hip, csrc/cls_ops.hip, csrc/optim_ops.hip, csrc/update_ops.hip), written
from the operations' definitions on plain numpy / torch-CPU float64 (gradients from torch.autograd). Nothing here calls into clip_lite_amd or the
wave simulator. Every function takes the STORAGE-ROUNDED inputs (a bf16 input is rounded before it gets here, as in tests/resnet_ref.py) and
returns every output of the kernel, all float64 numpy. tests/test_loss_ref_host.py checks every gradient against central finite differences.

The second half (`check_*`) holds the checks that the wave simulator and the device share. They see the kernels through a backend
(tests/loss_backends.py): `dev` puts a numpy array into the backend's storage, `host` reads it back as numpy, `call` invokes a C entry by name with
the arguments in the C order and returns its status. The bounds are those of tests/test_gpu_resnet_ops.py (ref = float64 on the stored inputs):
  element-wise, stored f32   |got - ref| <= 2e-5 * max|ref|
  element-wise, stored bf16  |got - ref| <= 2^-7 * |ref| + 2e-5 * max|ref|
  vector accumulators        |got - ref| <= 1e-4 * max|ref|                        (dw2, lse_r, lse_c, lse)
  scalar accumulators        |got - ref| <= 1e-5 * max(1, sum|terms|)              (loss sums, dtemp, db2, xent acc[0], sumsq)
  counters, padding, sentinels: exact. No element is skipped."""
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

BF16, F32 = 0, 1
T_CLIP = float(np.float32(np.log(1 / 0.07)))

Critic = namedtuple("Critic", "work sum_pos sum_neg terms_pos terms_neg df1 df2 dtemp dtemp_terms")
InfoNCE = namedtuple("InfoNCE", "lse_r lse_c sum_r sum_c terms_r terms_c dC dtemp dtemp_terms")
Prior = namedtuple("Prior", "logit sum terms dh1 dw2 db2 gl")
Xent = namedtuple("Xent", "lse loss top1 topk count dlogits terms")


def _t(a, grad=False):
    return torch.tensor(np.asarray(a, np.float64), dtype=torch.float64, requires_grad=grad)


def _np(t):
    return t.detach().numpy()


def softplus(x):
    """log(1 + exp(x)) without F.softplus's threshold (which is an approximation in float64)."""
    return torch.logaddexp(torch.zeros_like(x), x)


def roll_by_one(B):
    return (np.arange(B) + 1) % B


def cluster_pairing(B):
    """The hard-negative permutation [B/2 + i | (i + 1) mod B/2] (even B)."""
    h = B // 2
    return np.concatenate([np.arange(h) + h, (np.arange(h) + 1) % h])


def inverse_of(neg):
    inv = np.empty(len(neg), np.int64)
    inv[np.asarray(neg)] = np.arange(len(neg))
    return inv


# ------------------------------------------------------------------------------------------------ critic
def critic_loss(f1, f2, temperature, neg=None):
    """(sum softplus(-o+)/B, sum softplus(o-)/B, parts) of the dot critic on torch float64 tensors."""
    B = f1.shape[0]
    neg = torch.as_tensor(roll_by_one(B) if neg is None else np.asarray(neg), dtype=torch.long)
    na = f1.norm(dim=1).clamp_min(1e-12)
    nb = f2.norm(dim=1).clamp_min(1e-12)
    a, b = f1 / na[:, None], f2 / nb[:, None]            # F.normalize(eps=1e-12)
    cp, cn = (a * b).sum(1), (a * b[neg]).sum(1)
    ts = torch.exp(temperature)
    op, on = cp * ts, cn * ts
    tp, tn = softplus(-op) / B, softplus(on) / B
    return tp.sum(), tn.sum(), (na, nb, nb[neg], cp, cn, op, on, tp, tn)


def critic_ref(f1, f2, temperature, neg=None, gout=1.0):
    """gout: the upstream gradient times the launcher's `scale`."""
    f1, f2, t = _t(f1, True), _t(f2, True), _t(temperature, True)
    sp, sn, (na, nb, nc, cp, cn, op, on, tp, tn) = critic_loss(f1, f2, t, neg)
    d1, d2, dt = torch.autograd.grad((sp + sn) * gout, (f1, f2, t))
    work = torch.stack([na, nb, nc, cp, cn, op, on, torch.zeros_like(na)], 1)
    # per-row contributions to dtemp: d/dt of softplus(-o+) + softplus(o-) with do/dt = o
    dtt = gout / f1.shape[0] * (-torch.sigmoid(-op) * op + torch.sigmoid(on) * on)
    return Critic(_np(work), sp.item(), sn.item(), _np(tp), _np(tn), _np(d1), _np(d2), dt.item(), _np(dtt))


# ------------------------------------------------------------------------------------------------ l2_normalize
def l2_normalize_ref(x):
    x = _t(x)
    return _np(x / x.norm(dim=1, keepdim=True).clamp_min(1e-12))


def l2_normalize_bwd_ref(x, y, dy):
    """dx of y = x / max(|x|, eps) for the upstream dy, with the stored forward result y as the kernel's third input:
    dx = (dy - y <dy, y>) / max(|x|, eps). (With |x| < eps the exact Jacobian is dy / eps; y <dy, y> is then below 1e-16 of it.)"""
    x, y, dy = _t(x), _t(y), _t(dy)
    n = x.norm(dim=1, keepdim=True).clamp_min(1e-12)
    return _np((dy - y * (dy * y).sum(1, keepdim=True)) / n)


def l2_normalize_bwd_autograd(x, dy):
    x = _t(x, True)
    y = F.normalize(x, p=2, dim=-1, eps=1e-12)
    return _np(torch.autograd.grad((y * _t(dy)).sum(), x)[0])


# ------------------------------------------------------------------------------------------------ InfoNCE
def infonce_loss(Cm, temperature):
    """L = 1/(2B) [ sum_i (lse_j S_ij - S_ii) + sum_j (lse_i S_ij - S_jj) ], S = exp(temperature) * C; C is [B][B]."""
    B = Cm.shape[0]
    S = torch.exp(temperature) * Cm
    lr, lc = torch.logsumexp(S, 1), torch.logsumexp(S, 0)
    tr, tc = (lr - S.diagonal()) / (2 * B), (lc - S.diagonal()) / (2 * B)
    return tr.sum(), tc.sum(), (S, lr, lc, tr, tc)


def infonce_ref(Cm, temperature, gout=1.0):
    Cm, t = _t(Cm, True), _t(temperature, True)
    sr, sc, (S, lr, lc, tr, tc) = infonce_loss(Cm, t)
    dC, dt = torch.autograd.grad((sr + sc) * gout, (Cm, t))
    dtt = _np(dC) * _np(Cm)                  # dS/dtemp = S, dC = dL/dS * exp(t): dtemp = sum dL/dS * S = sum dC * C
    return InfoNCE(_np(lr), _np(lc), sr.item(), sc.item(), _np(tr), _np(tc), _np(dC), dt.item(), dtt)


def infonce_dC_float32(Cm, temperature, gout):
    """The backward's formula, g t (softmax_row + softmax_col - 2 delta), in plain torch.float32 (CPU) with float32 lse: what float32 can reach.
    Near a sharp diagonal softmax_row + softmax_col - 2 cancels, and the float32 rounding of S and lse (|S| up to 100) is what remains."""
    Cm, t = torch.tensor(np.asarray(Cm, np.float32)), torch.exp(torch.tensor(np.float32(temperature)).reshape(()))
    S = t * Cm
    lr, lc = torch.logsumexp(S, 1), torch.logsumexp(S, 0)
    g = torch.tensor(np.float32(gout)) / (2 * Cm.shape[0])
    return (g * t * (torch.exp(S - lr[:, None]) + torch.exp(S - lc[None, :]) - 2 * torch.eye(Cm.shape[0]))).numpy()


# ------------------------------------------------------------------------------------------------ prior tail
def prior_loss(h1, w2, b2, use_softplus):
    """Stacked rows [noise (B); features (B)]: logit = h1 . w2 + b2; sum over rows of -log D(u) / B and -log(1 - D(f)) / B, D = sigmoid(logit),
    written literally (use_softplus False) or as softplus(-s) / softplus(s)."""
    B = h1.shape[0] // 2
    s = h1 @ w2 + b2
    if use_softplus:
        terms = torch.cat([softplus(-s[:B]), softplus(s[B:])]) / B
    else:
        d = torch.sigmoid(s)
        terms = -torch.cat([torch.log(d[:B]), torch.log(1 - d[B:])]) / B
    return terms.sum(), s, terms


def prior_ref(h1, w2, b2, use_softplus=False, gout=1.0):
    """h1 = relu(pre-activation): dh1 is the gradient w.r.t. the pre-activation, i.e. masked by h1 > 0."""
    hn = np.asarray(h1, np.float64)
    pre, w2, b2 = _t(hn, True), _t(w2, True), _t(b2, True)
    total, s, terms = prior_loss(torch.relu(pre), w2, b2, use_softplus)
    s.retain_grad()
    (total * gout).backward()
    return Prior(_np(s), total.item(), _np(terms), _np(pre.grad), _np(w2.grad), float(b2.grad.sum()), _np(s.grad))


def loss_finalize_ref(acc, prior_weight):
    acc = np.asarray(acc, np.float64)
    cross, prior, visual, textual = acc[0] + acc[1], acc[2] + acc[3], acc[4] + acc[5], acc[6] + acc[7]
    return np.array([(1 - prior_weight) * (cross + visual + textual) + prior_weight * prior, cross, prior, visual, textual, 0, 0, 0])


# ------------------------------------------------------------------------------------------------ cross-entropy
def xent_ref(z, y, topk):
    """float64: per-row lse, summed loss over counted rows, top-1 / top-k counts with ties to the lower index, count, dlogits/gout (mean over the
    counted rows), the per-row loss terms. A class at -inf (a masked class, never the label) contributes nothing: exp 0, gradient exactly 0."""
    z = np.asarray(z).astype(np.float64)
    y = np.asarray(y)
    B, Cc = z.shape
    masked = np.isneginf(z)
    m = np.where(masked, -np.inf, z).max(1, keepdims=True)
    e = np.where(masked, 0.0, np.exp(np.where(masked, m, z) - m))
    lse = (np.log(e.sum(1, keepdims=True)) + m)[:, 0]
    ok = (y >= 0) & (y < Cc)
    n = int(ok.sum())
    loss = top1 = topk_n = 0.0
    d = np.zeros_like(z)
    terms = np.zeros(B)
    for i in range(B):
        if not ok[i]:
            continue
        zy = z[i, y[i]]
        rank = int((z[i] > zy).sum() + (z[i, :y[i]] == zy).sum())
        terms[i] = lse[i] - zy
        loss += terms[i]
        top1 += rank == 0
        topk_n += rank < topk
        d[i] = e[i] * np.exp(m[i, 0] - lse[i])
        d[i, y[i]] -= 1.0
    if n:
        d /= n
    return Xent(lse, loss, top1, topk_n, n, d, terms)


# ------------------------------------------------------------------------------------------------ parameter updates
def clip_factor(sumsq, gs, max_norm):
    return min(max_norm / (np.sqrt(float(sumsq)) * gs + 1e-6), 1.0) if max_norm > 0 else 1.0


def sgd_step_ref(p, g, v, slow, lr, wd, mu, max_norm, sync, alpha, gs, sumsq):
    """One element-wise SGD step in float64 (all scalars as the f32 values the kernel reads): pre-scale gs, clip factor, weight decay, momentum,
    Lookahead sync. Returns p, v, slow."""
    p, g, v, slow = (np.asarray(a, np.float64) for a in (p, g, v, slow))
    ge = g * (gs * clip_factor(sumsq, gs, max_norm)) + wd * p
    v = mu * v + ge
    p = p - lr * v
    if sync:
        p = alpha * p + (1 - alpha) * slow
        slow = p
    return p, v, slow


def adamw_step_ref(p, g, m, v2, slow, lr, wd, max_norm, sync, alpha, gs, b2, eps, bc1, bc2, omb1, omb2, sumsq):
    """torch.optim.AdamW's step as csrc/update_ops.hip states it: decoupled decay, exp_avg.lerp_, bias-corrected moments, then the Lookahead sync."""
    p, g, m, v2, slow = (np.asarray(a, np.float64) for a in (p, g, m, v2, slow))
    ge = g * (gs * clip_factor(sumsq, gs, max_norm))
    p = p * (1 - lr * wd)
    m = m + omb1 * (ge - m)
    v2 = b2 * v2 + omb2 * ge * ge
    p = p - (lr / bc1) * (m / (np.sqrt(v2) / np.sqrt(bc2) + eps))
    if sync:
        p = alpha * p + (1 - alpha) * slow
        slow = p
    return p, m, v2, slow


def to_bf16_bits(x):
    """float32 ndarray -> uint16 bf16 bits, round to nearest even (no NaN handling)."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_round(x):
    return (to_bf16_bits(x).astype(np.uint32) << 16).view(np.float32).reshape(np.shape(x))


def stored(x, dt):
    """x as float32 after rounding through the storage type."""
    x = np.ascontiguousarray(x, np.float32)
    return bf16_round(x) if dt == BF16 else x


# ================================================================================================ bounds
def elem(what, got, ref, dt, per_row=False, f32_eval=None):
    """per_row: max|ref| over each row of a 2-D tensor instead of the whole of it (a tighter bound, for rows of very different scales).
    f32_eval: the same formula evaluated in plain torch.float32 on the same inputs. Where THAT misses the f32 bound 2e-5 * max|ref|, the formula
    cannot meet it in float32 and the bound's first term becomes 4 x the float32 evaluation's largest error (one other summation order and a
    device expf / logf of a couple of ulps); the replacement is printed. The kernel's own error never enters a bound."""
    ref = np.asarray(ref, np.float64).reshape(got.shape)
    err = np.abs(got.astype(np.float64) - ref)
    top = np.abs(ref).max(1, keepdims=True) if per_row else (np.abs(ref).max() if ref.size else 0.0)
    flat = 2e-5 * top
    if f32_eval is not None:
        e32 = np.abs(np.asarray(f32_eval, np.float64).reshape(got.shape) - ref).max()
        print(f"ELEMERR {what}: kernel {err.max():.2e}  float32 {e32:.2e}  (bound 2e-5 * max|ref| = {np.max(flat):.2e})")
        if e32 > np.max(flat):
            print(f"BOUND REPLACED {what}: 2e-5 * max|ref| = {np.max(flat):.3e} -> 4 * float32 error = {4 * e32:.3e}")
            flat = 4 * e32
    bound = flat + (2.0 ** -7 * np.abs(ref) if dt == BF16 else 0.0)
    bad = ~(err <= bound)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} elements out of bound, max err {err.max():.3e}, max|ref| {np.max(top):.3e}"


def vec(what, got, ref, terms=None):
    """Vector accumulator: |got - ref| <= 1e-4 * max|ref|. terms [rows][n] float64 with ref = start + terms.sum(0): prints the kernel's error and
    the error of a float32 sum of the same terms, both relative to sum|terms|."""
    ref = np.asarray(ref, np.float64).reshape(got.shape)
    err = np.abs(got.astype(np.float64) - ref)
    top = np.abs(ref).max()
    if terms is not None:
        den = np.maximum(np.abs(terms).sum(0), 1e-300)
        plain = np.abs(terms.astype(np.float32).sum(0, dtype=np.float32).astype(np.float64) - terms.sum(0))
        print(f"REDERR {what}: kernel {(err / den).max():.2e}  float32 {(plain / den).max():.2e}")
    else:
        print(f"REDERR {what}: kernel {err.max() / max(top, 1e-300):.2e} of max|ref|")
    assert (err <= 1e-4 * top).all(), f"{what}: max err {err.max():.3e} > 1e-4 * {top:.3e}"


def scalar(what, got, ref, terms):
    """Scalar accumulator: |got - ref| <= 1e-5 * max(1, sum|terms|); ref = start value + sum(terms). Prints the error beside that of a sequential
    float32 sum of the float32-rounded terms."""
    terms = np.asarray(terms, np.float64).ravel()
    den = max(1.0, np.abs(terms).sum())
    err = abs(float(got) - float(ref))
    plain = abs(float(np.cumsum(terms.astype(np.float32), dtype=np.float32)[-1]) - terms.sum()) if terms.size else 0.0
    print(f"REDERR {what}: kernel {err / den:.2e}  float32 {plain / den:.2e}  (sum|terms| {np.abs(terms).sum():.3g})")
    assert err <= 1e-5 * den, f"{what}: |{got} - {ref}| = {err:.3e} > 1e-5 * {den:.3e}"


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


# ================================================================================================ shared checks (simulator and device)
FILL = 7.0


def _rng(*key):
    return np.random.default_rng([int(k) for k in key])


def negative_pairing(kind, B, rng):
    """None (roll by one) | 'cluster' | 'random' (a permutation with fixed points) -> (neg, neg_inv) int32 or (None, None)."""
    if kind is None:
        return None, None
    if kind == "cluster":
        neg = cluster_pairing(B)
    else:
        rest = np.array([i for i in range(B) if i not in (2, 5)])          # rows 2 and 5 are their own negatives
        neg = np.arange(B)
        neg[rest] = rng.permutation(rest)
        assert sorted(neg) == list(range(B)) and neg[2] == 2 and neg[5] == 5
    return neg.astype(np.int32), inverse_of(neg).astype(np.int32)


def check_critic(be, dt, B, D, pairing=None, repeat=False):
    """critic_jsd_fwd + critic_jsd_bwd at (B, D): all eight work columns, both sums (accumulated onto non-zero starts), df1, df2, dtemp; one
    sentinel row behind work / df1 / df2. repeat: run twice (for deterministic mode) and require bit-identical acc and dtemp."""
    rng = _rng(B, D, dt, 11)
    neg, neg_inv = negative_pairing(pairing, B, rng)
    f1 = stored(rng.standard_normal((B, D)), dt)
    f2 = stored(rng.standard_normal((B, D)) + 0.5 * f1, dt)          # correlated: cos+ is not near 0
    temp = np.array([T_CLIP], np.float32)
    gout, scale = np.array([1.7], np.float32), 0.9
    ref = critic_ref(f1, f2, temp[0], neg, gout=float(gout[0]) * float(np.float32(scale)))
    acc0, dtemp0 = np.array([0.25, -0.5], np.float32), np.array([0.375], np.float32)
    runs = []
    for _ in range(2 if repeat else 1):
        d = {k: be.dev(v, dt) for k, v in (("f1", f1), ("f2", f2))}
        work, acc, dtemp = be.dev(np.full((B + 1, 8), FILL), F32), be.dev(acc0, F32), be.dev(dtemp0, F32)
        df1, df2 = be.dev(np.full((B + 1, D), FILL), dt), be.dev(np.full((B + 1, D), FILL), dt)
        t, g, ng, ni = be.dev(temp, F32), be.dev(gout, F32), be.dev(neg, "i32"), be.dev(neg_inv, "i32")
        assert be.call("critic_jsd_fwd", dt, d["f1"], d["f2"], t, B, D, ng, work, acc) == 0
        assert be.call("critic_jsd_bwd", dt, d["f1"], d["f2"], t, work, g, scale, B, D, ng, ni, df1, df2, dtemp) == 0
        w, a, dtm, g1, g2 = be.host(work), be.host(acc), be.host(dtemp), be.host(df1), be.host(df2)
        what = f"critic ({B}, {D}) {pairing or 'roll'} {'bf16' if dt == BF16 else 'f32'}"
        for c, name in enumerate(("|a|", "|b|", "|b_neg|", "cos+", "cos-", "o+", "o-")):
            elem(f"{what} work[{name}]", w[:B, c], ref.work[:, c], F32)
        assert not w[:B, 7].any() and (w[B] == FILL).all(), f"{what}: work column 7 / sentinel row"
        scalar(f"{what} acc[0]", a[0], acc0[0] + ref.sum_pos, ref.terms_pos)
        scalar(f"{what} acc[1]", a[1], acc0[1] + ref.sum_neg, ref.terms_neg)
        scalar(f"{what} dtemp", dtm[0], dtemp0[0] + ref.dtemp, ref.dtemp_terms)
        elem(f"{what} df1", g1[:B], ref.df1, dt)
        elem(f"{what} df2", g2[:B], ref.df2, dt)
        assert (g1[B] == FILL).all() and (g2[B] == FILL).all(), f"{what}: sentinel rows of df1 / df2"
        assert same_bits(be.host(d["f1"]), f1) and same_bits(be.host(d["f2"]), f2)
        runs.append((a, dtm))
    if repeat:
        assert same_bits(runs[0][0], runs[1][0]) and same_bits(runs[0][1], runs[1][1]), "deterministic mode: acc / dtemp differ between two runs"


def check_critic_rejects(be, dt):
    """D % 8, D > 2048 and neg without neg_inv: the entry refuses (status -1) and touches nothing."""
    B = 4
    temp, gout = be.dev(np.array([T_CLIP], np.float32), F32), be.dev(np.ones(1, np.float32), F32)
    neg = be.dev(cluster_pairing(B).astype(np.int32), "i32")
    for D, with_neg in ((12, False), (2056, False), (8, True)):
        f = be.dev(np.ones((B, D)), dt)
        work, acc, dtemp = be.dev(np.full((B, 8), FILL), F32), be.dev(np.full(2, FILL), F32), be.dev(np.full(1, FILL), F32)
        df1, df2 = be.dev(np.full((B, D), FILL), dt), be.dev(np.full((B, D), FILL), dt)
        if not with_neg:
            assert be.call("critic_jsd_fwd", dt, f, f, temp, B, D, None, work, acc) == -1
        assert be.call("critic_jsd_bwd", dt, f, f, temp, work, gout, 1.0, B, D, neg if with_neg else None, None, df1, df2, dtemp) == -1
        for h in (work, acc, dtemp, df1, df2):
            assert (be.host(h) == FILL).all(), f"rejected call (D = {D}) wrote to a buffer"


def check_l2_normalize(be, dt, B, D):
    """l2_normalize and l2_normalize_bwd at (B, D), with an all-zero row (zeros out) and a row of 1e-20 (norm below eps: x / eps = 1e-8)."""
    rng = _rng(B, D, dt, 12)
    x = rng.standard_normal((B, D)) * np.exp(rng.standard_normal((B, 1)))
    zero_row, tiny_row = (B // 2, B - 1) if B >= 3 else (None, None)
    if zero_row is not None:
        x[zero_row] = 0.0
        x[tiny_row] = 1e-20
    x = stored(x, dt)
    what = f"l2_normalize ({B}, {D}) {'bf16' if dt == BF16 else 'f32'}"
    xd, out = be.dev(x, dt), be.dev(np.full((B + 1, D), FILL), dt)
    assert be.call("l2_normalize", dt, xd, out, B, D) == 0
    y = be.host(out)
    elem(what, y[:B], l2_normalize_ref(x), dt)
    assert (y[B] == FILL).all(), f"{what}: sentinel row"
    if zero_row is not None:
        assert not y[zero_row].any(), f"{what}: the all-zero row"
        t = stored(np.float32(1e-20), dt).astype(np.float64) / 1e-12
        assert np.abs(y[tiny_row] - t).max() <= (2.0 ** -7 if dt == BF16 else 2e-5) * t, f"{what}: the 1e-20 row must give 1e-8"
    dy = stored(rng.standard_normal((B, D)), dt)
    ys = y[:B].copy()                                          # the stored forward result is the backward's input
    dx = be.dev(np.full((B + 1, D), FILL), dt)
    assert be.call("l2_normalize_bwd", dt, xd, be.dev(ys, dt), be.dev(dy, dt), dx, B, D) == 0
    got = be.host(dx)
    # dx scales with 1 / max(|x|, eps), 1e12 in the zero and 1e-20 rows: max|ref| is taken per row, which is the bound's tighter reading
    elem(f"{what} bwd", got[:B], l2_normalize_bwd_ref(x, ys, dy), dt, per_row=True)
    assert (got[B] == FILL).all(), f"{what}: sentinel row of dx"


def check_infonce(be, dt, B, ld, ldd, temperature, with_dtemp=True, repeat=False):
    """infonce_fwd + infonce_bwd on a cosine matrix [B][ld] whose columns >= B hold 1e4 (they must enter nothing); dC is [B][ldd], zero in columns >= B."""
    rng = _rng(B, ld, ldd, 13)
    a = rng.standard_normal((B, 32))
    b = rng.standard_normal((B, 32)) + 0.7 * a
    cos = (a / np.linalg.norm(a, axis=1, keepdims=True)) @ (b / np.linalg.norm(b, axis=1, keepdims=True)).T
    Cm = np.full((B + 1, ld), 1e4, np.float32)
    Cm[:B, :B] = cos
    temp = np.array([temperature], np.float32)
    gout, scale = np.array([1.3], np.float32), 0.9
    ref = infonce_ref(Cm[:B, :B], temp[0], gout=float(gout[0]) * float(np.float32(scale)))
    acc0, dtemp0 = np.array([0.25, -0.5], np.float32), np.array([0.375], np.float32)
    what = f"infonce ({B}, {ld}, {ldd}) t={temperature:.3f} {'bf16' if dt == BF16 else 'f32'}"
    runs = []
    for _ in range(2 if repeat else 1):
        Cd, t, g = be.dev(Cm, F32), be.dev(temp, F32), be.dev(gout, F32)
        lse_r, lse_c = be.dev(np.full(B + 1, FILL), F32), be.dev(np.full(B + 1, FILL), F32)
        acc, dtemp = be.dev(acc0, F32), (be.dev(dtemp0, F32) if with_dtemp else None)
        dC = be.dev(np.full((B + 1, ldd), FILL), dt)
        assert be.call("infonce_fwd", Cd, ld, B, t, lse_r, lse_c, acc) == 0
        assert be.call("infonce_bwd", dt, Cd, ld, B, t, lse_r, lse_c, g, scale, dC, ldd, dtemp) == 0
        lr, lc, a_, d = be.host(lse_r), be.host(lse_c), be.host(acc), be.host(dC)
        vec(f"{what} lse_r", lr[:B], ref.lse_r)
        vec(f"{what} lse_c", lc[:B], ref.lse_c)
        assert lr[B] == FILL and lc[B] == FILL, f"{what}: sentinels behind lse"
        scalar(f"{what} acc[0]", a_[0], acc0[0] + ref.sum_r, ref.terms_r)
        scalar(f"{what} acc[1]", a_[1], acc0[1] + ref.sum_c, ref.terms_c)
        elem(f"{what} dC", d[:B, :B], ref.dC, dt, f32_eval=infonce_dC_float32(Cm[:B, :B], temp, float(gout[0]) * float(np.float32(scale))))
        assert not d[:B, B:].any(), f"{what}: dC columns >= B must be zero"
        assert (d[B] == FILL).all(), f"{what}: sentinel row of dC"
        if with_dtemp:
            dtm = be.host(dtemp)
            scalar(f"{what} dtemp", dtm[0], dtemp0[0] + ref.dtemp, ref.dtemp_terms)
        assert same_bits(be.host(Cd), Cm)
        runs.append((a_, be.host(dtemp) if with_dtemp else a_))
    if repeat:
        assert same_bits(runs[0][0], runs[1][0]) and same_bits(runs[0][1], runs[1][1]), "deterministic mode: acc / dtemp differ between two runs"


def check_prior_tail(be, dt, B, K, use_softplus, max_logit=6.0, repeat=False):
    """prior_tail_fwd + prior_tail_bwd at (B, K): logit, the sum, dh1 (through the ReLU mask; h1 has exact zeros), dw2 and db2 (accumulated onto
    non-zero starts). w2 is scaled so that max |logit| = max_logit."""
    rng = _rng(B, K, dt, int(use_softplus), int(max_logit), 14)
    h1 = stored(np.maximum(rng.standard_normal((2 * B, K)), 0), dt)
    assert (h1 == 0).any()
    w2 = rng.standard_normal(K)
    b2 = np.array([0.05], np.float32)
    w2 = (w2 * (max_logit - 0.1) / np.abs(h1.astype(np.float64) @ w2).max()).astype(np.float32)
    gout, scale = np.array([2.0], np.float32), 0.1
    ref = prior_ref(h1, w2, b2, use_softplus, gout=float(gout[0]) * float(np.float32(scale)))
    assert np.abs(ref.logit).max() <= max_logit + 0.05
    acc0, db0 = np.array([0.25], np.float32), np.array([-0.5], np.float32)
    dw0 = (0.01 * rng.standard_normal(K + 8)).astype(np.float32)
    what = f"prior ({B}, {K}) {'softplus' if use_softplus else 'log'} |logit|<={max_logit:g} {'bf16' if dt == BF16 else 'f32'}"
    runs = []
    for _ in range(2 if repeat else 1):
        hd, wd, bd, g = be.dev(h1, dt), be.dev(w2, F32), be.dev(b2, F32), be.dev(gout, F32)
        logit, acc = be.dev(np.full(2 * B + 1, FILL), F32), be.dev(acc0, F32)
        dh, dw, db = be.dev(np.full((2 * B + 1, K), FILL), dt), be.dev(dw0, F32), be.dev(db0, F32)
        assert be.call("prior_tail_fwd", dt, hd, wd, bd, B, K, int(use_softplus), logit, acc) == 0
        assert be.call("prior_tail_bwd", dt, hd, wd, logit, g, scale, B, K, dh, dw, db) == 0
        lg, a, gh, gw, gb = be.host(logit), be.host(acc), be.host(dh), be.host(dw), be.host(db)
        elem(f"{what} logit", lg[:2 * B], ref.logit, F32)
        assert lg[2 * B] == FILL, f"{what}: sentinel behind logit"
        scalar(f"{what} acc", a[0], acc0[0] + ref.sum, ref.terms)
        elem(f"{what} dh1", gh[:2 * B], ref.dh1, dt)
        assert not gh[:2 * B][h1 == 0].any(), f"{what}: dh1 must be zero where h1 is"
        assert (gh[2 * B] == FILL).all(), f"{what}: sentinel row of dh1"
        vec(f"{what} dw2", gw[:K], dw0[:K] + ref.dw2, terms=ref.gl[:, None] * h1.astype(np.float64))
        assert same_bits(gw[K:], dw0[K:]), f"{what}: sentinel tail of dw2"
        scalar(f"{what} db2", gb[0], db0[0] + ref.db2, ref.gl)
        runs.append((a, gw, gb))
    if repeat:
        assert all(same_bits(x, y) for x, y in zip(*runs)), "deterministic mode: acc / dw2 / db2 differ between two runs"


def check_loss_finalize(be):
    acc = np.array([0.3, 0.4, 1.0, 2.0, 0.05, 0.15, 0.25, 0.35], np.float32)
    out = be.dev(np.full(9, FILL), F32)
    assert be.call("loss_finalize", be.dev(acc, F32), 0.1, out) == 0
    got = be.host(out)
    elem("loss_finalize", got[:5], loss_finalize_ref(acc, float(np.float32(0.1)))[:5], F32)
    assert not got[5:8].any() and got[8] == FILL


def check_add(be, dt, n):
    """out = a + b over n elements: bf16 must equal the round-to-nearest-even of the f32 sum of the two stored values exactly; f32 is that sum."""
    rng = _rng(n, dt, 15)
    a = stored(rng.standard_normal(n, dtype=np.float32), dt)
    b = stored(rng.standard_normal(n, dtype=np.float32) * 3, dt)
    out = be.dev(np.full(n + 8, FILL), dt)
    assert be.call("add", dt, be.dev(a, dt), be.dev(b, dt), out, n) == 0
    got = be.host(out)
    assert same_bits(got[:n], stored(a + b, dt)), f"add n = {n}"
    assert (got[n:] == FILL).all(), f"add n = {n}: tail"


def xent_problem(Cc, B, rng):
    """Logits in [-8, 8] and labels that include -100, C and 2^40 where B allows; rows 0 and 2 tie the label with another class. The other logits are
    not put on a grid: with few distinct loss terms, a float32 sum of 8200 of them rounds the same way at every step, and such a sum in a random
    order already reaches 9e-6 of sum|terms| against 4e-6 for unquantised terms (20 orders each, on the host), too close to the bound of 1e-5."""
    z = (rng.standard_normal((B, Cc)) * 3).clip(-8, 8).astype(np.float32)
    y = rng.integers(0, Cc, B).astype(np.int64)
    if B >= 5:
        y[1], y[3], y[B - 1] = -100, Cc, 2 ** 40
    if Cc >= 3 and B >= 5:
        z[0, :] = np.minimum(z[0, :], 2.0)
        y[0] = Cc - 1
        z[0, [0, Cc - 1]] = 4.0              # the label ties with class 0: rank 1
        z[2, :] = np.minimum(z[2, :], 2.0)
        y[2] = 0
        z[2, [0, Cc - 1]] = 4.0              # the label ties with a higher class: rank 0
    return z, y


def mask_classes(z, y, rng):
    """-inf in one to C - 1 classes that are not the label, over the counted rows in turn: a single one at column 0 (a lane's first element
    before any finite one), a single one behind finite values, column 0 together with random ones, and everything except the label."""
    z = z.copy()
    B, Cc = z.shape
    k = 0
    for i in range(B):
        if not (0 <= y[i] < Cc) or Cc < 2:
            continue
        free = np.array([j for j in range(Cc) if j != y[i]])
        kind = k % 4
        if kind == 0:
            cols = free[:1]                                  # column 0 (or 1 when the label is 0)
        elif kind == 1:
            cols = free[-1:]
        elif kind == 2:
            cols = np.union1d(free[:1], rng.choice(free, max(1, len(free) // 3), replace=False))
        else:
            cols = free
        z[i, cols] = -np.inf
        k += 1
    return z


def check_xent(be, dt, Cc, B, topk, masked=False, all_ignored=False, repeat=False):
    """xent_fwd + xent_bwd at (C, B): ld = C rounded up to 4 plus 4 with NaN in columns >= C, ldd = C rounded up to 8 plus 8, Bp = B rounded up to
    8 plus 8. acc starts non-zero; lse, the four counters (exact) and the gradient against float64."""
    rng = _rng(Cc, B, 16)
    z, y = xent_problem(Cc, B, rng)
    if all_ignored:
        y[:] = np.array([-100, Cc, 2 ** 40, -1])[np.arange(B) % 4]
    if masked:
        z = mask_classes(z, y, rng)
        assert np.isneginf(z).any() and not np.isneginf(z[np.arange(B)[(y >= 0) & (y < Cc)], y[(y >= 0) & (y < Cc)]]).any()
    ld, ldd, Bp = (Cc + 3) // 4 * 4 + 4, (Cc + 7) // 8 * 8 + 8, (B + 7) // 8 * 8 + 8
    zb = np.full((B, ld), np.nan, np.float32)
    zb[:, :Cc] = z
    ref = xent_ref(z, y, topk)
    acc0 = np.array([0.25, 3.0, 5.0, 7.0], np.float32)
    gout = np.array([0.7], np.float32)
    what = f"xent (C {Cc}, B {B}) top{topk}{' masked' if masked else ''} {'bf16' if dt == BF16 else 'f32'}"
    runs = []
    for _ in range(2 if repeat else 1):
        zd, yd = be.dev(zb, F32), be.dev(y, "i64")
        lse, acc = be.dev(np.full(B + 1, FILL), F32), be.dev(acc0, F32)
        assert be.call("xent_fwd", zd, ld, B, Cc, yd, topk, lse, acc) == 0
        l, a = be.host(lse), be.host(acc)
        vec(f"{what} lse", l[:B], ref.lse)
        assert l[B] == FILL
        assert a[1] == acc0[1] + ref.top1 and a[2] == acc0[2] + ref.topk and a[3] == acc0[3] + ref.count, f"{what}: counters {a} vs {ref[1:5]}"
        if all_ignored:
            assert same_bits(a, acc0), f"{what}: acc must be unchanged when no row counts"
        scalar(f"{what} acc[0]", a[0], acc0[0] + ref.loss, ref.terms)
        # the backward reads the count from acc[3]: hand it the counters of this batch alone
        acc_b = be.dev(np.array([ref.loss, ref.top1, ref.topk, ref.count], np.float32), F32)
        dz = be.dev(np.full((Bp + 1, ldd), FILL), dt)
        assert be.call("xent_bwd", dt, zd, ld, B, Bp, Cc, lse, yd, acc_b, be.dev(gout, F32), dz, ldd) == 0
        d = be.host(dz)
        elem(f"{what} dlogits", d[:B, :Cc], float(gout[0]) * ref.dlogits, dt)
        assert not d[:Bp, Cc:].any() and not d[B:Bp].any(), f"{what}: padding rows / columns of dlogits must be zero"
        assert (d[Bp] == FILL).all(), f"{what}: sentinel row of dlogits"
        counted = (y >= 0) & (y < Cc)
        assert not d[:B][~counted].any(), f"{what}: rows with an ignored label must have zero gradient"
        if masked:
            assert not d[:B, :Cc][np.isneginf(z)].any(), f"{what}: the gradient at a masked class must be exactly 0"
        runs.append((l, a, d))
    if repeat:
        assert all(same_bits(p, q) for p, q in zip(*runs)), "deterministic mode: two runs differ"


def xent_reference(z, y, topk):
    """(lse, summed loss, top-1 count, top-k count, counted rows, dlogits / gout) as tests/test_wavesim_cls.py unpacks them."""
    return tuple(xent_ref(z, y, topk))[:6]


MASKED_ROW = (np.array([[-np.inf, 1, 2, 0.5, 0, -1, 3, 0.25]], np.float32), np.array([2], np.int64), 3.5407709)
