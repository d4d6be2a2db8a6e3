"""Float64 reference of the LARS update (csrc/update_ops.hip, optim.FusedLARS), evaluated on the stored f32 inputs and the f32 hyper-parameters the
kernel reads. Nothing here calls into clip_lite_amd. For every tensor t (loss_ref.sgd_step_ref's names):

    g' = g * gs * clip                               clip from the global sumsq, as loss_ref.clip_factor
    adapted:      pn = |p_t|, gn = gs * clip * |g_t|
                  q  = eta * pn / (gn + wd_t * pn + eps)   if pn > 0 and gn > 0, else 1
    not adapted:  q  = 1
    u = q * (g' + wd_t * p);  v = mu * v + u;  p -= lr_t * v;  then the Lookahead sync

tests/test_lars_ref_host.py holds this file to torch.optim.SGD and to loss_ref.sgd_step_ref.
"""
from collections import namedtuple

import numpy as np

import loss_ref as R
import update_table as U
from loss_ref import clip_factor
from update_table import CHUNK, N_SLOTS, OPTIONS, SENT, TABLE, Tensor, clip_setup, kept as _kept, table  # noqa: F401

Step = namedtuple("Step", "p v slow q u")                  # q, u: per element (q = 1 and u = 0 outside every tensor)


def f32(x):
    return float(np.float32(x))


def squared_norms(p, g, tensors):
    """[(sum p^2, sum g^2)] per tensor in float64, over the raw p and g."""
    p, g = np.asarray(p, np.float64), np.asarray(g, np.float64)
    return [((p[t.start:t.start + t.n] ** 2).sum(), (g[t.start:t.start + t.n] ** 2).sum()) for t in tensors]


def trust_ratio(pn, gn, wd, eta, eps):
    """q of one adapted tensor from |p|, |g'| (the pre-scaled, clipped gradient's norm)."""
    return eta * pn / (gn + wd * pn + eps) if pn > 0 and gn > 0 else 1.0


def lars_step_ref(p, g, v, slow, lr, wd, mu, max_norm, sync, alpha, gs, sumsq, eta, eps, tensors, norms=None):
    """One LARS step in float64. lr, wd: per-element arrays (constant within a tensor; lr already times the schedule's multiplier); tensors:
    [Tensor]; norms: [(sum p^2, sum g^2)] per tensor, default squared_norms(p, g, tensors). Elements outside every tensor come back unchanged."""
    p, g, v, slow = (np.array(a, np.float64) for a in (p, g, v, slow))
    lr, wd = np.asarray(lr, np.float64), np.asarray(wd, np.float64)
    if norms is None:
        norms = squared_norms(p, g, tensors)
    gmul = gs * clip_factor(sumsq, gs, max_norm)
    q, u = np.ones_like(p), np.zeros_like(p)
    for t, (pp, gg) in zip(tensors, norms):
        s = slice(t.start, t.start + t.n)
        if t.adapted and t.n:
            q[s] = trust_ratio(np.sqrt(pp), gmul * np.sqrt(gg), wd[t.start], eta, eps)
        u[s] = q[s] * (g[s] * gmul + wd[s] * p[s])
        v[s] = mu * v[s] + u[s]
        p[s] = p[s] - lr[s] * v[s]
        if sync:
            p[s] = alpha * p[s] + (1 - alpha) * slow[s]
            slow[s] = p[s]
    return Step(p, v, slow, q, u)


# ================================================================================================ shared checks (simulator and device)
# A backend is a callable be(bufs, rows, hp, ss, calls) -> dict of the buffers afterwards. bufs: numpy arrays p, g, v, slow (f32), cast (uint16 bf16
# bits, or None: no bf16 copy is given to the kernel), partials, norms (f32); rows: [(start, count, lr, wd, reserved)]; calls, run in order on copies
# of the buffers: ("norms" | "lars" | "sgd", first item, number of items). A norms call gets partials[2 first : 2 (first + n)], as FusedLARS.launch
# passes them. tests/test_wavesim_lars.py runs the kernels on the wave simulator, tests/test_gpu_lars_ops.py on the device.
# The item table is update_table.table().
ETA, EPS = 1.0, 1e-8                           # eta = 1: q u is of order one (at eta = 0.001 a wrong ratio hides under the SGD bound)
MEASURED = {}                                  # running maxima of what the checks print, by name


def _note(name, value):
    return U.note(MEASURED, name, value)


def problem(seed, adapt=True):
    rows, tensors, slots, heads, n = table(adapt)
    rng = np.random.default_rng(seed)
    inside = U.inside_of(tensors, n)
    p, g, v, slow = (np.where(inside, rng.standard_normal(n), SENT).astype(np.float32) for _ in range(4))
    for t, (_, _, special) in zip(tensors, TABLE):
        if special == "g0":
            g[t.start:t.start + t.n] = 0.0
        if special == "p0":
            p[t.start:t.start + t.n] = 0.0
    bufs, lr, wd = U.finish_problem({"p": p, "g": g, "v": v, "slow": slow}, rows, n)
    return bufs, rows, tensors, slots, heads, inside, lr, wd


def _hp(max_norm=0.0, sync=False, gs=1.0):
    return np.array([0.5, 0.9, max_norm, float(sync), 0.5, gs, ETA, EPS], np.float32)


def _check_norms_of(what, out, bufs, tensors, slots, launched):
    """norms / partials after a norms call over the tensors `launched` (indices): the launched slots against float64, every other slot untouched."""
    U.check_norm_slots("LARSERR", what, out["norms"], (("p", bufs["p"]), ("g", bufs["g"])), tensors, slots, launched, MEASURED)


def check_norms(be):
    """Each sum within 1e-5 * max(1, sum of terms) of float64; two runs bit-identical; the slots no launched tensor owns, the partial pairs of
    not-adapted items and everything behind both buffers untouched; p and g unchanged. Then a launch of the items of tensors 3 .. 7 only: the
    slots of tensors 0 and 2 stay untouched and the launched ones equal the full launch bit for bit."""
    bufs, rows, tensors, slots, heads, inside, _, _ = problem(31)
    n = len(rows)
    outs = [be(bufs, rows, _hp(), np.zeros(1, np.float32), [("norms", 0, n)]) for _ in range(2)]
    for name in ("norms", "partials"):
        assert R.same_bits(outs[0][name], outs[1][name]), f"two runs differ in {name}"
    out = outs[0]
    _check_norms_of("full table", out, bufs, tensors, slots, range(len(tensors)))
    adapted_item = np.array([r[4] != 0 for r in rows])
    pairs = out["partials"][:2 * n].reshape(n, 2)
    assert (pairs[~adapted_item] == SENT).all() and (out["partials"][2 * n:] == SENT).all(), "partials of not-adapted items / behind the buffer"
    assert (pairs[adapted_item] != SENT).all()
    for name in ("p", "g", "v", "slow", "cast"):
        _kept(name, out[name], bufs[name], np.ones(len(bufs[name]), bool))
    k = heads[3]
    sub = be(bufs, rows, _hp(), np.zeros(1, np.float32), [("norms", k, n - k)])
    _check_norms_of("items of tensors 3 .. 7", sub, bufs, tensors, slots, range(3, len(tensors)))
    for i in range(3, len(tensors)):
        if slots[i] is not None:
            assert R.same_bits(sub["norms"][2 * slots[i]:2 * slots[i] + 2], out["norms"][2 * slots[i]:2 * slots[i] + 2]), i
    assert (sub["partials"][:2 * k] == SENT).all()


def check_step(be, sync, cast, clip, gs):
    """norms + lars_step over the whole table against lars_step_ref fed the float64 norms. Per element
    |got - ref| <= 1e-6 * max(1, |ref|) + 2e-5 * |delta_ref|, delta_ref = this step's q u for v, lr mult q u for p and slow: the SGD kernel's bound
    plus the trust ratio's (two sums each within 1e-5 -> their roots within 5e-6 -> the ratio within 1e-5, doubled for the f32 roundings that
    form q)."""
    bufs, rows, tensors, slots, heads, inside, lr, wd = problem(32)
    if not cast:
        bufs = dict(bufs, cast=None)
    cast0 = R.to_bf16_bits(np.full(len(inside), 3.0, np.float32))
    max_norm, ss = clip_setup(clip, bufs["g"], inside, gs)
    hp = _hp(max_norm, sync, gs)
    h = [float(x) for x in hp]
    ref = lars_step_ref(bufs["p"], bufs["g"], bufs["v"], bufs["slow"], lr * h[0], wd, h[1], h[2], sync, h[4], h[5], float(ss), h[6], h[7], tensors)
    for t, (_, slot, special) in zip(tensors, TABLE):          # the table does what it says: ratios of order one, 1 where a norm is zero
        q = ref.q[t.start]
        assert q == 1.0 if (slot is None or special) else (1e-2 < q < 1e2 and q != 1.0), (t, q)
    n = len(rows)
    out = be(bufs, rows, hp, np.array([ss], np.float32), [("norms", 0, n), ("lars", 0, n)])
    dv = np.abs(ref.u)
    for name, r, delta in (("p", ref.p, lr * h[0] * dv), ("v", ref.v, dv), ("slow", ref.slow, lr * h[0] * dv if sync else 0 * dv)):
        err = np.abs(out[name].astype(np.float64) - r)[inside]
        bound = (1e-6 * np.maximum(1.0, np.abs(r)) + 2e-5 * delta)[inside]
        print(f"LARSERR step {name} sync={sync} clip={clip} gs={gs}: max err / bound = {(err / bound).max():.3f}, max err / max(1, |ref|) = "
              f"{(err / np.maximum(1, np.abs(r[inside]))).max():.2e}, running max of err / bound {_note('step ' + name, (err / bound).max()):.3f}")
        assert (err <= bound).all(), (name, float((err / bound).max()))
    for name in ("p", "g", "v", "slow"):
        _kept(name, out[name], bufs[name], ~inside)
    assert not out["g"][inside].any(), "g must be zero inside items"
    if not sync:
        _kept("slow (no sync)", out["slow"], bufs["slow"], np.ones(len(inside), bool))
    else:
        assert np.array_equal(out["slow"][inside], out["p"][inside]), "after a sync the slow weights are the fast ones"
    if cast:
        _kept("cast", out["cast"], cast0, ~inside)
        assert np.array_equal(out["cast"][inside], R.to_bf16_bits(out["p"])[inside]), "the bf16 copy must be the round-to-nearest-even of the returned p"
    else:
        assert out["cast"] is None
    _check_norms_of("step", out, bufs, tensors, slots, range(len(tensors)))


def check_not_adapted_is_sgd(be):
    """The same table with every reserved word 0: clite_lars_step's p, v, slow, g and bf16 copy are clite_sgd_step's bit for bit (sync and clipping
    on, and off), and neither norms nor partials is written."""
    bufs, rows, tensors, slots, heads, inside, _, _ = problem(33, adapt=False)
    n = len(rows)
    for sync, clip, gs in ((True, "active", 0.25), (False, "disabled", 1.0)):
        max_norm, ss = clip_setup(clip, bufs["g"], inside, gs)
        hp, ssa = _hp(max_norm, sync, gs), np.array([ss], np.float32)
        a = be(bufs, rows, hp, ssa, [("norms", 0, n), ("lars", 0, n)])
        b = be(bufs, rows, hp, ssa, [("sgd", 0, n)])
        for name in ("p", "g", "v", "slow", "cast"):
            assert R.same_bits(a[name], b[name]), f"{name} differs from clite_sgd_step (sync={sync}, clip={clip})"
        assert not R.same_bits(a["p"], bufs["p"])
        assert (a["norms"] == SENT).all() and (a["partials"] == SENT).all()


def check_split_launch(be):
    """Items [0, k) then [k, n), k on a tensor boundary (norms and update of each range, as FusedLARS.launch(span) enqueues them), equal one launch
    bit for bit — on a sync step with clipping active."""
    bufs, rows, tensors, slots, heads, inside, _, _ = problem(34)
    n = len(rows)
    max_norm, ss = clip_setup("active", bufs["g"], inside, 0.25)
    hp, ssa = _hp(max_norm, True, 0.25), np.array([ss], np.float32)
    one = be(bufs, rows, hp, ssa, [("norms", 0, n), ("lars", 0, n)])
    for ti in (5, 6):          # in front of the four-item tensor, and behind it
        k = heads[ti]
        two = be(bufs, rows, hp, ssa, [("norms", 0, k), ("lars", 0, k), ("norms", k, n - k), ("lars", k, n - k)])
        for name in ("p", "g", "v", "slow", "cast", "norms", "partials"):
            assert R.same_bits(one[name], two[name]), f"{name}: split at item {k} differs from one launch"
