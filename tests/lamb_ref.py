"""Float64 reference of the LAMB update (csrc/update_ops.hip, optim.FusedLAMB; You et al. 2020, Algorithm 2), evaluated on the stored f32 inputs and
the f32 hyper-parameters the kernel reads. Nothing here calls into clip_lite_amd. For every tensor t (loss_ref.adamw_step_ref's names):

    g' = g * gs * clip                               clip from the global sumsq, as loss_ref.clip_factor
    m  = m + omb1 (g' - m);  v2 = b2 v2 + omb2 g'^2
    u  = (m / bc1) / (sqrt(v2 / bc2) + eps);  r = u + wd_t p
    adapted:      q = |p_t| / |r_t| if both norms > 0, else 1; with trust_clip q = min(q, 1)        (|p| before the update, |r| after the moments')
    not adapted:  q = 1
    p -= lr_t q r;  then the Lookahead sync

tests/test_lamb_ref_host.py holds this file to torch.optim.AdamW, to loss_ref.adamw_step_ref and to a restatement of Algorithm 2.
"""
from collections import namedtuple

import numpy as np

import loss_ref as R
import update_table as U
from lars_ref import f32  # noqa: F401
from loss_ref import clip_factor
from update_table import CHUNK, N_SLOTS, OPTIONS, SENT, TABLE, Tensor, clip_setup, kept as _kept  # noqa: F401

Step = namedtuple("Step", "p m v2 slow q r")               # q, r: per element (q = 1 and r = 0 outside every tensor)


def squared_norms(p, r, tensors):
    """[(sum p^2, sum r^2)] per tensor in float64."""
    p, r = np.asarray(p, np.float64), np.asarray(r, np.float64)
    return [((p[t.start:t.start + t.n] ** 2).sum(), (r[t.start:t.start + t.n] ** 2).sum()) for t in tensors]


def trust_ratio(pn, rn, trust_clip=False):
    """q of one adapted tensor from |p| and |r|."""
    q = pn / rn if pn > 0 and rn > 0 else 1.0
    return min(q, 1.0) if trust_clip else q


def lamb_step_ref(p, g, m, v2, slow, lr, wd, max_norm, sync, alpha, gs, b2, eps, bc1, bc2, omb1, omb2, sumsq, trust_clip, tensors, norms=None):
    """One LAMB step in float64. lr, wd: per-element arrays (constant within a tensor; lr already times the schedule's multiplier); tensors:
    [Tensor]; norms: [(sum p^2, sum r^2)] per tensor, default the float64 ones. Elements outside every tensor come back unchanged."""
    p, g, m, v2, slow = (np.array(a, np.float64) for a in (p, g, m, v2, slow))
    lr, wd = np.asarray(lr, np.float64), np.asarray(wd, np.float64)
    gmul = gs * clip_factor(sumsq, gs, max_norm)
    q, r = np.ones_like(p), np.zeros_like(p)
    for t in tensors:
        s = slice(t.start, t.start + t.n)
        ge = g[s] * gmul
        m[s] = m[s] + omb1 * (ge - m[s])
        v2[s] = b2 * v2[s] + omb2 * ge * ge
        r[s] = (m[s] / bc1) / (np.sqrt(v2[s] / bc2) + eps) + wd[s] * p[s]
    if norms is None:
        norms = squared_norms(p, r, tensors)
    for t, (pp, rr) in zip(tensors, norms):
        s = slice(t.start, t.start + t.n)
        if t.adapted and t.n:
            q[s] = trust_ratio(np.sqrt(pp), np.sqrt(rr), trust_clip)
        p[s] = p[s] - lr[s] * q[s] * r[s]
        if sync:
            p[s] = alpha * p[s] + (1 - alpha) * slow[s]
            slow[s] = p[s]
    return Step(p, m, v2, slow, q, r)


# ================================================================================================ shared checks (simulator and device)
# A backend is a callable be(bufs, rows, hp, ss, calls) -> dict of the buffers afterwards. bufs: numpy arrays p, g, m, v2, slow (f32), cast (uint16
# bf16 bits, or None: no bf16 copy is given to the kernel), partials, norms (f32); rows: [(start, count, lr, wd, reserved)]; calls, run in order on
# copies of the buffers: ("moments" | "lamb" | "adamw", first item, number of items). A moments call gets partials[2 first : 2 (first + n)], as
# FusedLAMB.launch passes them. tests/test_wavesim_lamb.py runs the kernels on the wave simulator, tests/test_gpu_lamb_ops.py on the device.
#
# The item table is update_table.table(): tensors of 4 (thread 0 alone), 1028 (second sweep), 8192 (exactly one item) and 8192 * 3 + 1020 elements (four
# items, ragged last), two not-adapted tensors between adapted ones, an adapted tensor with g = 0, zero moments and wd = 0 (r = 0, so q = 1: its
# weight decay is the one figure changed against lars_ref's table) and one with p = 0 (q = 1; it still moves by lr u). Sentinels in every gap,
# behind every buffer, in the norm slots no tensor owns and in the partial pairs of not-adapted items. The adapted tensors' parameters are
# scaled by 3 or by 0.3 (|u| is at most of order one per element), so that some trust ratios are above 1 and some below: TRUST_CLIP bites.
B1, B2, EPS = 0.9, 0.999, 1e-6
P_SCALE = (3.0, 0.3)                           # of tensor i: P_SCALE[(i // 2) % 2] (adapted tensors 0, 5 -> 3; 2, 3 -> 0.3)
MEASURED = {}                                  # running maxima of what the checks print, by name


def _note(name, value):
    return U.note(MEASURED, name, value)


def table(adapt=True):
    """update_table.table() with the weight decay of the g = 0 tensor set to 0."""
    rows, tensors, slots, heads, n = U.table(adapt)
    for t, (_, _, special) in zip(tensors, TABLE):
        if special == "g0":
            rows = [(s, c, lr, 0.0 if t.start <= s < t.start + t.n else wd, tag) for s, c, lr, wd, tag in rows]
    return rows, tensors, slots, heads, n


def problem(seed, adapt=True, step=1000):
    """step 1: the zero moments FusedLAMB starts from; a later step: random m and v2 >= m^2, as test_gpu_optim_ops.test_adamw_step_matches_float64."""
    rows, tensors, slots, heads, n = table(adapt)
    rng = np.random.default_rng(seed)
    inside = U.inside_of(tensors, n)
    p, g, slow = (np.where(inside, rng.standard_normal(n), SENT).astype(np.float32) for _ in range(3))
    g = np.where(inside, g * 0.01, SENT).astype(np.float32)
    if step == 1:
        m, v2 = (np.where(inside, 0.0, SENT).astype(np.float32) for _ in range(2))
    else:
        m = np.where(inside, rng.standard_normal(n) * 0.01, SENT).astype(np.float32)
        v2 = np.where(inside, m.astype(np.float64) ** 2 * (1 + rng.random(n)), SENT).astype(np.float32)
    for i, (t, (_, _, special)) in enumerate(zip(tensors, TABLE)):
        s = slice(t.start, t.start + t.n)
        p[s] *= np.float32(P_SCALE[(i // 2) % 2])
        if special == "g0":
            g[s] = m[s] = v2[s] = 0.0
        if special == "p0":
            p[s] = 0.0
    bufs, lr, wd = U.finish_problem({"p": p, "g": g, "m": m, "v2": v2, "slow": slow}, rows, n)
    return bufs, rows, tensors, slots, heads, inside, lr, wd


def _hp(max_norm=0.0, sync=False, gs=1.0, step=1000, trust_clip=False):
    """As FusedLAMB.upload_hp: the bias corrections and 1 - beta formed in double on the host, uploaded as f32; sixteen floats."""
    return np.array([0.5, B1, max_norm, float(sync), 0.5, gs, B2, EPS, 1.0 - B1 ** step, 1.0 - B2 ** step, 1.0 - B1, 1.0 - B2, float(trust_clip),
                     0.0, 0.0, 0.0], np.float32)


def _ref(bufs, lr, wd, hp, ss, tensors):
    h = [float(x) for x in hp]
    return lamb_step_ref(bufs["p"], bufs["g"], bufs["m"], bufs["v2"], bufs["slow"], lr * h[0], wd, h[2], h[3] != 0, h[4], h[5], h[6], h[7], h[8], h[9],
                         h[10], h[11], float(ss), h[12] != 0, tensors)


def _check_norms_of(what, out, bufs, ref, tensors, slots, launched):
    """norms after a moments call over the tensors `launched` (indices): the launched slots against float64, every other slot untouched."""
    U.check_norm_slots("LAMBERR", what, out["norms"], (("p", bufs["p"]), ("r", ref.r)), tensors, slots, launched, MEASURED)


def _check_moments(what, out, ref, inside):
    """m, v2 within 1e-5 * max|ref| (tests/test_gpu_optim_ops.py's moment bound of the AdamW kernel)."""
    for name, r in (("m", ref.m), ("v2", ref.v2)):
        err, top = np.abs(out[name].astype(np.float64) - r)[inside].max(), np.abs(r[inside]).max()
        print(f"LAMBERR {what} {name}: max err {err:.2e}, bound {1e-5 * top:.2e}, running max of err / bound {_note('moments ' + name, err / (1e-5 * top)):.4f}")
        assert err <= 1e-5 * top, (what, name, err, top)


STEPS = [1, 1000]


def check_norms(be, step):
    """lamb_moments alone. Each of sum p^2, sum r^2 within 1e-5 * max(1, sum of terms) of float64 (the project's sumsq bound); two runs
    bit-identical; the slots no launched tensor owns, the partial pairs of not-adapted items and everything behind both buffers untouched; p and g
    (and slow, the bf16 copy) come back bit for bit; m and v2 within the AdamW kernel test's moment bound inside items and untouched outside. Then
    a launch of the items of tensors 3 .. 7 only: the slots and moments of tensors 0 .. 2 stay untouched and the launched ones equal the full
    launch bit for bit."""
    bufs, rows, tensors, slots, heads, inside, lr, wd = problem(31 + step, step=step)
    n = len(rows)
    max_norm, ss = clip_setup("active", bufs["g"], inside, 0.25)
    hp, ssa = _hp(max_norm, False, 0.25, step), np.array([ss], np.float32)
    ref = _ref(bufs, lr, wd, hp, ss, tensors)
    outs = [be(bufs, rows, hp, ssa, [("moments", 0, n)]) for _ in range(2)]
    for name in ("norms", "partials", "m", "v2"):
        assert R.same_bits(outs[0][name], outs[1][name]), f"two runs differ in {name}"
    out = outs[0]
    _check_norms_of(f"step {step} full table", out, bufs, ref, tensors, slots, range(len(tensors)))
    _check_moments(f"step {step} full table", out, ref, inside)
    adapted_item = np.array([r[4] != 0 for r in rows])
    pairs = out["partials"][:2 * n].reshape(n, 2)
    assert (pairs[~adapted_item] == SENT).all() and (out["partials"][2 * n:] == SENT).all(), "partials of not-adapted items / behind the buffer"
    assert (pairs[adapted_item] != SENT).all()
    for name in ("p", "g", "slow", "cast"):
        _kept(name, out[name], bufs[name], np.ones(len(bufs[name]), bool))
    for name in ("m", "v2"):
        _kept(name, out[name], bufs[name], ~inside)
    k = heads[3]
    sub = be(bufs, rows, hp, ssa, [("moments", k, n - k)])
    _check_norms_of(f"step {step} items of tensors 3 .. 7", sub, bufs, ref, tensors, slots, range(3, len(tensors)))
    for i in range(3, len(tensors)):
        if slots[i] is not None:
            assert R.same_bits(sub["norms"][2 * slots[i]:2 * slots[i] + 2], out["norms"][2 * slots[i]:2 * slots[i] + 2]), i
    assert (sub["partials"][:2 * k] == SENT).all()
    before = np.arange(len(inside)) < tensors[3].start
    for name in ("m", "v2"):
        _kept(name + " of the tensors not launched", sub[name], bufs[name], before)
        assert R.same_bits(sub[name][~before], out[name][~before])


def check_step(be, sync, cast, clip, gs, step, trust_clip):
    """lamb_moments + lamb_step over the whole table against lamb_step_ref fed the float64 norms. Per element of p and slow
    |got - ref| <= 2e-6 * max(1, max|ref|) + 2e-5 * |delta_ref|, delta_ref = lr mult q r: the AdamW kernel's bound (tests/test_gpu_optim_ops.py:
    2e-6 * max(1, max|ref|), test_gpu_optim.py's figure against torch.optim.AdamW) plus the trust ratio's (tests/test_gpu_lars_ops.py: two sums
    each within 1e-5 -> their roots within 5e-6 -> the ratio within 1e-5, doubled for the f32 roundings that form q). m, v2 within 1e-5 * max|ref|."""
    bufs, rows, tensors, slots, heads, inside, lr, wd = problem(32 + step, step=step)
    if not cast:
        bufs = dict(bufs, cast=None)
    cast0 = R.to_bf16_bits(np.full(len(inside), 3.0, np.float32))
    max_norm, ss = clip_setup(clip, bufs["g"], inside, gs)
    hp = _hp(max_norm, sync, gs, step, trust_clip)
    h = [float(x) for x in hp]
    ref = _ref(bufs, lr, wd, hp, ss, tensors)
    free = _ref(bufs, lr, wd, _hp(max_norm, sync, gs, step, False), ss, tensors)          # the ratios before TRUST_CLIP
    qs = []
    for t, (_, slot, special) in zip(tensors, TABLE):          # the table does what it says
        q, qf = ref.q[t.start], free.q[t.start]
        if slot is None or special:
            assert q == 1.0 and qf == 1.0, (t, q)
        else:
            assert 1e-2 < qf < 1e2 and abs(qf - 1.0) > 0.1 and q == (min(qf, 1.0) if trust_clip else qf), (t, q, qf)
            qs.append(qf)
    assert min(qs) < 1.0 < max(qs), "TRUST_CLIP is only tested if ratios above 1 and ratios below 1 both occur"
    t0 = tensors[7]
    assert TABLE[7][2] == "p0" and np.abs(ref.p[t0.start:t0.start + t0.n]).min() > 0, "the p = 0 tensor still moves by lr u"
    n = len(rows)
    out = be(bufs, rows, hp, np.array([ss], np.float32), [("moments", 0, n), ("lamb", 0, n)])
    delta = np.abs(lr * h[0] * ref.q * ref.r)
    what = f"step={step} sync={sync} clip={clip} gs={gs} trust_clip={trust_clip}"
    for name, r, d in (("p", ref.p, delta), ("slow", ref.slow, delta if sync else 0 * delta)):
        err = np.abs(out[name].astype(np.float64) - r)[inside]
        bound = (2e-6 * max(1.0, np.abs(r[inside]).max()) + 2e-5 * d)[inside]
        print(f"LAMBERR step {name} {what}: max err / bound = {(err / bound).max():.3f}, max err {err.max():.2e}, running max of err / bound "
              f"{_note('step ' + name, (err / bound).max()):.3f}")
        assert (err <= bound).all(), (name, float((err / bound).max()))
    _check_moments(what, out, ref, inside)
    for name in ("p", "g", "m", "v2", "slow"):
        _kept(name, out[name], bufs[name], ~inside)
    assert not out["g"][inside].any(), "g must be zero inside items"
    g0 = tensors[6]
    assert TABLE[6][2] == "g0"
    if not sync:
        _kept("slow (no sync)", out["slow"], bufs["slow"], np.ones(len(inside), bool))
        _kept("p of the tensor with r = 0", out["p"][g0.start:g0.start + g0.n], bufs["p"][g0.start:g0.start + g0.n], np.ones(g0.n, bool))
    else:
        assert np.array_equal(out["slow"][inside], out["p"][inside]), "after a sync the slow weights are the fast ones"
    if cast:
        _kept("cast", out["cast"], cast0, ~inside)
        assert np.array_equal(out["cast"][inside], R.to_bf16_bits(out["p"])[inside]), "the bf16 copy must be the round-to-nearest-even of the returned p"
    else:
        assert out["cast"] is None
    _check_norms_of(what, out, bufs, ref, tensors, slots, range(len(tensors)))


def check_not_adapted_is_adamw(be):
    """The same table with every reserved word 0: clite_lamb_moments + clite_lamb_step give clite_adamw_step's p, g, m, v2, slow and bf16 copy bit
    for bit (sync and clipping on, and off; step 1 and a later step; with and without the bf16 copy, which are two instantiations of both
    kernels), and neither norms nor partials is written."""
    for step, sync, clip, gs, cast in ((1000, True, "active", 0.25, True), (1, False, "disabled", 1.0, True), (1000, True, "inactive", 1.0, False)):
        bufs, rows, tensors, slots, heads, inside, _, _ = problem(33 + step, adapt=False, step=step)
        if not cast:
            bufs = dict(bufs, cast=None)
        n = len(rows)
        max_norm, ss = clip_setup(clip, bufs["g"], inside, gs)
        hp, ssa = _hp(max_norm, sync, gs, step, True), np.array([ss], np.float32)
        a = be(bufs, rows, hp, ssa, [("moments", 0, n), ("lamb", 0, n)])
        b = be(bufs, rows, hp, ssa, [("adamw", 0, n)])
        for name in ("m", "v2", "p", "g", "slow") + (("cast",) if cast else ()):
            assert R.same_bits(a[name], b[name]), f"{name} differs from clite_adamw_step (step={step}, sync={sync}, clip={clip}, cast={cast})"
        assert not R.same_bits(a["p"], bufs["p"])
        assert (a["norms"] == SENT).all() and (a["partials"] == SENT).all()


def check_split_launch(be):
    """Items [0, k) then [k, n), k on a tensor boundary (moments and update of each range, as FusedLAMB.launch(span) enqueues them), equal one
    launch bit for bit - on a sync step with clipping active."""
    bufs, rows, tensors, slots, heads, inside, _, _ = problem(34)
    n = len(rows)
    max_norm, ss = clip_setup("active", bufs["g"], inside, 0.25)
    hp, ssa = _hp(max_norm, True, 0.25), np.array([ss], np.float32)
    one = be(bufs, rows, hp, ssa, [("moments", 0, n), ("lamb", 0, n)])
    for ti in (5, 6):          # in front of the four-item tensor, and behind it
        k = heads[ti]
        two = be(bufs, rows, hp, ssa, [("moments", 0, k), ("lamb", 0, k), ("moments", k, n - k), ("lamb", k, n - k)])
        for name in ("p", "g", "m", "v2", "slow", "cast", "norms", "partials"):
            assert R.same_bits(one[name], two[name]), f"{name}: split at item {k} differs from one launch"
