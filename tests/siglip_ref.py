"""float64 reference of the SigLIP pairwise sigmoid loss (csrc/siglip_ops.hip; Zhai et al. 2023, Algorithm 1) and the checks the wave simulator and
the device share, in the shape of tests/loss_ref.py, whose bounds (`scalar`, `elem`, `same_bits`) are used unchanged.

  x_ij = exp(temperature) * C[i][j] + bias,  z_ij = +1 if i == j else -1,  L = 1/B * sum_ij softplus(-z_ij x_ij)

The reference is written from that definition on torch-CPU float64 with gradients from torch.autograd; nothing here calls into clip_lite_amd or
the simulator. tests/test_siglip_ref_host.py checks it against central finite differences and against the paper's pseudocode."""
import ctypes as C
from collections import namedtuple

import numpy as np
import torch

import loss_ref as R
from loss_backends import BF16, F32, HipBackend, SimBackend

T_INIT, B_INIT = float(np.float32(np.log(10.0))), -10.0          # the paper's initial values: t' = log 10, b = -10
T100 = float(np.float32(np.log(100.0)))

SigLIP = namedtuple("SigLIP", "loss row_terms dC dtemp dtemp_terms dbias dbias_terms")

_V, _I, _F = C.c_void_p, C.c_int, C.c_float
SIGNATURES = {
    "siglip_fwd": [_V, _I, _I, _V, _V, _V, _V],
    "siglip_bwd": [_I, _V, _I, _I, _V, _V, _V, _F, _V, _I, _V, _V, _V],
}


class SiglipSimBackend(SimBackend):
    def __init__(self):
        super().__init__()
        for n, sig in SIGNATURES.items():
            getattr(self.L, "clite_" + n).argtypes = sig + [_V]


class SiglipHipBackend(HipBackend):
    def set_deterministic(self, on):
        self.hip.set_deterministic(on)


def siglip_loss(Cm, temperature, bias):
    """(L, per-row terms [B], x) on torch float64 tensors; C is [B][B]."""
    B = Cm.shape[0]
    z = 2 * torch.eye(B, dtype=torch.float64) - 1
    x = torch.exp(temperature) * Cm + bias
    rows = R.softplus(-z * x).sum(1) / B
    return rows.sum(), rows, x


def siglip_ref(Cm, temperature, bias, gout=1.0):
    """gout: the upstream gradient times the launcher's `scale`. dtemp_terms / dbias_terms: the [B][B] contributions of every pair."""
    Cm, t, b = R._t(Cm, True), R._t(temperature, True), R._t(bias, True)
    L, rows, x = siglip_loss(Cm, t, b)
    x.retain_grad()
    (L * gout).backward()
    dx = x.grad                                                   # gout * dL/dx
    tt = dx * (torch.exp(t) * Cm).detach()                        # dx/dtemp = t C
    return SigLIP(L.item(), R._np(rows), R._np(Cm.grad), t.grad.item(), R._np(tt), b.grad.item(), R._np(dx))


def siglip_dC_float32(Cm, temperature, bias, gout):
    """The backward's formula, g t (-z sigmoid(-z x)) / B, in plain torch.float32 (CPU): what float32 can reach (x = t C + bias is rounded at
    |x| up to 110, and exp(temperature) is a float32)."""
    Cm = torch.tensor(np.asarray(Cm, np.float32))
    B = Cm.shape[0]
    t = torch.exp(torch.tensor(np.float32(temperature)).reshape(()))
    x = t * Cm + torch.tensor(np.float32(bias))
    z = 2 * torch.eye(B, dtype=torch.float32) - 1
    return (torch.tensor(np.float32(gout)) / B * t * (-z * torch.sigmoid(-z * x))).numpy()


def cosines(B, rng):
    """[B][B] cosines of correlated unit vectors: the diagonal stands out, as after some training."""
    a = rng.standard_normal((B, 32))
    b = rng.standard_normal((B, 32)) + 0.7 * a
    return (a / np.linalg.norm(a, axis=1, keepdims=True)) @ (b / np.linalg.norm(b, axis=1, keepdims=True)).T


def check_siglip(be, dt, B, ld, ldd, temperature, bias, repeat=False):
    """siglip_fwd + siglip_bwd on a cosine matrix [B][ld] whose columns >= B hold 1e4 (they must enter nothing); dC is [B][ldd], zero in columns
    >= B, with a sentinel row behind it; acc, dtemp, dbias start non-zero. repeat: twice with the deterministic mode off and twice with it on,
    each pair bit-identical (the kernels use no float atomics in either mode)."""
    rng = R._rng(B, ld, ldd, 23)
    Cm = np.full((B + 1, ld), 1e4, np.float32)
    Cm[:B, :B] = cosines(B, rng)
    temp, bia = np.array([temperature], np.float32), np.array([bias], np.float32)
    gout, scale = np.array([1.3], np.float32), 0.9
    gs = float(gout[0]) * float(np.float32(scale))
    ref = siglip_ref(Cm[:B, :B], temp[0], bia[0], gout=gs)
    acc0, dtemp0, dbias0 = np.array([0.25, -0.5], np.float32), np.array([0.375], np.float32), np.array([-0.125], np.float32)
    what = f"siglip ({B}, {ld}, {ldd}) t={temperature:.3f} b={bias:g} {'bf16' if dt == BF16 else 'f32'}"
    f32_eval = siglip_dC_float32(Cm[:B, :B], temp[0], bia[0], gs)

    def run():
        Cd, t, b, g = be.dev(Cm, F32), be.dev(temp, F32), be.dev(bia, F32), be.dev(gout, F32)
        part = be.dev(np.full(2 * B + 1, R.FILL), F32)
        acc, dtemp, dbias = be.dev(acc0, F32), be.dev(dtemp0, F32), be.dev(dbias0, F32)
        dC = be.dev(np.full((B + 1, ldd), R.FILL), dt)
        assert be.call("siglip_fwd", Cd, ld, B, t, b, part, acc) == 0
        a_ = be.host(acc)
        assert be.call("siglip_bwd", dt, Cd, ld, B, t, b, g, scale, dC, ldd, part, dtemp, dbias) == 0
        d, dtm, dbs, pt = be.host(dC), be.host(dtemp), be.host(dbias), be.host(part)
        R.scalar(f"{what} acc[0]", a_[0], acc0[0] + ref.loss, ref.row_terms)
        assert R.same_bits(a_[1:], acc0[1:]) and R.same_bits(be.host(acc), a_), f"{what}: acc[1] must be left alone (and backward must not touch acc)"
        R.elem(f"{what} dC", d[:B, :B], ref.dC, dt, f32_eval=f32_eval)
        assert not d[:B, B:].any(), f"{what}: dC columns >= B must be zero"
        assert (d[B] == R.FILL).all(), f"{what}: sentinel row of dC"
        R.scalar(f"{what} dtemp", dtm[0], dtemp0[0] + ref.dtemp, ref.dtemp_terms)
        R.scalar(f"{what} dbias", dbs[0], dbias0[0] + ref.dbias, ref.dbias_terms)
        assert pt[2 * B] == R.FILL, f"{what}: sentinel behind part"
        assert R.same_bits(be.host(Cd), Cm)
        return a_, d, dtm, dbs

    if not repeat:
        run()
        return
    for on in (False, True):
        be.set_deterministic(on)
        try:
            first, second = run(), run()
        finally:
            be.set_deterministic(False)
        assert all(R.same_bits(p, q) for p, q in zip(first, second)), f"{what}: two runs differ (deterministic mode {'on' if on else 'off'})"


def check_siglip_no_scalar_grads(be, dt, B=24):
    """dtemp and dbias are optional, each on its own: the other one and dC still come out."""
    rng = R._rng(B, 29)
    Cm = cosines(B, rng).astype(np.float32)
    temp, bia, gout = np.array([T_INIT], np.float32), np.array([B_INIT], np.float32), np.array([1.0], np.float32)
    ref = siglip_ref(Cm, temp[0], bia[0])
    for with_t, with_b in ((True, False), (False, True), (False, False)):
        Cd, t, b, g = be.dev(Cm, F32), be.dev(temp, F32), be.dev(bia, F32), be.dev(gout, F32)
        part, dC = be.dev(np.zeros(2 * B), F32), be.dev(np.full((B, B), R.FILL), dt)
        dtemp, dbias = (be.dev(np.zeros(1), F32) if with_t else None), (be.dev(np.zeros(1), F32) if with_b else None)
        assert be.call("siglip_bwd", dt, Cd, B, B, t, b, g, 1.0, dC, B, part, dtemp, dbias) == 0
        R.elem(f"siglip no-scalar dC {with_t} {with_b}", be.host(dC), ref.dC, dt, f32_eval=siglip_dC_float32(Cm, temp[0], bia[0], 1.0))
        if with_t:
            R.scalar("siglip dtemp alone", be.host(dtemp)[0], ref.dtemp, ref.dtemp_terms)
        if with_b:
            R.scalar("siglip dbias alone", be.host(dbias)[0], ref.dbias, ref.dbias_terms)


def check_siglip_refusals(be):
    """B <= 0, ld < B, ldd < B, ldd % 8, an unknown dtype and a NULL among the required pointers: status -1, and no buffer is written."""
    B = 8
    for dt in (BF16, F32):
        bufs = {"C": be.dev(np.full((B, B), 0.5), F32), "t": be.dev(np.array([T_INIT]), F32), "b": be.dev(np.array([B_INIT]), F32),
                "g": be.dev(np.ones(1), F32), "part": be.dev(np.full(2 * B, R.FILL), F32), "acc": be.dev(np.full(2, R.FILL), F32),
                "dC": be.dev(np.full((B, 16), R.FILL), dt), "dtemp": be.dev(np.full(1, R.FILL), F32), "dbias": be.dev(np.full(1, R.FILL), F32)}

        def fwd(B_=B, ld=B, **nulls):
            a = {k: (None if k in nulls else v) for k, v in bufs.items()}
            return be.call("siglip_fwd", a["C"], ld, B_, a["t"], a["b"], a["part"], a["acc"])

        def bwd(dtype=dt, B_=B, ld=B, ldd=B, **nulls):
            a = {k: (None if k in nulls else v) for k, v in bufs.items()}
            return be.call("siglip_bwd", dtype, a["C"], ld, B_, a["t"], a["b"], a["g"], 1.0, a["dC"], ldd, a["part"], a["dtemp"], a["dbias"])

        assert fwd(B_=0) == -1 and fwd(B_=-8) == -1 and fwd(ld=B - 1) == -1
        for k in ("C", "t", "b", "part", "acc"):
            assert fwd(**{k: True}) == -1, f"siglip_fwd with a NULL {k}"
        assert bwd(B_=0) == -1 and bwd(ld=B - 1) == -1 and bwd(ldd=B - 8) == -1 and bwd(ldd=B + 4) == -1 and bwd(dtype=7) == -1
        for k in ("C", "t", "b", "g", "dC", "part"):
            assert bwd(**{k: True}) == -1, f"siglip_bwd with a NULL {k}"
        for k in ("part", "acc", "dC", "dtemp", "dbias"):
            assert (be.host(bufs[k]) == R.FILL).all(), f"a refused call wrote to {k}"
