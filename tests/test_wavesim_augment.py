"""CPU-side (wave simulator) checks of the augmentation kernels (csrc/augment_ops.hip) against the NumPy float64 restatement of the pixel
function (tests/augment_ref.py): N = 3 views of canvases of three different extents in one batch, at S = 16 and S = 10; crops that are exact,
upscale, downscale and touch every border; flip; each colour op alone and all four in several orders; both output forms over sentinel-filled
buffers; refused tables. Tolerance: 0.02 level of 255 (3.5e-4 after normalisation: 0.02 / 255 / 0.224) - about 50 f32 operations on values
<= 255 at 2^-24 relative each are 1e-3 level, with a margin of 20. Runs without a GPU."""
import ctypes as C

import numpy as np
import pytest

import augment_ref as R
from simlib import lib, ptr, to_bf16

_P, _I, _L = C.c_void_p, C.c_int, C.c_int64
PW = 16
NCHW, NHWC4, BF16, F32 = 0, 1, 0, 1
LEVEL = 0.02 / 255.0


def _bind():
    L = lib()
    L.clite_augment_gray_mean.argtypes = [_P, _P, _L, _P, _I, _I, _P, _P, _P, _P, _P]
    L.clite_augment_apply.argtypes = [_I, _I, _P, _P, _L, _P, _P, _I, _I, _P, _I, _I, _I, _P, _P, _P]
    return L


_rng = np.random.default_rng(11)
CANVASES = [_rng.integers(0, 256, (23, 37, 3), dtype=np.uint8), _rng.integers(0, 256, (40, 19, 3), dtype=np.uint8),
            _rng.integers(0, 256, (16, 16, 3), dtype=np.uint8)]
CAP = 40 * 37 * 3


def _pack(canvases=CANVASES, cap=CAP):
    buf = np.full((len(canvases), cap), 0xA5, np.uint8)          # the slack of a slot holds garbage: nothing may depend on it
    hw = np.zeros((len(canvases), 2), np.int32)
    for n, c in enumerate(canvases):
        buf[n, :c.size] = c.reshape(-1)
        hw[n] = c.shape[:2]
    return buf, hw


def row(box, flip=0, jit=0, fb=1.0, fc=1.0, fs=1.0, fh=0.0, order=(0, 1, 2, 3), norm=1):
    r = np.zeros(PW, np.float32)
    r[0:4] = box
    r[4], r[5], r[6], r[7], r[8], r[9] = flip, jit, fb, fc, fs, fh
    r[10:14] = order
    r[14] = norm
    return r


def _gray(L, buf, hw, plan, S, host=True):
    N = len(plan)
    mean = np.full(N, np.nan, np.float32)
    work = np.full(N * ((S * S + 255) // 256), np.nan, np.float32)
    rc = L.clite_augment_gray_mean(ptr(buf), ptr(hw), buf.shape[1], ptr(plan), N, S, ptr(mean), ptr(work), ptr(plan) if host else None,
                                   ptr(hw) if host else None, None)
    return rc, mean


def _apply(L, buf, hw, plan, mean, S, form, dtype, host=True):
    N = len(plan)
    pad, Hp, Wp = (0, S, S) if form == NCHW else (3, S + 6, S + 8 + (S + 8) % 2)
    if form == NCHW:
        out = np.full((N, 3, S, S), np.nan, np.float32)
    elif dtype == F32:
        out = np.full((N, Hp, Wp, 4), np.nan, np.float32)
    else:
        out = np.full((N, Hp, Wp, 4), 0x7FC0, np.uint16)          # bf16 NaN
    rc = L.clite_augment_apply(form, dtype, ptr(buf), ptr(hw), buf.shape[1], ptr(plan), ptr(mean), N, S, ptr(out), pad, Hp, Wp,
                               ptr(plan) if host else None, ptr(hw) if host else None, None)
    return rc, out


def _check(plan, S, canvases=CANVASES):
    """both kernels and every output form of one plan against the reference"""
    L = _bind()
    plan = np.ascontiguousarray(np.stack(plan), np.float32)
    buf, hw = _pack(canvases)
    rc, mean = _gray(L, buf, hw, plan, S)
    assert rc == 0
    want_mean = np.array([R.gray_mean(c, r, S) for c, r in zip(canvases, plan)])
    assert not np.isnan(mean).any()
    assert np.abs(mean - want_mean).max() <= 0.02, (mean, want_mean)
    for n, r in enumerate(plan):
        if r[5] == 0:
            assert mean[n] == 0
    rc, out = _apply(L, buf, hw, plan, mean, S, NCHW, F32)
    assert rc == 0
    assert not np.isnan(out).any(), "an element of the f32 form was not written"
    want = R.views(canvases, plan, S)
    for n, r in enumerate(plan):
        tol = LEVEL / (0.224 if r[14] else 1.0)
        err = np.abs(out[n] - want[n]).max()
        assert err <= tol, (n, err, tol)
    # the stem form: the same values, bit for bit, at (pad, pad) of a zero plane
    for dtype in (F32, BF16):
        rc, st = _apply(L, buf, hw, plan, mean, S, NHWC4, dtype)
        assert rc == 0
        N, Hp, Wp = st.shape[:3]
        full = np.zeros((N, Hp, Wp, 4), np.float32)
        full[:, 3:3 + S, 3:3 + S, :3] = out.transpose(0, 2, 3, 1)
        if dtype == F32:
            np.testing.assert_array_equal(st.view(np.uint32), full.view(np.uint32))
        else:
            np.testing.assert_array_equal(st, to_bf16(full))
    return out, mean


def test_identity_crop_is_exact():
    S = 16
    plan = [row((0, 0, 16, 16), norm=0), row((1, 20, 16, 16), norm=0), row((0, 0, 16, 16), norm=0)]
    out, _ = _check(plan, S)
    crops = [CANVASES[0][0:16, 0:16], CANVASES[1][20:36, 1:17], CANVASES[2]]
    for n, c in enumerate(crops):
        np.testing.assert_array_equal(out[n], (c.astype(np.float32) / np.float32(255)).transpose(2, 0, 1))


@pytest.mark.parametrize("S", [16, 10])
def test_resample_upscale_downscale_borders_flip(S):
    _check([row((5, 3, 9, 7)), row((0, 0, 19, 40)), row((2.5, 1.25, 11.5, 13.0))], S)                      # upscale 7 x 9; whole canvas; fractional box
    d = 2.3 * S                                                                                              # downscale by 2.3 on the axes that are long enough
    _check([row((0, 0, d, 23)) if S == 16 else row((7, 0, d, d)), row((0, 40 - d, 19, d)), row((0, 0, 16, 16))], S)
    _check([row((0, 0, 12, 10)), row((19 - 8, 40 - 30, 8, 30)), row((0, 16 - 5, 16, 5))], S)                # boxes on the left / top, right / bottom borders
    _check([row((5, 3, 9, 7), flip=1), row((0, 0, 19, 40), flip=1, norm=0), row((0, 0, 16, 16), flip=1)], S)


@pytest.mark.parametrize("S", [16, 10])
def test_each_colour_op_alone(S):
    box = [(3, 2, 30, 20), (1, 5, 17, 30), (0, 0, 16, 16)]
    for kw in (dict(fb=1.37), dict(fb=0.62), dict(fc=1.4), dict(fc=0.6), dict(fs=1.39), dict(fs=0.61), dict(fh=0.1), dict(fh=-0.07)):
        _check([row(b, jit=1, **kw) for b in box], S)


@pytest.mark.parametrize("order", [(1, 0, 2, 3), (0, 2, 3, 1), (3, 2, 1, 0), (2, 3, 0, 1), (0, 1, 2, 3)])
def test_all_ops_in_several_orders(order):
    """contrast first, contrast last and in between; one view of the batch without jitter, one without normalisation"""
    S = 16
    plan = [row((3, 2, 30, 20), jit=1, fb=1.3, fc=0.7, fs=1.35, fh=0.08, order=order, flip=1),
            row((1, 5, 17, 30), jit=0, fb=1.3, fc=0.7, fs=1.35, fh=0.08, order=order),
            row((0, 0, 16, 16), jit=1, fb=0.7, fc=1.38, fs=0.65, fh=-0.1, order=order, norm=0)]
    _check(plan, S)
    _check(plan, 10)


def test_gray_mean_is_reproducible_and_needs_no_host_mirror():
    L = _bind()
    S = 16
    plan = np.stack([row((3, 2, 30, 20), jit=1, fb=1.3, fc=0.7, order=(2, 0, 1, 3)), row((1, 5, 17, 30)), row((0, 0, 16, 16), jit=1, fc=1.2)])
    buf, hw = _pack()
    a = _gray(L, buf, hw, plan, S, host=True)[1]
    b = _gray(L, buf, hw, plan, S, host=False)[1]
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))


def test_bad_tables_are_refused_or_harmless():
    L = _bind()
    S = 4
    buf, hw = _pack()
    good = np.stack([row((0, 0, 16, 16)), row((0, 0, 16, 16)), row((0, 0, 16, 16))])
    mean = np.zeros(3, np.float32)
    over = good.copy()
    over[1, 2] = 4 * S + 1                                       # scale above 4 on x
    assert _gray(L, buf, hw, over, S)[0] == -4
    assert _apply(L, buf, hw, over, mean, S, NCHW, F32)[0] == -4
    over[1, 2], over[1, 3] = 16, 4 * S + 0.5                      # ... on y
    assert _apply(L, buf, hw, over, mean, S, NHWC4, BF16)[0] == -4
    bad_hw = hw.copy()
    bad_hw[2] = (200, 200)                                       # does not fit its slot
    assert L.clite_augment_apply(NCHW, F32, ptr(buf), ptr(bad_hw), buf.shape[1], ptr(good), ptr(mean), 3, S, ptr(np.zeros((3, 3, S, S), np.float32)),
                                 0, S, S, ptr(good), ptr(bad_hw), None) == -2
    outside = good.copy()
    outside[0, 0] = 30                                           # x0 + cw > w
    assert _apply(L, buf, hw, outside, mean, S, NCHW, F32)[0] == -3
    perm = good.copy()
    perm[0, 10:14] = (0, 0, 1, 2)
    assert _apply(L, buf, hw, perm, mean, S, NCHW, F32)[0] == -3
    nan = good.copy()
    nan[2, 6] = np.nan
    assert _gray(L, buf, hw, nan, S)[0] == -3
    assert L.clite_augment_apply(7, F32, ptr(buf), ptr(hw), buf.shape[1], ptr(good), ptr(mean), 3, S, ptr(np.zeros((3, 3, S, S), np.float32)),
                                 0, S, S, None, None, None) == -1
    assert L.clite_augment_apply(NCHW, BF16, ptr(buf), ptr(hw), buf.shape[1], ptr(good), ptr(mean), 3, S, ptr(np.zeros((3, 3, S, S), np.float32)),
                                 0, S, S, None, None, None) == -1
    assert L.clite_augment_apply(NHWC4, BF16, ptr(buf), ptr(hw), buf.shape[1], ptr(good), ptr(mean), 3, S, ptr(np.zeros((3, 9, 12, 4), np.uint16)),
                                 3, 9, 12, None, None, None) == -1          # Hp < S + 2 pad
    assert L.clite_augment_gray_mean(None, ptr(hw), buf.shape[1], ptr(good), 3, S, ptr(mean), ptr(mean), None, None, None) == -1
    # without the mirrors the same tables run and stay inside their buffers: a view whose extent does not fit is zeros, the others are right
    rc, out = _apply(L, buf, bad_hw, outside, mean, S, NCHW, F32, host=False)
    assert rc == 0 and not np.isnan(out[1:]).any()          # (view 0's box leaves its canvas: its taps are clipped, its values undefined)
    assert not out[2].any()
    want = R.view(CANVASES[1], good[1], S)
    assert np.abs(out[1] - want).max() <= LEVEL / 0.224
