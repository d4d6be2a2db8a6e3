"""CPU-side (wave simulator) checks of clite_augment_apply_post (csrc/augment_ops.hip: gray and blur behind the colour jitter) against
tests/augment_post_ref.py, on the three canvases of tests/test_wavesim_augment.py: gray alone, blur at k = 3, 5, 7, gray + blur + jitter + flip and
a batch that mixes blurred and plain rows at S = 16 and S = 10; S = 4, the smallest blurred view; S = 36, which spans two 32-pixel tiles on both
axes with a 4-pixel remainder (where the halo indexing can go wrong); an all-zero table and the plain rows of a mixed batch bit-equal to
clite_augment_apply; both NHWC4 forms bit-equal to the f32 form over sentinel-filled buffers; the refused tables.

Tolerance: the 0.02 level of 255 of tests/test_wavesim_augment.py (about 50 f32 operations at 2^-24 relative on values <= 255 are 1e-3 level, margin
20). Blur is a convex combination, so it does not amplify the incoming error, and its 14 multiply-adds on values <= 255 add about 2e-4 level:
the bound holds with a margin above 10. Runs without a GPU."""
import ctypes as C

import numpy as np
import pytest

import augment_post_ref as PR
import test_wavesim_augment as T
from simlib import ptr, to_bf16

_P, _I, _L = C.c_void_p, C.c_int, C.c_int64
NCHW, NHWC4, BF16, F32 = T.NCHW, T.NHWC4, T.BF16, T.F32
LEVEL = 0.02 / 255.0
TILE = 32
row, post_row = T.row, PR.post_row
BOXES = [(3, 2, 30, 20), (1, 5, 17, 30), (0, 0, 16, 16)]


def _bind():
    L = T._bind()
    L.clite_augment_apply_post.argtypes = [_I, _I, _P, _P, _L, _P, _P, _P, _I, _I, _P, _I, _I, _I, _P, _P, _P, _P]
    return L


def _apply_post(L, buf, hw, plan, post, mean, S, form, dtype, host=True):
    N = len(plan)
    pad, Hp, Wp = (0, S, S) if form == NCHW else (3, S + 6, S + 8 + (S + 8) % 2)
    if form == NCHW:
        out = np.full((N, 3, S, S), np.nan, np.float32)
    elif dtype == F32:
        out = np.full((N, Hp, Wp, 4), np.nan, np.float32)
    else:
        out = np.full((N, Hp, Wp, 4), 0x7FC0, np.uint16)          # bf16 NaN
    rc = L.clite_augment_apply_post(form, dtype, ptr(buf), ptr(hw), buf.shape[1], ptr(plan), ptr(post), ptr(mean), N, S, ptr(out), pad, Hp, Wp,
                                    ptr(plan) if host else None, ptr(hw) if host else None, ptr(post) if host else None, None)
    return rc, out


def _tables(plan, post, canvases):
    plan = np.ascontiguousarray(np.stack(plan), np.float32)
    post = np.ascontiguousarray(np.stack(post), np.float32)
    buf, hw = T._pack(canvases)
    return plan, post, buf, hw


def _check(plan, post, S, canvases=T.CANVASES):
    """the f32 form against the reference, both stem forms against the f32 form"""
    L = _bind()
    plan, post, buf, hw = _tables(plan, post, canvases)
    rc, mean = T._gray(L, buf, hw, plan, S)
    assert rc == 0
    rc, out = _apply_post(L, buf, hw, plan, post, mean, S, NCHW, F32)
    assert rc == 0
    assert not np.isnan(out).any(), "an element of the f32 form was not written"
    want = PR.views(canvases, plan, post, S)
    for n, r in enumerate(plan):
        tol = LEVEL / (0.224 if r[14] else 1.0)
        err = np.abs(out[n] - want[n]).max()
        assert err <= tol, (n, err, tol)
    for dtype in (F32, BF16):          # the same values, bit for bit, at (3, 3) of a zero plane
        rc, st = _apply_post(L, buf, hw, plan, post, mean, S, NHWC4, dtype)
        assert rc == 0
        N, Hp, Wp = st.shape[:3]
        full = np.zeros((N, Hp, Wp, 4), np.float32)
        full[:, 3:3 + S, 3:3 + S, :3] = out.transpose(0, 2, 3, 1)
        if dtype == F32:
            np.testing.assert_array_equal(st.view(np.uint32), full.view(np.uint32))
        else:
            np.testing.assert_array_equal(st, to_bf16(full))
    return out


def _plain(plan, S, form, dtype, canvases=T.CANVASES):
    """what clite_augment_apply gives for the same plan"""
    L = _bind()
    plan = np.ascontiguousarray(np.stack(plan), np.float32)
    buf, hw = T._pack(canvases)
    rc, mean = T._gray(L, buf, hw, plan, S)
    assert rc == 0
    rc, out = T._apply(L, buf, hw, plan, mean, S, form, dtype)
    assert rc == 0
    return out


@pytest.mark.parametrize("S", [16, 10])
def test_gray_alone(S):
    _check([row(b) for b in BOXES], [post_row(gray=1)] * 3, S)
    out = _check([row(b, norm=0, jit=1, fs=1.3, fh=0.05) for b in BOXES], [post_row(gray=1)] * 3, S)
    assert (out[:, 0] == out[:, 1]).all() and (out[:, 1] == out[:, 2]).all()          # without normalisation: three equal channels


@pytest.mark.parametrize("S", [16, 10])
@pytest.mark.parametrize("k", [3, 5, 7])
def test_blur_alone(S, k):
    _check([row(b) for b in BOXES], [post_row(k=k)] * 3, S)
    _check([row((5, 3, 9, 7), norm=0), row((0, 0, 19, 40)), row((2.5, 1.25, 11.5, 13.0))], [post_row(k=k)] * 3, S)


@pytest.mark.parametrize("S", [16, 10])
def test_gray_blur_jitter_flip(S):
    plan = [row(BOXES[0], jit=1, fb=1.3, fc=0.7, fs=1.35, fh=0.08, order=(1, 0, 2, 3), flip=1),
            row(BOXES[1], jit=1, fb=0.7, fc=1.38, fs=0.65, fh=-0.1, order=(3, 2, 1, 0), flip=1, norm=0),
            row(BOXES[2], jit=1, fb=1.2, fc=1.3, fs=0.8, fh=0.05, order=(0, 2, 3, 1))]
    _check(plan, [post_row(gray=1, k=7), post_row(gray=1, k=5), post_row(gray=1, k=3)], S)
    _check(plan, [post_row(k=7), post_row(k=3), post_row(k=5)], S)          # coloured values through the blur


@pytest.mark.parametrize("S", [16, 10])
def test_mixed_batch_and_its_plain_rows(S):
    plan = [row(BOXES[0], jit=1, fb=1.3, fc=0.7, fs=1.35, fh=0.08, flip=1), row(BOXES[1]), row(BOXES[2], jit=1, fc=1.2, norm=0)]
    post = [post_row(k=5), post_row(), post_row()]
    out = _check(plan, post, S)
    old = _plain(plan, S, NCHW, F32)
    np.testing.assert_array_equal(out[1:].view(np.uint32), old[1:].view(np.uint32))
    assert np.abs(out[0] - old[0]).max() > 10 * LEVEL          # (and the blurred row is blurred)
    out = _check(plan, [post_row(), post_row(gray=1, k=7), post_row()], S)
    np.testing.assert_array_equal(out[[0, 2]].view(np.uint32), old[[0, 2]].view(np.uint32))


def test_smallest_blurred_view():
    for k in (3, 5, 7):
        _check([row(b, jit=1, fb=1.1, fs=1.2) for b in ((3, 2, 12, 10), (1, 5, 9, 14), (0, 0, 16, 16))],          # (at most 4 x the view)
               [post_row(k=k), post_row(gray=1, k=k), post_row(k=k)], 4)


def test_view_that_spans_tiles_with_a_remainder():
    """S = tile + 4: two tiles per axis, the second 4 pixels wide; N = 1 keeps the simulator's run short"""
    S = TILE + 4
    for n, k in ((0, 7), (1, 5)):
        _check([row(BOXES[n], jit=1, fb=1.2, fc=0.8, fs=1.3, fh=0.05, flip=n)], [post_row(gray=n, k=k)], S, canvases=T.CANVASES[n:n + 1])
    out = _check([row(BOXES[1])], [post_row(gray=1)], S, canvases=T.CANVASES[1:2])          # the path without LDS
    assert out.shape == (1, 3, S, S)


@pytest.mark.parametrize("S", [16, 36])
def test_all_zero_table_is_bit_equal_to_the_plain_entry(S):
    L = _bind()
    plan = [row(BOXES[0], jit=1, fb=1.3, fc=0.7, fs=1.35, fh=0.08, order=(2, 0, 1, 3), flip=1), row(BOXES[1]), row(BOXES[2], jit=1, fh=-0.07, norm=0)]
    plan, post, buf, hw = _tables(plan, [post_row()] * 3, T.CANVASES)
    assert not post.any()
    rc, mean = T._gray(L, buf, hw, plan, S)
    assert rc == 0
    for form, dtype in ((NCHW, F32), (NHWC4, F32), (NHWC4, BF16)):
        rc, got = _apply_post(L, buf, hw, plan, post, mean, S, form, dtype)
        assert rc == 0
        rc, want = T._apply(L, buf, hw, plan, mean, S, form, dtype)
        assert rc == 0
        bits = np.uint16 if dtype == BF16 else np.uint32
        np.testing.assert_array_equal(got.view(bits), want.view(bits))


def test_bad_post_tables_are_refused_or_harmless():
    L = _bind()
    S = 8
    plan, good, buf, hw = _tables([row((0, 0, 8, 8))] * 3, [post_row(k=7), post_row(gray=1), post_row(k=3)], T.CANVASES)
    mean = np.zeros(3, np.float32)

    def rc_of(post, S=S, form=NCHW, dtype=F32):
        return _apply_post(L, buf, hw, plan, np.ascontiguousarray(post, np.float32), mean, S, form, dtype)[0]

    assert rc_of(good) == 0
    for col, v in ((0, 2.0), (1, 0.5), (0, np.nan), (1, -1.0)):          # a flag that is not 0 or 1
        bad = good.copy()
        bad[1, col] = v
        assert rc_of(bad) == -3, (col, v)
    for v in (np.nan, np.inf, -0.25):                                    # a weight that is not finite or is negative, on any row
        bad = good.copy()
        bad[1, 4] = v
        assert rc_of(bad, form=NHWC4, dtype=BF16) == -3, v
    bad = good.copy()
    bad[0, 2] += 0.0021                                                  # |sum - 1| > 1e-3 on a blurred row ...
    assert rc_of(bad) == -3
    near = good.copy()
    near[0, 2] += 0.0005
    assert rc_of(near) == 0
    off = good.copy()
    off[1, 2:6] = (0.9, 0.3, 0, 0)                                       # ... but not on a row without blur
    assert rc_of(off) == 0
    assert rc_of(good, S=3) == -3                                        # a blurred view below 4 pixels
    assert rc_of(np.stack([post_row(gray=1)] * 3), S=3) == 0
    out = np.zeros((3, 3, S, S), np.float32)
    assert L.clite_augment_apply_post(NCHW, F32, ptr(buf), ptr(hw), buf.shape[1], ptr(plan), None, ptr(mean), 3, S, ptr(out), 0, S, S,
                                      None, None, None, None) == -1      # a null table
    assert L.clite_augment_apply_post(NCHW, BF16, ptr(buf), ptr(hw), buf.shape[1], ptr(plan), ptr(good), ptr(mean), 3, S, ptr(out), 0, S, S,
                                      None, None, None, None) == -1
    over = plan.copy()
    over[1, 2] = 4 * S + 1                                               # the plan's own refusals come first
    assert _apply_post(L, buf, hw, over, good, mean, S, NCHW, F32)[0] == -4
    # without the mirror the refused tables run and stay inside their buffers (the simulator's buffers are exact: an overrun corrupts the
    # sentinels around the output or faults): blur on a 3-pixel view, weights that are no filter
    wild = good.copy()
    wild[0, 2:6] = (5.0, -1.0, 3.0, 0.5)
    for S_ in (3, 2, 1):
        rc, st = _apply_post(L, buf, hw, plan, wild, mean, S_, NHWC4, F32, host=False)
        assert rc == 0
        assert not np.isnan(st).any()
        assert not st[:, :3].any() and not st[:, :, :3].any() and not st[..., 3].any()
