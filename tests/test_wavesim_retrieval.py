"""CPU-side (wave simulator) checks of the retrieval rank kernels (csrc/retrieval_ops.hip) against the ranks of itm_eval's stable argsorts:
random scores, heavy ties (0.0 and -0.0 included), unsorted and scattered caption lists, an image without captions, padding columns that
must be ignored, and shapes that fill no block evenly, on both the 16-byte vector path and the scalar path. Runs without a GPU."""
import ctypes as C

import numpy as np
import pytest

from simlib import lib, ptr

_P, _I = C.c_void_p, C.c_int


def _bind():
    L = lib()
    L.clite_retrieval_rank_i2t.argtypes = [_P, _I, _I, _I, _P, _P, _P, _P]
    L.clite_retrieval_rank_t2i.argtypes = [_P, _I, _I, _I, _P, _P, _P, _P]
    return L


def _want(s, img2txt, txt2img):
    """ranks from np.argsort(-s, kind="stable") as itm_eval forms them; Nt for an image without captions"""
    from clip_lite_amd.retrieval import host_ranks
    return host_ranks(s, img2txt, txt2img)


def _layout(rng, Ni, Nt, empty=()):
    """caption lists: every caption belongs to one image; lists come out unsorted and non-contiguous"""
    owners = rng.integers(0, Ni, Nt)
    for r in empty:
        owners[owners == r] = (r + 1) % Ni
    img2txt = [list(rng.permutation(np.flatnonzero(owners == i))) for i in range(Ni)]
    return img2txt, [int(o) for o in owners]


def _run(L, s_full, Nt, img2txt, txt2img):
    Ni, ld = s_full.shape
    off = np.zeros(Ni + 1, np.int32)
    off[1:] = np.cumsum([len(c) for c in img2txt])
    idx = np.array([t for c in img2txt for t in c] or [0], np.int32)
    t2i = np.array(txt2img, np.int32)
    r_i = np.full(Ni, -7, np.int32)
    r_t = np.full(Nt, -7, np.int32)
    work = np.full(((Ni + 127) // 128, Nt), -7, np.int32)            # CLITE_RETRIEVAL_T2I_ROWS = 128; every entry is written
    assert L.clite_retrieval_rank_i2t(ptr(s_full), ld, Ni, Nt, ptr(off), ptr(idx), ptr(r_i), None) == 0
    assert L.clite_retrieval_rank_t2i(ptr(s_full), ld, Ni, Nt, ptr(t2i), ptr(r_t), ptr(work), None) == 0
    return r_i, r_t


def _padded(s, ld, fill=1e30):
    out = np.full((s.shape[0], ld), fill, np.float32)
    out[:, :s.shape[1]] = s
    return out


@pytest.mark.parametrize("Ni,Nt,ld", [(37, 181, 184), (5, 23, 23), (70, 61, 64), (131, 300, 301), (3, 8400, 8408)])
def test_random_scores(Ni, Nt, ld):
    L = _bind()
    rng = np.random.default_rng(Ni * 1000 + Nt)
    s = rng.standard_normal((Ni, Nt)).astype(np.float32)
    img2txt, txt2img = _layout(rng, Ni, Nt)
    for t, i in enumerate(txt2img):          # positives likely near the top, not certain
        s[i, t] += 1.5
    got = _run(L, _padded(s, ld), Nt, img2txt, txt2img)
    want = _want(s, img2txt, txt2img)
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])


@pytest.mark.parametrize("Ni,Nt,ld", [(41, 203, 208), (9, 50, 51), (140, 37, 40)])
def test_heavy_ties_and_signed_zero(Ni, Nt, ld):
    L = _bind()
    rng = np.random.default_rng(Nt)
    vals = np.array([-0.5, -0.0, 0.0, 0.25, 0.5, 1.0], np.float32)
    s = vals[rng.integers(0, len(vals), (Ni, Nt))]
    img2txt, txt2img = _layout(rng, Ni, Nt, empty=(3,))
    assert img2txt[3] == []
    got = _run(L, _padded(s, ld), Nt, img2txt, txt2img)
    want = _want(s, img2txt, txt2img)
    assert got[0][3] == Nt                   # no captions: a miss at every k
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])


def test_padding_columns_are_never_read():
    """similarity()'s padding columns score 0 and would outrank every negative score; here they hold +1e30 and must change nothing"""
    L = _bind()
    rng = np.random.default_rng(3)
    Ni, Nt, ld = 12, 45, 48
    s = -np.abs(rng.standard_normal((Ni, Nt))).astype(np.float32)
    img2txt, txt2img = _layout(rng, Ni, Nt)
    want = _want(s, img2txt, txt2img)
    for fill in (1e30, 0.0):
        got = _run(L, _padded(s, ld, fill), Nt, img2txt, txt2img)
        np.testing.assert_array_equal(got[0], want[0])
        np.testing.assert_array_equal(got[1], want[1])


def test_scalar_path_on_unaligned_base():
    """a base that is not 16-byte aligned takes the scalar loads"""
    L = _bind()
    rng = np.random.default_rng(4)
    Ni, Nt, ld = 19, 33, 36
    s = rng.standard_normal((Ni, Nt)).astype(np.float32)
    img2txt, txt2img = _layout(rng, Ni, Nt)
    buf = np.zeros(Ni * ld + 4, np.float32)
    base = next(k for k in range(4) if (buf[k:].ctypes.data % 16) != 0)
    view = buf[base:base + Ni * ld].reshape(Ni, ld)
    view[:] = _padded(s, ld)
    got = _run(L, view, Nt, img2txt, txt2img)
    want = _want(s, img2txt, txt2img)
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])


def test_bad_arguments_are_refused():
    L = _bind()
    s = np.zeros((2, 8), np.float32)
    off = np.array([0, 1, 2], np.int32)
    idx = np.array([0, 1], np.int32)
    r = np.zeros(8, np.int32)
    assert L.clite_retrieval_rank_i2t(ptr(s), 4, 2, 8, ptr(off), ptr(idx), ptr(r), None) != 0       # ld < Nt
    w = np.zeros(8, np.int32)
    assert L.clite_retrieval_rank_t2i(ptr(s), 8, 0, 8, ptr(idx), ptr(r), ptr(w), None) != 0         # no rows
    assert L.clite_retrieval_rank_t2i(None, 8, 2, 8, ptr(idx), ptr(r), ptr(w), None) != 0
    assert L.clite_retrieval_rank_t2i(ptr(s), 8, 2, 8, ptr(idx), ptr(r), None, None) != 0            # no workspace
