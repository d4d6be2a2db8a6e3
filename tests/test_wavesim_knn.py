"""CPU-side (wave simulator) checks of the k-NN kernels (csrc/knn_ops.hip) through the C ABI: the streaming top-k selection against the stable
argsort (heavy ties, every chunking, padded tiles, signed zeros), the weighted vote against float64, and the refused arguments. Runs without a
GPU."""
import ctypes as C

import numpy as np
import pytest

import knn_ref
from simlib import lib, ptr

_P, _I, _F = C.c_void_p, C.c_int, C.c_float


def _bind():
    L = lib()
    L.clite_knn_topk_merge.argtypes = [_P, _I, _I, _I, _I, _I, _I, _P, _P, _P]
    L.clite_knn_vote.argtypes = [_P, _P, _P, _I, _I, _I, _I, _P, _I, _F, _P, _P, _P]
    return L


def _merge(L):
    def merge(tile, lds, Q, Nc, base, K, have, top_s, top_i):
        assert L.clite_knn_topk_merge(ptr(tile), lds, Q, Nc, base, K, have, ptr(top_s), ptr(top_i), None) == 0
    return merge


def _check_all_feeds(s, K, chunks):
    merge = _merge(_bind())
    want_s, want_i = knn_ref.topk_ref(s, K)
    N = s.shape[1]
    feeds = [(N, 0), (N, 5), (N, 4 + (-N) % 4)] + [(c, 0) for c in chunks]      # one chunk: tight, scalar path with padding, vector path with padding
    for chunk, pad in feeds:
        got_s, got_i = knn_ref.feed(merge, s, K, chunk, pad)
        np.testing.assert_array_equal(got_i, want_i, err_msg=f"chunk {chunk} pad {pad}")
        np.testing.assert_array_equal(got_s, want_s, err_msg=f"chunk {chunk} pad {pad}")


@pytest.mark.parametrize("Q,N,K", knn_ref.SELECTION_SHAPES)
def test_selection_is_the_stable_argsort_under_every_chunking(Q, N, K):
    s = knn_ref.tie_scores(Q, N)
    assert np.all(s == np.round(s)) and np.abs(s).max() < 129
    if N >= 700:
        assert 30 <= len(np.unique(s[0])) <= 90          # ties everywhere
    _check_all_feeds(s, K, (64, 100, 1))


def test_selection_treats_signed_zeros_as_equal():
    rng = np.random.default_rng(5)
    vals = np.array([-0.5, -0.0, 0.0, 0.25, -0.0, 0.0], np.float32)
    s = vals[rng.integers(0, len(vals), (2, 300))]
    assert np.signbit(s[0][s[0] == 0]).any() and not np.signbit(s[0][s[0] == 0]).all()
    merge = _merge(_bind())
    want_s, want_i = knn_ref.topk_ref(s, 200)
    for chunk in (300, 64, 7):
        got_s, got_i = knn_ref.feed(merge, s, 200, chunk)
        np.testing.assert_array_equal(got_i, want_i)
        np.testing.assert_array_equal(got_s, want_s)


def test_selection_when_every_element_improves_the_list():
    """An ascending row: every element beats the threshold, so the candidate area overflows in every batch."""
    s = np.arange(3000, dtype=np.float32)[None, :].repeat(2, 0)
    s[1] = -s[1]
    merge = _merge(_bind())
    want_s, want_i = knn_ref.topk_ref(s, 200)
    for chunk in (3000, 1024):
        got_s, got_i = knn_ref.feed(merge, s, 200, chunk)
        np.testing.assert_array_equal(got_i, want_i)
        np.testing.assert_array_equal(got_s, want_s)


def test_selection_passes_over_nan_scores_and_marks_the_entries_it_cannot_fill():
    """A NaN is never selected. A row with fewer other scores than the list asks for ends in entries of score -inf and index INT32_MAX, which
    a later chunk's scores replace: the lists equal the stable argsort of the row without its NaNs."""
    merge = _merge(_bind())
    rng = np.random.default_rng(9)
    s = knn_ref.tie_scores(2, 300)
    s[0, rng.permutation(300)[:150]] = np.nan            # row 0: 150 scores left for a list of 200
    s[1, rng.permutation(300)[:20]] = np.nan
    s[0, :40] = np.nan                                   # and its first chunk of 40 holds nothing at all
    for chunk in (300, 40, 7):
        got_s, got_i = knn_ref.feed(merge, s, 200, chunk)
        for q in range(2):
            keep = np.flatnonzero(~np.isnan(s[q]))
            want_s, want_i = knn_ref.topk_ref(s[q, keep][None, :], 200)
            n = want_i.shape[1]
            np.testing.assert_array_equal(got_i[q, :n], keep[want_i[0]])
            np.testing.assert_array_equal(got_s[q, :n], want_s[0])
            assert np.all(got_i[q, n:] == 2**31 - 1) and np.all(np.isneginf(got_s[q, n:]))


def _vote(L, top_s, top_i, labels, C_, ks, inv_T, with_scores=True):
    Q, K = top_s.shape
    pred = np.full((len(ks), Q, 5), -7, np.int32)
    cs = np.full((len(ks), Q, C_), -7.0, np.float32) if with_scores else None
    kv = np.array(ks, np.int32)
    assert L.clite_knn_vote(ptr(top_s), ptr(top_i), ptr(labels), Q, K, len(labels), C_, ptr(kv), len(ks), inv_T, ptr(cs), ptr(pred), None) == 0
    return cs, pred


# seeds chosen so that the float64 scores alone leave no (k, query) pair with two of its six best classes within 1e-4 relative
@pytest.mark.parametrize("Q,K,N,C_,seed", [(4, 200, 700, 10, 0), (3, 20, 50, 3, 0), (2, 256, 300, 1000, 0)])
def test_vote_matches_float64(Q, K, N, C_, seed):
    L = _bind()
    top_s, top_i, labels = knn_ref.vote_inputs(seed, Q, K, N, C_)
    ks = sorted({min(k, K) for k in (1, 10, 20, 200)})
    inv_T = float(np.float32(1 / 0.07))
    want, want_pred = knn_ref.vote_ref(top_s, top_i, labels, C_, ks, inv_T)
    got, pred = _vote(L, top_s, top_i, labels, C_, ks, inv_T)
    # f32 sums of at most 256 terms in (0, 1]: 1e-5 relative
    err = np.abs(got - want) / np.maximum(want, 1e-300)
    print(f"class score error vs float64: {err[want > 0].max():.2e}")
    assert np.all(got[want == 0] == 0) and err[want > 0].max() <= 1e-5
    ok = knn_ref.separated(want, 1e-4)
    print(f"excluded (k, query) pairs: {(~ok).sum()} of {ok.size}")
    assert (~ok).mean() <= 0.02
    np.testing.assert_array_equal(pred[ok], want_pred[ok])
    if C_ < 5:
        assert np.all(pred[:, :, C_:] == -1) and np.all(pred[:, :, :C_] >= 0)
    _, pred2 = _vote(L, top_s, top_i, labels, C_, ks, inv_T, with_scores=False)      # class_scores may be NULL
    np.testing.assert_array_equal(pred2, pred)


def test_vote_breaks_equal_scores_by_class():
    """Two neighbours of equal similarity vote for classes 7 and 2: equal scores, the lower class first; unvoted classes follow by class."""
    L = _bind()
    top_s = np.array([[0.5, 0.5, 0.25, 0.25]], np.float32)
    top_i = np.array([[3, 0, 1, 2]], np.int32)
    labels = np.array([2, 9, 4, 7], np.int32)            # ranks vote 7, 2, 9, 4
    got, pred = _vote(L, top_s, top_i, labels, 12, [2, 4], 4.0)
    np.testing.assert_array_equal(pred[0, 0], [2, 7, 0, 1, 3])
    np.testing.assert_array_equal(pred[1, 0], [2, 7, 4, 9, 0])
    assert got[1, 0, 2] == got[1, 0, 7] == 1.0 and got[1, 0, 4] == got[1, 0, 9] == pytest.approx(np.exp(-1.0), rel=1e-6)


def test_vote_skips_entries_outside_the_bank_or_the_classes():
    L = _bind()
    top_s = np.array([[0.9, 0.8, 0.7, 0.6]], np.float32)
    top_i = np.array([[1, 99, -1, 0]], np.int32)         # 99 and -1 are outside the bank of 3 rows
    labels = np.array([1, 0, 5], np.int32)
    got, pred = _vote(L, top_s, top_i, labels, 3, [4], 1.0)
    assert got[0, 0, 0] == 1.0 and got[0, 0, 2] == 0.0 and got[0, 0, 1] == pytest.approx(np.exp(float(np.float32(0.6) - np.float32(0.9))), rel=1e-6)
    np.testing.assert_array_equal(pred[0, 0], [0, 1, 2, -1, -1])


def test_bad_arguments_are_refused_and_write_nothing():
    L = _bind()
    s = np.zeros((2, 8), np.float32)
    ts, ti = np.full((2, 300), -7.0, np.float32), np.full((2, 300), -7, np.int32)
    P = ptr

    def merge(scores=s, lds=8, Q=2, Nc=8, base=0, K=4, have=0, a=ts, b=ti):
        return L.clite_knn_topk_merge(P(scores), lds, Q, Nc, base, K, have, P(a), P(b), None)

    for kw in (dict(K=257), dict(K=0), dict(have=5), dict(have=-1), dict(Nc=0), dict(Nc=-3), dict(lds=7), dict(scores=None), dict(a=None),
               dict(b=None), dict(base=2**31 - 8), dict(base=-1), dict(Q=0)):
        assert merge(**kw) != 0, kw
    assert np.all(ts == -7) and np.all(ti == -7)
    assert merge(base=2**31 - 9) == 0                    # base + Nc == INT32_MAX is the last one accepted
    assert ti[0, 0] == 2**31 - 9

    top_s, top_i, labels = knn_ref.vote_inputs(0, 2, 8, 20, 4)
    pred, cs, ks = np.full((2, 2, 5), -7, np.int32), np.full((2, 2, 4), -7.0, np.float32), np.array([1, 8], np.int32)

    def vote(a=top_s, b=top_i, lab=labels, Q=2, K=8, N=20, C_=4, kv=ks, nk=2, inv_T=1.0, c=cs, pr=pred):
        return L.clite_knn_vote(P(a), P(b), P(lab), Q, K, N, C_, P(kv), nk, inv_T, P(c), P(pr), None)

    for kw in (dict(C_=16385), dict(C_=0), dict(K=257), dict(K=0), dict(nk=9), dict(nk=0), dict(kv=np.array([8, 1], np.int32)),
               dict(kv=np.array([1, 9], np.int32)), dict(kv=np.array([0, 8], np.int32)), dict(kv=np.array([4, 4], np.int32)), dict(kv=None),
               dict(a=None), dict(b=None), dict(lab=None), dict(pr=None), dict(Q=0), dict(N=0), dict(inv_T=float("nan")), dict(inv_T=-1.0)):
        assert vote(**kw) != 0, kw
    assert np.all(pred == -7) and np.all(cs == -7)
    assert vote() == 0 and np.all(pred[:, :, :4] >= 0)
