"""CPU-side (wave simulator) checks of the k-means kernels (csrc/kmeans_ops.hip): the assignment against a NumPy f32 restatement of the same
formula (identical f32 scores in, so equality is exact, ties included), the changed-row counter, the squared distances, and accumulate /
update against float64 within the recursive-sum bound of tests/kmeans_ref.py, bit-identical across two runs and across both deterministic
settings. Shapes that fill no block, an unaligned base, bad arguments. Runs without a GPU."""
import ctypes as C

import numpy as np
import pytest

import kmeans_ref as R
from simlib import lib, ptr

_P, _I, _F, _U64 = C.c_void_p, C.c_int, C.c_float, C.c_uint64


def _bind():
    L = lib()
    L.clite_kmeans_row_norms.argtypes = [_P, _I, _I, _I, _F, _P, _P]
    L.clite_kmeans_assign.argtypes = [_P, _I, _P, _P, _I, _I, _P, _P, _P, _P]
    L.clite_kmeans_accumulate.argtypes = [_P, _I, _P, _P, _I, _I, _I, _P, _P, _P, _U64, _P]
    L.clite_kmeans_update.argtypes = [_P, _U64, _P, _I, _I, _I, _P, _I, _P, _P]
    L.clite_set_deterministic.argtypes = [_I]
    return L


def _work(N, D, K):
    from clip_lite_amd import hip
    nbytes = hip.kmeans_work_bytes(N, D, K)
    buf = np.zeros(nbytes // 4 + 4, np.float32)
    off = next(k for k in range(4) if buf[k:].ctypes.data % 16 == 0)
    w = buf[off:off + nbytes // 4]
    w.view(np.int32)[:] = -0x01010102            # poison: nothing may rely on a zeroed workspace
    return w, nbytes


def _want_assign(s, hc, K, xnorm=None):
    """The kernel's formula in NumPy f32: v = hc - s (one rounding), the first minimum among the values that are not NaN, else 0."""
    v = (hc[None, :K].astype(np.float32) - s[:, :K].astype(np.float32)).astype(np.float32)
    nan = np.isnan(v)
    a = np.argmin(np.where(nan, np.float32(np.inf), v), axis=1)
    first_ok = np.argmax(~nan, axis=1)
    all_inf = np.all(nan | np.isposinf(v), axis=1)            # +inf everywhere it is not NaN: the lowest k that is not NaN
    a = np.where(all_inf, first_ok, a)
    a = np.where(nan.all(axis=1), 0, a).astype(np.int32)
    if xnorm is None:
        return a, None
    best = v[np.arange(len(a)), a]
    d = (xnorm.astype(np.float32) + np.float32(2) * best).astype(np.float32)
    d = np.where(nan.all(axis=1), np.float32(0), np.maximum(d, np.float32(0))).astype(np.float32)
    return a, d


def _run_assign(L, s, lds_view, hc, N, K, prev, xnorm=None):
    a = prev.copy()
    dist = np.full(N, -7, np.float32) if xnorm is not None else None
    ch = np.array([5], np.int32)
    assert L.clite_kmeans_assign(ptr(s), lds_view, ptr(hc), ptr(xnorm), N, K, ptr(a), ptr(dist), ptr(ch), None) == 0
    return a, dist, int(ch[0]) - 5


def _padded(s, ld, fill):
    out = np.full((s.shape[0], ld), fill, np.float32)
    out[:, :s.shape[1]] = s
    return out


@pytest.mark.parametrize("N,K,ld", [(1, 2, 8), (37, 10, 16), (1000, 65, 72), (300, 2, 8), (77, 1024, 1024), (130, 257, 264), (64, 17, 24)])
def test_assign_random_scores(N, K, ld):
    L = _bind()
    rng = np.random.default_rng(N * 7 + K)
    if N < K:
        N = K
    s = rng.standard_normal((N, K)).astype(np.float32)
    hc = np.abs(rng.standard_normal(K)).astype(np.float32)
    xn = (np.abs(rng.standard_normal(N)) + 1).astype(np.float32)
    prev = rng.integers(0, K, N).astype(np.int32)
    want, wd = _want_assign(s, hc, K, xn)
    for fill in (1e30, -1e30):                      # padding columns are never compared
        a, d, ch = _run_assign(L, _padded(s, ld, fill), ld, hc, N, K, prev, xn)
        np.testing.assert_array_equal(a, want)
        np.testing.assert_array_equal(d, wd)
        assert ch == int(np.sum(prev != want))


@pytest.mark.parametrize("N,K,ld", [(200, 10, 16), (90, 65, 72), (40, 6, 8)])
def test_assign_ties_signed_zero_and_nan(N, K, ld):
    L = _bind()
    rng = np.random.default_rng(K)
    vals = np.array([-0.5, -0.0, 0.0, 0.25, 0.5], np.float32)
    s = vals[rng.integers(0, len(vals), (N, K))]
    hc = np.zeros(K, np.float32)
    hc[::2] = -0.0                                   # duplicated centroids: 0.0 - s and -0.0 - s tie
    s[3, :] = np.nan                                 # all NaN: 0
    s[4, :] = np.nan
    s[4, K - 1] = 1.0                                # one candidate, at the last k
    s[5, 0] = np.nan                                 # a NaN at k = 0 never wins
    s[6, :] = -np.inf                                # every value +inf: the lowest k
    s[6, 0] = np.nan
    prev = np.full(N, -1, np.int32)
    want, _ = _want_assign(s, hc, K)
    assert want[3] == 0 and want[4] == K - 1 and want[5] != 0 and want[6] == 1
    a, _, ch = _run_assign(L, _padded(s, ld, -9.0), ld, hc, N, K, prev)
    np.testing.assert_array_equal(a, want)
    assert ch == N
    a2, _, ch2 = _run_assign(L, _padded(s, ld, -9.0), ld, hc, N, K, a)
    np.testing.assert_array_equal(a2, want)
    assert ch2 == 0


def test_assign_scalar_path_on_unaligned_base():
    L = _bind()
    rng = np.random.default_rng(11)
    N, K, ld = 53, 21, 23                            # ld % 4 != 0 as well
    s = rng.standard_normal((N, K)).astype(np.float32)
    hc = rng.standard_normal(K).astype(np.float32)
    buf = np.zeros(N * ld + 4, np.float32)
    base = next(k for k in range(4) if buf[k:].ctypes.data % 16 != 0)
    view = buf[base:base + N * ld].reshape(N, ld)
    view[:] = _padded(s, ld, 1e30)
    want, _ = _want_assign(s, hc, K)
    a, _, _ = _run_assign(L, view, ld, hc, N, K, np.full(N, -1, np.int32))
    np.testing.assert_array_equal(a, want)


def _accumulate_update(L, X, ldx, assign, dist, N, D, K, C_old):
    work, nbytes = _work(N, D, K)
    counts = np.full(K, -3, np.int32)
    inertia = np.array([-1.0], np.float64)
    Cm = np.array(C_old, np.float32, copy=True)
    hc = np.full(K, -1, np.float32)
    assert L.clite_kmeans_accumulate(ptr(X), ldx, ptr(assign), ptr(dist), N, D, K, ptr(counts), ptr(inertia), ptr(work), nbytes, None) == 0
    assert L.clite_kmeans_update(ptr(work), nbytes, ptr(counts), N, D, K, ptr(Cm), D, ptr(hc), None) == 0
    return counts, float(inertia[0]), Cm, hc


def _check_centroids(X, assign, K, C_old, counts, Cm, hc):
    np.testing.assert_array_equal(counts, np.bincount(assign, minlength=K))
    want = R.means(X, assign, C_old)
    bound = R.centroid_bound(X, assign, K)
    err = np.abs(Cm.astype(np.float64) - want)
    assert np.all(err <= bound), float((err - bound).max())
    empty = counts == 0
    np.testing.assert_array_equal(Cm[empty], np.asarray(C_old, np.float32)[empty])          # an empty cluster keeps its centroid, bit for bit
    half = 0.5 * np.sum(Cm.astype(np.float64) ** 2, axis=1)
    np.testing.assert_allclose(hc, half, rtol=(R.gamma(X.shape[1]) + 2 * R.U), atol=0)


@pytest.mark.parametrize("N,D,K", [(2, 8, 2), (37, 96, 10), (1000, 768, 10), (1000, 96, 65), (700, 8, 65), (300, 1032, 3), (3000, 8, 1023), (3000, 8, 1024)])
def test_accumulate_update_against_float64_and_bitwise_repeatable(N, D, K):
    L = _bind()
    rng = np.random.default_rng(N + D + K)
    X = rng.standard_normal((N, D)).astype(np.float32)
    assign = rng.integers(0, K, N).astype(np.int32)
    assign[:K] = np.arange(K)
    if K > 3:
        assign[assign == 2] = 1                      # an empty cluster
    if N >= 600:
        assign[100:500] = 0                          # one cluster of several chunks
    dist = np.abs(rng.standard_normal(N)).astype(np.float32)
    C_old = rng.standard_normal((K, D)).astype(np.float32)
    runs = []
    for det in (0, 1, 0):
        L.clite_set_deterministic(det)
        runs.append(_accumulate_update(L, X, D, assign, dist, N, D, K, C_old))
    L.clite_set_deterministic(0)
    counts, inertia, Cm, hc = runs[0]
    _check_centroids(X, assign, K, C_old, counts, Cm, hc)
    assert abs(inertia - float(dist.astype(np.float64).sum())) <= R.gamma(256) * float(dist.sum())
    for other in runs[1:]:
        np.testing.assert_array_equal(other[0], counts)
        assert other[1] == inertia
        assert other[2].tobytes() == Cm.tobytes() and other[3].tobytes() == hc.tobytes()


def test_accumulate_strided_and_unaligned_rows():
    """a row stride above D, and a base that is not 16-byte aligned (scalar path): the same bits as the aligned, dense copy"""
    L = _bind()
    rng = np.random.default_rng(5)
    N, D, K, ld = 150, 24, 7, 29
    X = rng.standard_normal((N, D)).astype(np.float32)
    assign = rng.integers(0, K, N).astype(np.int32)
    C_old = np.zeros((K, D), np.float32)
    ref = _accumulate_update(L, X, D, assign, None, N, D, K, C_old)
    buf = np.zeros(N * ld + 4, np.float32)
    base = next(k for k in range(4) if buf[k:].ctypes.data % 16 != 0)
    view = buf[base:base + N * ld].reshape(N, ld)
    view[:, :D] = X
    view[:, D:] = 1e30
    got = _accumulate_update(L, view, ld, assign, None, N, D, K, C_old)
    assert got[2].tobytes() == ref[2].tobytes() and got[3].tobytes() == ref[3].tobytes()
    _check_centroids(X, assign, K, C_old, got[0], got[2], got[3])
    xn = np.zeros(N, np.float32)
    assert L.clite_kmeans_row_norms(ptr(view), ld, N, D, 0.5, ptr(xn), None) == 0
    np.testing.assert_allclose(xn, 0.5 * np.sum(X.astype(np.float64) ** 2, axis=1), rtol=R.gamma(D) + 2 * R.U)


def test_one_lloyd_step_matches_reference_on_separated_blobs():
    """scores from NumPy f32 -> assign -> accumulate -> update: the float64 step's labels (no row under tau_n here) and its centroids"""
    L = _bind()
    N, D, K = 600, 96, 5
    X, _ = R.blobs(N, D, K, 1.0, seed=2)
    C0 = X[R.init_rows(N, K, seed=3)]
    a64, d64, gap = R.assign_step(X, C0)
    share = float(np.mean(R.exempt_rows(X, C0, gap)))
    print(f"rows under tau_n: {100 * share:.3f} %")
    assert share <= R.EXEMPT_CAP
    s = (X @ C0.T).astype(np.float32)
    hc = np.zeros(K, np.float32)
    xn = np.zeros(N, np.float32)
    assert L.clite_kmeans_row_norms(ptr(C0), D, K, D, 0.5, ptr(hc), None) == 0
    assert L.clite_kmeans_row_norms(ptr(X), D, N, D, 1.0, ptr(xn), None) == 0
    a, dist, ch = _run_assign(L, _padded(s, 8, 0.0), 8, hc, N, K, np.full(N, -1, np.int32), xn)
    keep = ~R.exempt_rows(X, C0, gap)
    np.testing.assert_array_equal(a[keep], a64[keep])
    np.testing.assert_allclose(dist, d64, rtol=0, atol=8 * R.gamma(D))      # unit rows: gamma_D (|x|^2 + 2 (|x| |c| + |c|^2)) plus the final roundings
    counts, inertia, Cm, hc2 = _accumulate_update(L, X, D, a, dist, N, D, K, C0)
    _check_centroids(X, a, K, C0, counts, Cm, hc2)


def test_bad_arguments_are_refused():
    L = _bind()
    N, D, K = 16, 8, 4
    X = np.zeros((N, D), np.float32)
    s = np.zeros((N, 8), np.float32)
    hc = np.zeros(K, np.float32)
    a = np.zeros(N, np.int32)
    ch = np.zeros(1, np.int32)
    cnt = np.zeros(K, np.int32)
    work, nbytes = _work(N, D, K)
    Cm = np.zeros((K, D), np.float32)
    assert L.clite_kmeans_assign(None, 8, ptr(hc), None, N, K, ptr(a), None, ptr(ch), None) != 0
    assert L.clite_kmeans_assign(ptr(s), 3, ptr(hc), None, N, K, ptr(a), None, ptr(ch), None) != 0           # lds < K
    assert L.clite_kmeans_assign(ptr(s), 8, ptr(hc), None, N, 1, ptr(a), None, ptr(ch), None) != 0           # K < 2
    assert L.clite_kmeans_assign(ptr(s), 8, ptr(hc), None, 3, K, ptr(a), None, ptr(ch), None) != 0           # N < K
    assert L.clite_kmeans_assign(ptr(s), 8, ptr(hc), None, N, K, ptr(a), ptr(hc), ptr(ch), None) != 0        # dist without xnorm
    assert L.clite_kmeans_row_norms(ptr(X), 4, N, D, 1.0, ptr(hc), None) != 0                                 # ld < D
    assert L.clite_kmeans_row_norms(ptr(X), 12, N, 12, 1.0, ptr(hc), None) != 0                               # D % 8
    assert L.clite_kmeans_accumulate(ptr(X), 4, ptr(a), None, N, D, K, ptr(cnt), None, ptr(work), nbytes, None) != 0      # ld < D
    assert L.clite_kmeans_accumulate(ptr(X), D, ptr(a), None, N, D, 1, ptr(cnt), None, ptr(work), nbytes, None) != 0      # K < 2
    assert L.clite_kmeans_accumulate(ptr(X), D, ptr(a), None, 3, D, K, ptr(cnt), None, ptr(work), nbytes, None) != 0      # N < K
    assert L.clite_kmeans_accumulate(ptr(X), D, ptr(a), None, N, D, 1025, ptr(cnt), None, ptr(work), nbytes, None) != 0   # K > 1024
    assert L.clite_kmeans_accumulate(ptr(X), D, None, None, N, D, K, ptr(cnt), None, ptr(work), nbytes, None) != 0
    assert L.clite_kmeans_accumulate(ptr(X), D, ptr(a), None, N, D, K, ptr(cnt), None, ptr(work), nbytes - 4, None) != 0  # workspace too small
    assert L.clite_kmeans_update(ptr(work), nbytes, ptr(cnt), N, D, K, None, D, ptr(hc), None) != 0
    assert L.clite_kmeans_update(ptr(work), nbytes, ptr(cnt), N, D, K, ptr(Cm), 4, ptr(hc), None) != 0       # ldc < D


def test_workspace_formula_matches_header():
    """hip.kmeans_work_bytes == CLITE_KMEANS_WORK_BYTES as the C compiler evaluates it; under 1 GiB at COCO scale with K = 1024"""
    import os
    import subprocess
    import tempfile
    from clip_lite_amd import hip
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cases = [(118287, 768, 1024), (118287, 768, 10), (37, 96, 10), (2, 8, 2), (1000, 768, 65)]
    body = "".join(f'  printf("%llu\\n", (unsigned long long)CLITE_KMEANS_WORK_BYTES({n}, {d}, {k}));\n' for n, d, k in cases)
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "w.c")
        open(src, "w").write('#include <stdio.h>\n#include "clite.h"\nint main(void) {\n' + body + "  return 0;\n}\n")
        subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), src, "-o", os.path.join(tmp, "w")])
        got = [int(x) for x in subprocess.check_output([os.path.join(tmp, "w")], text=True).split()]
    assert got == [hip.kmeans_work_bytes(*c) for c in cases]
    assert got[0] < 1 << 30
