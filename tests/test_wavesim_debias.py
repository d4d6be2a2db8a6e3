"""CPU-side (wave simulator) checks of the bias-evaluation kernels (csrc/debias_ops.hip) through the C ABI: the principal directions and the
streaming row pass against float64 (tests/debias_ref.py), bitwise-equal reruns, null outputs, and the refused arguments. Runs without a GPU.

Tolerances: 8 x the deviation from float64 of a float32 NumPy evaluation of the same formulas at the same inputs (debias_ref.pca_bars /
rows_bars), as in tests/test_gpu_debias.py, whose docstring records the measured values."""
import ctypes as C

import numpy as np
import pytest

import debias_ref as ref
from simlib import lib, ptr

_P, _I = C.c_void_p, C.c_int


def _bind():
    L = lib()
    L.clite_debias_pca.argtypes = [_P, _I, _I, _I, _P, _P, _P, _P, _P]
    L.clite_debias_rows.argtypes = [_P, _P, _I, _I, _I, _P, _P, _P, _P]
    return L


def _pca(L, d, R):
    P, D = d.shape
    lam, V = np.full(P, -7.0, np.float32), np.full((R, D), -7.0, np.float32)
    work, info = np.zeros(P * P, np.float32), np.full(2, -7, np.int32)
    assert L.clite_debias_pca(ptr(d), P, D, R, ptr(lam), ptr(V), ptr(work), ptr(info), None) == 0
    return lam, V, info


def _rows(L, x, V, want=(True, True, True)):
    N, D = x.shape
    R = V.shape[0]
    xn = np.full((N, D), -7.0, np.float32) if want[0] else None
    xd = np.full((N, D), -7.0, np.float32) if want[1] else None
    coef = np.full((N, R), -7.0, np.float32) if want[2] else None
    assert L.clite_debias_rows(ptr(x), ptr(V), N, D, R, ptr(xn), ptr(xd), ptr(coef), None) == 0
    return xn, xd, coef


@pytest.mark.parametrize("P,D,R", ref.PCA_SHAPES)
def test_directions_match_float64_and_repeat_bitwise(P, D, R):
    L = _bind()
    d = ref.pair_diffs(P, D)
    lam, V, info = _pca(L, d, R)
    assert info[0] == 0 and 0 <= info[1] <= 30
    bars, base = ref.pca_bars(d, R)
    got = ref.pca_errors(d, R, lam, V)
    print(f"projector / orthonormality / eigenvalue error: kernel {got}, float32 NumPy {base}, bars {bars}, sweeps {info[1]}")
    for g, b in zip(got, bars):
        assert g <= b
    assert got[1] <= ref.orthonormality_bar()                           # the Gram-Schmidt pass: orthonormal to rounding at every shape
    assert np.all(np.diff(lam) <= 0) and np.all(lam >= 0)
    np.testing.assert_array_equal(V, ref.sign_rule(V))
    lam2, V2, info2 = _pca(L, d, R)
    assert lam2.tobytes() == lam.tobytes() and V2.tobytes() == V.tobytes() and np.array_equal(info, info2)


def test_directions_of_rank_one_differences_flag_the_second_as_noise():
    """Every pair differs along one vector: the second eigenvalue is rounding noise, far below the 1e-4 that debias.directions accepts."""
    L = _bind()
    rng = np.random.default_rng(3)
    d = (rng.standard_normal((6, 1)) * rng.standard_normal((1, 64))).astype(np.float32)
    lam, V, info = _pca(L, d, 2)
    assert info[0] == 0
    assert lam[1] < 1e-4 * lam[0]
    want = d[0] / np.linalg.norm(d[0])
    assert abs(abs(float(V[0] @ want)) - 1) < 1e-5


def test_directions_of_differences_whose_squares_overflow_end_with_non_finite_eigenvalues():
    """Finite differences of magnitude 1e20: the f32 Gram matrix is infinite. The kernel stops at once, reports eigenvalues that are not
    finite (debias.directions raises on them) and indexes nothing out of range on the way."""
    L = _bind()
    d = np.full((3, 16), 1e20, np.float32) * np.arange(1, 4, dtype=np.float32)[:, None]
    lam, V, info = _pca(L, d, 2)
    assert info[1] == 0 and not np.isfinite(lam).any()


@pytest.mark.parametrize("N,D,R", ref.ROWS_SHAPES)
def test_rows_match_float64_and_repeat_bitwise(N, D, R):
    L = _bind()
    x, V, special = ref.rows_inputs(N, D, R)
    xn, xd, coef = _rows(L, x, V)
    bars, base = ref.rows_bars(x, V)
    got = ref.rows_errors(x, V, xn, xd, coef)
    print(f"xn / xd / coef error: kernel {got}, float32 NumPy {base}, bars {bars}")
    for g, b in zip(got, bars):
        assert g <= b
    bar = bars[1]
    keep = np.ones(N, bool)
    if "zero" in special:
        z = special["zero"]
        keep[z] = False
        assert not xn[z].any() and not xd[z].any() and not coef[z].any()
        o = special["orthogonal"]
        assert np.abs(xd[o] - xn[o]).max() <= bar
    assert np.abs(xd.astype(np.float64) @ V.astype(np.float64).T).max() <= bar * np.sqrt(D)
    for out in (xn, xd):
        assert np.abs(np.linalg.norm(out[keep].astype(np.float64), axis=1) - 1).max() <= bar * np.sqrt(D)
    # any output may be NULL; the others keep their bits. A row's result does not depend on the other rows, so the first and the last
    # (special) rows stand for a long bank here: the simulator runs one OS thread per lane.
    sub = np.unique(np.r_[np.arange(min(N, 5)), np.arange(max(N - 3, 0), N)])
    for want in [(a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)]:
        for got_, full in zip(_rows(L, np.ascontiguousarray(x[sub]), V, want), (xn, xd, coef)):
            assert got_ is None or got_.tobytes() == full[sub].tobytes()


@pytest.mark.parametrize("D,R", [(8, 1), (136, 2), (4096, 8)])
def test_row_equal_to_a_component_leaves_nothing(D, R):
    """Components without any rounding (Hadamard rows over a power of two): a multiple of a component has coef = |x| and y = 0 exactly, so xd
    is zero; a combination of components likewise."""
    L = _bind()
    V = ref.exact_components(R, D)
    x = np.stack([4.0 * V[R - 1], -0.5 * V[0], V.sum(0)]).astype(np.float32)
    xn, xd, coef = _rows(L, x, V)
    assert not xd.any()
    want = np.zeros((3, R), np.float32)
    want[0, R - 1], want[1, 0], want[2] = 4.0, -0.5, 1.0
    np.testing.assert_array_equal(coef, want)
    np.testing.assert_array_equal(np.abs(coef[:2]).sum(1), np.linalg.norm(x[:2].astype(np.float64), axis=1).astype(np.float32))
    np.testing.assert_allclose(xn[0], V[R - 1], atol=1e-7)


def test_bad_arguments_are_refused_and_write_nothing():
    L = _bind()
    d = ref.pair_diffs(3, 16)
    lam, V = np.full(3, -7.0, np.float32), np.full((2, 16), -7.0, np.float32)
    work, info = np.full(9, -7.0, np.float32), np.full(2, -7, np.int32)
    P = ptr

    def pca(a=d, P_=3, D=16, R=2, e=lam, c=V, w=work, i=info):
        return L.clite_debias_pca(P(a) if a is not None else None, P_, D, R, P(e), P(c), P(w), P(i), None)

    for kw in (dict(P_=0), dict(P_=65), dict(D=0), dict(D=12), dict(D=4104), dict(R=0), dict(R=4), dict(R=9), dict(a=None), dict(e=None),
               dict(c=None), dict(w=None), dict(i=None), dict(a=d.reshape(-1)[1:])):
        assert pca(**kw) != 0, kw
    assert np.all(lam == -7) and np.all(V == -7) and np.all(work == -7) and np.all(info == -7)
    assert pca() == 0 and info[0] == 0

    x = np.ones((2, 16), np.float32)
    comp = ref.exact_components(2, 16)
    outs = [np.full((2, 16), -7.0, np.float32), np.full((2, 16), -7.0, np.float32), np.full((2, 2), -7.0, np.float32)]

    def rows(a=x, c=comp, N=2, D=16, R=2, xn=outs[0], xd=outs[1], cf=outs[2]):
        return L.clite_debias_rows(P(a), P(c), N, D, R, P(xn), P(xd), P(cf), None)

    for kw in (dict(N=0), dict(D=0), dict(D=12), dict(D=4104), dict(R=0), dict(R=9), dict(a=None), dict(c=None),
               dict(a=x.reshape(-1)[1:]), dict(xn=outs[0].reshape(-1)[1:]), dict(xd=outs[1].reshape(-1)[1:])):
        assert rows(**kw) != 0, kw
    assert all(np.all(o == -7) for o in outs)
    assert rows(xn=None, xd=None, cf=None) == 0 and all(np.all(o == -7) for o in outs)          # nothing asked for: nothing launched
    assert rows() == 0 and not any(np.any(o == -7) for o in outs)
