"""CPU-side (wave simulator) checks of the classification kernels (csrc/cls_ops.hip: clite_xent_fwd / clite_xent_bwd) against a float64
numpy evaluation of nn.CrossEntropyLoss (ignore_index -100, mean over the counted rows) and TopkAccuracy. Runs without a GPU."""
import ctypes as C

import numpy as np
import pytest

from loss_ref import MASKED_ROW, xent_reference as _reference
from simlib import lib, outbuf, ptr, val

BF16, F32 = 0, 1


def _bind():
    L = lib()
    L.clite_xent_fwd.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.clite_xent_bwd.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_int, C.c_void_p]
    return L


def _run(L, z, ld, y, topk, Bp, ldd, dtype, gout=0.7):
    B, Cc = z.shape
    zb = np.zeros((B, ld), np.float32)
    zb[:, :Cc] = z
    zb[:, Cc:] = 1e4                    # padding columns must not enter any sum
    lse = np.zeros(B, np.float32)
    acc = np.zeros(4, np.float32)
    lab = np.ascontiguousarray(y, np.int64)
    assert L.clite_xent_fwd(ptr(zb), ld, B, Cc, ptr(lab), topk, ptr(lse), ptr(acc), None) == 0
    g = np.array([gout], np.float32)
    dz = outbuf((Bp, ldd), dtype)
    dz[:] = 0x3F80 if dtype == BF16 else 1.0          # poison: every element must be written
    # the kernel reads rows < B of the logits only: give it exactly B rows
    assert L.clite_xent_bwd(dtype, ptr(zb), ld, B, Bp, Cc, ptr(lse), ptr(lab), ptr(acc), ptr(g), ptr(dz), ldd, None) == 0
    return lse, acc, val(dz, dtype)


CASES = [(2, 64), (10, 7), (10, 1), (1000, 7), (1000, 1), (8142, 1), (8142, 7), (37, 64)]


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("Cc,B", CASES)
def test_xent_matches_float64(Cc, B, dtype):
    L = _bind()
    rng = np.random.default_rng(Cc * 100 + B)
    z = (rng.standard_normal((B, Cc)) * 3).astype(np.float32)
    y = rng.integers(0, Cc, B)
    if B >= 7:
        y[3] = -100                     # ignored rows: no loss, no count, zero gradient
    ld = (Cc + 3) // 4 * 4 + 4          # ld > C
    ldd = (Cc + 7) // 8 * 8
    Bp = (B + 7) // 8 * 8 + 8           # Bp > B
    topk = 5
    lse, acc, dz = _run(L, z, ld, y, topk, Bp, ldd, dtype)
    rl, rloss, rt1, rtk, rn, rd = _reference(z, y, topk)
    assert np.abs(lse - rl).max() < 1e-4 * max(1.0, np.abs(rl).max())
    assert acc[3] == rn and acc[1] == rt1 and acc[2] == rtk
    assert abs(acc[0] - rloss) < 1e-5 * max(1.0, abs(rloss))
    got = dz[:B, :Cc]
    tol = 1e-2 if dtype == BF16 else 1e-5
    assert np.abs(got - 0.7 * rd).max() <= tol * max(np.abs(0.7 * rd).max(), 1e-6)
    assert not dz[B:].any()             # padding rows
    assert not dz[:, Cc:].any()         # padding columns
    if B >= 7:
        assert not dz[3].any()          # ignored row


def test_xent_tie_goes_to_lower_index_and_topk_counts():
    L = _bind()
    z = np.zeros((3, 10), np.float32)
    z[0, [2, 5]] = 4.0                  # label 5 ties with class 2: rank 1 (not top-1), inside top-2
    z[1, [2, 5]] = 4.0                  # label 2 ties with class 5: rank 0
    z[2] = np.arange(10, dtype=np.float32)  # label 7: two classes above it
    y = np.array([5, 2, 7])
    lse, acc, _ = _run(L, z, 12, y, 2, 8, 16, F32)
    assert acc[1] == 1 and acc[2] == 2 and acc[3] == 3
    lse, acc, _ = _run(L, z, 12, y, 3, 8, 16, F32)
    assert acc[1] == 1 and acc[2] == 3


def test_xent_all_ignored_gives_zero_gradient():
    L = _bind()
    z = np.random.default_rng(1).standard_normal((4, 10)).astype(np.float32)
    lse, acc, dz = _run(L, z, 12, np.full(4, -100), 1, 8, 16, F32)
    assert acc[3] == 0 and acc[0] == 0 and not dz.any()


def test_xent_rejects_bad_shapes():
    L = _bind()
    z = np.zeros((2, 12), np.float32)
    lab = np.zeros(2, np.int64)
    lse, acc = np.zeros(2, np.float32), np.zeros(4, np.float32)
    assert L.clite_xent_fwd(ptr(z), 10, 2, 10, ptr(lab), 1, ptr(lse), ptr(acc), None) == -1      # ld % 4
    assert L.clite_xent_fwd(ptr(z), 12, 2, 13, ptr(lab), 1, ptr(lse), ptr(acc), None) == -1      # C > ld
    g, dz = np.ones(1, np.float32), np.zeros((2, 12), np.float32)
    assert L.clite_xent_bwd(F32, ptr(z), 12, 2, 2, 10, ptr(lse), ptr(lab), ptr(acc), ptr(g), ptr(dz), 12, None) == -1   # ldd % 8
    assert L.clite_xent_bwd(F32, ptr(z), 12, 2, 1, 10, ptr(lse), ptr(lab), ptr(acc), ptr(g), ptr(dz), 16, None) == -1   # Bp < B


def test_xent_deterministic_mode_repeats_bitwise():
    L = _bind()
    rng = np.random.default_rng(7)
    B, Cc = 64, 1000
    z = (rng.standard_normal((B, Cc)) * 5).astype(np.float32)
    y = rng.integers(0, Cc, B)
    L.clite_set_deterministic(1)
    try:
        runs = [_run(L, z, 1000, y, 5, 64, 1000, F32) for _ in range(2)]
    finally:
        L.clite_set_deterministic(0)
    for a, b in zip(runs[0], runs[1]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    rl, rloss, _, _, rn, _ = _reference(z, y, 5)
    assert runs[0][1][3] == rn and abs(runs[0][1][0] - rloss) < 1e-5 * rloss


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_xent_masked_classes_contribute_nothing(dtype):
    """nn.CrossEntropyLoss with a class at -inf that is not the label: a finite loss, nothing from that class, gradient exactly 0 there. The first
    row starts a lane with -inf before any finite value; the others have one behind finite values, in other lanes' first columns, in a second
    trip of the column loop, and in every class but the label."""
    L = _bind()
    z, y, want = MASKED_ROW
    lse, acc, dz = _run(L, z, 8, y, 1, 8, 8, dtype)
    assert abs(lse[0] - want) < 1e-5 and abs(acc[0] - (want - 2.0)) < 1e-5 and acc[1] == 0 and acc[3] == 1
    rng = np.random.default_rng(5)
    B, Cc = 6, 1030
    z = (rng.standard_normal((B, Cc)) * 3).astype(np.float32)
    y = np.array([0, 5, 1029, 300, 7, 4])
    z[0, 1] = -np.inf                       # behind a finite value in lane 0
    z[1, 0:1024:4] = -np.inf                # the first column of every lane's every chunk
    z[2, 1024:1029] = -np.inf               # lanes 0 and 1 in the second trip of the 1024-column loop
    z[3, :300] = z[3, 301:] = -np.inf       # every class but the label
    z[4, rng.choice(np.setdiff1d(np.arange(Cc), [7]), 400, replace=False)] = -np.inf
    lse, acc, dz = _run(L, z, 1032, y, 5, 16, 1032, dtype)
    rl, rloss, rt1, rtk, rn, rd = _reference(z, y, 5)
    assert np.isfinite(lse).all() and np.abs(lse - rl).max() < 1e-4 * max(1.0, np.abs(rl).max())
    assert acc[3] == rn and acc[1] == rt1 and acc[2] == rtk
    assert abs(acc[0] - rloss) < 1e-5 * max(1.0, abs(rloss))
    got = dz[:B, :Cc]
    tol = 1e-2 if dtype == BF16 else 1e-5
    assert np.abs(got - 0.7 * rd).max() <= tol * np.abs(0.7 * rd).max()
    assert not got[np.isneginf(z)].any()
    assert not dz[B:].any() and not dz[:, Cc:].any()
