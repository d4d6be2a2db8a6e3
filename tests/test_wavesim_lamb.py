"""The LAMB kernels (csrc/update_ops.hip: clite_lamb_moments, clite_lamb_step) on the wave simulator, with the checks of tests/test_gpu_lamb_ops.py
(tests/lamb_ref.py: the hand-made item table, the float64 reference, the bounds). Runs without a GPU.

Measured on the simulator (`pytest -s`, LAMBERR lines; maxima over the file's cases; no figure feeds a bound):
  norms     error / max(1, sum of terms): sum p^2 6.1e-08, sum r^2 2.0e-07 (both the 4-element tensor)                (bound 1e-5)
  moments   max error / bound: m 0.011 (2.2e-10 against 2.0e-08)   v2 0.019 (7.7e-14 against 4.0e-12)             (bound 1e-5 * max|ref|)
  step      max error / bound: p, slow 0.034 (max |got - ref| 4.8e-07)
"""
import ctypes as C

import numpy as np
import pytest

import lamb_ref as L
from simlib import lib, ptr


class Item(C.Structure):
    _fields_ = [("start", C.c_uint64), ("count", C.c_uint32), ("lr", C.c_float), ("wd", C.c_float), ("reserved", C.c_uint32)]


V, I = C.c_void_p, C.c_int
MOMENTS_ARGS = [V, V, V, V, V, I, V, V, V, V, I, V]
STEP_ARGS = [V, V, V, V, V, V, V, I, V, V, V, I, V]


def sim(bufs, rows, hp, ss, calls):
    S = lib()
    S.clite_lamb_moments.argtypes = MOMENTS_ARGS
    S.clite_lamb_step.argtypes = STEP_ARGS
    S.clite_adamw_step.argtypes = [V, V, V, V, V, V, V, I, V, V, V]
    b = {k: (None if a is None else a.copy()) for k, a in bufs.items()}
    items = (Item * len(rows))(*[Item(*r) for r in rows])
    n_slots = len(b["norms"]) // 2
    for what, first, n in calls:
        it = C.c_void_p(C.addressof(items) + first * C.sizeof(Item))
        if what == "moments":
            part = C.c_void_p(b["partials"].ctypes.data + 8 * first)
            rc = S.clite_lamb_moments(ptr(b["p"]), ptr(b["g"]), ptr(b["m"]), ptr(b["v2"]), it, n, ptr(hp), ptr(ss), part, ptr(b["norms"]), n_slots, None)
        elif what == "lamb":
            rc = S.clite_lamb_step(ptr(b["p"]), ptr(b["g"]), ptr(b["m"]), ptr(b["v2"]), ptr(b["slow"]), ptr(b["cast"]), it, n, ptr(hp), ptr(ss),
                                   ptr(b["norms"]), n_slots, None)
        else:
            rc = S.clite_adamw_step(ptr(b["p"]), ptr(b["g"]), ptr(b["m"]), ptr(b["v2"]), ptr(b["slow"]), ptr(b["cast"]), it, n, ptr(hp), ptr(ss), None)
        assert rc == 0, (what, rc)
    return b


@pytest.mark.parametrize("step", L.STEPS)
def test_moments_and_norms(step):
    L.check_norms(sim, step)


@pytest.mark.parametrize("trust_clip", [False, True])
@pytest.mark.parametrize("step", L.STEPS)
@pytest.mark.parametrize("sync,cast,clip,gs", L.OPTIONS)
def test_step_matches_float64(sync, cast, clip, gs, step, trust_clip):
    L.check_step(sim, sync, cast, clip, gs, step, trust_clip)


def test_not_adapted_table_is_adamw_step_bitwise():
    L.check_not_adapted_is_adamw(sim)


def test_split_launch_on_a_tensor_boundary_equals_one_launch_bitwise():
    L.check_split_launch(sim)


def test_launchers_refuse_missing_arguments():
    S = lib()
    x = np.zeros(16, np.float32)
    items = (Item * 1)(Item(0, 4, 0.1, 0.0, 1))
    S.clite_lamb_moments.argtypes = MOMENTS_ARGS
    S.clite_lamb_step.argtypes = STEP_ARGS
    X = ptr(x)
    assert S.clite_lamb_moments(X, X, X, X, items, 0, X, X, X, X, 1, None) == -1
    assert S.clite_lamb_moments(X, X, X, X, items, 1, X, X, None, X, 1, None) == -1
    assert S.clite_lamb_moments(X, X, None, X, items, 1, X, X, X, X, 1, None) == -1
    assert S.clite_lamb_moments(X, X, X, X, items, 1, X, X, X, X, -1, None) == -1
    assert S.clite_lamb_step(X, X, X, X, X, None, items, 0, X, X, X, 1, None) == -1
    assert S.clite_lamb_step(X, X, X, X, X, None, items, 1, X, X, None, 1, None) == -1
    assert S.clite_lamb_step(X, X, X, None, X, None, items, 1, X, X, X, 1, None) == -1
    assert S.clite_lamb_step(X, X, X, X, X, None, items, 1, X, X, X, -1, None) == -1
    assert not x.any()
