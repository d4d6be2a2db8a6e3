"""The LARS kernels (csrc/update_ops.hip: clite_lars_norms, clite_lars_step) on the wave simulator, with the checks of tests/test_gpu_lars_ops.py
(tests/lars_ref.py: the hand-made item table, the float64 reference, the bounds). Runs without a GPU."""
import ctypes as C

import numpy as np
import pytest

import lars_ref as L
from simlib import lib, ptr


class Item(C.Structure):
    _fields_ = [("start", C.c_uint64), ("count", C.c_uint32), ("lr", C.c_float), ("wd", C.c_float), ("reserved", C.c_uint32)]


def sim(bufs, rows, hp, ss, calls):
    S = lib()
    V, I = C.c_void_p, C.c_int
    S.clite_lars_norms.argtypes = [V, V, V, I, V, V, I, V]
    S.clite_lars_step.argtypes = [V, V, V, V, V, V, I, V, V, V, I, V]
    S.clite_sgd_step.argtypes = [V, V, V, V, V, V, I, V, V, V]
    b = {k: (None if a is None else a.copy()) for k, a in bufs.items()}
    items = (Item * len(rows))(*[Item(*r) for r in rows])
    n_slots = len(b["norms"]) // 2
    for what, first, n in calls:
        it = C.c_void_p(C.addressof(items) + first * C.sizeof(Item))
        if what == "norms":
            part = C.c_void_p(b["partials"].ctypes.data + 8 * first)
            rc = S.clite_lars_norms(ptr(b["p"]), ptr(b["g"]), it, n, part, ptr(b["norms"]), n_slots, None)
        elif what == "lars":
            rc = S.clite_lars_step(ptr(b["p"]), ptr(b["g"]), ptr(b["v"]), ptr(b["slow"]), ptr(b["cast"]), it, n, ptr(hp), ptr(ss), ptr(b["norms"]),
                                   n_slots, None)
        else:
            rc = S.clite_sgd_step(ptr(b["p"]), ptr(b["g"]), ptr(b["v"]), ptr(b["slow"]), ptr(b["cast"]), it, n, ptr(hp), ptr(ss), None)
        assert rc == 0, (what, rc)
    return b


def test_norms():
    L.check_norms(sim)


@pytest.mark.parametrize("sync,cast,clip,gs", L.OPTIONS)
def test_step_matches_float64(sync, cast, clip, gs):
    L.check_step(sim, sync, cast, clip, gs)


def test_not_adapted_table_is_sgd_step_bitwise():
    L.check_not_adapted_is_sgd(sim)


def test_split_launch_on_a_tensor_boundary_equals_one_launch_bitwise():
    L.check_split_launch(sim)


def test_launchers_refuse_missing_arguments():
    S = lib()
    x = np.zeros(8, np.float32)
    items = (Item * 1)(Item(0, 4, 0.1, 0.0, 1))
    S.clite_lars_norms.argtypes = [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 2 + [C.c_int, C.c_void_p]
    assert S.clite_lars_norms(ptr(x), ptr(x), items, 0, ptr(x), ptr(x), 1, None) == -1
    assert S.clite_lars_norms(ptr(x), ptr(x), items, 1, None, ptr(x), 1, None) == -1
    assert S.clite_lars_norms(ptr(x), ptr(x), items, 1, ptr(x), ptr(x), -1, None) == -1
