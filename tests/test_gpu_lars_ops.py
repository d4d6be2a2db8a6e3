"""Kernel-level GPU checks of the LARS kernels (csrc/update_ops.hip) through clip_lite_amd.hip: lars_norms and lars_step called directly with the
hand-made OptimItem table of tests/lars_ref.py (the checks are shared with tests/test_wavesim_lars.py). Reference: lars_ref.lars_step_ref, float64
on the stored f32 inputs and the f32 hyper-parameters the kernel reads, fed the float64 norms. eta = 1, so that q u is of order one.

Table (sentinels in every gap, behind every buffer, in the norm slots no tensor owns and in the partial pairs of not-adapted items): tensors of 4
(thread 0 alone), 1028 (second sweep), 8192 (exactly one item) and 8192 * 3 + 1020 elements (four items, ragged last), an adapted tensor with g = 0
and one with p = 0 (q = 1), two not-adapted tensors (reserved = 0) between adapted ones.

Bounds: each of sum p^2, sum g^2 within 1e-5 * max(1, sum of terms) of float64 (the project's sumsq bound) and bit-identical between two runs; slots
of tensors outside the launched range untouched. p, v, slow per element within 1e-6 * max(1, |ref|) + 2e-5 * |delta_ref|, delta_ref = this step's
q u for v and lr mult q u for p and slow: the SGD kernel's bound plus the trust ratio's (two sums each within 1e-5 -> their roots within 5e-6 -> the
ratio within 1e-5, doubled for the f32 roundings that form q). The bf16 copy equals the round-to-nearest-even of the RETURNED p bit for bit; g is
zero inside items; everything outside items comes back bit for bit. With every reserved word 0 the output is clite_sgd_step's bit for bit; a launch
of items [0, k) then [k, n), k on a tensor boundary, equals one launch bit for bit.

Measured on an MI355X (`pytest -s`, LARSERR lines; maxima over the file's cases; no figure feeds a bound):
  norms   error / max(1, sum of terms): 1.1e-07 (260-element tensor, sum p^2); the four-item tensor 5.9e-08            (bound 1e-5)
  step    max error / bound: p, slow 0.107   v 0.101;   max |got - ref| / max(1, |ref|): p, slow 1.2e-07   v 5.1e-07
"""
import ctypes as C

import numpy as np
import pytest
import torch

import lars_ref as L

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _hip():
    from clip_lite_amd import hip
    return hip


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def device(bufs, rows, hp, ss, calls):
    hip = _hip()
    arr = (hip.OptimItem * len(rows))(*[hip.OptimItem(*r) for r in rows])
    items = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(DEV)
    d = {k: (None if a is None else _dev(a.view(np.int16) if a.dtype == np.uint16 else a)) for k, a in bufs.items()}
    cast = None if d["cast"] is None else d["cast"].view(torch.bfloat16)
    hpd, ssd = _dev(hp), _dev(ss)
    for what, first, n in calls:
        it = C.c_void_p(items.data_ptr() + first * C.sizeof(hip.OptimItem))
        if what == "norms":
            hip.lars_norms(d["p"], d["g"], it, n, d["partials"][2 * first:2 * (first + n)], d["norms"])
        elif what == "lars":
            hip.lars_step(d["p"], d["g"], d["v"], d["slow"], cast, it, n, hpd, ssd, d["norms"])
        else:
            hip.sgd_step(d["p"], d["g"], d["v"], d["slow"], cast, it, n, hpd, ssd)
    torch.cuda.synchronize()
    return {k: (None if t is None else (t.cpu().numpy().view(np.uint16) if bufs[k].dtype == np.uint16 else t.cpu().numpy())) for k, t in d.items()}


def test_norms_match_float64_repeat_bitwise_and_leave_other_slots():
    L.check_norms(device)


@pytest.mark.parametrize("sync,cast,clip,gs", L.OPTIONS)
def test_lars_step_matches_float64(sync, cast, clip, gs):
    L.check_step(device, sync, cast, clip, gs)


def test_not_adapted_table_is_sgd_step_bitwise():
    L.check_not_adapted_is_sgd(device)


def test_split_launch_on_a_tensor_boundary_equals_one_launch_bitwise():
    L.check_split_launch(device)
