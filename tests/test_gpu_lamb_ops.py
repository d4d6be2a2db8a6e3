"""Kernel-level GPU checks of the LAMB kernels (csrc/update_ops.hip) through clip_lite_amd.hip: lamb_moments and lamb_step called directly with the
hand-made OptimItem table of tests/lamb_ref.py (the checks are shared with tests/test_wavesim_lamb.py). Reference: lamb_ref.lamb_step_ref, float64
on the stored f32 inputs and the f32 hyper-parameters the kernel reads, fed the float64 norms.

Table (lars_ref's; sentinels in every gap, behind every buffer, in the norm slots no tensor owns and in the partial pairs of not-adapted items):
tensors of 4 (thread 0 alone), 1028 (second sweep), 8192 (exactly one item) and 8192 * 3 + 1020 elements (four items, ragged last), an adapted
tensor with g = 0, zero moments and wd = 0 (r = 0, so q = 1) and one with p = 0 (q = 1; it moves by lr u), two not-adapted tensors (reserved = 0)
between adapted ones. Step 1 from zero moments and step 1000 from random m, v2 >= m^2; TRUST_CLIP off and on, the parameters scaled so that
ratios above 1 and below 1 both occur (asserted on the reference).

Bounds: each of sum p^2, sum r^2 within 1e-5 * max(1, sum of terms) of float64 (the project's sumsq bound) and bit-identical between two runs; slots
of tensors outside the launched range untouched; p and g come back from lamb_moments bit for bit; m, v2 within 1e-5 * max|ref| (the AdamW kernel
test's moment bound). p, slow per element within 2e-6 * max(1, max|ref|) + 2e-5 * |delta_ref|, delta_ref = lr mult q r: the AdamW kernel's bound
(tests/test_gpu_optim_ops.py) plus the trust ratio's (tests/test_gpu_lars_ops.py: two sums each within 1e-5 -> their roots within 5e-6 -> the
ratio within 1e-5, doubled for the f32 roundings that form q). The bf16 copy equals the round-to-nearest-even of the RETURNED p bit for bit; g is
zero inside items; everything outside items comes back bit for bit. With every reserved word 0 the output is clite_adamw_step's bit for bit; a
launch of items [0, k) then [k, n), k on a tensor boundary, equals one launch bit for bit.

Measured on an MI355X (`pytest -s`, LAMBERR lines; maxima over the file's cases; no figure feeds a bound):
  norms     error / max(1, sum of terms): sum p^2 5.7e-08 (the 8192-element tensor), sum r^2 2.0e-07 (the 4-element tensor)     (bound 1e-5)
  moments   max error / bound: m 0.011 (2.2e-10 against 2.0e-08)   v2 0.019 (7.7e-14 against 4.0e-12)             (bound 1e-5 * max|ref|)
  step      max error / bound: p, slow 0.034 (max |got - ref| 4.8e-07, half an ulp of the largest parameters)
"""
import ctypes as C

import numpy as np
import pytest
import torch

import lamb_ref as L

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
        if what == "moments":
            hip.lamb_moments(d["p"], d["g"], d["m"], d["v2"], it, n, hpd, ssd, d["partials"][2 * first:2 * (first + n)], d["norms"])
        elif what == "lamb":
            hip.lamb_step(d["p"], d["g"], d["m"], d["v2"], d["slow"], cast, it, n, hpd, ssd, d["norms"])
        else:
            hip.adamw_step(d["p"], d["g"], d["m"], d["v2"], d["slow"], cast, it, n, hpd, ssd)
    torch.cuda.synchronize()
    return {k: (None if t is None else (t.cpu().numpy().view(np.uint16) if bufs[k].dtype == np.uint16 else t.cpu().numpy())) for k, t in d.items()}


@pytest.mark.parametrize("step", L.STEPS)
def test_moments_and_norms_match_float64_repeat_bitwise_and_leave_other_slots(step):
    L.check_norms(device, step)


@pytest.mark.parametrize("trust_clip", [False, True])
@pytest.mark.parametrize("step", L.STEPS)
@pytest.mark.parametrize("sync,cast,clip,gs", L.OPTIONS)
def test_lamb_step_matches_float64(sync, cast, clip, gs, step, trust_clip):
    L.check_step(device, sync, cast, clip, gs, step, trust_clip)


def test_not_adapted_table_is_adamw_step_bitwise():
    L.check_not_adapted_is_adamw(device)


def test_split_launch_on_a_tensor_boundary_equals_one_launch_bitwise():
    L.check_split_launch(device)
