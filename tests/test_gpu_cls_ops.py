"""Kernel-level GPU checks of the classification head's kernels (csrc/cls_ops.hip: xent_fwd / xent_bwd) through clip_lite_amd.hip against the
float64 evaluation of nn.CrossEntropyLoss (ignore_index -100) and TopkAccuracy in tests/loss_ref.py. The check is loss_ref.check_xent, shared with
the wave simulator: ld = C rounded up to 4 plus 4 with NaN in the columns >= C (they must reach nothing), ldd = C rounded up to 8 plus 8, Bp = B
rounded up to 8 plus 8, outputs pre-filled with 7.0 and followed by a sentinel row, acc started at {0.25, 3, 5, 7}. Labels include -100, C (out of
range) and 2^40; two rows tie the label with another class, once above and once below it. Masked classes: -inf in one to C - 1 classes that are
not the label, at column 0 (a lane's first element, before any finite value), behind finite values, at random columns, and everywhere but the label.
A -inf at the label, +inf and NaN logits are outside nn.CrossEntropyLoss's finite results and are not tested.

Bounds (loss_ref.vec / scalar / elem): lse 1e-4 * max|ref|; acc[0] 1e-5 * max(1, sum|terms|); dlogits f32 2e-5 * max|ref|, bf16 2^-7 * |ref| +
2e-5 * max|ref|; the counters acc[1..3], the zeros of padding rows / columns, ignored rows and masked classes, and the sentinels: exact. No bound
was replaced through the float32 procedure.

Which device path the shapes take (one 64-lane workgroup per row; a lane reads 4 columns per chunk, 4 chunks 256 columns apart per trip, a trip
covers 1024 columns; the backward covers 512 columns of dlogits per trip):
  (C 1, B 10)      lane 0, one live element; lse = z, loss 0
  (C 3, B 8200)    forward grid capped at 8192: workgroups 0..7 own two rows and add their two losses from registers; backward Bp = 8208: 16 own two
  (C 10, B 7)      lanes 0..2, the third with two live elements
  (C 1003, B 64)   one trip, the fourth chunk live in lanes 0..58 with 3 elements in the last; backward two trips; deterministic mode: one workgroup
                   walks all 64 rows
  (C 1030, B 9)    lanes 0 and 1 take a second trip (lane 1 with two live elements); backward three trips
  (C 2052, B 5)    three trips, the third with lane 0 alone; backward five trips

Measured on an MI355X (`pytest -s`, REDERR lines; maxima over the file's cases; neither figure feeds a bound):
  acc[0], error / max(1, sum|terms|), kernel / sequential float32 sum: (C 10, B 7) 6.4e-08 / 4.2e-08   (1003, 64) 1.7e-07 / 1.0e-07
          (1030, 9) 1.3e-08 / 1.3e-08   (2052, 5) 9.5e-08 / 6.6e-08   (3, 8200) 3.2e-06 / 2.5e-06: 8192 float atomics onto a sum of 1.6e4, whose
          ulp is 1e-3, in an order that changes from run to run; a float32 sum of the same terms in a random order loses 1e-06 to 3.5e-06
          lse 7.6e-08 of max|ref|
  Against the library before the lse_merge change, every masked-class case fails with lse = nan (the ten parametrised cases and the row of the report).
"""
import numpy as np
import pytest

import loss_ref as R
from loss_backends import BF16, F32, HipBackend

pytestmark = pytest.mark.gpu
DTS = [BF16, F32]
SHAPES = [(1, 10), (3, 8200), (10, 7), (1003, 64), (1030, 9), (2052, 5)]


@pytest.fixture(scope="module")
def be():
    return HipBackend()


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("k", [1, 5, "C+3"])
@pytest.mark.parametrize("Cc,B", SHAPES)
def test_xent_matches_float64(be, dt, Cc, B, k):
    R.check_xent(be, dt, Cc, B, Cc + 3 if k == "C+3" else k)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("Cc,B", [s for s in SHAPES if s[0] >= 2])
def test_xent_masked_classes_contribute_nothing(be, dt, Cc, B):
    R.check_xent(be, dt, Cc, B, 5, masked=True)


def test_xent_masked_row_of_the_report(be):
    """[-inf, 1, 2, 0.5, 0, -1, 3, 0.25] with label 2: lse = 3.5407709, where lane 0 meets -inf before any finite value."""
    z, y, want = R.MASKED_ROW
    lse, acc = be.dev(np.zeros(1), F32), be.dev(np.zeros(4), F32)
    assert be.call("xent_fwd", be.dev(z, F32), 8, 1, 8, be.dev(y, "i64"), 1, lse, acc) == 0
    assert abs(be.host(lse)[0] - want) <= 1e-4 * want
    a = be.host(acc)
    assert abs(a[0] - (want - 2.0)) <= 1e-5 * max(1.0, want - 2.0) and list(a[1:]) == [0, 0, 1]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("Cc,B", [(10, 7), (3, 8200)])
def test_xent_all_rows_ignored(be, dt, Cc, B):
    """acc unchanged bit for bit, gradient all zero."""
    R.check_xent(be, dt, Cc, B, 5, all_ignored=True)


def test_xent_ties_go_to_the_lower_index(be):
    z = np.zeros((3, 12), np.float32)
    z[0, [2, 5]] = 4.0                      # label 5 ties with class 2: rank 1 (not top-1), inside top-2
    z[1, [2, 5]] = 4.0                      # label 2 ties with class 5: rank 0
    z[2, :10] = np.arange(10)               # label 7: two classes above it
    z[:, 10:] = np.nan
    y = np.array([5, 2, 7], np.int64)
    for topk, want in ((2, [1, 2, 3]), (3, [1, 3, 3]), (13, [1, 3, 3])):
        lse, acc = be.dev(np.zeros(3), F32), be.dev(np.zeros(4), F32)
        assert be.call("xent_fwd", be.dev(z, F32), 12, 3, 10, be.dev(y, "i64"), topk, lse, acc) == 0
        assert list(be.host(acc)[1:]) == want, (topk, be.host(acc))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("masked", [False, True])
def test_xent_deterministic_mode_repeats_bitwise(be, deterministic_reductions, dt, masked):
    R.check_xent(be, dt, 1003, 64, 5, masked=masked, repeat=True)
