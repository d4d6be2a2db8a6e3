"""Kernel-level GPU checks of the loss kernels (csrc/loss_ops.hip) through clip_lite_amd.hip against the float64 references of tests/loss_ref.py,
evaluated on the SAME storage-rounded inputs: the dot critic's JSD forward / backward, l2_normalize and its backward, InfoNCE forward / backward,
the prior discriminator's tail in both forms, loss_finalize and add. bf16 and f32 wherever the kernel has both. The checks themselves are
loss_ref.check_*, shared with the wave simulator (tests/test_loss_ref_host.py): outputs are pre-filled with 7.0, every buffer carries a sentinel
row or tail that must come back untouched, every accumulator (acc, dtemp, dw2, db2) starts non-zero and must be added to.

Bounds (ref = float64 on the stored inputs, max|ref| over the compared tensor; loss_ref.elem / vec / scalar):
  element-wise f32 2e-5 * max|ref| | bf16 2^-7 * |ref| + 2e-5 * max|ref| | lse_r, lse_c, dw2: 1e-4 * max|ref|
  loss sums, dtemp, db2: 1e-5 * max(1, sum|terms|) | padding, sentinels, add: exact.
One bound is replaced, by the rule in loss_ref.elem (the same formula in plain torch.float32 misses the bound -> 4 x that evaluation's error):
  infonce dC at (10, 16, 16), t = log 100: 2e-5 * max|ref| = 1.12e-08 -> 4 x 2.79e-06 = 1.12e-05. The softmax there is sharp (max|dC| = 5.6e-04, the
  diagonal's softmax_row + softmax_col - 2 is a difference of numbers near 1) and S = 100 C carries half an ulp of 1.9e-06.
  The kernel first measured 2.0e-05 there, 7 x the float32 evaluation: its backward formed t * C - lse as one fma while lse came from the rounded
  t * C. csrc/loss_ops.hip now uses the rounded product at every use (`scaled`), after which the kernel's error EQUALS the float32 evaluation's.
l2_normalize_bwd takes max|ref| per row (tighter): dx scales with 1 / max(|x|, eps), which is 1e12 in the all-zero and the 1e-20 row.

Which device path the shapes take (from the launchers in csrc/loss_ops.hip; a workgroup is 4 waves, one wave owns one row):
  critic (1, 8)        1 workgroup, 1 live wave, 1 chunk: one live lane in slot 0; the row is its own negative
  critic (2, 8)        1 workgroup, 2 live waves
  critic (7, 520)      2 workgroups, the last with 3 live waves; 65 chunks: slot 0 full, lane 0 alone in slot 1
  critic (33, 1024)    9 workgroups, the last with 1 live wave; 128 chunks: slots 0 and 1 full
  critic (130, 2048)   33 workgroups (the last with 2 live waves) adding into the same two floats; 256 chunks: all four slots full
                       deterministic mode: one wave of one workgroup strides over all 130 rows
  l2_normalize (8197, 8)  2050 workgroups asked, the cap of 2048 x 4 waves leaves five waves a second row; (7, 520), (5, 2048) as the critic's slots
  infonce B = 8, 10    one lane trip in the lse kernels (rows with stride 1, columns with stride ld); 2 / 3 workgroups
  infonce (72, 80, 72)    lanes 0..7 take a second trip; backward: 9 live lanes of 8 columns; 18 workgroups
  infonce (133, 140, 136) three trips (lanes 0..4 the third), 34 workgroups, the last with 1 live wave; backward 17 live lanes, the last chunk
                       half padding; deterministic mode: one wave over all rows
  infonce (264, 264, 264) five trips (lanes 0..7 the fifth), ld = ldd = B: no padding column; backward 33 live lanes (a second backward trip
                       needs ldd > 512 and is not reached by the shapes above)
  prior (1, 8)         2 rows: 1 workgroup, 2 live waves, 1 chunk
  prior (5, 200)       10 rows, 3 workgroups; 25 chunks: one_chunk, dw2 from registers, 25 live lanes add
  prior (5, 512)       64 chunks: one_chunk with every lane holding a chunk (the boundary)
  prior (5, 520)       65 chunks: one_chunk false, dw2 by per-element atomics, lane 0 takes a second trip
  prior (37, 520)      74 rows: forward 19 workgroups; backward capped at 16 workgroups = 64 waves, waves 0..9 own two rows; atomic branch
  prior (128, 1024)    256 rows: forward 64 workgroups; backward 16 workgroups, every wave owns four rows; 128 chunks = two trips, atomic branch
  add 8 / 4104 / 4194312  1 thread | 513 chunks on 3 workgroups, the last with one live thread | 524289 chunks on the capped 2048 x 256 threads:
                       thread 0 of workgroup 0 takes a second trip

Measured on an MI355X (`pytest -s` prints every figure as REDERR; error / max(1, sum|terms|) for the scalars, error / max|ref| for the vectors, the
maximum over the file's cases; beside it the same for a sequential float32 sum of the float64 terms; neither feeds a bound):
  critic   acc[0] 8.9e-08 / 4.6e-10   acc[1] 1.5e-07 / 2.4e-07   dtemp 3.2e-07 / 2.3e-07
  infonce  acc[0] 4.4e-07 / 1.9e-07   acc[1] 1.8e-07 / 1.4e-07   dtemp 2.6e-06 / 3.6e-06   lse_r, lse_c 8.2e-08 of max|ref|
           dC, f32 storage, max |got - ref| kernel / torch.float32 (bound): (8, 8, 8) 5.1e-07 / 4.8e-07 (3.8e-05), at t = log 100 7.4e-06 / 7.4e-06
           (2.9e-04); (10, 16, 16) 6.1e-07 / 6.1e-07 (5.2e-06), at log 100 2.8e-06 / 2.8e-06 (replaced: 1.1e-05; bf16 storage 3.7e-06);
           (72, 80, 72) 9.2e-08 / 1.2e-07 (4.6e-06), at log 100 2.2e-06 / 2.2e-06 (3.3e-05); (133, 140, 136) 4.1e-08 / 6.2e-08 (2.5e-06), at
           log 100 1.4e-06 / 1.4e-06 (1.8e-05); (264, 264, 264) 3.0e-08 / 3.0e-08 (1.3e-06), at log 100 9.5e-07 / 9.5e-07 (8.9e-06)
  prior    acc 1.2e-07 / 1.3e-07   db2 3.0e-07 / 3.7e-08   dw2 4.7e-07 / 4.1e-07 of the column's sum|terms| at (128, 1024) and (37, 520); at B <= 5
           up to 2.8e-05, which is the f32 rounding of the non-zero start value against column sums a thousand times smaller than it
The scalar bound of 1e-5 sits 4 to 100 times above these figures, the kernels at the level of a plain float32 sum.
"""
import numpy as np
import pytest

import loss_ref as R
from loss_backends import BF16, F32, HipBackend

pytestmark = pytest.mark.gpu
DTS = [BF16, F32]
T100 = float(np.log(100.0))


@pytest.fixture(scope="module")
def be():
    return HipBackend()


def _pairings(B):
    return [None] + (["cluster"] if B % 2 == 0 and B >= 4 else []) + (["random"] if B >= 7 else [])


CRITIC = [(B, D, p) for B, D in [(1, 8), (2, 8), (7, 520), (33, 1024), (130, 2048)] for p in _pairings(B)]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("B,D,pairing", CRITIC)
def test_critic_matches_float64(be, dt, B, D, pairing):
    R.check_critic(be, dt, B, D, pairing)


@pytest.mark.parametrize("dt", DTS)
def test_critic_rejects_bad_shapes_and_touches_nothing(be, dt):
    R.check_critic_rejects(be, dt)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("pairing", [None, "cluster"])
def test_critic_deterministic_mode_repeats_bitwise(be, deterministic_reductions, dt, pairing):
    R.check_critic(be, dt, 130, 2048, pairing, repeat=True)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("B,D", [(1, 8), (7, 520), (5, 2048), (8197, 8)])
def test_l2_normalize_forward_and_backward(be, dt, B, D):
    R.check_l2_normalize(be, dt, B, D)


INFONCE = [(8, 8, 8), (10, 16, 16), (72, 80, 72), (133, 140, 136), (264, 264, 264)]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("t", [R.T_CLIP, T100])
@pytest.mark.parametrize("B,ld,ldd", INFONCE)
def test_infonce_matches_float64(be, dt, B, ld, ldd, t):
    R.check_infonce(be, dt, B, ld, ldd, t)


@pytest.mark.parametrize("dt", DTS)
def test_infonce_accepts_no_dtemp(be, dt):
    R.check_infonce(be, dt, 72, 80, 72, R.T_CLIP, with_dtemp=False)


@pytest.mark.parametrize("dt", DTS)
def test_infonce_deterministic_mode_repeats_bitwise(be, deterministic_reductions, dt):
    R.check_infonce(be, dt, 133, 140, 136, R.T_CLIP, repeat=True)


PRIOR = [(1, 8), (5, 200), (5, 512), (5, 520), (37, 520), (128, 1024)]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("use_softplus", [False, True])
@pytest.mark.parametrize("B,K", PRIOR)
def test_prior_tail_matches_float64(be, dt, B, K, use_softplus):
    R.check_prior_tail(be, dt, B, K, use_softplus, max_logit=6.0)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("B,K", [(37, 520), (128, 1024)])
def test_prior_tail_softplus_across_threshold(be, dt, B, K):
    """Logits out to +-30: softplus_f's x > 20 branch on both sides (softplus(-s) for the noise rows, softplus(s) for the feature rows)."""
    R.check_prior_tail(be, dt, B, K, True, max_logit=30.0)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("use_softplus", [False, True])
def test_prior_tail_deterministic_mode_repeats_bitwise(be, deterministic_reductions, dt, use_softplus):
    R.check_prior_tail(be, dt, 37, 520, use_softplus, repeat=True)


def test_loss_finalize(be):
    R.check_loss_finalize(be)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("n", [8, 4104, 4194312])
def test_add_is_the_rounded_f32_sum(be, dt, n):
    R.check_add(be, dt, n)
