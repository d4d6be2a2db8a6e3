"""The SigLIP loss kernels (csrc/siglip_ops.hip: clite_siglip_fwd, clite_siglip_bwd) on the wave simulator, with the checks of
tests/test_gpu_siglip.py (tests/siglip_ref.py: float64 reference, the bounds of tests/loss_ref.py).

Shapes (B, ld, ldd):
  (8, 8, 8)          one lane of one wave carries a row; 2 workgroups
  (24, 32, 24)       padded ld: the vector load of lane 2 stops at column 24 of 32; three live lanes
  (72, 72, 72)       nine live lanes, 18 workgroups
  (136, 144, 136)    ld > ldd = B: 17 live lanes, and C's padding columns lie outside every store; 34 workgroups
  (520, 520, 520)    f32 only: columns 512..519 are lane 0's second trip, and the simulator build caps the row kernels at 128 workgroups = 512 rows,
                     so rows 512..519 are a second pass of the first two workgroups
(temperature, bias): (log 10, -10), the initial values, where every negative sits near sigmoid(-10); (log 100, -3), a sharp diagonal."""
import numpy as np
import pytest

import simlib
import siglip_ref as S
from loss_backends import BF16, F32

DTS = [BF16, F32]
SHAPES = [(8, 8, 8), (24, 32, 24), (72, 72, 72), (136, 144, 136)]
POINTS = [(S.T_INIT, S.B_INIT), (S.T100, -3.0)]


@pytest.fixture(scope="module")
def be():
    return S.SiglipSimBackend()


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("t,b", POINTS)
@pytest.mark.parametrize("B,ld,ldd", SHAPES)
def test_siglip_matches_float64(be, dt, B, ld, ldd, t, b):
    S.check_siglip(be, dt, B, ld, ldd, t, b)


@pytest.mark.parametrize("t,b", POINTS)
def test_siglip_second_sweep_and_second_grid_pass(be, t, b):
    S.check_siglip(be, F32, 520, 520, 520, t, b)


@pytest.mark.parametrize("dt", DTS)
def test_siglip_repeats_bitwise_in_both_modes(be, dt):
    S.check_siglip(be, dt, 136, 144, 136, S.T_INIT, S.B_INIT, repeat=True)


@pytest.mark.parametrize("dt", DTS)
def test_siglip_unaligned_ld_takes_single_loads(be, dt):
    """ld = 27 is no multiple of 4: rows do not start on 16 bytes, so every element is loaded on its own."""
    S.check_siglip(be, dt, 24, 27, 24, S.T_INIT, S.B_INIT)


@pytest.mark.parametrize("dt", DTS)
def test_siglip_finite_at_the_extremes(be, dt):
    """cosines +-1 at t = 100, bias = -10 and +10: |x| reaches 110 and nothing becomes inf or NaN."""
    B = 8
    Cm = np.where(np.arange(B)[:, None] % 2 == np.arange(B)[None, :] % 3, 1.0, -1.0).astype(np.float32)
    for bias in (-10.0, 10.0):
        ref = S.siglip_ref(Cm, np.float32(S.T100), bias)
        Cd, t, b, g = be.dev(Cm, F32), be.dev(np.array([S.T100]), F32), be.dev(np.array([bias]), F32), be.dev(np.ones(1), F32)
        part, acc, dC = be.dev(np.zeros(2 * B), F32), be.dev(np.zeros(2), F32), be.dev(np.zeros((B, B)), dt)
        dtemp, dbias = be.dev(np.zeros(1), F32), be.dev(np.zeros(1), F32)
        assert be.call("siglip_fwd", Cd, B, B, t, b, part, acc) == 0
        assert be.call("siglip_bwd", dt, Cd, B, B, t, b, g, 1.0, dC, B, part, dtemp, dbias) == 0
        got = [be.host(h) for h in (acc, dC, dtemp, dbias)]
        assert all(np.isfinite(v).all() for v in got)
        S.R.scalar(f"extremes b={bias} loss", got[0][0], ref.loss, ref.row_terms)
        S.R.elem(f"extremes b={bias} dC", got[1], ref.dC, dt, f32_eval=S.siglip_dC_float32(Cm, S.T100, bias, 1.0))
        S.R.scalar(f"extremes b={bias} dtemp", got[2][0], ref.dtemp, ref.dtemp_terms)
        S.R.scalar(f"extremes b={bias} dbias", got[3][0], ref.dbias, ref.dbias_terms)


@pytest.mark.parametrize("dt", DTS)
def test_siglip_scalar_gradients_are_optional(be, dt):
    S.check_siglip_no_scalar_grads(be, dt)


def test_siglip_refusals(be):
    simlib.clear_launch_log()
    S.check_siglip_refusals(be)
    assert simlib.launch_log() == [], "a refused call launched a kernel"


def test_siglip_launches(be):
    """Dry run: each entry is a row kernel of min(ceil(B / 4), cap) workgroups of four waves and then the one-wave fold; the backward skips the fold
    when neither scalar gradient is asked for. The simulator build's cap is 128 workgroups."""
    x = np.zeros(8, np.float32)
    simlib.set_dry_run(True)
    try:
        for B, grid in ((8, 2), (24, 6), (72, 18), (136, 34), (510, 128), (520, 128), (4096, 128)):
            for dt, inst in ((BF16, "siglip_bwd_kernel<__bf16>"), (F32, "siglip_bwd_kernel<float>")):
                simlib.clear_launch_log()
                assert be.call("siglip_fwd", x, B, B, x, x, x, x) == 0
                assert be.call("siglip_bwd", dt, x, B, B, x, x, x, 1.0, x, (B + 7) // 8 * 8, x, x, x) == 0
                assert be.call("siglip_bwd", dt, x, B, B, x, x, x, 1.0, x, (B + 7) // 8 * 8, x, None, x) == 0
                assert be.call("siglip_bwd", dt, x, B, B, x, x, x, 1.0, x, (B + 7) // 8 * 8, x, None, None) == 0
                log = simlib.launch_log()
                names = [n.split("::")[-1].split("(")[0] for n, _, _ in log]
                assert names == ["siglip_fwd_kernel", "siglip_fold_kernel", inst, "siglip_fold_kernel", inst, "siglip_fold_kernel", inst], log
                assert [(g, b) for _, g, b in log] == [((grid, 1, 1), 256) if "fold" not in n else ((1, 1, 1), 64) for n in names], log
    finally:
        simlib.set_dry_run(False)
        simlib.clear_launch_log()
