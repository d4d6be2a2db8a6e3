"""The exact tile-edge cases of tests/gemm_exact.py on the wave-simulator build (no GPU): a subset of the table tests/test_gpu_gemm_edges.py runs on the
real kernels goes through the same builder, backend interface and checker - which proves here that the reference, the placement (NaN slack, 7.0
sentinels) and the 2^24 condition are right - and the WHOLE GPU table goes through the launchers in dry run, to show which kernel instantiation
families it reaches. The simulator emulates the buffer descriptor's range check (an offset past the operand's span reads zero), not the LDS-DMA
ring's timing or the MFMA hardware: those are what the GPU file is for."""
import re

import pytest

import gemm_exact as X
from gemm_exact import BF16, F32, CV, G

AUTO, W128, W256x128, W256, NARROW = range(5)
SMALL_GROUP = dict(convs=X.GROUP_CONVS[:2] + X.GROUP_CONVS[6:], linears=X.GROUP_LINEARS[2:3])          # (the simulator costs seconds per large member)

SUBSET = [
    # gemm_nt: the 3-stage ring with the plain-store and with the generic epilogue, the 4-stage ring, the two-K-group kernel, each wide tile
    (AUTO, G("gemm_nt", BF16, 129, 136, 72, "bf16")), (AUTO, G("gemm_nt", BF16, 63, 72, 40, "f32")), (AUTO, G("gemm_nt", BF16, 255, 264, 136, "relu_preact")),
    (NARROW, G("gemm_nt", BF16, 257, 264, 264, "bias")), (W128, G("gemm_nt", BF16, 257, 264, 136, "f32")), (W256x128, G("gemm_nt", BF16, 255, 136, 264, "bf16")),
    (W256, G("gemm_nt", BF16, 257, 264, 264, "residual")), (NARROW, G("gemm_nt", BF16, 63, 72, 40, "colsum")), (W128, G("gemm_nt", BF16, 127, 136, 72, "colsum_bias")),
    (AUTO, G("gemm_nt", BF16, 129, 72, 520, "ws_full")), (AUTO, G("gemm_nt", BF16, 65, 72, 2304, "ws")), (AUTO, G("gemm_nt", BF16, 7, 56, 24, "ld2")),
    # gemm_nn (the k-strided B operand)
    (AUTO, G("gemm_nn", BF16, 129, 136, 40, "f32")), (W128, G("gemm_nn", BF16, 257, 264, 136, "bf16")), (W256x128, G("gemm_nn", BF16, 129, 256, 128, "dact")),
    (W256, G("gemm_nn", BF16, 255, 264, 136, "alpha_half")), (NARROW, G("gemm_nn", BF16, 1, 8, 8, "alpha_m2")), (AUTO, G("gemm_nn", BF16, 256, 136, 256, "ws_f32")),
    (AUTO, G("gemm_nn", BF16, 64, 120, 56, "ld2_f32")),
    # gemm_tn: any K, float-atomic accumulation onto the pre-fill, split K
    (AUTO, G("gemm_tn", BF16, 264, 264, 129, "atomic")), (NARROW, G("gemm_tn", BF16, 128, 56, 263, "atomic_m2")), (W128, G("gemm_tn", BF16, 136, 72, 9, "f32")),
    (AUTO, G("gemm_tn", BF16, 8, 136, 1, "bf16")), (AUTO, G("gemm_tn", BF16, 72, 264, 520, "atomic")), (W256, G("gemm_tn", BF16, 136, 136, 72, "colsum_rows1")),
    # F32 storage, as it is and as split bf16; the deterministic mode with and without statistics
    (AUTO, G("gemm_nt", F32, 127, 136, 72, "colsum")), (AUTO, G("gemm_nt", F32, 65, 128, 64, "relu_preact", split=1)), (AUTO, G("gemm_tn", F32, 136, 72, 9, "atomic")),
    (AUTO, G("gemm_nn", F32, 63, 72, 40, "f32", split=1)), (AUTO, G("gemm_nt", BF16, 129, 256, 128, "colsum", det=1)), (W128, G("gemm_nn", BF16, 63, 72, 40, "colsum_rows1", det=1)),
    (AUTO, G("gemm_tn", BF16, 136, 8, 256, "atomic", det=1)),
    # one convolution of each kind (and conv_patch.hip under the automatic policy)
    (AUTO, CV("conv_fwd", BF16, (2, 7, 9, 64, 64, 3, 1, 1), "colsum", slack=0)), (W128, CV("conv_fwd", BF16, (2, 7, 9, 64, 64, 3, 1, 1), "colsum", slack=0)),
    (AUTO, CV("conv_fwd", BF16, (43, 1, 3, 136, 160, 1, 1, 0), "bf16")), (W256x128, CV("conv_fwd", BF16, (2, 7, 9, 64, 160, 3, 2, 1), "f32")),
    (AUTO, CV("conv_dgrad", BF16, (2, 8, 8, 40, 72, 1, 1, 0), "bf16")), (W256, CV("conv_dgrad", BF16, (1, 5, 5, 64, 160, 3, 1, 1), "f32")),
    (AUTO, CV("conv_dgrad_wt", BF16, (2, 7, 9, 72, 64, 1, 2, 0), "inplace")), (AUTO, CV("conv_dgrad_wt", BF16, (2, 8, 8, 64, 64, 3, 1, 1), "bf16", slack=0)),
    (AUTO, CV("conv_dgrad_s2", BF16, (2, 8, 8, 64, 64, 3, 2, 1), "bf16")), (W128, CV("conv_dgrad_s2_wt", BF16, (1, 6, 10, 128, 64, 3, 2, 1), "f32")),
    (AUTO, CV("conv_wgrad", BF16, (43, 1, 3, 136, 160, 1, 1, 0), "wgrad")), (AUTO, CV("conv_wgrad", F32, (2, 7, 9, 64, 64, 3, 1, 1), "wgrad")),
    (AUTO, X.group_case(BF16, **SMALL_GROUP)), (AUTO, X.group_case(BF16, det=1, **SMALL_GROUP)),
]


@pytest.fixture(scope="module")
def sim():
    from gemm_backends import SimBackend
    s = SimBackend()
    yield s
    s.set_tile_policy(AUTO)


@pytest.mark.parametrize("policy,case", SUBSET, ids=["p%d-%s" % (p, X.case_id(c)) for p, c in SUBSET])
def test_subset_matches_the_float64_reference_bit_for_bit(sim, policy, case):
    sim.set_tile_policy(policy)
    b = X.build(case)
    rcs, got = sim.run(b)
    assert not any(rcs), rcs
    X.check(b, got)


def test_subset_is_part_of_the_gpu_table():
    ids = {X.case_id(c) for dt in (BF16, F32) for c in X.full_table(dt)}
    for _, c in SUBSET:
        assert c["op"] == "wgrad_group" or X.case_id(c) in ids, X.case_id(c)


def test_refused_shapes_return_an_error_and_write_nothing(sim):
    for dt in (BF16, F32):
        for case in X.refusal_cases(dt):
            b = X.build(case)
            rcs, got = sim.run(b)
            assert all(rc != 0 for rc in rcs), (case["refuse"], rcs)
            X.check_untouched(b, got)


@pytest.mark.parametrize("dt", [BF16, F32], ids=["bf16", "f32"])
def test_every_case_of_the_gpu_table_stays_below_2_to_the_24(dt):
    """build() asserts it for each case (Built.need): the largest partial sum of the reference, statistics and epilogue terms included"""
    worst = max(X.build(c).bound for c in X.full_table(dt))
    assert 0 < worst < X.LIMIT / 8          # (the table is nowhere near the limit: the long-K cases reach 2^17)


# The kernel instantiation families the GPU table must reach: (what, a regular expression on the logged instantiation).
# ring depth and epilogue instantiation are the last template arguments of igemm_dma_kernel<T, CFG, LA, LB, STAGES, EPI, SPLIT>.
FAMILIES = [
    ("3-stage ring, generic epilogue", r"::igemm_dma_kernel<__bf16, .*, 3>\(|::igemm_dma_kernel<__bf16, .*, 3, 0, false>\("),
    ("3-stage ring, plain-store epilogue", r"::igemm_dma_kernel<__bf16, .*, 3, 2(, false)?>\("),
    ("4-stage ring", r"::igemm_dma_kernel<__bf16, .*, 4(, 0, false)?>\("),
    ("f32 ring", r"::igemm_dma_kernel<float, .*, [34](, 0, false)?>\("),
    ("f32 ring as split bf16", r"::igemm_dma_kernel<float, .*, [34], 0, true>\("),
    ("two-K-group kernel", r"::igemm_dma_kernel_g2<__bf16, "),
    ("wide 128 x 128", r"::igemm_wide_kernel<clite::WideCfg<128, 128, "),
    ("wide 256 x 128", r"::igemm_wide_kernel<clite::WideCfg<256, 128, "),
    ("wide 256 x 256", r"::igemm_wide_kernel<clite::WideCfg<256, 256, "),
    ("wide, plain-store epilogue", r"::igemm_wide_kernel<.*, [23], 2>\("),
    ("256 x 64 tile", r"clite::TileCfg<256, 64, "),
    ("64 x 128 weight-gradient tile", r"clite::TileCfg<64, 128, "),
    ("128 x 64 weight-gradient tile", r"clite::TileCfg<128, 64, "),
    ("split-K finish", r"::splitk_finish_kernel<__bf16>"),
    ("conv patch kernel", r"::conv3x3_patch_kernel<0>"),
    ("grouped weight gradient", r"::wgrad_group_kernel<|::igemm_group"),
    ("deterministic statistics", r"::colstats_det_kernel<__bf16>"),
    ("deterministic statistics, f32", r"::colstats_det_kernel<float>"),
]
# Arms the table leaves to the existing tests, with the reason:
#  * the row-range persistent forward form (igemm_dma_bn_kernel FORM 4) needs more than 2 x CLITE_BN_SLOTS = 1024 output tiles on the GPU, i.e.
#    >= 131 072 rows: tests/test_gpu_igemm.py's full-size convolutions and tests/test_wavesim_igemm.py (4 slots in the simulator build) cover it;
#  * the BatchNorm-backward epilogue forms (igemm_dma_bn_kernel FORM 0 - 3, 5) divide by a batch count and centre on a mean - not exact in integers:
#    tests/test_gpu_dgrad_epilogue.py holds them to float64 references;
#  * GELU, tanh and dropout epilogues (WideEpiForm 3 - 5) are not exact: tests/test_gpu_bert_linears.py;
#  * the automatic policy's own choice of a wide tile needs K >= 512 AND more than 256 tiles of 128 x 128 for the two larger tiles: the forced
#    policies run the same instantiations here, tests/test_gpu_igemm.py's full-size shapes the automatic choice.


def test_gpu_table_reaches_every_kernel_family_of_the_launchers(sim):
    """the ENTIRE table of tests/test_gpu_gemm_edges.py through the launchers in dry run, under every tile policy it runs with"""
    log, xcd, patch = [], [], set()
    for policy, dt in [(p, BF16) for p in range(5)] + [(AUTO, F32)]:
        sim.set_tile_policy(policy)
        for case in X.full_table(dt):
            rcs, launches = sim.dispatch(X.build(case, dry=True))
            assert not any(rcs), (X.case_id(case), policy, rcs)
            assert launches, X.case_id(case)
            log += launches
            if policy == AUTO and case.get("slack") == 0 and "conv3x3_patch_kernel" in launches[0][0]:
                patch.add(case["op"])
            if case["shape"] in ((136, 136, 2304), (129, 136, 2304)) and case["form"] in ("atomic", "ws") and not case["det"]:
                xcd.append((X.case_id(case), launches[0][1]))
    names = sorted({n for n, _, _ in log})
    for what, pattern in FAMILIES:
        rx = re.compile(pattern)
        assert any(rx.search(n) for n in names), (what, names)
    assert patch == {"conv_fwd", "conv_dgrad_wt"}          # conv_patch.hip serves the forward and the input gradient on transposed weights
    # the XCD-owned split-K grid: 4 output tiles of 128 x 128 and K = 2304 give 9 (gemm_tn: pick_splits) or 16 (the workspace form and ep.atomic on
    # gemm_nt / _nn: fewtile_want) K splits (gemm_tn with f32 storage, whose K tile is 16: 18), i.e. >= 8: a 1-D grid of 8 * ceil(splits / 8) * tiles = 64 (96) workgroups instead of (4, 1, splits)
    assert len(xcd) >= 12
    for cid, grid in xcd:
        assert grid == ((96 if cid.startswith("gemm_tn-f32-") else 64), 1, 1), (cid, grid)
