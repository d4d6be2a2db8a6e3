"""The CLIP text tower's kernels on the wave simulator (csrc/bert_ops.hip: the causal attention families, token assembly, end-of-text gather /
scatter) through the C ABI: the checks of tests/cliptext_checks.py, shared with tests/test_gpu_cliptext.py, and which kernels the causal and the
non-causal entry points launch. Runs without a GPU.

The simulator takes the shapes of cliptext_checks.SHAPES it runs in seconds - one partial tile, a full tile, the first key of a second tile -
and CLIP's 77 tokens (three tiles) and the 128-token cap (four) on one sample and one or two heads instead of (2, 77, 8) and (2, 128, 4), which
take it a quarter of a minute each: one-tile and multi-tile shapes for the VALU (f32) and for the MFMA (bf16) family alike, and every
wave-specialised body of the bf16 kernels (two, three and four tiles)."""
import ctypes as C

import numpy as np
import pytest
import torch

import cliptext_checks as K
import simlib
from loss_backends import BF16, F32
from simlib import ptr

SIM_SHAPES = [(3, 7, 2), (2, 32, 4), (3, 33, 2), (1, 77, 2), (1, 128, 1)]


@pytest.fixture(scope="module")
def be():
    return K.Sim()


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("B,L,H", SIM_SHAPES)
def test_causal_attention_matches_float64(be, dtype, B, L, H):
    K.check_against_float64(be, dtype, B, L, H)


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("i0", [40, 31])
def test_nothing_behind_a_token_reaches_it(be, dtype, i0):
    """i0 = 40 sits inside the second tile of 77 tokens, i0 = 31 on a tile edge"""
    K.check_causality(be, dtype, 77, i0, B=1, H=1)


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_nothing_behind_a_token_reaches_it_one_tile(be, dtype):
    K.check_causality(be, dtype, 20, 9, B=2, H=1)


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("L", [20, 40])
def test_null_mask_is_the_all_ones_mask(be, dtype, L):
    K.check_null_mask(be, dtype, L, B=1, H=2)


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_last_token_gather_and_scatter(be, dtype):
    K.check_gather_scatter(be, dtype, raw=True)


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_token_assembly(be, dtype):
    K.check_embed(be, dtype)


def test_refusals(be):
    K.check_refusals(be)
    simlib.clear_launch_log()


def test_dispatch(be):
    """The non-causal entry points launch at L = 30 and L = 64 what they launched before the causal kernels existed - the same families, grids and
    blocks, and nothing causal; the causal entries launch their own families by the same length rule, and nothing at 129 tokens."""
    lb = be.L
    B, H = 5, 3
    non_causal = {30: ("attention_mfma_fwd_kernel", "attention_fwd_kernel", ((4, 1, 1), 256), ((8, 1, 1), 128), ((15, 1, 1), 64)),
                  64: ("attention_long_mfma_fwd_kernel", "attention_long_fwd_kernel", ((15, 1, 1), 128), ((15, 1, 1), 128), ((15, 1, 1), 256))}
    causal = {30: ("attention_causal_mfma_fwd_kernel", "attention_causal_fwd_kernel"), 64: ("attention_causal_long_mfma_fwd_kernel", "attention_causal_long_fwd_kernel"),
              77: ("attention_causal_long_mfma_fwd_kernel", "attention_causal_long_fwd_kernel")}
    simlib.set_dry_run(True)
    try:
        for L, (mfma, valu, g_fwd, g_bwd, g_valu) in non_causal.items():
            qkv, ctx = np.zeros((B * L, 3 * H * 64), np.float32), np.zeros((B * L, H * 64), np.float32)
            for dtype, family, grids in [(BF16, mfma, (g_fwd, g_bwd)), (F32, valu, (g_valu, g_valu))]:
                simlib.clear_launch_log()
                assert lb.clite_attention_fwd(dtype, ptr(qkv), None, ptr(ctx), B, L, H, 0.0, 0, 0, None) == 0
                assert lb.clite_attention_bwd(dtype, ptr(qkv), None, ptr(ctx), ptr(qkv), B, L, H, 0.0, 0, 0, None) == 0
                log = simlib.launch_log()
                assert len(log) == 2 and not any("causal" in n for n, _, _ in log), log
                assert family + "<" in log[0][0] and family.replace("fwd", "bwd") + "<" in log[1][0], log
                assert [(g, b) for _, g, b in log] == list(grids), log
        for L, (mfma, valu) in causal.items():
            qkv, ctx = np.zeros((B * L, 3 * H * 64), np.float32), np.zeros((B * L, H * 64), np.float32)
            for dtype, family in [(BF16, mfma), (F32, valu)]:
                simlib.clear_launch_log()
                assert lb.clite_attention_causal_fwd(dtype, ptr(qkv), None, ptr(ctx), B, L, H, None) == 0
                assert lb.clite_attention_causal_bwd(dtype, ptr(qkv), None, ptr(ctx), ptr(qkv), B, L, H, None) == 0
                log = simlib.launch_log()
                assert len(log) == 2 and family in log[0][0] and family.replace("fwd", "bwd") in log[1][0], log
        # the bf16 long kernels: one wave per 32-query tile
        simlib.clear_launch_log()
        qkv = np.zeros((B * 128, 3 * H * 64), np.float32)
        for L in (33, 64, 65, 96, 97, 128):
            assert lb.clite_attention_causal_fwd(BF16, ptr(qkv), None, ptr(qkv), B, L, H, None) == 0
        assert [b for _, _, b in simlib.launch_log()] == [128, 128, 192, 192, 256, 256]
        K.check_refusals(be)
        assert lb.clite_attention_causal_fwd(2, ptr(qkv), None, ptr(qkv), B, 30, H, None) == -1          # no such dtype
        assert lb.clite_attention_causal_fwd(BF16, None, None, ptr(qkv), B, 30, H, None) == -1
        assert lb.clite_attention_causal_bwd(BF16, ptr(qkv), None, None, ptr(qkv), B, 30, H, None) == -1
        assert simlib.launch_log() == []
    finally:
        simlib.set_dry_run(False)
        simlib.clear_launch_log()


# ---------------------------------------------------------------------------------------------------- the executor on the simulator
@pytest.fixture
def sim_hip(monkeypatch):
    from clip_lite_amd import hip
    simlib.build_sim()
    monkeypatch.setattr(hip, "_lib", hip._bind(C.CDLL(simlib.SIM_SO)))
    monkeypatch.setattr(hip, "_allow_host_tensors", True)
    return hip


def test_executor_matches_reference_in_exact_f32(sim_hip):
    """the tower's module tree at simulator size - one layer, 64 wide with one head, 60 ids, 12 positions - with ragged captions padded to 10"""
    holder, sd = K.build_tower(1, "cpu", False, small=(60, 64, 1), context_length=12)
    ids, mask = K.captions([10, 1, 6, 3], 10, vocab=60)
    dfeat = torch.randn(4, 64, generator=torch.Generator().manual_seed(1))
    K.check_tower_f32(holder, sd, 1, 1, ids, mask, dfeat)


def test_tower_launches_the_causal_kernels_only(sim_hip):
    holder, _ = K.build_tower(1, "cpu", False, small=(60, 64, 1), context_length=40)
    ids, mask = K.captions([40, 7], 40, vocab=60)
    simlib.set_dry_run(True)
    simlib.clear_launch_log()
    try:
        holder.text_encoder({"input_ids": ids, "attention_mask": mask}).backward(torch.ones(2, 64))
        names = [n for n, _, _ in simlib.launch_log()]
    finally:
        simlib.set_dry_run(False)
        simlib.clear_launch_log()
    att = [n.split("<")[0].split("::")[-1] for n in names if "attention" in n]
    assert att == ["attention_causal_long_fwd_kernel", "attention_causal_long_bwd_kernel"], att
    for family in ("embed_clip_fwd_kernel", "last_token_gather_kernel", "last_token_scatter_kernel", "embed_bwd_kernel"):
        assert sum(family in n for n in names) == 1, (family, names)
