"""CPU-side (wave simulator) checks of the attention kernels for 33..128 tokens (csrc/bert_ops.hip, attention_long_{fwd,bwd}_kernel on the VALU in
exact f32 and attention_long_mfma_{fwd,bwd}_kernel in bf16) against tests/attention_long_ref.py in float64. Runs without a GPU.

Every buffer has exactly B*L rows, so a read or write past row L of the last sample leaves the array. Bounds are those of tests/test_gpu_ops.py:
1e-5 of max|ref| in f32; in bf16 1e-2 forward and 2e-2 backward. The bf16 bounds are first checked against the rounding emulation alone at the cap
(test_bf16_emulation_alone_is_inside_the_bounds): at (1, 128, 2) the emulation's error is 3.0e-3 forward and 3.5e-3 backward, inside the bounds, so
they stand as they are."""
import ctypes as C

import numpy as np
import pytest
import torch

import attention_long_ref as R
import simlib
from simlib import lib, outbuf, ptr, to_bf16, val

BF16, F32 = 0, 1
V, I, F, U64, U32 = C.c_void_p, C.c_int, C.c_float, C.c_uint64, C.c_uint32
FWD_SIG = [I, V, V, V, I, I, I, F, U64, U32, V]
BWD_SIG = [I, V, V, V, V, I, I, I, F, U64, U32, V]
TOL = {BF16: (1e-2, 2e-2), F32: (1e-5, 1e-5)}
SHAPES = [(2, 33, 2), (1, 64, 1), (2, 97, 3), (1, 128, 2)]      # one key past a tile; an exact tile boundary; a ragged last tile; the cap


def _lib():
    L = lib()
    L.clite_attention_fwd.argtypes = FWD_SIG
    L.clite_attention_bwd.argtypes = BWD_SIG
    return L


def _problem(B, L, H, seed):
    """bf16-representable inputs (both dtypes see the same values): qkv, dctx as float32 tensors, and the ragged mask"""
    g = torch.Generator().manual_seed(seed)
    qkv = (torch.randn(B * L, 3 * H * 64, generator=g) * 0.7).bfloat16().float()
    dctx = torch.randn(B * L, H * 64, generator=g).bfloat16().float()
    return qkv, dctx, R.masks(B, L, seed)


def _buf(x, dtype):
    a = np.ascontiguousarray(x.numpy(), np.float32)
    return to_bf16(a) if dtype == BF16 else a


def _run(dtype, qkv, mask, dctx, B, L, H, drop=(0.0, 0, 0), backward=True):
    lb = _lib()
    qb, mb = _buf(qkv, dtype), np.ascontiguousarray(mask.numpy(), np.int64)
    ctx = outbuf((B * L, H * 64), dtype)
    assert lb.clite_attention_fwd(dtype, ptr(qb), ptr(mb), ptr(ctx), B, L, H, *drop, None) == 0
    dqkv = None
    if backward:
        dob = _buf(dctx, dtype)
        dqkv = outbuf((B * L, 3 * H * 64), dtype)
        assert lb.clite_attention_bwd(dtype, ptr(qb), ptr(mb), ptr(dob), ptr(dqkv), B, L, H, *drop, None) == 0
        dqkv = torch.tensor(val(dqkv, dtype))
    return torch.tensor(val(ctx, dtype)), dqkv


def test_bf16_emulation_alone_is_inside_the_bounds():
    """Exact arithmetic with only the kernels' bf16 roundings, at the cap: what no bf16 kernel of this scheme can beat."""
    B, L, H = 1, 128, 2
    qkv, dctx, mask = _problem(B, L, H, 128)
    ref_ctx, ref_dqkv = R.reference(qkv, mask, dctx, B, L, H)
    emu_ctx, emu_dqkv = R.emulate_bf16(qkv, mask, dctx, B, L, H)
    ef, eb = R.rel_err(emu_ctx, ref_ctx), R.rel_err(emu_dqkv, ref_dqkv)
    print(f"bf16 emulation at L = 128: forward {ef:.3e}, backward {eb:.3e}")
    assert ef < TOL[BF16][0] and eb < TOL[BF16][1]


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("B,L,H", SHAPES)
def test_forward_and_backward_match_float64(dtype, B, L, H):
    qkv, dctx, mask = _problem(B, L, H, L)
    ref_ctx, ref_dqkv = R.reference(qkv, mask, dctx, B, L, H)
    ctx, dqkv = _run(dtype, qkv, mask, dctx, B, L, H)
    ef, eb = R.rel_err(ctx, ref_ctx), R.rel_err(dqkv, ref_dqkv)
    print(f"dtype {dtype} (B, L, H) = {(B, L, H)}: forward {ef:.3e}, backward {eb:.3e}")
    assert ef < TOL[dtype][0]
    assert eb < TOL[dtype][1]


def test_dispatch_by_length():
    """L <= 32 launches the kernels it always launched, 33 the new family, 129 nothing; the MPNet entry point keeps its 32-token limit."""
    lb = _lib()
    lb.clite_attention_bias_fwd.argtypes = FWD_SIG[:3] + [V] + FWD_SIG[3:]
    B, H = 2, 2
    simlib.set_dry_run(True)
    try:
        for L, mfma, valu in [(30, "attention_mfma_fwd_kernel", "attention_fwd_kernel"), (32, "attention_mfma_fwd_kernel", "attention_fwd_kernel"),
                              (33, "attention_long_mfma_fwd_kernel", "attention_long_fwd_kernel")]:
            qkv = np.zeros((B * L, 3 * H * 64), np.float32)
            ctx = np.zeros((B * L, H * 64), np.float32)
            for dtype, family in [(BF16, mfma), (F32, valu)]:
                simlib.clear_launch_log()
                assert lb.clite_attention_fwd(dtype, ptr(qkv), None, ptr(ctx), B, L, H, 0.0, 0, 0, None) == 0
                log = simlib.launch_log(clear=False)
                assert len(log) == 1 and len(simlib.launched(family)) == 1, log
                assert lb.clite_attention_bwd(dtype, ptr(qkv), None, ptr(ctx), ptr(qkv), B, L, H, 0.0, 0, 0, None) == 0
                assert len(simlib.launched(family.replace("fwd", "bwd"))) == 1, simlib.launch_log(clear=False)
        # the 32-token grids and blocks, untouched: four (batch, head) pairs per 256-thread workgroup forward, two per 128 backward
        simlib.clear_launch_log()
        lb.clite_attention_fwd(BF16, ptr(qkv), None, ptr(ctx), 5, 30, 3, 0.0, 0, 0, None)
        lb.clite_attention_bwd(BF16, ptr(qkv), None, ptr(ctx), ptr(qkv), 5, 30, 3, 0.0, 0, 0, None)
        assert [(g, b) for _, g, b in simlib.launch_log()] == [((4, 1, 1), 256), ((8, 1, 1), 128)]
        simlib.clear_launch_log()
        big = np.zeros((B * 129, 3 * H * 64), np.float32)
        for dtype in (BF16, F32):
            assert lb.clite_attention_fwd(dtype, ptr(big), None, ptr(big), B, 129, H, 0.0, 0, 0, None) == -1
            assert lb.clite_attention_bwd(dtype, ptr(big), None, ptr(big), ptr(big), B, 129, H, 0.0, 0, 0, None) == -1
            assert lb.clite_attention_bias_fwd(dtype, ptr(big), None, ptr(big), ptr(big), B, 33, H, 0.0, 0, 0, None) == -1
        assert simlib.launch_log() == []
    finally:
        simlib.set_dry_run(False)
        simlib.clear_launch_log()


@pytest.fixture(scope="module")
def dropped():
    """(2, 80, 2), p = 0.1: the multipliers recovered from the exact-f32 forward through two one-hot probes of V (keys 0..63, then 64..79)."""
    B, L, H, p = 2, 80, 2, 0.1
    drop = (p, 1234567, 9)
    qkv, dctx, _ = _problem(B, L, H, 80)
    mask = torch.ones(B, L, dtype=torch.long)
    mask[1, 72:] = 0
    outs = []
    for j0 in (0, 64):
        probe = R.one_hot_probe(qkv, B, L, H, j0)
        outs.append(_run(F32, probe, mask, dctx, B, L, H, drop, backward=False)[0])
        outs.append(_run(F32, probe, mask, dctx, B, L, H, backward=False)[0])
    mult, seen = R.multipliers(outs[0], outs[1], outs[2], outs[3], B, L, H, p)
    return B, L, H, drop, qkv, dctx, mask, mult, seen


def test_dropout_multipliers_are_zero_or_scale(dropped):
    B, L, H, drop, _, _, _, mult, seen = dropped
    assert mult.numel() == 25600
    assert (((mult - 1 / 0.9).abs() < 1e-3) | (mult.abs() < 1e-6)).all()
    keep = (mult > 0.5).double().mean().item()
    print(f"keep rate {keep:.4f} over {mult.numel()} draws ({int(seen.sum())} observable)")
    assert abs(keep - 0.9) < 0.02


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_dropout_same_mask_in_both_families_and_directions(dropped, dtype):
    """The float64 reference with the mask recovered from the f32 forward matches forward AND backward of both families."""
    B, L, H, drop, qkv, dctx, mask, mult, _ = dropped
    keep = (mult > 0.5).double() / 0.9
    ref_ctx, ref_dqkv = R.reference(qkv, mask, dctx, B, L, H, keep=keep)
    ctx, dqkv = _run(dtype, qkv, mask, dctx, B, L, H, drop)
    ef, eb = R.rel_err(ctx, ref_ctx), R.rel_err(dqkv, ref_dqkv)
    print(f"dropout, dtype {dtype}: forward {ef:.3e}, backward {eb:.3e}")
    assert ef < TOL[dtype][0]
    assert eb < TOL[dtype][1]


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_backward_is_bit_exact_across_runs(dtype):
    B, L, H = 2, 97, 3
    qkv, dctx, mask = _problem(B, L, H, 5)
    a = _run(dtype, qkv, mask, dctx, B, L, H, (0.1, 42, 3))
    b = _run(dtype, qkv, mask, dctx, B, L, H, (0.1, 42, 3))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.isfinite(a[1]).all()
