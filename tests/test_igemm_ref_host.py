"""CPU checks of tests/igemm_ref.py, the float64 references tests/test_gpu_dgrad_epilogue.py holds the BatchNorm-backward dgrad epilogues to: each
function against an independent formulation (float64 autograd of torch.nn.functional.conv2d, explicit loops), then one tiny case per epilogue form
through the wave-simulator build of the kernels (tests/simlib.py; it has 4 resident slots, so a handful of tiles already takes the row-range
persistent schedule) with the SAME reference and the SAME bound functions the GPU file uses, and a dry run of the launchers that pins the kernel each one-tile GPU
case names in its docstring. No GPU needed."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import igemm_ref as IR
from simlib import Bn, Conv, clear_launch_log, from_bf16, launch_log, lib, make_ep, prep, ptr

BF16, F32 = 0, 1


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


# ------------------------------------------------------------------------------------------------ the references themselves
@pytest.mark.parametrize("N,H,W,Cc,K,R,stride,pad", [(2, 5, 6, 16, 8, 1, 1, 0), (3, 9, 7, 8, 16, 1, 2, 0), (2, 6, 7, 8, 8, 3, 1, 1), (2, 9, 7, 8, 16, 3, 2, 1),
                                                      (1, 6, 10, 8, 8, 3, 2, 1)])
def test_dgrad_and_forward_references_match_float64_autograd(N, H, W, Cc, K, R, stride, pad):
    g = torch.Generator().manual_seed(H * W + K)
    w = torch.randn(K, R, R, Cc, generator=g, dtype=torch.float64)
    x = torch.randn(N, H, W, Cc, generator=g, dtype=torch.float64).requires_grad_(True)
    y = F.conv2d(x.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2), stride=stride, padding=pad)
    Ho, Wo = y.shape[2], y.shape[3]
    assert (Ho, Wo) == (IR.conv_out(H, R, stride, pad), IR.conv_out(W, R, stride, pad))
    dy = torch.randn(N, Ho, Wo, K, generator=g, dtype=torch.float64)
    y.backward(dy.permute(0, 3, 1, 2))
    got = IR.dgrad_ref(dy, w, N, H, W, stride, pad)
    assert got.dtype == torch.float64 and got.shape == (N * H * W, Cc)
    assert torch.allclose(got, x.grad.reshape(N * H * W, Cc), rtol=0, atol=1e-12)
    assert torch.allclose(IR.conv_fwd_ref(x.detach(), w, stride, pad), y.detach().permute(0, 2, 3, 1).reshape(-1, K), rtol=0, atol=1e-12)
    # the scales: the same sums over magnitudes, so they dominate the values and equal them on non-negative operands
    S = IR.dgrad_scale(dy, w, N, H, W, stride, pad)
    assert bool((S >= got.abs() - 1e-12).all())
    assert torch.equal(S, IR.dgrad_ref(dy.abs(), w.abs(), N, H, W, stride, pad))
    Sf = IR.conv_fwd_scale(x.detach(), w, stride, pad)
    assert bool((Sf >= IR.conv_fwd_ref(x.detach(), w, stride, pad).abs() - 1e-12).all())
    # low-precision inputs are upcast, not computed in their own type
    assert IR.dgrad_ref(dy.bfloat16(), w.bfloat16(), N, H, W, stride, pad).dtype == torch.float64


def test_subsample_and_scatter_maps_match_explicit_loops():
    N, H, W, Cc = 2, 4, 6, 3
    compact = torch.arange(N * (H // 2) * (W // 2) * Cc, dtype=torch.float32).reshape(-1, Cc) + 1
    full = IR.subsample_expand(compact, N, H, W)
    assert full.dtype == torch.float64 and full.shape == (N * H * W, Cc)
    for n in range(N):
        for h in range(H):
            for w in range(W):
                row = full[(n * H + h) * W + w]
                if h % 2 or w % 2:
                    assert not row.any()
                else:
                    assert torch.equal(row, compact[(n * (H // 2) + h // 2) * (W // 2) + w // 2].double())
    for (Ho, Wo, Hh, Ww, stride, oh, ow) in [(5, 4, 9, 7, 2, 0, 0), (3, 5, 6, 10, 2, 1, 0), (3, 5, 6, 10, 2, 1, 1), (2, 3, 4, 9, 3, 0, 0)]:
        rows = IR.scatter_rows(N, Ho, Wo, Hh, Ww, stride, oh, ow)
        want = [(n * Hh + ho * stride + oh) * Ww + wo * stride + ow for n in range(N) for ho in range(Ho) for wo in range(Wo)]
        assert rows.dtype == torch.int64 and rows.tolist() == want and len(set(want)) == len(want) and max(want) < N * Hh * Ww
    # the four parity classes of a stride-2 grid cover every pixel once
    allrows = torch.cat([IR.scatter_rows(N, 3, 5, 6, 10, 2, ph, pw) for ph in (0, 1) for pw in (0, 1)])
    assert sorted(allrows.tolist()) == list(range(N * 6 * 10))


def test_reductions_epilogue_and_bit_packing_match_loops():
    g = torch.Generator().manual_seed(3)
    M, Cc, R = 37, 16, 3
    stored = torch.randn(M, Cc, generator=g).bfloat16()
    y = (torch.randn(M, Cc, generator=g) + 2).bfloat16()
    stats = torch.randn(R, 3, Cc, generator=g)
    inv = 1.0 / (4 * M)
    red = IR.bn_reductions_ref(stored, y, stats, inv)
    inv32 = float(np.float32(inv))
    for c in range(Cc):
        mean = sum(float(stats[r, 0, c]) for r in range(R)) * inv32
        s1 = sum(float(stored[m, c]) for m in range(M))
        s2 = sum(float(stored[m, c]) * (float(y[m, c]) - mean) for m in range(M))
        sq = sum(float(stored[m, c]) ** 2 for m in range(M))
        assert abs(red.mean[c].item() - mean) < 1e-12
        assert abs(red.S1[c].item() - s1) < 1e-10 and abs(red.S2[c].item() - s2) < 1e-10 and abs(red.Sq[c].item() - sq) < 1e-10
    fwd = IR.bn_reductions_ref(stored)
    assert fwd.S2 is None and torch.equal(fwd.Sq, red.Sq) and torch.equal(fwd.S1, red.S1)
    # epilogue orders, mask sources, scale
    acc, S_acc = torch.randn(M, Cc, generator=g, dtype=torch.float64), torch.rand(M, Cc, generator=g, dtype=torch.float64) + 3
    aux, r, bias = torch.randn(M, Cc, generator=g), torch.randn(M, Cc, generator=g), torch.randn(Cc, generator=g)
    bits = IR.pack_bits(aux > 0)
    assert bits.shape == (M, Cc // 8) and torch.equal(IR.unpack_bits(bits, Cc), aux > 0)
    assert int(bits[0, 0]) == sum((1 << e) for e in range(8) if aux[0, e] > 0)
    for after in (False, True):
        for src in ("bits", "aux"):
            e = IR.epilogue_ref(acc, S_acc, alpha=0.5, bias=bias, bits=bits if src == "bits" else None, aux=aux if src == "aux" else None, residual=r,
                                mask_after_residual=after)
            for m in (0, 5, M - 1):
                for c in (0, 7, Cc - 1):
                    a = 0.5 * acc[m, c].item() + float(bias[c])
                    k = 1.0 if aux[m, c] > 0 else 0.0
                    want = (a + float(r[m, c])) * k if after else a * k + float(r[m, c])
                    assert abs(e.v[m, c].item() - want) < 1e-12 and e.m[m, c].item() == k
                    assert abs(e.S[m, c].item() - (0.5 * S_acc[m, c].item() + abs(float(bias[c])) + abs(float(r[m, c])))) < 1e-12
    e = IR.epilogue_ref(acc, S_acc)
    assert torch.equal(e.v, acc) and torch.equal(e.S, S_acc) and bool((e.m == 1).all())
    # the bound functions reject what they should: one element off by more than the bound, a masked element that is not exactly 0, a wrong sum
    ok = IR.epilogue_ref(acc, S_acc, bits=bits)
    IR.assert_elements("self", ok.v.float(), ok, 64, IR.RHO_F32)
    off = ok.v.clone()
    live = (ok.m == 1).nonzero()[0]
    off[live[0], live[1]] *= 1 + 2.0 ** -7
    with pytest.raises(AssertionError):
        IR.assert_elements("off", off, IR.Epi(ok.v, S_acc * 1e-6, ok.m), 64, IR.RHO_BF16)
    dead = (ok.m == 0).nonzero()[0]
    leak = ok.v.clone()
    leak[dead[0], dead[1]] = 1e-30
    with pytest.raises(AssertionError):
        IR.assert_elements("leak", leak, ok, 64, IR.RHO_BF16)
    IR.assert_reductions("sum", ok.v.sum(0).float(), ok.v.sum(0), ok.v)
    with pytest.raises(AssertionError):
        IR.assert_reductions("sum", (ok.v.sum(0) * (1 + 1e-3)).float(), ok.v.sum(0), ok.v)


# ------------------------------------------------------------------------------------------------ one tiny case per form through the simulator
SENT = 7.0


def _sentinel(shape, dtype):
    return np.full(shape, 0x40E0, np.uint16) if dtype == BF16 else np.full(shape, SENT, np.float32)          # bf16 bits of 7.0


def _vals(buf, f32):
    return buf if f32 else from_bf16(buf)


def _split(total, R):
    """[C] f64 totals -> [R + 1][3][C] f32: rows 0 of replicas 0..R-1 sum to (about) the totals over uneven parts; row 2 and replica R are sentinels."""
    t = np.full((R + 1, 3, total.shape[0]), SENT, np.float32)
    t[:R, :2] = 0
    w = np.arange(1, R + 1, dtype=np.float64) ** 2
    t[:R, 0] = (total[None, :] * (w / w.sum())[:, None]).astype(np.float32)
    return t


def _bn_kernel(form, persistent_grid=None):
    (name, grid, block), = launch_log()
    assert "::igemm_dma_bn_kernel<" in name and f", {form}, false, false, false>(" in name, name
    if persistent_grid is not None:
        assert grid[0] == persistent_grid, (grid, persistent_grid)


def _sim_dgrad(N, H, W, Cc, K, R, stride, pad, *, dtype=BF16, mask="bits", res=None, after=False, out_f32=False, alpha=1.0, rows_factor=1, pad_cols=0, seed=0):
    """One BatchNorm-backward dgrad through the simulator (clite_conv_dgrad_wt), checked like the GPU cases: elements, exact zeros, sentinels, reductions."""
    rng = np.random.default_rng(seed)
    Ho, Wo = IR.conv_out(H, R, stride, pad), IR.conv_out(W, R, stride, pad)
    M, ldc, Rr = N * H * W, Cc + pad_cols, 3
    f32o = out_f32 or dtype == F32
    w, _ = prep(rng.standard_normal((K, R, R, Cc), dtype=np.float32) * 0.2, dtype)
    _, wtb = prep(np.ascontiguousarray(w.transpose(3, 1, 2, 0)), dtype)
    dy, dyb = prep(rng.standard_normal((N, Ho, Wo, K), dtype=np.float32), dtype)
    aux, auxb = prep(rng.standard_normal((M, ldc), dtype=np.float32), dtype)
    bits = np.packbits(aux > 0, axis=-1, bitorder="little")
    y, yb = prep(rng.standard_normal((M, ldc), dtype=np.float32) + 2.0, dtype)
    fst = _split(rows_factor * y[:, :Cc].astype(np.float64).sum(0), Rr)
    inv = 1.0 / (rows_factor * M)
    out = _sentinel((M, ldc), F32 if f32o else BF16)
    r = resb = None
    if res == "full":
        rfull, resb = prep(rng.standard_normal((M, ldc), dtype=np.float32), dtype)
        r = _t(rfull[:, :Cc])
    elif res == "compact":
        rc, resb = prep(rng.standard_normal((N * (H // 2) * (W // 2), ldc), dtype=np.float32), dtype)
        r = IR.subsample_expand(_t(rc[:, :Cc]), N, H, W)
    elif res == "inplace":
        rfull, out = prep(rng.standard_normal((M, ldc), dtype=np.float32), dtype)
        resb, r = out, _t(rfull[:, :Cc].copy())
        old = out.copy()
    dst = _split(np.zeros(Cc), Rr)
    ep = make_ep(out, ldc, out_f32=f32o, alpha=alpha, residual=resb, colsum=dst, relu_bits=bits if mask == "bits" else None,
                 dact_aux=auxb if mask == "aux" else None, dact=1 if mask == "aux" else 0)
    ep.colsum_replicas, ep.colsum_stride = Rr, 3 * Cc
    ep.bn_y, ep.bn_stats, ep.bn_replicas, ep.bn_rstride, ep.bn_inv_count, ep.mask_after_residual = ptr(yb), ptr(fst), Rr, 3 * Cc, inv, int(after)
    ep.residual_subsample = 2 if res == "compact" else 0
    cv = Conv(dtype, N, H, W, Cc, K, R, R, stride, pad, Ho, Wo)
    clear_launch_log()
    assert lib().clite_conv_dgrad_wt(ptr(dyb), ptr(wtb), C.byref(cv), C.byref(ep), None) == 0
    what = f"sim dgrad {N}x{H}x{W} C{Cc} K{K} R{R} s{stride} mask={mask} res={res} after={int(after)}"
    acc, S_acc = IR.dgrad_ref(_t(dy), _t(w), N, H, W, stride, pad), IR.dgrad_scale(_t(dy), _t(w), N, H, W, stride, pad)
    e = IR.epilogue_ref(acc, S_acc, alpha=alpha, bits=_t(bits) if mask == "bits" else None, aux=_t(aux[:, :Cc]) if mask == "aux" else None, residual=r,
                        mask_after_residual=after)
    got = _t(_vals(out, f32o)[:, :Cc])
    IR.assert_elements(what, got, e, R * R * K, IR.RHO_F32 if f32o else IR.RHO_BF16)
    if pad_cols:
        keep = old[:, Cc:] if res == "inplace" else _sentinel((M, pad_cols), F32 if f32o else BF16)
        assert np.array_equal(out[:, Cc:], keep), "columns [C, ldc) were written"
    red = IR.bn_reductions_ref(got, _t(y[:, :Cc]), _t(fst[:Rr]), inv)
    tot = _t(dst[:Rr].astype(np.float64).sum(0).astype(np.float32))
    IR.assert_reductions(what + " S1", tot[0], red.S1, red.t1)
    IR.assert_reductions(what + " S2", tot[1], red.S2, red.t2)
    assert (dst[:Rr, 2] == SENT).all() and (dst[Rr] == SENT).all(), "statistics rows beyond the two sums were written"


def _policy(p):
    assert lib().clite_set_tile_policy(p) == 0


@pytest.fixture
def auto_policy():
    _policy(0)
    yield
    _policy(0)


def test_sim_form0_runtime_flags(auto_policy):
    """FORM 0: the tensor mask before the residual, alpha = 0.5, f32 store of bf16 operands; 256 x 64 tile family (C = 40), two row tiles."""
    _sim_dgrad(2, 10, 15, 40, 32, 1, 1, 0, mask="aux", res="full", after=False, out_f32=True, alpha=0.5, seed=1)
    _bn_kernel(0)


@pytest.mark.parametrize("policy", [0, 1])
def test_sim_form1_ragged_columns(policy):
    """FORM 1 at C = 136, ldc = C + 8 (a column tile with 8 live columns), M = 189 (a partial row tile); policy 1: wide_epilogue_bn."""
    _policy(policy)
    try:
        _sim_dgrad(3, 9, 7, 136, 96, 1, 1, 0, pad_cols=8, seed=2)
        if policy == 0:
            _bn_kernel(1)
        else:
            (name, _, block), = launch_log()
            assert "igemm_wide_kernel<" in name and block == 512, name
    finally:
        _policy(0)


def test_sim_form2_in_place_stem_count_row_range_schedule(auto_policy):
    """FORM 2 in place (residual is the output) with bn_inv_count = 1 / (4 M), 1100 rows of 40 columns: 5 tiles of 256 x 64 > 4 slots, so 4 workgroups
    walk 280 rows each (260 the last): a full tile and a partial one of 24 rows (4 in the last range)."""
    _sim_dgrad(1, 20, 55, 40, 32, 1, 1, 0, res="inplace", after=True, rows_factor=4, pad_cols=8, seed=3)
    _bn_kernel(2, persistent_grid=4)


def test_sim_form3_subsampled_residual_row_range_schedule(auto_policy):
    """FORM 3, (3, 10, 14) x 136: 4 x 2 tiles > 4 slots -> 2 ranges of 216 / 204 rows per column tile (128 + a partial tile)."""
    _sim_dgrad(3, 10, 14, 136, 64, 1, 1, 0, res="compact", after=True, seed=4)
    _bn_kernel(3, persistent_grid=4)


def test_sim_form5_folded_batchnorm_backward(auto_policy):
    """FORM 5 (clite_conv_dgrad_bnfold): acc = [dz | y] against the prepared weights w2 [Cin][2][K] (slot 0 multiplies y, slot 1 dz), + the constant
    row, masked by the bits. The reference is evaluated on the w2 / bias clite_bn_fold_prepare stored."""
    rng = np.random.default_rng(5)
    M, K, Cin, Rr = 300, 64, 40, 3
    L = lib()
    a, _ = prep(np.maximum(rng.standard_normal((M, Cin), dtype=np.float32) + 0.3, 0), BF16)
    Wv, Wb = prep(rng.standard_normal((K, Cin), dtype=np.float32) * (2.0 / Cin) ** 0.5, BF16)
    y, yb = prep(a @ Wv.T + 0.5, BF16)
    dz, dzb = prep((rng.standard_normal((M, K), dtype=np.float32) * 0.1) * (rng.random((M, K)) > 0.4), BF16)
    gamma = (rng.random(K) + 0.5).astype(np.float32)
    st = np.zeros((Rr, 3, K), np.float32)
    st[:, 0], st[:, 1] = y.sum(0) / Rr, (y * y).sum(0) / Rr
    mean = y.astype(np.float64).mean(0)
    pre = np.zeros((Rr, 3, K), np.float32)
    pre[:, 0], pre[:, 1] = dz.astype(np.float64).sum(0) / Rr, (dz * (y - mean)).astype(np.float64).sum(0) / Rr
    y2, y2b = prep(rng.standard_normal((M, Cin), dtype=np.float32) + 2.0, BF16)
    st2 = _split(y2.astype(np.float64).sum(0), Rr)
    bits = np.packbits(rng.random((M, Cin)) > 0.3, axis=-1, bitorder="little")
    pair = np.concatenate([dzb.reshape(1, M, K), yb.reshape(1, M, K)], axis=0).copy()
    Wt = np.ascontiguousarray(Wb.T)
    w2, bias, coef = np.zeros((Cin, 2, K), np.uint16), np.zeros(Cin, np.float32), np.zeros((3, K), np.float32)
    dgamma, dbeta = np.zeros(K, np.float32), np.zeros(K, np.float32)
    rm, rv = np.zeros(K, np.float32), np.ones(K, np.float32)
    p = Bn(M, K, ptr(st), ptr(gamma), ptr(np.zeros(K, np.float32)), ptr(rm), ptr(rv), 1, 0, 0.1, 1e-5, 0, Rr, 3 * K, 0)
    L.clite_bn_fold_prepare.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 6
    assert L.clite_bn_fold_prepare(C.byref(p), ptr(pre), ptr(Wt), Cin, ptr(w2), ptr(bias), ptr(coef), ptr(dgamma), ptr(dbeta), None) == 0
    dz2 = _sentinel((M, Cin), BF16)
    d2 = _split(np.zeros(Cin), Rr)
    ep = make_ep(dz2, Cin, bias=bias, colsum=d2, relu_bits=bits)
    ep.colsum_replicas, ep.colsum_stride = Rr, 3 * Cin
    ep.bn_y, ep.bn_stats, ep.bn_replicas, ep.bn_rstride, ep.bn_inv_count = ptr(y2b), ptr(st2), Rr, 3 * Cin, 1.0 / M
    L.clite_conv_dgrad_bnfold.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    clear_launch_log()
    assert L.clite_conv_dgrad_bnfold(ptr(pair), ptr(w2), M, K, Cin, C.byref(ep), None) == 0
    _bn_kernel(5)
    w2v = _t(from_bf16(w2)).double()
    acc = _t(y).double() @ w2v[:, 0].t() + _t(dz).double() @ w2v[:, 1].t()
    S_acc = _t(y).double().abs() @ w2v[:, 0].abs().t() + _t(dz).double().abs() @ w2v[:, 1].abs().t()
    e = IR.epilogue_ref(acc, S_acc, bias=_t(bias), bits=_t(bits))
    got = _t(from_bf16(dz2))
    IR.assert_elements("sim fold dz2", got, e, 2 * K, IR.RHO_BF16)
    red = IR.bn_reductions_ref(got, _t(y2), _t(st2[:Rr]), 1.0 / M)
    tot = _t(d2[:Rr].astype(np.float64).sum(0).astype(np.float32))
    IR.assert_reductions("sim fold S1", tot[0], red.S1, red.t1)
    IR.assert_reductions("sim fold S2", tot[1], red.S2, red.t2)
    assert (d2[:Rr, 2] == SENT).all() and (d2[Rr] == SENT).all()


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_sim_in_place_scatter_add(auto_policy, dtype):
    """1 x 1 / stride 2 dgrad accumulated in place (residual is the output): the dense GEMM over the 3 x 5 x 4 output pixels scattered through RowMap;
    on-lattice pixels = old + dgrad, every other pixel and the columns [C, ldc) keep their bits."""
    rng = np.random.default_rng(6)
    N, H, W, Cc, K, ldc = 3, 9, 7, 40, 32, 48
    Ho, Wo = 5, 4
    w, _ = prep(rng.standard_normal((K, 1, 1, Cc), dtype=np.float32) * 0.2, dtype)
    _, wtb = prep(np.ascontiguousarray(w.transpose(3, 1, 2, 0)), dtype)
    dy, dyb = prep(rng.standard_normal((N, Ho, Wo, K), dtype=np.float32), dtype)
    oldv, dx = prep(rng.standard_normal((N * H * W, ldc), dtype=np.float32), dtype)
    old, oldv = dx.copy(), oldv.copy()
    cv = Conv(dtype, N, H, W, Cc, K, 1, 1, 2, 0, Ho, Wo)
    assert lib().clite_conv_dgrad_wt(ptr(dyb), ptr(wtb), C.byref(cv), C.byref(make_ep(dx, ldc, residual=dx)), None) == 0
    rows = IR.scatter_rows(N, Ho, Wo, H, W, 2)
    acc, S_acc = IR.dgrad_ref(_t(dy), _t(w), N, H, W, 2, 0), IR.dgrad_scale(_t(dy), _t(w), N, H, W, 2, 0)
    e = IR.epilogue_ref(acc[rows], S_acc[rows], residual=_t(oldv[:, :Cc])[rows])
    got = _t(_vals(dx, dtype == F32))
    IR.assert_elements("sim scatter", got[rows][:, :Cc], e, K, IR.RHO_F32 if dtype == F32 else IR.RHO_BF16)
    off = np.ones(N * H * W, bool)
    off[rows.numpy()] = False
    assert not acc[torch.from_numpy(off)].any()          # the reference agrees that those pixels receive nothing
    assert np.array_equal(dx[off], old[off]) and np.array_equal(dx[:, Cc:], old[:, Cc:])


def test_sim_form4_forward_row_range_schedule(auto_policy):
    """FORM 4: conv_fwd 1 x 1, 32 -> 136, 585 rows: 5 x 2 tiles > 8 -> 2 ranges of 296 / 289 rows per column tile (two full tiles and a partial one).
    bf16 store, statistics = sum and sum of squares of the stored values."""
    rng = np.random.default_rng(7)
    N, H, W, Cc, K, Rr = 3, 13, 15, 32, 136, 3
    M = N * H * W
    x, xb = prep(rng.standard_normal((N, H, W, Cc), dtype=np.float32), BF16)
    w, wb = prep(rng.standard_normal((K, 1, 1, Cc), dtype=np.float32) * 0.2, BF16)
    out = _sentinel((M, K + 8), BF16)
    cs = _split(np.zeros(K), Rr)
    ep = make_ep(out, K + 8, colsum=cs)
    ep.colsum_replicas, ep.colsum_stride = Rr, 3 * K
    cv = Conv(BF16, N, H, W, Cc, K, 1, 1, 1, 0, H, W)
    clear_launch_log()
    assert lib().clite_conv_fwd(ptr(xb), ptr(wb), C.byref(cv), C.byref(ep), None) == 0
    _bn_kernel(4, persistent_grid=4)
    e = IR.epilogue_ref(IR.conv_fwd_ref(_t(x), _t(w), 1, 0), IR.conv_fwd_scale(_t(x), _t(w), 1, 0))
    got = _t(from_bf16(out)[:, :K])
    IR.assert_elements("sim fwd", got, e, Cc, IR.RHO_BF16)
    assert (out[:, K:] == 0x40E0).all()
    red = IR.bn_reductions_ref(got)
    tot = _t(cs[:Rr].astype(np.float64).sum(0).astype(np.float32))
    IR.assert_reductions("sim fwd sum", tot[0], red.S1, red.t1)
    IR.assert_reductions("sim fwd sumsq", tot[1], red.Sq, red.tq)
    assert (cs[:Rr, 2] == SENT).all() and (cs[Rr] == SENT).all()


# ------------------------------------------------------------------------------------------------ the kernel each GPU case names
def _dry_kernel(dtype, shape, policy, **flags):
    """Kernel instantiation clite_conv_dgrad_wt selects for the BatchNorm-backward epilogue with `flags` (dry run: logged, not executed)."""
    from simlib import set_dry_run
    N, H, W, Cc, K, R, stride, pad = shape
    z = np.zeros(16, np.float32)
    ep = make_ep(z, Cc, out_f32=flags.get("out_f32", False), alpha=flags.get("alpha", 1.0), residual=z if flags.get("res") else None, colsum=z,
                 relu_bits=None if flags.get("aux") else z, dact_aux=z if flags.get("aux") else None, dact=1 if flags.get("aux") else 0)
    ep.colsum_replicas, ep.colsum_stride = 3, 3 * Cc
    ep.bn_y, ep.bn_stats, ep.bn_replicas, ep.bn_rstride, ep.bn_inv_count, ep.mask_after_residual = ptr(z), ptr(z), 3, 3 * Cc, 0.5, int(flags.get("after", False))
    ep.residual_subsample = 2 if flags.get("res") == "compact" else 0
    cv = Conv(dtype, N, H, W, Cc, K, R, R, stride, pad, IR.conv_out(H, R, stride, pad), IR.conv_out(W, R, stride, pad))
    _policy(policy)
    set_dry_run(True)
    try:
        clear_launch_log()
        assert lib().clite_conv_dgrad_wt(ptr(z), ptr(z), C.byref(cv), C.byref(ep), None) == 0
        (name, _, block), = launch_log()
    finally:
        set_dry_run(False)
        _policy(0)
    if "igemm_wide_kernel<" in name:
        assert block == 512
        return "wide"
    assert "::igemm_dma_bn_kernel<" in name and block == 256, name
    return next(f for f in (0, 1, 2, 3, 5) if f", {f}, false, false, false>(" in name)


@pytest.mark.parametrize("policy", [0, 1, 2, 3, 4])
def test_gpu_cases_select_the_kernel_their_docstring_names(policy):
    """The FORM / kernel family tests/test_gpu_dgrad_epilogue.py states for its one-tile cases, from the launchers themselves (form selection and the
    hand-over to the 8-wave kernels do not depend on the number of resident slots, which is all the simulator build changes)."""
    A1, A3, A5, A6 = (3, 9, 7, 136, 96, 1, 1, 0), (3, 10, 14, 136, 64, 1, 1, 0), (3, 10, 10, 40, 96, 1, 1, 0), (2, 9, 7, 96, 64, 3, 1, 1)
    wide = policy in (1, 2, 3)
    want = lambda form: "wide" if wide else form
    assert _dry_kernel(BF16, A1, policy) == want(1)
    assert _dry_kernel(BF16, A1, policy, res="full", after=True) == want(2)
    assert _dry_kernel(BF16, A3, policy, res="compact", after=True) == 3                    # rm.on == 2: never wide
    assert _dry_kernel(BF16, A1, policy, res="full") == want(0)
    assert _dry_kernel(BF16, A1, policy, res="full", aux=True) == want(0)
    assert _dry_kernel(BF16, A1, policy, res="full", aux=True, after=True) == want(0)
    assert _dry_kernel(BF16, A1, policy, out_f32=True) == want(0)
    assert _dry_kernel(BF16, A1, policy, alpha=0.5) == want(0)
    assert _dry_kernel(BF16, A5, policy) == 1 and _dry_kernel(BF16, A5, policy, res="full", after=True) == 2          # 256 x 64 tiles: never wide
    assert _dry_kernel(BF16, A6, policy) == ("wide" if policy != 4 else 1)                  # Ktot = 576: wide under the automatic policy too
    assert _dry_kernel(BF16, A6[:6] + (2, 1), policy, res="full", after=True) == ("wide" if policy != 4 else 2)
    assert _dry_kernel(F32, A1, policy) == 0 and _dry_kernel(F32, A3, policy, res="compact", after=True) == 0
