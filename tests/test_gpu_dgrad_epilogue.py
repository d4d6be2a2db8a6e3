"""GPU checks of the BatchNorm-backward dgrad epilogues (csrc/igemm.h igemm_epilogue_bn FORM 0 - 5 inside csrc/igemm_dma.h igemm_dma_bn_kernel, one
tile per workgroup and row-range persistent; csrc/igemm_wide.h wide_epilogue_bn; csrc/gemm.hip colstats_det_kernel) and of the in-place / scattered
generic epilogue, through clip_lite_amd.hip as the executor calls it, against the float64 references of tests/igemm_ref.py evaluated on the SAME
storage-rounded operands (made on the GPU, copied to the CPU). tests/test_igemm_ref_host.py validates those references and runs the same checks
through the wave simulator.

Every case: elements |got - v| <= rho |v| + Ktot 2^-23 S (rho = 2^-8 bf16 / 2^-23 f32 storage; derivation in igemm_ref.py), exactly 0 where the mask
bit is 0, everything finite; untouched memory (columns [C, ldc), off-lattice pixels, statistics row 2 and the replica past the last) keeps its
sentinel bit-exactly; reductions of the STORED tensor per channel within 1e-4 max|ref|. No element is excluded. Outputs are prefilled with 7.0,
bn_y is offset by +2, the forward statistics arrive split unevenly (1 : 4 : 9) over 3 replicas. bf16 cases pass the transposed weight copy (wt=True).

Which device path each case takes (csrc/gemm.hip with_cols / launch / launch_bn_dgrad / launch_persistent_fwd / row_slices, csrc/gemm_wide.hip
launch_wide). Tiles: <= 64 output columns -> 256 x 64, otherwise 128 x 128. Policy 0 sends nothing here to the 8-wave kernels except A6 (every
other K < 512); policies 1 / 2 / 3 force the 128 x 128 / 256 x 128 / 256 x 256 wide tile (wide_epilogue_bn, run-time flags) wherever launch_wide
admits the launch: 128-column tile family only, not rm.on == 2 (A3 / B3), not f32; policy 4 keeps the 4-wave kernels. On the 4-wave kernel the
FORM is 1 (bits + bn), 2 (+ residual, mask after), 3 (+ subsampled residual), 5 (+ bias) for bf16 storage, transposed weights, alpha = 1; 0 otherwise.
  A1  (3,9,7) K 96 -> C 136, ldc 144   M = 189: 2 row tiles (128 + 61) x 2 column tiles (128 + 8 live columns) = 4 workgroups. FORM 1.
  A2  A1 + residual, mask after        FORM 2. Same tiles.
  A3  (3,10,14) K 64 -> C 136          M = 420: 4 row tiles (3 x 128 + 36) x 2. FORM 3 under EVERY policy (rm.on == 2 is refused by launch_wide).
  A4  A1's geometry, FORM 0            before: bits, mask before the residual; aux0 / aux1: dact_aux mask before / after the residual; f32out: out_f32
                                       on bf16 operands; alpha: alpha = 0.5. Each fails one condition of launch_bn_dgrad's form selection.
  A5  (3,10,10) K 96 -> C 40, ldc 48   M = 300: 256 x 64 tiles, 2 row tiles (256 + 44) x 1 with 40 live columns. 4-wave under every policy (launch_on_wide
                                       takes the 128 x 128 family only). FORMs 1 and 2.
  A6  (2,9,7) K 64 -> C 96, 3 x 3      M = 126, Ktot = 576: one partial 128 x 128 tile. Policy 0: Ktot >= 512 and one round of tiles -> the 128 x 128 wide
                                       kernel; policy 4: 4-wave FORM 1 / 2, the windowed gather (stride 1 pad 1; stride 2 pad 1 -> Ho x Wo = 5 x 4).
  A7  A1, A2, A3 in f32                T = float: FORM 0 of the 4-wave kernel (launch_on_wide and the forms are bf16 only), BK = 16.
  A8  fold, M 300, K 64 (Ktot 128)     Cin 136: 3 x 2 tiles (128, 128, 44 rows), FORM 5 / wide under 1 - 3; Cin 40: 2 tiles of 256 x 64 (256 + 44), FORM 5.
  B   row-range persistent (tiles > 512, R S == 1 or the fold's concat gather, not deterministic); policies 0 and 4 take the same kernel (K < 512).
  B1  (21,57,55) K 64 -> C 128         M = 65835: 515 x 1 tiles; row_slices -> 136 rows per workgroup, 485 workgroups: a full tile + a partial one of 8 rows
                                       (the last range: 11 rows). FORM 1.
  B2  (11,55,57) K 64 -> C 256         M = 34485: 270 x 2 tiles; 136 rows per workgroup, 254 x 2 workgroups: 128 + 8 rows (last range 77). FORM 2.
  B3  (12,54,56) K 64 -> C 256         M = 36288: 284 x 2 tiles; 144 rows per workgroup, 252 x 2 workgroups: 128 + 16 rows. FORM 3.
  B4  fold, M 65835, K 64, Cin 128     515 tiles, as B1 with Ktot = 128. FORM 5 (launch_fold_dgrad_rows serves K = 256, Cin = 64 only).
  B5  (42,56,56) K 256 -> C 64         the stem form: M = 131712 -> 515 tiles of 256 x 64; 264 rows per workgroup, 499 workgroups: 256 + 8 rows (last range
                                       240). FORM 2 with residual = out (in place), bn = (ymax, stats, 4 M): bn_inv_count != 1 / M.
  B6  forward, tiles > 1024, Ktot = 64 (2 K tiles). Policy 0: FORM 4 on the row ranges below; policy 4 (launch_persistent_fwd asks for the automatic
      policy): one tile per workgroup on igemm_dma_kernel's 3-stage ring with the plain-store epilogue (EPI 2).
      (21,57,55) 64 -> 256             M = 65835: 515 x 2 tiles; 264 rows per workgroup, 250 x 2 workgroups: 128 + 128 + 8 rows
      (84,56,56) 64 -> 64              M = 263424: 1029 tiles of 256 x 64; 520 rows per workgroup, 507 workgroups: 256 + 256 + 8 rows
      (84,56,56) 64 -> 256 stride 2    M = 65856 output pixels: 515 x 2 tiles; 264 rows per workgroup, 250 x 2 workgroups, the strided gather
  C1  (3,9,7) K 96 -> C 136            generic epilogue (igemm_epilogue / the wide kernels' run-time form under 1 - 3), dx += dgrad in place, dense.
  C2  (3,9,7) -> 5 x 4, 1 x 1 stride 2 conv_dgrad's scatter form: the dense GEMM over the 60 output pixels, rows mapped by RowMap (on = 1); C 136: one row
                                       tile x 2 column tiles; C 40: one 256 x 64 tile. ldc = C + 8.
  C3  (2,6,10), 3 x 3 s2 p1, K 128     conv_dgrad_s2: four class launches of 30 rows each (Ktot = 128 / 256 / 256 / 512), RowMap with offsets, FORM 1 (C 64:
                                       256 x 64 tile; C 128: 128 x 128, wide under 1 - 3 and, for the class with Ktot = 512, under policy 0 too).
  D   deterministic mode: the same launches with colsum taken away + colstats_det_kernel over the stored tensor (C3: through the RowMap; C2 with colsum
      leaves the scatter form for the dense gather over all 189 pixels, in place). One tile per workgroup always (launch_bn_dgrad excludes it from the row ranges).

Measured on an MI355X (`pytest -s`, the REDERR lines): max over each group's cases and channels of |got - ref| / sum|terms|, kernel / plain torch.float32
.sum(0) of the same terms (neither figure feeds a bound; the bound 1e-4 max|ref| is 1e-6 .. 1e-5 on this scale):
  A1, A4-f32out, A4-alpha    S1 5.7e-08 / 5.5e-08   S2 9.5e-08 / 6.1e-08
  A2                         S1 0 / 0   S2 8.2e-08 / 5.9e-08
  A3                         S1 4.6e-09 / 4.6e-09   S2 3.7e-08 / 2.9e-08
  A4-before                  S1 8.3e-09 / 8.3e-09   S2 5.9e-08 / 5.9e-08
  A4-aux0                    S1 0 / 0   S2 7.4e-08 / 3.9e-08
  A4-aux1                    S1 3.0e-09 / 3.0e-09   S2 6.9e-08 / 4.5e-08
  A5 FORM 1                  S1 8.8e-09 / 8.8e-09   S2 4.9e-08 / 2.9e-08
  A5 FORM 2                  S1 0 / 0   S2 5.0e-08 / 4.1e-08
  A6 s1 FORM 1               S1 0 / 0   S2 9.7e-08 / 5.9e-08
  A6 s1 FORM 2               S1 5.3e-09 / 5.3e-09   S2 8.6e-08 / 5.3e-08
  A6 s2 FORM 1               S1 0 / 0   S2 1.1e-07 / 6.1e-08
  A7 A1 f32                  S1 3.2e-08 / 5.1e-08   S2 5.5e-08 / 5.5e-08
  A7 A2 f32                  S1 3.4e-08 / 4.8e-08   S2 6.6e-08 / 4.0e-08
  A7 A3 f32                  S1 2.0e-08 / 3.0e-08   S2 4.4e-08 / 3.0e-08
  A8 Cin 136                 S1 3.9e-09 / 3.0e-09   S2 4.6e-08 / 3.4e-08
  A8 Cin 40                  S1 2.8e-09 / 2.8e-09   S2 5.2e-08 / 2.9e-08
  B1                         S1 3.6e-09 / 3.0e-09   S2 6.7e-09 / 4.4e-09
  B2                         S1 2.6e-09 / 3.0e-09   S2 1.2e-08 / 7.2e-09
  B3                         S1 2.6e-09 / 2.0e-09   S2 1.3e-08 / 5.2e-09
  B4                         S1 2.6e-09 / 1.0e-09   S2 7.0e-09 / 3.4e-09
  B5                         S1 1.7e-09 / 1.5e-09   S2 4.4e-09 / 2.6e-09
  B6 (21,57,55) 64 -> 256    sum 3.1e-09 / 1.6e-09   sumsq 3.2e-07 / 2.1e-07
  B6 (84,56,56) 64 -> 64     sum 1.8e-09 / 1.4e-09   sumsq 4.6e-07 / 3.5e-07
  B6 stride 2                sum 2.8e-09 / 2.1e-09   sumsq 3.8e-07 / 1.9e-07
  C3 C 64                    S1 0 / 0   S2 5.8e-08 / 7.2e-08
  C3 C 128                   S1 9.3e-09 / 9.3e-09   S2 7.9e-08 / 5.3e-08
  D A1                       S1 5.8e-09 / 7.0e-09   S2 7.1e-08 / 5.4e-08
  D A2                       S1 0 / 0   S2 6.2e-08 / 5.9e-08
  D A3                       S1 4.6e-09 / 4.6e-09   S2 4.3e-08 / 2.9e-08
  D C3 C 64                  S1 0 / 0   S2 3.7e-08 / 7.2e-08
  D C3 C 128                 S1 3.7e-09 / 6.4e-09   S2 6.5e-08 / 5.3e-08
  D C2 C 136 bf16            sum 2.1e-09 / 2.1e-09   sumsq 9.1e-08 / 1.9e-07
  D C2 C 40 bf16             sum 2.5e-10 / 2.5e-10   sumsq 1.0e-07 / 1.3e-07
  D C2 C 136 f32             sum 3.0e-08 / 2.3e-08   sumsq 1.2e-07 / 1.8e-07
  D C2 C 40 f32              sum 3.1e-08 / 2.8e-08   sumsq 9.4e-08 / 1.5e-07
(the maximum over the policies a case runs under - B6: 0 and 4; S1 is exact, 0, where a column's bf16 terms sum without rounding in f32)
"""
import contextlib
import functools
from types import SimpleNamespace

import pytest
import torch

import igemm_ref as IR

pytestmark = pytest.mark.gpu
BF16, F32 = 0, 1
DEV = "cuda"
POLICIES = [0, 1, 2, 3, 4]
RR = 3                      # statistics replicas
SENT = 7.0


def _hip():
    from clip_lite_amd import hip
    return hip


@contextlib.contextmanager
def _policy(p):
    hip = _hip()
    hip.set_tile_policy(p)
    try:
        yield hip
    finally:
        hip.set_tile_policy(0)


def _td(dt):
    return torch.bfloat16 if dt == BF16 else torch.float32


def _rho(td):
    return IR.RHO_BF16 if td == torch.bfloat16 else IR.RHO_F32


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _randn(g, *shape):
    return torch.randn(*shape, device=DEV, generator=g)


def _sentinel(shape, td):
    return torch.full(shape, SENT, device=DEV, dtype=td)


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _stats_buf(C):
    """[RR + 1][3][C]: rows 0 / 1 of the RR replicas zero (the accumulators), row 2 and the replica past the last one sentinels."""
    t = _sentinel((RR + 1, 3, C), torch.float32)
    t[:RR, :2] = 0
    return t


def _split_stats(total):
    """[C] float64 totals -> the statistics buffer whose rows 0 sum to (the f32 roundings of) the totals over UNEVEN parts 1 : 4 : 9."""
    t = _stats_buf(total.shape[0])
    w = torch.arange(1, RR + 1, dtype=torch.float64) ** 2
    t[:RR, 0] = (total.cpu()[None, :] * (w / w.sum())[:, None]).float().to(DEV)
    return t


def _check_stats_untouched(dst, what):
    assert bool((dst[:RR, 2] == SENT).all()) and bool((dst[RR] == SENT).all()), f"{what}: statistics rows beyond the two sums were written"


def _totals(dst):
    return dst[:RR].double().sum(0).float().cpu()


# ------------------------------------------------------------------------------------------------ the dgrad cases
@functools.lru_cache(maxsize=2)
def _dgrad_case(dt, N, H, W, Cc, K, R, stride, pad, mask="bits", res=None, after=False, out_f32=False, alpha=1.0, rows_factor=1, pad_cols=0, seed=0):
    """Operands on the GPU and the float64 reference of one BatchNorm-backward dgrad; built once, shared by the policies."""
    hip = _hip()
    td = _td(dt)
    g = _gen(1000 * seed + N * H * W + Cc + K)
    c = SimpleNamespace(dt=dt, td=td, N=N, H=H, W=W, Cc=Cc, K=K, R=R, stride=stride, pad=pad, mask=mask, res=res, after=after, alpha=alpha,
                        rows_factor=rows_factor, ldc=Cc + pad_cols, M=N * H * W, Ktot=R * R * K)
    c.td_out = torch.float32 if (out_f32 or dt == F32) else torch.bfloat16
    c.cv = hip.conv_desc(dt, N, H, W, Cc, K, R, R, stride, pad)
    w = (_randn(g, K, R, R, Cc) * 0.2).to(td)
    c.wt = w.permute(3, 1, 2, 0).contiguous()
    c.dy = _randn(g, N, c.cv.Ho, c.cv.Wo, K).to(td)
    c.aux = _randn(g, c.M, c.ldc).to(td)
    c.bits = IR.pack_bits(c.aux > 0)
    c.y = (_randn(g, c.M, c.ldc) + 2.0).to(td)
    c.fst = _split_stats(rows_factor * c.y[:, :Cc].double().sum(0))
    c.rows0 = rows_factor * c.M
    r = c.resbuf = c.old = None
    if res == "full":
        c.resbuf = _randn(g, c.M, c.ldc).to(td)
        r = c.resbuf[:, :Cc].cpu()
    elif res == "compact":
        c.resbuf = _randn(g, N * (H // 2) * (W // 2), c.ldc).to(td)
        r = IR.subsample_expand(c.resbuf[:, :Cc].cpu(), N, H, W)
    elif res == "inplace":
        assert c.td_out == td
        c.old = _randn(g, c.M, c.ldc).to(td)
        r = c.old[:, :Cc].cpu()
    acc = IR.dgrad_ref(c.dy.cpu(), w.cpu(), N, H, W, stride, pad)
    S_acc = IR.dgrad_scale(c.dy.cpu(), w.cpu(), N, H, W, stride, pad)
    c.e = IR.epilogue_ref(acc, S_acc, alpha=alpha, bits=c.bits.cpu() if mask == "bits" else None, aux=c.aux[:, :Cc].cpu() if mask == "aux" else None,
                          residual=r, mask_after_residual=after)
    c.y_cpu, c.fst_cpu = c.y[:, :Cc].cpu(), c.fst[:RR].cpu()
    c.tag = f"dgrad[{'bf16' if dt == BF16 else 'f32'},{N}x{H}x{W},C{Cc},K{K},R{R}s{stride},mask={mask},res={res},after={int(after)}]"
    return c


def _launch_dgrad(hip, c, colsum=True):
    out = c.old.clone() if c.res == "inplace" else _sentinel((c.M, c.ldc), c.td_out)
    dst = _stats_buf(c.Cc)
    ep = hip.epilogue(out, c.ldc, alpha=c.alpha, residual=out if c.res == "inplace" else c.resbuf, relu_bits=c.bits if c.mask == "bits" else None,
                      dact_aux=c.aux if c.mask == "aux" else None, dact=hip.DACT_RELU if c.mask == "aux" else 0, mask_after_residual=c.after,
                      colsum=hip.Stats(dst, RR, c.Cc) if colsum else None, bn=(c.y, hip.Stats(c.fst, RR, c.Cc), c.rows0),
                      out_f32=c.td_out == torch.float32, residual_subsample=2 if c.res == "compact" else 0)
    hip.conv_dgrad(c.dy, c.wt, c.cv, ep, wt=True)
    torch.cuda.synchronize()
    return out, dst


def _check_dgrad(c, out, dst, tag):
    got = out[:, :c.Cc].cpu()
    IR.assert_elements(tag, got, c.e, c.Ktot, _rho(c.td_out))
    if c.ldc > c.Cc:
        keep = c.old[:, c.Cc:] if c.res == "inplace" else _sentinel((c.M, c.ldc - c.Cc), c.td_out)
        assert torch.equal(_bits(out[:, c.Cc:].contiguous()), _bits(keep.contiguous())), f"{tag}: columns [C, ldc) were written"
    red = IR.bn_reductions_ref(got, c.y_cpu, c.fst_cpu, 1.0 / c.rows0)
    tot = _totals(dst)
    IR.assert_reductions(tag + " S1", tot[0], red.S1, red.t1)
    IR.assert_reductions(tag + " S2", tot[1], red.S2, red.t2)
    _check_stats_untouched(dst, tag)


def _run(policy, *args, **kw):
    c = _dgrad_case(*args, **kw)
    with _policy(policy) as hip:
        out, dst = _launch_dgrad(hip, c)
    _check_dgrad(c, out, dst, f"p{policy} {c.tag}")


A1 = (3, 9, 7, 136, 96, 1, 1, 0)
A3 = (3, 10, 14, 136, 64, 1, 1, 0)
A5 = (3, 10, 10, 40, 96, 1, 1, 0)
A_FORMS = {
    "A1": (A1, dict(pad_cols=8, seed=1)),
    "A2": (A1, dict(res="full", after=True, pad_cols=8, seed=2)),
    "A3": (A3, dict(res="compact", after=True, seed=3)),
    "A4-before": (A1, dict(res="full", after=False, seed=4)),
    "A4-aux0": (A1, dict(mask="aux", res="full", after=False, seed=5)),
    "A4-aux1": (A1, dict(mask="aux", res="full", after=True, seed=6)),
    "A4-f32out": (A1, dict(out_f32=True, seed=7)),
    "A4-alpha": (A1, dict(alpha=0.5, seed=8)),
    "A5-form1": (A5, dict(pad_cols=8, seed=9)),
    "A5-form2": (A5, dict(res="full", after=True, pad_cols=8, seed=10)),
    "A6-s1-form1": ((2, 9, 7, 96, 64, 3, 1, 1), dict(seed=11)),
    "A6-s1-form2": ((2, 9, 7, 96, 64, 3, 1, 1), dict(res="full", after=True, seed=12)),
    "A6-s2-form1": ((2, 9, 7, 96, 64, 3, 2, 1), dict(seed=13)),
}


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("name", list(A_FORMS))
def test_every_form_one_tile_per_workgroup(name, policy):
    """A1 - A6: every form on ragged row and column tiles, under every tile policy."""
    shape, kw = A_FORMS[name]
    _run(policy, BF16, *shape, **kw)


@pytest.mark.parametrize("name", ["A1", "A2", "A3"])
def test_f32_storage(name):
    """A7: T = float through igemm_dma_bn_kernel (FORM 0, f32 store); independent of the tile policy."""
    shape, kw = A_FORMS[name]
    _run(0, F32, *shape, **kw)


B_FORMS = {
    "B1": ((21, 57, 55, 128, 64, 1, 1, 0), dict(seed=21)),
    "B2": ((11, 55, 57, 256, 64, 1, 1, 0), dict(res="full", after=True, seed=22)),
    "B3": ((12, 54, 56, 256, 64, 1, 1, 0), dict(res="compact", after=True, seed=23)),
    "B5": ((42, 56, 56, 64, 256, 1, 1, 0), dict(res="inplace", after=True, rows_factor=4, seed=25)),
}


@pytest.mark.parametrize("policy", [0, 4])
@pytest.mark.parametrize("name", list(B_FORMS))
def test_row_range_persistent_schedule(name, policy):
    """B1 - B3, B5: more tiles than resident slots; every workgroup walks a full tile and a partial one."""
    shape, kw = B_FORMS[name]
    _run(policy, BF16, *shape, **kw)


# ------------------------------------------------------------------------------------------------ the folded BatchNorm backward (FORM 5)
@functools.lru_cache(maxsize=1)
def _fold_case(M, K, Cin):
    """clite_bn_fold_prepare on the GPU, then the float64 reference of dz2 = ([dz | y] w2^T + bias) * mask on the w2 / bias it stored (bf16 / f32
    operands of the GEMM under test), and beside it the existing folded test's reference (BatchNorm backward, then the convolution's) in float64."""
    hip = _hip()
    g = _gen(M + K + Cin)
    c = SimpleNamespace(M=M, K=K, Cin=Cin, Ktot=2 * K)
    a = torch.relu(_randn(g, M, Cin) + 0.3).bfloat16()
    Wk = (_randn(g, K, Cin) * (2.0 / Cin) ** 0.5).bfloat16()
    y = (a.float() @ Wk.float().t()).bfloat16()
    dz = (_randn(g, M, K) * 0.1 + 0.02 * _randn(g, K)).bfloat16()
    dz = dz * (torch.rand(M, K, device=DEV, generator=g) > 0.4)
    gamma = torch.rand(K, device=DEV, generator=g) + 0.5
    y64, dz64 = y.double(), dz.double()
    mean = y64.mean(0)
    var = ((y64 - mean) ** 2).mean(0)
    rstd = 1.0 / torch.sqrt(var + 1e-5)
    S1, S2 = dz64.sum(0), (dz64 * (y64 - mean)).sum(0)
    st, pre = _split_stats(y64.sum(0))[:RR].contiguous(), _split_stats(S1)[:RR].contiguous()
    w = torch.arange(1, RR + 1, dtype=torch.float64, device=DEV) ** 2
    st[:, 1] = ((y64 * y64).sum(0)[None, :] * (w / w.sum())[:, None]).float()
    pre[:, 1] = (S2[None, :] * (w / w.sum())[:, None]).float()
    st[:, 2], pre[:, 2] = 0, 0
    c.y2 = (_randn(g, M, Cin) + 2.0).bfloat16()
    c.fst = _split_stats(c.y2.double().sum(0))
    c.bits = IR.pack_bits(torch.rand(M, Cin, device=DEV, generator=g) > 0.3)
    c.pair = torch.empty(2, M, K, device=DEV, dtype=torch.bfloat16)
    c.pair[0], c.pair[1] = dz, y
    rm, rv = torch.zeros(K, device=DEV), torch.ones(K, device=DEV)
    dgamma, dbeta = torch.zeros(K, device=DEV), torch.zeros(K, device=DEV)
    desc = hip.bn_desc(M, K, hip.Stats(st, RR, K), gamma, torch.zeros(K, device=DEV), rm, rv, True, False, 0.1, 1e-5, False)
    c.f = hip.bn_fold_prepare(desc, hip.Stats(pre, RR, K), Wk.t().contiguous(), Cin, dgamma, dbeta)
    torch.cuda.synchronize()
    w2 = c.f.w2.double().cpu()                       # [Cin][2][K]: slot 0 multiplies y, slot 1 dz
    yc, dzc = y64.cpu(), dz64.cpu()
    acc = yc @ w2[:, 0].t() + dzc @ w2[:, 1].t()
    S_acc = yc.abs() @ w2[:, 0].abs().t() + dzc.abs() @ w2[:, 1].abs().t()
    c.e = IR.epilogue_ref(acc, S_acc, bias=c.f.bias.cpu(), bits=c.bits.cpu())
    xhat = (y64 - mean) * rstd
    dy = gamma.double() * rstd * (dz64 - S1 / M - xhat * (dz64 * xhat).sum(0) / M)
    c.want64 = (dy @ Wk.double()).cpu() * c.e.m
    c.y2_cpu, c.fst_cpu = c.y2.cpu(), c.fst[:RR].cpu()
    return c


@pytest.mark.parametrize("M,K,Cin,policy", [(300, 64, 136, p) for p in POLICIES] + [(300, 64, 40, p) for p in POLICIES] + [(65835, 64, 128, p) for p in (0, 4)])
def test_folded_batchnorm_backward_dz2(M, K, Cin, policy):
    """A8 / B4: clite_conv_dgrad_bnfold's dz2 and its two reductions (FORM 5; the large case on the row-range schedule, policies 0 and 4)."""
    c = _fold_case(M, K, Cin)
    tag = f"p{policy} fold[{M},K{K},Cin{Cin}]"
    dz2, d2 = _sentinel((M, Cin), torch.bfloat16), _stats_buf(Cin)
    with _policy(policy) as hip:
        hip.conv_dgrad_bnfold(c.pair, c.f.w2, M, K, Cin, hip.epilogue(dz2, Cin, relu_bits=c.bits, colsum=hip.Stats(d2, RR, Cin),
                                                                      bn=(c.y2, hip.Stats(c.fst, RR, Cin), M), bias=c.f.bias))
        torch.cuda.synchronize()
    got = dz2.cpu()
    IR.assert_elements(tag, got, c.e, c.Ktot, IR.RHO_BF16)
    # the BatchNorm-backward-then-convolution definition: the prepared weights are bf16 roundings (2^-9 each) of f32 coefficients times the weights
    assert bool(((got.double() - c.want64).abs() <= 2.0 ** -8 * (c.want64.abs() + c.e.S)).all()), f"{tag}: off the float64 BatchNorm backward"
    red = IR.bn_reductions_ref(got, c.y2_cpu, c.fst_cpu, 1.0 / M)
    tot = _totals(d2)
    IR.assert_reductions(tag + " S1", tot[0], red.S1, red.t1)
    IR.assert_reductions(tag + " S2", tot[1], red.S2, red.t2)
    _check_stats_untouched(d2, tag)


# ------------------------------------------------------------------------------------------------ B6: the forward FORM 4
@pytest.mark.parametrize("policy", [0, 4])
@pytest.mark.parametrize("N,H,W,Cin,K,stride", [(21, 57, 55, 64, 256, 1), (84, 56, 56, 64, 64, 1), (84, 56, 56, 64, 256, 2)])
def test_forward_1x1_bare_store_with_statistics(N, H, W, Cin, K, stride, policy):
    """B6: conv_fwd 1 x 1, bare bf16 store + colsum, more than 1024 tiles. Automatic policy: FORM 4 on the row-range schedule; policy 4: one tile per
    workgroup on the plain-store ring kernel. Statistics = sum and sum of squares of the stored values."""
    g = _gen(N + H + K + stride)
    x = _randn(g, N, H, W, Cin).bfloat16()
    w = (_randn(g, K, 1, 1, Cin) * 0.2).bfloat16()
    with _policy(policy) as hip:
        cv = hip.conv_desc(BF16, N, H, W, Cin, K, 1, 1, stride, 0)
        M = N * cv.Ho * cv.Wo
        out, cs = _sentinel((M, K), torch.bfloat16), _stats_buf(K)
        hip.conv_fwd(x, w, cv, hip.epilogue(out, K, colsum=hip.Stats(cs, RR, K)))
        torch.cuda.synchronize()
    tag = f"p{policy} fwd[{N}x{H}x{W},{Cin}->{K},s{stride}]"
    e = IR.epilogue_ref(IR.conv_fwd_ref(x.cpu(), w.cpu(), stride, 0), IR.conv_fwd_scale(x.cpu(), w.cpu(), stride, 0))
    got = out.cpu()
    IR.assert_elements(tag, got, e, Cin, IR.RHO_BF16)
    red = IR.bn_reductions_ref(got)
    tot = _totals(cs)
    IR.assert_reductions(tag + " sum", tot[0], red.S1, red.t1)
    IR.assert_reductions(tag + " sumsq", tot[1], red.Sq, red.tq)
    _check_stats_untouched(cs, tag)


# ------------------------------------------------------------------------------------------------ C: in-place and scattered outputs
@functools.lru_cache(maxsize=2)
def _inplace_case(dt, N, H, W, Cc, K, stride, pad_cols):
    """dx += dgrad of a 1 x 1 convolution (stride 1: dense; stride 2: only the lattice pixels receive anything), generic epilogue."""
    hip = _hip()
    td = _td(dt)
    g = _gen(N * H * W + Cc + K + stride + dt)
    c = SimpleNamespace(dt=dt, td=td, Cc=Cc, K=K, ldc=Cc + pad_cols, M=N * H * W, stride=stride)
    c.cv = hip.conv_desc(dt, N, H, W, Cc, K, 1, 1, stride, 0)
    w = (_randn(g, K, 1, 1, Cc) * 0.2).to(td)
    c.wt = w.permute(3, 1, 2, 0).contiguous()
    c.dy = _randn(g, N, c.cv.Ho, c.cv.Wo, K).to(td)
    c.old = _randn(g, c.M, c.ldc).to(td)
    acc = IR.dgrad_ref(c.dy.cpu(), w.cpu(), N, H, W, stride, 0)
    S_acc = IR.dgrad_scale(c.dy.cpu(), w.cpu(), N, H, W, stride, 0)
    c.rows = IR.scatter_rows(N, c.cv.Ho, c.cv.Wo, H, W, stride)
    c.off = torch.ones(c.M, dtype=torch.bool)
    c.off[c.rows] = False
    assert not acc[c.off].any()
    c.e = IR.epilogue_ref(acc[c.rows], S_acc[c.rows], residual=c.old[:, :Cc].cpu()[c.rows])
    return c


def _check_inplace(c, dx, tag):
    got = dx.cpu()
    old = c.old.cpu()
    IR.assert_elements(tag, got[c.rows][:, :c.Cc], c.e, c.K, _rho(c.td))
    assert torch.equal(_bits(got[c.off]), _bits(old[c.off])), f"{tag}: an off-lattice pixel changed"
    assert torch.equal(_bits(got[:, c.Cc:].contiguous()), _bits(old[:, c.Cc:].contiguous())), f"{tag}: columns [C, ldc) changed"


INPLACE = [(dt, p) for dt in (BF16, F32) for p in (POLICIES if dt == BF16 else [0])]


@pytest.mark.parametrize("dt,policy", INPLACE)
def test_generic_epilogue_in_place_dense(dt, policy):
    """C1: hip.epilogue(dx, C, residual=dx), 1 x 1 stride 1, M = 189, C = 136."""
    c = _inplace_case(dt, 3, 9, 7, 136, 96, 1, 0)
    dx = c.old.clone()
    with _policy(policy) as hip:
        hip.conv_dgrad(c.dy, c.wt, c.cv, hip.epilogue(dx, c.ldc, residual=dx), wt=True)
        torch.cuda.synchronize()
    _check_inplace(c, dx, f"p{policy} inplace dense {'bf16' if dt == BF16 else 'f32'}")


@pytest.mark.parametrize("Cc", [136, 40])
@pytest.mark.parametrize("dt,policy", INPLACE)
def test_strided_1x1_scatter_add_in_place(dt, policy, Cc):
    """C2: 1 x 1 stride 2 pad 0, (3, 9, 7) -> 5 x 4, residual = dx: lattice pixels = old + dgrad, every other pixel and the columns [C, C + 8) bit-exact."""
    c = _inplace_case(dt, 3, 9, 7, Cc, 96, 2, 8)
    dx = c.old.clone()
    with _policy(policy) as hip:
        hip.conv_dgrad(c.dy, c.wt, c.cv, hip.epilogue(dx, c.ldc, residual=dx), wt=True)
        torch.cuda.synchronize()
    _check_inplace(c, dx, f"p{policy} scatter C{Cc} {'bf16' if dt == BF16 else 'f32'}")


@functools.lru_cache(maxsize=2)
def _s2_case(Cc):
    return _dgrad_case(BF16, 2, 6, 10, Cc, 128, 3, 2, 1, seed=30 + Cc)


def _launch_s2(hip, c, colsum=True):
    out, dst = _sentinel((c.M, c.ldc), c.td_out), _stats_buf(c.Cc)
    hip.conv_dgrad_s2(c.dy, c.wt, c.cv, lambda: hip.epilogue(out, c.ldc, relu_bits=c.bits, colsum=hip.Stats(dst, RR, c.Cc) if colsum else None,
                                                             bn=(c.y, hip.Stats(c.fst, RR, c.Cc), c.rows0)), wt=True)
    torch.cuda.synchronize()
    return out, dst


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("Cc", [64, 128])
def test_stride2_parity_classes_accumulate_one_set_of_statistics(Cc, policy):
    """C3: conv_dgrad_s2 with the FORM 1 epilogue: the four class launches write every pixel once (no sentinel survives, every element within the bound
    of the full dgrad) and their accumulated statistics are those of the whole tensor."""
    c = _s2_case(Cc)
    with _policy(policy) as hip:
        assert hip.s2_classes_ok(c.cv)
        out, dst = _launch_s2(hip, c)
    _check_dgrad(c, out, dst, f"p{policy} s2class C{Cc}")


# ------------------------------------------------------------------------------------------------ D: deterministic mode
def _twice(launch):
    (o1, d1), (o2, d2) = launch(), launch()
    assert torch.equal(_bits(o1), _bits(o2)), "outputs of two deterministic launches differ"
    assert torch.equal(d1.view(torch.int32), d2.view(torch.int32)), "statistics of two deterministic launches differ"
    return o1, d1


@pytest.mark.parametrize("name", ["A1", "A2", "A3"])
def test_deterministic_mode_dgrad_statistics(deterministic_reductions, name):
    """colstats_det_kernel over the tensor the (statistics-free) dgrad launch stored: same bounds, two launches bit-identical."""
    shape, kw = A_FORMS[name]
    c = _dgrad_case(BF16, *shape, **kw)
    with _policy(0) as hip:
        assert hip.is_deterministic()
        out, dst = _twice(lambda: _launch_dgrad(hip, c))
    _check_dgrad(c, out, dst, f"det {c.tag}")


@pytest.mark.parametrize("Cc", [64, 128])
def test_deterministic_mode_parity_classes_through_the_row_map(deterministic_reductions, Cc):
    c = _s2_case(Cc)
    with _policy(0) as hip:
        assert hip.is_deterministic()
        out, dst = _twice(lambda: _launch_s2(hip, c))
    _check_dgrad(c, out, dst, f"det s2class C{Cc}")


@pytest.mark.parametrize("Cc", [136, 40])
@pytest.mark.parametrize("dt", [BF16, F32])
def test_deterministic_mode_strided_1x1_in_place_with_colsum(deterministic_reductions, dt, Cc):
    """C2 with colsum: statistics (sum, sum of squares) of the stored dx over ALL pixels, two launches bit-identical."""
    c = _inplace_case(dt, 3, 9, 7, Cc, 96, 2, 8)
    tag = f"det scatter C{Cc} {'bf16' if dt == BF16 else 'f32'}"

    def launch():
        dx, cs = c.old.clone(), _stats_buf(Cc)
        hip.conv_dgrad(c.dy, c.wt, c.cv, hip.epilogue(dx, c.ldc, residual=dx, colsum=hip.Stats(cs, RR, Cc)), wt=True)
        torch.cuda.synchronize()
        return dx, cs

    with _policy(0) as hip:
        assert hip.is_deterministic()
        dx, cs = _twice(launch)
    _check_inplace(c, dx, tag)
    red = IR.bn_reductions_ref(dx[:, :Cc].cpu())
    tot = _totals(cs)
    IR.assert_reductions(tag + " sum", tot[0], red.S1, red.t1)
    IR.assert_reductions(tag + " sumsq", tot[1], red.Sq, red.tq)
    _check_stats_untouched(cs, tag)
