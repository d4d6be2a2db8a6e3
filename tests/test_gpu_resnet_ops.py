"""Kernel-level GPU checks of the image encoder's streaming kernels (csrc/resnet_ops.hip, csrc/stem_bn.h) through clip_lite_amd.hip against the
float64 references of tests/resnet_ref.py, evaluated on the SAME storage-rounded inputs: BatchNorm apply / backward reduce / backward apply /
centered variance, the 3x3/2 max-pool, the fused stem BN + ReLU + max-pool family against the unfused sequence and the reference, the global
average pool, image_to_nhwc4 and colsum. Every test runs in bf16 and f32.

Bounds (ref = float64 reference, max|ref| over the compared tensor):
  element-wise, stored f32   |got - ref| <= 2e-5 * max|ref|                       (tests/test_wavesim_ops.py's f32 figure)
  element-wise, stored bf16  |got - ref| <= 2^-7 * |ref| + 2e-5 * max|ref|        (one bf16 ulp of the stored value + the f32 compute error)
  reductions / accumulators  |got - ref| <= 1e-4 * max|ref| per channel           (dstats, dgamma, dbeta, colsum, running statistics, centered sum)
  integer outputs (idx, relu_bits), copies (dz, ymax) and fused-against-unfused pooled / idx / running statistics: exact.
No window is skipped in an idx comparison: the stem reference pools the a0 that was ROUNDED to the storage type, and the tests assert that
rounding created no tie the unrounded values did not have.

Which device path the shapes take (from bn_grid / ew_grid / clite_colsum in csrc/resnet_ops.hip):
  BatchNorm (70, 8)        CPR = 1: the full xor tree (32 .. 1), one workgroup, one 256-row sweep with 186 dead lanes
  BatchNorm (1001, 64)     CPR = 8, 8 workgroups of 128 rows, the last with 105; LDS fold over 4 waves
  BatchNorm (333, 1024)    CPR = 128: no shuffle step, the two-wave-pair LDS fold; 42 workgroups of 8 rows, the last with 5
  BatchNorm (77, 2048)     CPR = 256: every thread its own chunk, no fold; 20 workgroups of 4 rows, the last with 1
  BatchNorm (262181, 64)   f32: 64.01 MiB per tensor -> the non-temporal kernels; bf16: 32 MiB -> the cached kernels. 8194 sweeps ask for 1025
                           workgroups, the cap of 1024 makes it 9 sweeps = 288 rows each: 911 persistent workgroups, the last with 101 rows
  max-pool (11, 225, 223, 64)  forward 1 113 728 work items on 4096 x 256 threads: 1048576 take one trip, 65152 a second; backward
                           4 415 400 items: four trips and a partial fifth. The other shapes: one trip
  stem (3, 113, 111), (4, 112, 112): forward 9576 / 12544 pooled rows -> 75 / 98 workgroups; the apply pass over 2 x 2 groups runs 2 sweeps per
                           workgroup (150 / 196 workgroups, the last partial at (3, 113, 111)); more than 2 sweeps needs >= 786k pixels and is not reached here
  colsum (1001, 72) no fold, gx = 1, 63 slabs of 16 rows; (333, 264) gx = 2 with one live chunk in the second group; (1000, 64) the nfold view
                           [250][256]; (255, 64) 255 % 4 != 0: no fold; (262184, 64) the nfold view [65546][256] and, at >= 65536 rows of it, the 1024-slab
                           variant: 1009 slabs of 65 rows, the last with 26
  avgpool (300, 49, 512) 19200 threads = 75 full workgroups; (37, 5, 136) 629 threads: the third workgroup holds 117

Measured on an MI355X (printed by every run, `pytest -s`): max over channels of |got - ref| / sum|terms| for the reductions, with the error of a plain
torch.float32 `.sum(0)` of the same terms against float64 beside it (kernel / torch.float32; neither figure feeds a bound):
(each line: bf16 kernel / torch | f32 kernel / torch, the maximum over the test's cases)
  BatchNorm (70, 8)         S1 0 / 0 | 3.2e-08 / 2.4e-08   S2 4.0e-08 / 4.7e-08 | 3.7e-08 / 8.5e-08   dgamma 5.4e-08 / 6.4e-08 | 5.7e-08 / 5.2e-08
                            dbeta 1.7e-08 / 0 | 4.9e-08 / 2.4e-08   centered 1.5e-07 / 1.9e-07 | 1.4e-07 / 1.1e-07
  BatchNorm (1001, 64)      S1 5.7e-09 / 5.7e-09 | 1.2e-08 / 1.7e-08   S2 2.2e-08 / 1.9e-08 | 1.7e-08 / 1.9e-08   dgamma 2.6e-08 / 2.0e-08 | 2.0e-08 / 2.4e-08
                            dbeta 7.1e-09 / 5.7e-09 | 1.2e-08 / 1.7e-08   centered 9.5e-08 / 1.3e-07 | 9.5e-08 / 1.1e-07
  BatchNorm (333, 1024)     S1 7.6e-09 / 7.6e-09 | 2.6e-08 / 3.6e-08   S2 3.4e-08 / 6.9e-08 | 3.9e-08 / 5.0e-08   dgamma 7.3e-08 / 5.0e-08 | 5.4e-08 / 5.4e-08
                            dbeta 1.6e-08 / 7.6e-09 | 3.8e-08 / 3.6e-08   centered 1.1e-07 / 2.3e-07 | 1.0e-07 / 2.1e-07
  BatchNorm (77, 2048)      S1 2.4e-08 / 2.4e-08 | 6.2e-08 / 6.6e-08   S2 6.2e-08 / 8.9e-08 | 6.7e-08 / 7.8e-08   dgamma 1.1e-07 / 8.3e-08 | 2.2e-07 / 7.8e-08
                            dbeta 3.3e-08 / 2.4e-08 | 8.7e-08 / 6.6e-08   centered 1.2e-07 / 2.2e-07 | 1.2e-07 / 1.6e-07
  BatchNorm (262181, 64)    S1 1.1e-09 / 1.4e-09 | 2.6e-09 / 1.4e-09   S2 3.3e-09 / 1.8e-09 | 3.1e-09 / 2.5e-09   dgamma 3.1e-09 / 2.2e-09 | 3.2e-09 / 1.5e-09
                            dbeta 1.2e-09 / 1.4e-09 | 2.7e-09 / 1.4e-09   centered 1.6e-07 / 1.2e-07 | 1.6e-07 / 1.5e-07
                            (the centered figure carries the f32 rounding of the mean the kernel forms from the f32 statistics; torch's is taken on exact terms)
  stem, fused and unfused alike, M <= 288 (three small shapes)   S1 0 / 0 | 6.7e-08 / 6.4e-08   S2 6.2e-08 / 6.3e-08 | 6.9e-08 / 4.9e-08
                            dgamma 1.1e-07 / 7.4e-08 | 9.3e-08 / 6.2e-08   dbeta 2.6e-08 / 0 | 5.4e-08 / 6.4e-08
  stem (3, 113, 111, 64)    unfused S1 3.6e-09 / 1.6e-09 | 7.8e-09 / 7.0e-09   S2 1.5e-08 / 7.3e-09 | 1.2e-08 / 7.9e-09   dgamma 1.6e-08 / 7.1e-09 | 1.2e-08 / 6.6e-09
                            fused   S1 3.6e-09 / 1.6e-09 | 5.9e-09 / 7.0e-09   S2 8.6e-09 / 7.3e-09 | 1.2e-08 / 7.9e-09   dgamma 8.9e-09 / 7.1e-09 | 1.3e-08 / 6.6e-09
  stem (4, 112, 112, 64)    unfused S1 2.0e-09 / 3.9e-09 | 9.5e-09 / 9.5e-09   S2 1.2e-08 / 7.9e-09 | 9.1e-09 / 5.2e-09   dgamma 1.2e-08 / 5.0e-09 | 8.7e-09 / 5.5e-09
                            fused   S1 2.6e-09 / 3.9e-09 | 4.9e-09 / 9.5e-09   S2 9.8e-09 / 7.9e-09 | 7.4e-09 / 5.2e-09   dgamma 9.6e-09 / 5.0e-09 | 8.1e-09 / 5.5e-09
  colsum (1001, 72) 6.4e-09 / 2.5e-09 | 1.7e-08 / 1.6e-08   (333, 264) 9.4e-09 / 9.2e-09 | 4.1e-08 / 3.1e-08   (1000, 64) 5.5e-09 / 2.4e-09 | 4.5e-08 / 1.2e-08
                            (255, 64) 9.9e-09 / 2.4e-09 | 4.0e-08 / 1.4e-08   (262184, 64) 5.9e-09 / 7.5e-10 | 5.6e-09 / 9.9e-10
  deterministic mode        BatchNorm (1001, 64) S1 2.6e-09 / 2.6e-09 | 1.4e-08 / 9.9e-09   S2 1.5e-08 / 2.5e-08 | 1.8e-08 / 2.5e-08   centered 9.9e-08 / 1.3e-07 | 1.2e-07 / 1.1e-07
                            BatchNorm (333, 1024) S1 1.2e-08 / 1.2e-08 | 4.2e-08 / 3.5e-08   S2 5.1e-08 / 4.6e-08 | 5.7e-08 / 6.3e-08   centered 2.7e-07 / 1.9e-07 | 1.7e-07 / 1.6e-07
                            stem (7, 11, 13, 64) S1 4.9e-09 / 4.9e-09 | 2.5e-08 / 2.7e-08   S2 2.6e-08 / 1.9e-08 | 3.0e-08 / 2.6e-08   colsum (1001, 64) 6.3e-09 / 4.9e-09 | 1.9e-08 / 1.2e-08
The bound of 1e-4 * max|ref| corresponds to 1e-6 .. 1e-5 on this scale: the kernels sit at the level of a plain f32 sum, one to two orders below it.
"""
import pytest
import torch

import resnet_ref as RR

pytestmark = pytest.mark.gpu
BF16, F32 = 0, 1
DTS = [BF16, F32]
EPS, MOM = 1e-5, 0.1
DEV = "cuda"


def _hip():
    from clip_lite_amd import hip
    return hip


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _randn(g, *shape):
    return torch.randn(*shape, device=DEV, generator=g)


def _fill(shape, td, value=7.0):
    """An output buffer with a non-zero pattern: an element the kernel does not write stays wrong."""
    return torch.full(shape, value, device=DEV).to(td)


def _elem(what, got, ref, dt):
    ref = ref.reshape(got.shape)
    err = (got.double() - ref).abs()
    top = ref.abs().max().item()
    bound = 2e-5 * top + (2.0 ** -7 * ref.abs() if dt == BF16 else 0.0)
    bad = err > bound
    assert not bool(bad.any()) and bool(torch.isfinite(got.float()).all()), \
        f"{what}: {int(bad.sum())} of {bad.numel()} elements out of bound, max err {err.max().item():.3e}, max|ref| {top:.3e}"


def _reduction(what, got, ref, terms=None):
    """Per channel |got - ref| <= 1e-4 * max|ref|. terms [M][C] float64 (ref = a constant + terms.sum(0)): prints the measured
    max |got - ref| / sum|terms| and, beside it, what torch.float32 .sum(0) of the same terms loses against float64."""
    assert got.dtype == torch.float32
    err = (got.double() - ref).abs()
    top = ref.abs().max().item()
    if terms is not None:
        denom = terms.abs().sum(0).clamp_min(1e-300)
        plain = (terms.float().sum(0).double() - terms.sum(0)).abs()
        print(f"REDERR {what}: kernel {(err / denom).max().item():.2e}  torch.float32 {(plain / denom).max().item():.2e}")
    assert bool((err <= 1e-4 * top).all()), f"{what}: max err {err.max().item():.3e} > 1e-4 * {top:.3e}"


def _split(total, R):
    """[k][C] f32 totals -> [R][3][C] replicated accumulator whose rows 0..k-1 sum to the totals over UNEVEN parts (1 : 4 : 9 : ...)."""
    k, C = total.shape
    t = torch.zeros(R, 3, C, device=DEV)
    w = torch.arange(1, R + 1, dtype=torch.float32) ** 2
    w = (w / w.sum()).tolist()
    for r in range(R - 1):
        t[r, :k] = total * w[r]
    t[R - 1, :k] = total - t[:R - 1, :k].sum(0)
    return t


def _stats(hip, x, R):
    x = x.double()
    return hip.Stats(_split(torch.stack([x.sum(0), (x * x).sum(0)]).float(), R), R, x.shape[1])


def _pack(x):
    """[M][C] -> uint8 [M][C / 8], bit e of byte (m, c / 8) = x[m][c + e] > 0 (clite_bn.relu_bits)."""
    w = (2 ** torch.arange(8, device=x.device)).to(torch.int32)
    return ((x > 0).view(x.shape[0], -1, 8).to(torch.int32) * w).sum(-1).to(torch.uint8)


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


# ------------------------------------------------------------------------------------------------ a. BatchNorm
BN_SHAPES = [(70, 8, 3), (1001, 64, 3), (333, 1024, 8), (77, 2048, 5), (262181, 64, 8)]


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("dual", [False, True])
@pytest.mark.parametrize("M,C,R", BN_SHAPES)
@pytest.mark.parametrize("dt", DTS)
def test_batchnorm_apply_backward_and_centered_variance_match_float64(dt, M, C, R, dual, relu):
    """bn_apply (plain residual / dual-BN residual, ReLU on / off, running statistics updated), bn_bwd_reduce, bn_bwd_apply (dgamma / dbeta onto
    prefilled buffers), bn_centered_var and a centered apply. The statistics arrive split unevenly over R replicas."""
    hip = _hip()
    td = hip.TORCH_DTYPE[dt]
    g = _gen(M + C + 2 * dual + relu)
    y = (_randn(g, M, C) * 2 + 0.5).to(td)
    res = _randn(g, M, C).to(td)
    gamma, beta, g2, b2 = 1 + 0.1 * _randn(g, C), 0.1 * _randn(g, C), 1 + 0.1 * _randn(g, C), 0.1 * _randn(g, C)
    rm0, rv0, rm20, rv20 = 0.3 * _randn(g, C), 1 + 0.5 * torch.rand(C, device=DEV, generator=g), 0.3 * _randn(g, C), 1 + 0.5 * torch.rand(C, device=DEV, generator=g)
    rm, rv, rm2, rv2 = rm0.clone(), rv0.clone(), rm20.clone(), rv20.clone()
    st, rst = _stats(hip, y, R), _stats(hip, res, R)
    st_in = st.t.clone()
    multi_wg = (M, C) != (70, 8)                          # the one shape with a single workgroup
    tag = f"bn[{'bf16' if dt == BF16 else 'f32'},{M}x{C},dual={int(dual)},relu={int(relu)}]"

    def desc(update, centered=False, bits=None):
        return hip.bn_desc(M, C, st, gamma, beta, rm, rv, True, update, MOM, EPS, relu, res_bn=(rst, g2, b2, rm2, rv2) if dual else None, centered=centered, relu_bits=bits)

    out = _fill((M, C), td)
    bits = torch.full((M, C // 8), 0xAA, device=DEV, dtype=torch.uint8) if relu else None
    hip.bn_apply(dt, desc(True, bits=bits), y, res, out)
    ref = RR.bn_train_ref(y, gamma, beta, EPS, res=res, res_bn=(g2, b2, (rm20, rv20)) if dual else None, relu=relu, momentum=MOM, running=(rm0, rv0))
    _elem(tag + " out", out, ref.out, dt)
    _reduction(tag + " running_mean", rm, ref.running_mean)
    _reduction(tag + " running_var", rv, ref.running_var)
    if dual:
        _reduction(tag + " res running_mean", rm2, ref.res_running_mean)
        _reduction(tag + " res running_var", rv2, ref.res_running_var)
    else:
        assert torch.equal(rm2, rm20) and torch.equal(rv2, rv20)
    if relu:
        assert torch.equal(bits, _pack(out))
    rm_after, rv_after = rm.clone(), rv.clone()

    # backward of the main branch, the mask taken from the stored output
    dout = _randn(g, M, C).to(td)
    mask = out if relu else None
    b = RR.bn_bwd_ref(dout, mask, y, gamma, EPS)
    yc = y.double() - ref.mean
    dst = hip.Stats(torch.zeros(R, 3, C, device=DEV), R, C)
    hip.bn_bwd_reduce(dt, dout, mask, y, st, dst, M, C)
    tot = dst.t.double().sum(0).float()
    _reduction(tag + " S1", tot[0], b.S1, b.dz)
    _reduction(tag + " S2", tot[1], b.S2, b.dz * yc)
    assert not bool(dst.t[:, 2].any())
    if multi_wg:
        assert bool(dst.t[:, :2].abs().sum((1, 2)).gt(0).all()), "a replica of dstats received nothing"
    dy, dz = _fill((M, C), td), _fill((M, C), td)
    dg0, db0 = 1 + _randn(g, C), 1 + _randn(g, C)
    dg, db = dg0.clone(), db0.clone()
    hip.bn_bwd_apply(dt, desc(False), dout, mask, y, dst, dy, dz, dg, db)
    _elem(tag + " dy", dy, b.dy, dt)
    assert torch.equal(dz.double(), b.dz)
    xhat = yc / torch.sqrt(ref.var + EPS)
    _reduction(tag + " dgamma", dg, dg0.double() + b.dgamma, b.dz * xhat)
    _reduction(tag + " dbeta", db, db0.double() + b.dbeta, b.dz)
    assert torch.equal(rm, rm_after) and torch.equal(rv, rv_after) and torch.equal(st.t, st_in)          # update off: untouched

    # two-pass variance: row 2 of the replicated statistics, then an apply that reads it
    hip.bn_centered_var(dt, y, st, M, C)
    _reduction(tag + " centered", st.t[:, 2].double().sum(0).float(), (yc * yc).sum(0), yc * yc)
    assert torch.equal(st.t[:, :2], st_in[:, :2])
    if multi_wg:
        assert bool(st.t[:, 2].abs().sum(1).gt(0).all()), "a replica of the centered sum received nothing"
    if dual:
        hip.bn_centered_var(dt, res, rst, M, C)
    outc = _fill((M, C), td)
    hip.bn_apply(dt, desc(False, centered=True), y, res, outc)
    _elem(tag + " centered out", outc, ref.out, dt)


# ------------------------------------------------------------------------------------------------ b. max-pool
@pytest.mark.parametrize("N,H,W,C", [(2, 9, 8, 16), (1, 12, 13, 8), (3, 7, 7, 2048), (11, 225, 223, 64)])
@pytest.mark.parametrize("dt", DTS)
def test_maxpool_values_and_window_codes_are_exact_with_ties(dt, N, H, W, C):
    hip = _hip()
    td = hip.TORCH_DTYPE[dt]
    g = _gen(H * W + C)
    x = (torch.round(_randn(g, N, H, W, C) * 2) / 2).to(td)          # coarse values: ties
    Ho, Wo = RR.pool_out(H), RR.pool_out(W)
    out, idx = _fill((N, Ho, Wo, C), td), torch.full((N, Ho, Wo, C), 255, device=DEV, dtype=torch.uint8)
    hip.maxpool_fwd(dt, x, out, idx, N, H, W, C)
    val, code = RR.maxpool_ref(x)
    taps, ok = RR.maxpool_taps(x)
    assert bool((((taps == val) & ok).sum(0) >= 2).any()), "no window with a tie"
    del taps
    assert torch.equal(out.double(), val)
    assert torch.equal(idx.long(), code)
    dout = _randn(g, N, Ho, Wo, C).to(td)
    dx = _fill((N, H, W, C), td)
    hip.maxpool_bwd(dt, dout, idx, dx, N, H, W, C)
    _elem("maxpool dx", dx, RR.maxpool_bwd_ref(dout, code, H, W), dt)


# ------------------------------------------------------------------------------------------------ c. fused stem
def _stem_problem(hip, dt, N, H, W, C, R=3, seed=0):
    td = hip.TORCH_DTYPE[dt]
    g = _gen(H * 100 + W + C + seed)
    M = N * H * W
    # coarse values and a plain gamma / beta on the first chunk so that post-BN ties and exact zeros at the ReLU occur
    y = (torch.round(_randn(g, M, C) * 2) / 2).to(td)
    gamma, beta = 1 + 0.1 * _randn(g, C), 0.1 * _randn(g, C)
    gamma[:8], beta[:8] = 1.0, 0.0
    return td, g, M, y, gamma, beta, _stats(hip, y, R)


@pytest.mark.parametrize("N,H,W,C", [(2, 9, 8, 64), (1, 12, 13, 64), (3, 113, 111, 64), (4, 112, 112, 64), (2, 9, 8, 128)])
@pytest.mark.parametrize("dt", DTS)
def test_fused_stem_equals_unfused_sequence_and_float64(dt, N, H, W, C):
    """stem_bn_pool_fwd against bn_apply -> maxpool_fwd: pooled, idx and the running statistics BIT-equal (the claim above stem_bn_pool_fwd_kernel: both
    kernels must contract (y - mean) * a + b alike), and both equal to the reference that rounds a0 to the storage type before the max.
    stem_bn_pool_bwd against maxpool_bwd -> bn_bwd_reduce -> bn_bwd_apply and the reference. Then the pooled-size operands of the _ex entry
    point (ymax, relu_bits) and stem_bn_pool_bwd_apply on reductions formed from them."""
    hip = _hip()
    R_ = 3
    td, g, M, y, gamma, beta, st = _stem_problem(hip, dt, N, H, W, C, R_)
    Ho, Wo = RR.pool_out(H), RR.pool_out(W)
    P = N * Ho * Wo
    tag = f"stem[{'bf16' if dt == BF16 else 'f32'},{N}x{H}x{W}x{C}]"
    rm0, rv0 = 0.3 * _randn(g, C), 1 + 0.5 * torch.rand(C, device=DEV, generator=g)
    rm_u, rv_u, rm_f, rv_f = rm0.clone(), rv0.clone(), rm0.clone(), rv0.clone()

    def desc(rm, rv, update, bits=None):
        return hip.bn_desc(M, C, st, gamma, beta, rm, rv, True, update, MOM, EPS, True, relu_bits=bits)

    a0 = _fill((M, C), td)
    hip.bn_apply(dt, desc(rm_u, rv_u, True), y, None, a0)
    p_u, i_u = _fill((P, C), td), torch.full((P, C), 255, device=DEV, dtype=torch.uint8)
    hip.maxpool_fwd(dt, a0, p_u, i_u, N, H, W, C)
    p_f, i_f = _fill((P, C), td), torch.full((P, C), 254, device=DEV, dtype=torch.uint8)
    hip.stem_bn_pool_fwd(dt, desc(rm_f, rv_f, True), y, p_f, i_f, N, H, W)
    assert torch.equal(_bits(p_f), _bits(p_u))
    assert torch.equal(i_f, i_u)
    assert torch.equal(rm_f, rm_u) and torch.equal(rv_f, rv_u)

    bn = RR.bn_train_ref(y, gamma, beta, EPS, relu=True, momentum=MOM, running=(rm0, rv0))
    a0r = RR.round_to(bn.out, td)
    val, code = RR.maxpool_ref(a0r.view(N, H, W, C))
    # a window could be skipped only if rounding a0 to the storage type had created a tie at the top that the unrounded values do not have
    taps_r, ok = RR.maxpool_taps(a0r.view(N, H, W, C))
    taps_u, _ = RR.maxpool_taps(bn.out.view(N, H, W, C))
    ninf = torch.full_like(taps_u, float("-inf"))
    n_r = ((taps_r == val) & ok).sum(0)
    n_u = ((taps_u == torch.where(ok, taps_u, ninf).max(0).values) & ok).sum(0)
    skipped = n_r != n_u
    assert skipped.double().mean().item() == 0.0
    assert bool((n_r >= 2).any()), "no window with a tie"
    del taps_r, taps_u, ninf
    assert torch.equal(i_u.view(N, Ho, Wo, C).long(), code)
    _elem(tag + " a0", a0, bn.out, dt)
    _elem(tag + " pooled", p_u, val, dt)
    assert bool((p_u == 0).any())
    _reduction(tag + " running_mean", rm_f, bn.running_mean)
    _reduction(tag + " running_var", rv_f, bn.running_var)
    assert torch.equal(a0 > 0, a0r.view(M, C) > 0)

    # backward
    dpool = _randn(g, P, C).to(td)
    d = desc(rm_u, rv_u, False)
    dg0, db0 = 1 + _randn(g, C), 1 + _randn(g, C)
    da0 = _fill((M, C), td)
    hip.maxpool_bwd(dt, dpool, i_u, da0, N, H, W, C)
    ds_u = hip.Stats(torch.zeros(R_, 3, C, device=DEV), R_, C)
    hip.bn_bwd_reduce(dt, da0, a0, y, st, ds_u, M, C)
    dy_u, dg_u, db_u = _fill((M, C), td), dg0.clone(), db0.clone()
    hip.bn_bwd_apply(dt, d, da0, a0, y, ds_u, dy_u, None, dg_u, db_u)
    ds_f = hip.Stats(torch.zeros(R_, 3, C, device=DEV), R_, C)
    dy_f, dg_f, db_f = _fill((M, C), td), dg0.clone(), db0.clone()
    hip.stem_bn_pool_bwd(dt, d, dpool, i_f, y, ds_f, dy_f, dg_f, db_f, N, H, W)
    assert torch.equal(rm_u, rm_f) and torch.equal(rv_u, rv_f)          # update off: untouched

    da0_ref = RR.round_to(RR.maxpool_bwd_ref(dpool.view(N, Ho, Wo, C), code, H, W), td).view(M, C)
    b = RR.bn_bwd_ref(da0_ref, a0r.view(M, C), y, gamma, EPS)
    yc = y.double() - bn.mean
    xhat = yc / torch.sqrt(bn.var + EPS)
    tu, tf = ds_u.t.double().sum(0).float(), ds_f.t.double().sum(0).float()
    for name, t in (("unfused", tu), ("fused", tf)):
        _reduction(f"{tag} {name} S1", t[0], b.S1, b.dz)
        _reduction(f"{tag} {name} S2", t[1], b.S2, b.dz * yc)
    _reduction(tag + " fused S1 vs unfused", tf[0], tu[0].double())
    _reduction(tag + " fused S2 vs unfused", tf[1], tu[1].double())
    if M > 256:
        assert bool(ds_f.t[:, :2].abs().sum((1, 2)).gt(0).all()), "a replica of the fused dstats received nothing"
    _elem(tag + " unfused dy", dy_u, b.dy, dt)
    _elem(tag + " fused dy", dy_f, b.dy, dt)
    _elem(tag + " fused dy vs unfused", dy_f, dy_u.double(), dt)
    for name, dgx, dbx in (("unfused", dg_u, db_u), ("fused", dg_f, db_f)):
        _reduction(f"{tag} {name} dgamma", dgx, dg0.double() + b.dgamma, b.dz * xhat)
        _reduction(f"{tag} {name} dbeta", dbx, db0.double() + b.dbeta, b.dz)
    _reduction(tag + " fused dgamma vs unfused", dg_f, dg_u.double())
    _reduction(tag + " fused dbeta vs unfused", db_f, db_u.double())

    # the _ex entry point: ymax = y at the argmax, relu_bits = pooled > 0, pooled / idx unchanged
    p_x, i_x = _fill((P, C), td), torch.full((P, C), 253, device=DEV, dtype=torch.uint8)
    ymax, bits = _fill((P, C), td), torch.full((P, C // 8), 0xAA, device=DEV, dtype=torch.uint8)
    hip.stem_bn_pool_fwd(dt, desc(rm_f, rv_f, False, bits=bits), y, p_x, i_x, N, H, W, ymax=ymax)
    assert torch.equal(_bits(p_x), _bits(p_f)) and torch.equal(i_x, i_f)
    assert torch.equal(ymax.double().view(N, Ho, Wo, C), RR.maxpool_gather(y.view(N, H, W, C), code))
    assert torch.equal(bits, _pack(p_x))
    # the reductions over the POOLED positions (sum dpool * relu', sum dpool * relu' * (ymax - mean)), split over the replicas, drive the apply pass
    dzp = torch.where(p_x > 0, dpool, torch.zeros_like(dpool))
    S1p, S2p = dzp.double().sum(0), (dzp.double() * (ymax.double() - bn.mean)).sum(0)
    if dt == F32:          # no rounding of a pixel's summed gradient in f32: the same sums as over the un-pooled tensor
        assert bool(((S1p - b.S1).abs() <= 1e-4 * b.S1.abs().max()).all()) and bool(((S2p - b.S2).abs() <= 1e-4 * b.S2.abs().max()).all())
    ds_p = hip.Stats(_split(torch.stack([S1p, S2p]).float(), R_), R_, C)
    dy_p = _fill((M, C), td)
    hip.stem_bn_pool_bwd_apply(dt, d, dzp, i_x, y, ds_p, dy_p, None, None, N, H, W)
    rstd = 1.0 / torch.sqrt(bn.var + EPS)
    dy_pref = gamma.double() * rstd * (b.dz - S1p / M - xhat * rstd * S2p / M)
    _elem(tag + " pooled-operand dy", dy_p, dy_pref, dt)
    if dt == F32:
        _elem(tag + " pooled-operand dy vs dy", dy_p, b.dy, dt)


# ------------------------------------------------------------------------------------------------ d. average pool
@pytest.mark.parametrize("N,HW,C", [(5, 49, 2048), (1, 1, 8), (300, 49, 512), (37, 5, 136)])
@pytest.mark.parametrize("dt", DTS)
def test_avgpool_forward_backward_match_float64(dt, N, HW, C):
    hip = _hip()
    td = hip.TORCH_DTYPE[dt]
    g = _gen(N + HW + C)
    x = _randn(g, N, HW, C).to(td)
    out = _fill((N, C), td)
    hip.avgpool_fwd(dt, x, out, N, HW, C)
    _elem("avgpool out", out, RR.avgpool_ref(x), dt)
    dout = _randn(g, N, C).to(td)
    dx = _fill((N, HW, C), td)
    hip.avgpool_bwd(dt, dout, dx, N, HW, C)
    _elem("avgpool dx", dx, RR.avgpool_bwd_ref(dout, HW), dt)


# ------------------------------------------------------------------------------------------------ e. image_to_nhwc4
@pytest.mark.parametrize("N,H,W,pad,Hp,Wp,offset", [(2, 6, 5, 3, 12, 16, 0), (3, 8, 260, 3, 14, 272, 0), (3, 8, 260, 3, 14, 272, 1)])
@pytest.mark.parametrize("dt", DTS)
def test_image_to_nhwc4_whole_padded_output(dt, N, H, W, pad, Hp, Wp, offset):
    """W % 4 != 0: the scalar path; W = 260: the 16-byte vector path with 69 lane groups per row (a second trip of the lane loop) and Wp beyond
    W + 2 * pad; offset = 1: the same shape from a pointer that is 4 bytes off 16-byte alignment, which must fall back to scalar loads."""
    hip = _hip()
    td = hip.TORCH_DTYPE[dt]
    g = _gen(W + offset)
    base = _randn(g, N * 3 * H * W + offset)
    img = base[offset:].view(N, 3, H, W)
    assert img.data_ptr() % 16 == 4 * offset and img.is_contiguous()
    out = _fill((N, Hp, Wp, 4), td)
    hip.image_to_nhwc4(dt, img, out, N, H, W, pad, Hp, Wp)
    ref = RR.image_to_nhwc4_ref(img, pad, Hp, Wp)
    _elem("image_to_nhwc4", out, ref, dt)
    assert torch.equal(out.double(), RR.round_to(ref, td))          # a conversion: the correctly rounded value, zeros exactly zero


# ------------------------------------------------------------------------------------------------ f. colsum
@pytest.mark.parametrize("M,N", [(1001, 72), (333, 264), (1000, 64), (255, 64), (262184, 64)])
@pytest.mark.parametrize("dt", DTS)
def test_colsum_accumulates_onto_prefilled_output(dt, M, N):
    hip = _hip()
    td = hip.TORCH_DTYPE[dt]
    g = _gen(M + N)
    x = _randn(g, M, N).to(td)
    out0 = 1 + _randn(g, N)
    out = out0.clone()
    hip.colsum(dt, x, out, M, N)
    _reduction(f"colsum[{'bf16' if dt == BF16 else 'f32'},{M}x{N}]", out, out0.double() + RR.colsum_ref(x), x.double())


# ------------------------------------------------------------------------------------------------ g. deterministic-reduction mode
@pytest.mark.parametrize("M,C", [(1001, 64), (333, 1024)])
@pytest.mark.parametrize("dt", DTS)
def test_deterministic_batchnorm_reductions_repeat_bitwise(deterministic_reductions, dt, M, C):
    hip = _hip()
    assert hip.is_deterministic()
    td = hip.TORCH_DTYPE[dt]
    g = _gen(M + C)
    R_ = 3
    y = (_randn(g, M, C) * 2 + 0.5).to(td)
    out, dout = _randn(g, M, C).to(td), _randn(g, M, C).to(td)
    gamma = 1 + 0.1 * _randn(g, C)
    b = RR.bn_bwd_ref(dout, out, y, gamma, EPS)
    yc = y.double() - y.double().mean(0)
    tag = f"det bn[{'bf16' if dt == BF16 else 'f32'},{M}x{C}]"
    runs = []
    for _ in range(2):
        st = _stats(hip, y, R_)
        dst = hip.Stats(torch.zeros(R_, 3, C, device=DEV), R_, C)
        hip.bn_bwd_reduce(dt, dout, out, y, st, dst, M, C)
        hip.bn_centered_var(dt, y, st, M, C)
        runs.append((dst.t.clone(), st.t.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    tot = runs[0][0].double().sum(0).float()
    _reduction(tag + " S1", tot[0], b.S1, b.dz)
    _reduction(tag + " S2", tot[1], b.S2, b.dz * yc)
    _reduction(tag + " centered", runs[0][1][:, 2].double().sum(0).float(), (yc * yc).sum(0), yc * yc)


@pytest.mark.parametrize("dt", DTS)
def test_deterministic_stem_reduce_and_colsum_repeat_bitwise(deterministic_reductions, dt):
    hip = _hip()
    assert hip.is_deterministic()
    N, H, W, C, R_ = 7, 11, 13, 64, 3                      # M = 1001
    td, g, M, y, gamma, beta, st = _stem_problem(hip, dt, N, H, W, C, R_, seed=5)
    Ho, Wo = RR.pool_out(H), RR.pool_out(W)
    P = N * Ho * Wo
    tag = f"det stem[{'bf16' if dt == BF16 else 'f32'},{M}x{C}]"
    rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    d = hip.bn_desc(M, C, st, gamma, beta, rm, rv, True, False, MOM, EPS, True)
    pooled, idx = _fill((P, C), td), torch.full((P, C), 255, device=DEV, dtype=torch.uint8)
    hip.stem_bn_pool_fwd(dt, d, y, pooled, idx, N, H, W)
    dpool = _randn(g, P, C).to(td)
    runs = []
    for _ in range(2):
        ds = hip.Stats(torch.zeros(R_, 3, C, device=DEV), R_, C)
        dy = _fill((M, C), td)
        hip.stem_bn_pool_bwd(dt, d, dpool, idx, y, ds, dy, None, None, N, H, W)
        runs.append((ds.t.clone(), dy.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(_bits(runs[0][1]), _bits(runs[1][1]))
    bn = RR.bn_train_ref(y, gamma, beta, EPS, relu=True)
    a0r = RR.round_to(bn.out, td)
    val, code = RR.maxpool_ref(a0r.view(N, H, W, C))
    assert torch.equal(idx.view(N, Ho, Wo, C).long(), code)
    da0 = RR.round_to(RR.maxpool_bwd_ref(dpool.view(N, Ho, Wo, C), code, H, W), td).view(M, C)
    b = RR.bn_bwd_ref(da0, a0r, y, gamma, EPS)
    tot = runs[0][0].double().sum(0).float()
    _reduction(tag + " S1", tot[0], b.S1, b.dz)
    _reduction(tag + " S2", tot[1], b.S2, b.dz * (y.double() - bn.mean))
    _elem(tag + " dy", runs[0][1], b.dy, dt)

    x = _randn(g, M, C).to(td)
    out0 = 1 + _randn(g, C)
    outs = []
    for _ in range(2):
        o = out0.clone()
        hip.colsum(dt, x, o, M, C)
        outs.append(o)
    assert torch.equal(outs[0], outs[1])
    _reduction(f"det colsum[{'bf16' if dt == BF16 else 'f32'},{M}x{C}]", outs[0], out0.double() + RR.colsum_ref(x), x.double())
