"""GPU checks, at kernel level and through the C ABI, of what the trained configuration (bf16, BERT dropout 0.1) runs and no other GPU test
compares with a reference:

B.1  BERT's four compile-time epilogue forms (gemm_wide.hip bert_form 3 - 6: FFN1 forward, FFN2's input gradient, the output projections, the
     residual-stream input gradients) on every tile family and on the 4-wave run-time-flag epilogue, and their exact-f32 counterparts, against
     float64 from the same (bf16-rounded) operands;
B.2  the bf16 epilogues' fast GELU (igemm.h gelu_fast_parts: hardware reciprocal and exp2) over every finite bf16 input;
B.3  every writer and every regenerator of a dropout mask against tests/dropout_ref.py, element for element: the GEMM epilogues, LayerNorm forward,
     LayerNorm backward's drop_in and drop_out, the attention kernels of both pitches, by-value and indirect seeds; and clite_uniform_fill.

Bounds. Outputs and stored pre-activations: 6e-3 of max|ref| for bf16 stores (tests/test_gpu_igemm.py), 1e-4 for f32. Column sums against the
sum of the STORED output: rows * 2^-23 * sum|stored| per column (twice the worst case of an f32 sum in any order). Masks: set equality.
Fast GELU: three times what tests/test_dropout_ref_host.py asserts for the float32 emulation with exact division and exp2 (the hardware
reciprocal and exp2 are ~1 ulp each and each adds at most 1.2e-7 to a quantity <= 0.5, doubling the emulation's error at worst; the third
multiple is margin)."""
import numpy as np
import pytest
import torch

import attention_long_ref as AR
import dropout_ref as D

pytestmark = pytest.mark.gpu
BF16, F32 = 0, 1
DEV = "cuda"
TD = {BF16: torch.bfloat16, F32: torch.float32}
P, SEED = 0.1, 20240607 + (3 << 32)          # (a seed that uses both key words)
SHAPES = [(200, 136, 104), (300, 264, 128), (180, 768, 768)]
MODES = [(BF16, 0), (BF16, 1), (BF16, 2), (BF16, 3), (BF16, 4), (F32, 0)]
MODE_IDS = ["bf16-auto", "bf16-w128", "bf16-w256x128", "bf16-w256", "bf16-narrow", "f32"]
BF16_MODES, BF16_IDS = MODES[:5], MODE_IDS[:5]


@pytest.fixture
def tile_policy(request):
    """The forced tile family of this case (include/clite.h: clite_set_tile_policy; 0 = automatic), as the autouse fixture of tests/test_gpu_igemm.py
    sets it; policy 0 is restored afterwards. f32 launches do not depend on the policy and run under 0 only."""
    from clip_lite_amd import hip
    hip.set_tile_policy(request.param)
    yield request.param
    hip.set_tile_policy(0)


def modes(which=MODES, ids=MODE_IDS):
    return pytest.mark.parametrize("dt,tile_policy", which, ids=ids, indirect=["tile_policy"])


def _hip():
    from clip_lite_amd import hip
    return hip


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _t(shape, g, dt, scale=1.0, shift=0.0):
    """Random operand as the kernels read it (device, compute dtype) and its exact values in float64 on the host."""
    x = (torch.randn(*shape, generator=g) * scale + shift).to(TD[dt])
    return x.to(DEV), x.double()


def _tol(dt):
    return 6e-3 if dt == BF16 else 1e-4


def _check(name, got, ref, tol):
    err = ((got.double().cpu() - ref).abs().max() / ref.abs().max().clamp_min(1e-6)).item()
    print(f"{name}: {err:.3e} of max|ref| (bound {tol:.0e})")
    assert err <= tol, (name, err)


def _gelu64(x):
    g, dg = D.gelu_exact(x.numpy())
    return torch.from_numpy(g), torch.from_numpy(dg)


# ================================================================================================ B.1 the four forms
@modes()
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_ffn1_forward_bias_preactivation_gelu(dt, tile_policy, M, N, K):
    """bert.py's FFN1: out = GELU(A B^T + bias), the pre-activation stored beside it (form 3)."""
    hip = _hip()
    g = _gen(M + N + K)
    (A, A64), (B, B64) = _t((M, K), g, dt), _t((N, K), g, dt, K ** -0.5)
    bias = torch.randn(N, generator=g)
    out, pre = torch.empty(M, N, device=DEV, dtype=TD[dt]), torch.empty(M, N, device=DEV, dtype=TD[dt])
    bias_d = bias.to(DEV)          # (every operand stays referenced until the results are read)
    hip.gemm_nt(dt, A, B, M, N, K, hip.epilogue(out, N, bias=bias_d, act=hip.ACT_GELU, preact=pre))
    z = A64 @ B64.t() + bias.double()
    _check("pre-activation", pre, z, _tol(dt))
    _check("GELU", out, _gelu64(z)[0], _tol(dt))


@modes()
@pytest.mark.parametrize("with_sums", [True, False], ids=["colsum", "nosum"])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_ffn2_input_gradient_gelu_derivative_and_bias_gradient(dt, tile_policy, M, N, K, with_sums):
    """bert.py's FFN2 input gradient: out = (A B^T) * GELU'(aux), with the column sums of what was stored added into row 0 of the sums buffer
    (colsum_rows = 1: the floats behind row 0 stay as they were) and without them (form 4)."""
    hip = _hip()
    g = _gen(M + N + K + 1)
    (A, A64), (B, B64), (aux, aux64) = _t((M, K), g, dt), _t((N, K), g, dt, K ** -0.5), _t((M, N), g, dt, 1.5)
    out = torch.empty(M, N, device=DEV, dtype=TD[dt])
    sums = torch.full((2, N), 7.0, device=DEV)
    sums[0] = 0.0
    hip.gemm_nt(dt, A, B, M, N, K, hip.epilogue(out, N, dact_aux=aux, dact=hip.DACT_GELU, colsum=sums if with_sums else None, colsum_rows=1))
    _check("dz * GELU'", out, (A64 @ B64.t()) * _gelu64(aux64)[1], _tol(dt))
    stored = out.double().cpu()
    if with_sums:
        err = (sums[0].double().cpu() - stored.sum(0)).abs()
        bound = M * 2.0 ** -23 * stored.abs().sum(0)
        print(f"column sums: worst error / bound {(err / bound).max().item():.3f}")
        assert (err <= bound).all()
    else:
        assert (sums[0] == 0.0).all()
    assert (sums[1] == 7.0).all()


@modes()
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_output_projection_bias_dropout_residual(dt, tile_policy, M, N, K):
    """bert.py's output projections: out = dropout(A B^T + bias) + residual (form 5). With z + bias near 4 and the residual in [-1, 1] an element
    was dropped exactly when the output IS the residual, bit for bit: the dropped set must be the complement of the numpy mask of
    (seed, site, row * N + col), and the kept elements (z + bias) / (1 - p) + residual."""
    hip = _hip()
    g = _gen(M + N + K + 2)
    (A, A64), (B, B64) = _t((M, K), g, dt, 0.3), _t((N, K), g, dt, 0.3 * K ** -0.5)
    bias = 4.0 + 0.1 * torch.randn(N, generator=g)
    res = (torch.rand(M, N, generator=g) * 2 - 1).to(TD[dt])
    out = torch.empty(M, N, device=DEV, dtype=TD[dt])
    site = 3
    bias_d, res_d = bias.to(DEV), res.to(DEV)
    hip.gemm_nt(dt, A, B, M, N, K, hip.epilogue(out, N, bias=bias_d, drop=(P, SEED, site), residual=res_d))
    got = out.cpu()
    keep = torch.from_numpy(D.hidden_keep(SEED, site, M, N, P))
    z = A64 @ B64.t() + bias.double()
    assert z.abs().min() > 3.0
    dropped = got == res
    assert abs(keep.double().mean().item() - 0.9) < 0.01
    assert torch.equal(dropped, ~keep), f"{(dropped != ~keep).sum().item()} elements differ from the numpy mask"
    ref = z / (1.0 - float(np.float32(P))) * keep + res.double()
    _check("dropout + residual", got, ref, _tol(dt))


@modes()
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_residual_stream_input_gradient(dt, tile_policy, M, N, K):
    """bert.py's residual-stream input gradients: out = A B^T + residual (form 6)."""
    hip = _hip()
    g = _gen(M + N + K + 3)
    (A, A64), (B, B64), (res, res64) = _t((M, K), g, dt), _t((N, K), g, dt, K ** -0.5), _t((M, N), g, dt)
    out = torch.empty(M, N, device=DEV, dtype=TD[dt])
    hip.gemm_nt(dt, A, B, M, N, K, hip.epilogue(out, N, residual=res))
    _check("+ residual", out, A64 @ B64.t() + res64, _tol(dt))


# ================================================================================================ B.2 the fast GELU on hardware
def _all_bf16():
    """[512][128] bf16 tensor holding every finite bf16 value (65 280 of them; the rest zeros) and the values in float64."""
    v = np.zeros(512 * 128, np.float32)
    v[:65280] = D.finite_bf16_values()
    x = torch.from_numpy(v).view(512, 128)
    return x.bfloat16().to(DEV), x.double()


def _identity_problem():
    """(A, B) with A B^T = the values exactly: B = I."""
    vals, x64 = _all_bf16()
    return vals, torch.eye(128).bfloat16().to(DEV), x64


def _ones_problem():
    """(A, B) with every accumulator exactly 1: first column of both = 1, the rest 0."""
    A, B = torch.zeros(512, 128), torch.zeros(128, 128)
    A[:, 0], B[:, 0] = 1.0, 1.0
    return A.bfloat16().to(DEV), B.bfloat16().to(DEV)


def _bf16_ordinal(t):
    """bf16 tensor -> int32 position on the number line of bf16 values (-0 and +0 coincide): neighbours differ by 1."""
    bits = t.contiguous().view(torch.int16).int() & 0xFFFF
    mag = bits & 0x7FFF
    return torch.where(bits >= 0x8000, -mag, mag)


def _within_one_bf16_ulp(got, ref64):
    want = ref64.float().bfloat16()
    d = (_bf16_ordinal(got.cpu()) - _bf16_ordinal(want)).abs()
    return (d <= 1) | ((got.cpu().double() - ref64).abs() <= 1e-30)


@modes(BF16_MODES, BF16_IDS)
def test_fast_gelu_on_hardware_over_every_finite_bf16(dt, tile_policy):
    """Every finite bf16 value through gelu_t<bf16> with no GEMM rounding (A = the values, B = I, f32 output: the run-time-flag epilogue), against
    float64 x Phi(x). Bound 3 * 1.35e-7 * max(1, |x|) = 4.05e-7 * max(1, |x|); no NaN. Observed on MI355X: 1.134e-7 * max(1, |x|) under every
    tile policy, which is the figure of the float32 emulation with exact division and exp2 as well."""
    hip = _hip()
    A, B, x64 = _identity_problem()
    out = torch.empty(512, 128, device=DEV)
    hip.gemm_nt(BF16, A, B, 512, 128, 128, hip.epilogue(out, 128, act=hip.ACT_GELU, out_f32=True))
    got = out.double().cpu()
    assert not torch.isnan(got).any()
    err = ((got - _gelu64(x64)[0]).abs() / x64.abs().clamp_min(1.0)).max().item()
    print(f"fast GELU on hardware: {err:.3e} * max(1, |x|) (bound {3 * D.GELU_EMU_ERR:.3e})")
    assert err <= 3 * D.GELU_EMU_ERR


@modes(BF16_MODES, BF16_IDS)
def test_fast_gelu_derivative_on_hardware_over_every_finite_bf16(dt, tile_policy):
    """Every finite bf16 value through gelu_grad_t<bf16> as dact_aux under accumulators that are exactly 1, f32 output, against float64
    Phi(x) + x phi(x). Bound 3 * 2.68e-7 = 8.04e-7; no NaN. Observed on MI355X: 2.279e-7 under every tile policy (emulation: 2.676e-7)."""
    hip = _hip()
    A, B = _ones_problem()
    aux, x64 = _all_bf16()
    out = torch.empty(512, 128, device=DEV)
    hip.gemm_nt(BF16, A, B, 512, 128, 128, hip.epilogue(out, 128, dact_aux=aux, dact=hip.DACT_GELU, out_f32=True))
    got = out.double().cpu()
    assert not torch.isnan(got).any()
    err = (got - _gelu64(x64)[1]).abs().max().item()
    print(f"fast GELU' on hardware: {err:.3e} (bound {3 * D.GELU_GRAD_EMU_ERR:.3e})")
    assert err <= 3 * D.GELU_GRAD_EMU_ERR


def _ulp_report(name, got, ref64, x64):
    ok = _within_one_bf16_ulp(got, ref64)
    bad = ~ok
    if bad.any():
        d = (_bf16_ordinal(got.cpu()) - _bf16_ordinal(ref64.float().bfloat16())).abs()[bad]
        print(f"{name}: {int(bad.sum())} of 65280 inputs off by more than one bf16 ulp (up to {int(d.max())}), x in [{x64[bad].min().item():.5g}, "
              f"{x64[bad].max().item():.5g}], largest |reference| among them {ref64[bad].abs().max().item():.3e}")
    else:
        print(f"{name}: every input within one bf16 ulp")
    return int(bad.sum())


@modes(BF16_MODES, BF16_IDS)
def test_stored_bf16_gelu_forms_are_within_one_ulp(dt, tile_policy):
    """Forms 3 and 4 (bf16 stores) on the same inputs: each output within one bf16 ulp of the float64 value rounded to bf16 (+ 1e-30 absolute:
    whether the bf16 MFMA flushes subnormal inputs is not relied on), the stored pre-activation likewise.

    The tail polynomial of igemm.h (gelu_fast_parts<TAIL>, taken below x = -5) is what meets this: Abramowitz & Stegun 7.1.26 alone bounds the
    ABSOLUTE error of erfc, and was off by up to 5 ulps on 72 inputs of GELU (x in [-11.31, -6.75]) and by up to 8 ulps on 132 inputs of GELU'
    (x in [-11.44, -5.34], where 0.5 - (0.5 - h) also cancels h away). MI355X, every tile policy: no input outside the bound."""
    hip = _hip()
    A, B, x64 = _identity_problem()
    g64, dg64 = _gelu64(x64)
    out, pre = torch.empty(512, 128, device=DEV, dtype=torch.bfloat16), torch.empty(512, 128, device=DEV, dtype=torch.bfloat16)
    zero_bias = torch.zeros(128, device=DEV)
    hip.gemm_nt(BF16, A, B, 512, 128, 128, hip.epilogue(out, 128, bias=zero_bias, act=hip.ACT_GELU, preact=pre))
    A1, B1 = _ones_problem()
    aux, _ = _all_bf16()
    out4 = torch.empty(512, 128, device=DEV, dtype=torch.bfloat16)
    hip.gemm_nt(BF16, A1, B1, 512, 128, 128, hip.epilogue(out4, 128, dact_aux=aux, dact=hip.DACT_GELU, colsum_rows=1))
    assert not torch.isnan(out.float()).any() and not torch.isnan(out4.float()).any()
    n_pre = _ulp_report("stored pre-activation", pre, x64, x64)
    n3 = _ulp_report("form 3, GELU", out, g64, x64)
    n4 = _ulp_report("form 4, GELU'", out4, dg64, x64)
    assert n_pre == 0
    assert n3 == 0 and n4 == 0, (n3, n4)


# ================================================================================================ B.3 masks
def _seed_arg(indirect, site):
    """(seed argument, site argument, tensor to keep alive): by value, or the device address of an int64 holding the seed with bit 31 of the site set."""
    if not indirect:
        return SEED, site, None
    cell = torch.tensor([SEED], dtype=torch.int64).to(DEV)
    return cell.data_ptr(), site | _hip().SEED_INDIRECT, cell


def _keep_fraction_ok(keep):
    return abs(float(keep.mean()) - 0.9) < 0.01


@modes()
@pytest.mark.parametrize("indirect", [False, True], ids=["byvalue", "indirect"])
@pytest.mark.parametrize("M,N,K", [(200, 136, 104), (180, 768, 768)])
def test_gemm_epilogue_writes_the_numpy_mask(dt, tile_policy, M, N, K, indirect):
    """A = 0, bias = 1, residual = 0: out != 0 is the mask the epilogue applied (bf16: form 5 on the 8-wave tiles, the run-time-flag epilogue on the
    4-wave kernel; f32: the exact-f32 kernel's)."""
    hip = _hip()
    A, B = torch.zeros(M, K, device=DEV, dtype=TD[dt]), torch.ones(N, K, device=DEV, dtype=TD[dt])
    out = torch.empty(M, N, device=DEV, dtype=TD[dt])
    seed, site, cell = _seed_arg(indirect, 11)
    bias, res = torch.ones(N, device=DEV), torch.zeros(M, N, device=DEV, dtype=TD[dt])
    hip.gemm_nt(dt, A, B, M, N, K, hip.epilogue(out, N, bias=bias, drop=(P, seed, site), residual=res))
    got = out.float().cpu().numpy()
    keep = D.hidden_keep(SEED, 11, M, N, P)
    assert _keep_fraction_ok(keep)
    assert ((got != 0) == keep).all(), f"{((got != 0) != keep).sum()} elements differ"
    assert np.abs(got[keep] - 1 / 0.9).max() <= 2.0 ** -8 * (1 / 0.9)


@pytest.mark.parametrize("dt", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("indirect", [False, True], ids=["byvalue", "indirect"])
@pytest.mark.parametrize("M,Cc", [(180, 768), (50, 2048)])
def test_layernorm_forward_writes_the_numpy_mask(dt, M, Cc, indirect):
    """Random input, beta = 0.1 (no output is exactly 0 unless dropped): out != 0 is the mask. 768 columns take the two-chunk kernel, 2048 the
    four-chunk one."""
    hip = _hip()
    x, _ = _t((M, Cc), _gen(M + Cc), dt)
    gamma, beta = torch.ones(Cc, device=DEV), torch.full((Cc,), 0.1, device=DEV)
    out, st = torch.empty_like(x), torch.empty(M, 2, device=DEV)
    seed, site, cell = _seed_arg(indirect, 7)
    hip.layernorm_fwd(dt, x, gamma, beta, 1e-12, out, st, M, Cc, (P, seed, site))
    plain = torch.empty_like(x)
    hip.layernorm_fwd(dt, x, gamma, beta, 1e-12, plain, st, M, Cc)
    assert (plain.float() != 0).all()
    keep = D.hidden_keep(SEED, 7, M, Cc, P)
    assert _keep_fraction_ok(keep)
    assert ((out.float().cpu().numpy() != 0) == keep).all()
    _check("kept values", out, plain.double().cpu() * torch.from_numpy(keep) / 0.9, 1e-2 if dt == BF16 else 1e-5)


@pytest.mark.parametrize("dt", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("M,Cc", [(180, 768), (50, 2048)])
def test_layernorm_backward_regenerates_the_numpy_masks(dt, M, Cc):
    """clite_layernorm_bwd with gamma = 1.
    drop_out (the mask of the dropout in front of the producer's residual add, applied to the second output): dx_masked != 0, with dx itself
    non-zero everywhere, is the mask; it is checked with drop_in on as well.
    drop_in (the mask of the dropout behind this LayerNorm, applied to dy): recovered exactly from dbeta = the column sums of the masked dy. Rows
    are taken 16 at a time with dy[r][c] = 2^(r mod 16) (zero elsewhere), so dbeta[c] * (1 - p) is the integer whose bit k says whether row
    16 * group + k kept column c; the sums stay below 2^16 / 0.9, where f32 sums in any order decode without ambiguity."""
    hip = _hip()
    g = _gen(M * Cc)
    x, _ = _t((M, Cc), g, dt)
    gamma, beta = torch.ones(Cc, device=DEV), torch.zeros(Cc, device=DEV)
    y, st = torch.empty_like(x), torch.empty(M, 2, device=DEV)
    hip.layernorm_fwd(dt, x, gamma, beta, 1e-12, y, st, M, Cc)
    d_in, d_out = (P, SEED, 4), (P, SEED, 6)
    keep_in, keep_out = D.hidden_keep(SEED, 4, M, Cc, P), D.hidden_keep(SEED, 6, M, Cc, P)
    assert _keep_fraction_ok(keep_in) and _keep_fraction_ok(keep_out) and not (keep_in == keep_out).all()
    dy, _ = _t((M, Cc), g, dt)
    for din in (hip.NO_DROP, d_in):
        dx, dxm = torch.empty_like(x), torch.empty_like(x)
        hip.layernorm_bwd(dt, dy, x, st, gamma, dx, dxm, None, None, M, Cc, din, d_out)
        assert (dx.float() != 0).all()
        assert ((dxm.float().cpu().numpy() != 0) == keep_out).all()
        _check("masked gradient", dxm, dx.double().cpu() * torch.from_numpy(keep_out) / 0.9, 1e-2 if dt == BF16 else 1e-5)
    got = np.zeros((M, Cc), bool)
    for r0 in range(0, M, 16):
        rows = min(16, M - r0)
        dyb = torch.zeros(M, Cc)
        dyb[r0:r0 + rows] = (2.0 ** torch.arange(rows))[:, None]
        dbeta, dyb_d, dxb = torch.zeros(Cc, device=DEV), dyb.to(TD[dt]).to(DEV), torch.empty_like(x)
        hip.layernorm_bwd(dt, dyb_d, x, st, gamma, dxb, None, None, dbeta, M, Cc, d_in)
        code = dbeta.double().cpu().numpy() * (1.0 - float(np.float32(P)))
        n = np.rint(code).astype(np.int64)
        assert np.abs(code - n).max() < 0.05 and n.min() >= 0 and n.max() < 2 ** rows
        for k in range(rows):
            got[r0 + k] = (n >> k) & 1
    assert (got == keep_in).all(), f"{(got != keep_in).sum()} elements differ"


@pytest.mark.parametrize("B,L,H", [(3, 30, 4), (2, 40, 2)])
def test_attention_kernels_draw_the_numpy_mask(B, L, H):
    """The V = identity-columns probe of tests/test_gpu_ops.py (ctx[i][j] is then the dropped probability of key j) on the exact-f32 kernel, with
    and without dropout: the kept set of every attended (i, j) must be attention_keep's (element index ((b * H + h) * P + i) * P + j, P = 32 for
    30 tokens and 128 for 40). The f32 and the bf16 MFMA kernels, forward and backward, must then match a float64 attention that uses the numpy
    mask: f32 1e-5, bf16 1e-2 forward and 2e-2 backward of max|ref| (tests/test_gpu_ops.py)."""
    hip = _hip()
    g = _gen(B * 100 + L)
    qkv = (torch.randn(B * L, 3 * H * 64, generator=g) * 0.7).bfloat16().float()
    dctx = torch.randn(B * L, H * 64, generator=g).bfloat16().float()
    mask = torch.ones(B, L, dtype=torch.long)
    mask[1, L - 9:] = 0
    drop = (P, SEED, 9)
    probe = AR.one_hot_probe(qkv, B, L, H, 0).to(DEV)
    pd, p0 = torch.empty(B * L, H * 64, device=DEV), torch.empty(B * L, H * 64, device=DEV)
    mask_d = mask.to(DEV)
    hip.attention_fwd(F32, probe, mask_d, pd, B, L, H, drop)
    hip.attention_fwd(F32, probe, mask_d, p0, B, L, H)
    pd, p0 = (t.cpu().view(B, L, H, 64)[..., :L].permute(0, 2, 1, 3).numpy() for t in (pd, p0))          # [B][H][i][j]
    valid = np.broadcast_to((mask != 0).numpy()[:, None, None, :], p0.shape)
    assert (p0[valid] > 1e-20).all()
    keep = D.attention_keep(SEED, 9, B, H, L, P)
    assert _keep_fraction_ok(keep)
    assert ((pd[valid] != 0) == keep[valid]).all(), f"{((pd != 0) != keep)[valid].sum()} elements differ"
    mult = torch.from_numpy(keep.astype(np.float64)) / (1.0 - float(np.float32(P)))
    ref_ctx, ref_dqkv = AR.reference(qkv, mask, dctx, B, L, H, keep=mult)
    for dt, fwd, bwd in ((F32, 1e-5, 1e-5), (BF16, 1e-2, 2e-2)):
        x, d = qkv.to(TD[dt]).to(DEV), dctx.to(TD[dt]).to(DEV)
        ctx, dqkv = torch.empty(B * L, H * 64, device=DEV, dtype=TD[dt]), torch.empty_like(x)
        hip.attention_fwd(dt, x, mask_d, ctx, B, L, H, drop)
        hip.attention_bwd(dt, x, mask_d, d, dqkv, B, L, H, drop)
        _check("attention forward", ctx, ref_ctx, fwd)
        _check("attention backward", dqkv, ref_dqkv, bwd)


def test_uniform_fill_is_the_numpy_stream():
    """clite_uniform_fill (the prior noise): f32 output bitwise equal to the numpy stream and in [0, 1); bf16 output = that value rounded to bf16."""
    hip = _hip()
    n = 20000
    ref = D.uniform8(SEED, 2, n)
    u = torch.empty(n, device=DEV)
    hip.uniform_fill(F32, u, n, SEED, 2)
    got = u.cpu().numpy()
    assert (got.view(np.uint32) == ref.view(np.uint32)).all() and got.min() >= 0 and got.max() < 1
    ub = torch.empty(n, device=DEV, dtype=torch.bfloat16)
    hip.uniform_fill(BF16, ub, n, SEED, 2)
    assert torch.equal(ub.cpu(), torch.from_numpy(ref).bfloat16())
