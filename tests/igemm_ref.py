"""float64 references of the implicit-GEMM convolutions and of their BatchNorm-backward / forward-statistics epilogues (csrc/igemm.h: igemm_epilogue_bn,
csrc/igemm_wide.h: wide_epilogue_bn, csrc/gemm.hip: colstats_det_kernel), written from their definitions on plain torch tensors, and the bounds the
tests hold the kernels to. Nothing here calls into clip_lite_amd: tests/test_igemm_ref_host.py checks every function against an independent
formulation (autograd of torch.nn.functional.conv2d, explicit loops) and runs one tiny case per epilogue form through the wave simulator;
tests/test_gpu_dgrad_epilogue.py compares the HIP kernels with them on an MI355X.

Layouts are the kernels': activations and gradients NHWC (the GEMM sees them as [rows][channels]), weights KRSC. Inputs of any float type are
upcast; every result is float64 on the inputs' device.

The two bounds (both derived, neither measured):
  elements     |got - v| <= rho * |v| + Ktot * 2^-23 * S
               rho = 2^-8 for bf16 storage (round to nearest: half an ulp of a value with 8 significant bits), 2^-23 for f32 storage. S is the
               same expression as v with every operand replaced by its magnitude (S_acc = dgrad of |dy| and |w|; S = |alpha| S_acc + |bias| + |r|):
               an f32 accumulation of Ktot exact bf16 products in ANY order is off by at most Ktot * 2^-24 * S_acc, the alpha / bias / residual
               steps add three more roundings of at most 2^-24 * S each; the term is that, doubled.
  reductions   per channel |got - ref| <= 1e-4 * max|ref| (the project's reduction bound, tests/test_gpu_resnet_ops.py), with ref evaluated in
               float64 on the tensor the kernel STORED. assert_reductions prints the measured |got - ref| / sum|terms| and the same figure of a
               plain torch.float32 .sum(0) of the terms beside it; neither figure feeds the bound."""
from collections import namedtuple

import torch

from resnet_ref import round_to  # noqa: F401  (re-exported: the storage rounding of the references)

Epi = namedtuple("Epi", "v S m")
BnRed = namedtuple("BnRed", "S1 S2 Sq mean t1 t2 tq")

RHO_BF16, RHO_F32, U23 = 2.0 ** -8, 2.0 ** -23, 2.0 ** -23


def conv_out(n, r, stride, pad):
    return (n + 2 * pad - r) // stride + 1


def dgrad_ref(dy, w_krsc, N, H, W, stride, pad):
    """Input gradient of the convolution y[n][ho][wo][k] = sum_{r,s,c} x[n][ho*stride - pad + r][wo*stride - pad + s][c] * w[k][r][s][c] as the
    scatter its definition gives: every output pixel adds dy[n][ho][wo][:] @ w[:][r][s][:] to the input pixel each tap read.
    dy [N][Ho][Wo][K] (or [N*Ho*Wo][K]), w_krsc [K][R][S][C]; returns float64 [N*H*W][C]."""
    K, R, S, C = w_krsc.shape
    Ho, Wo = conv_out(H, R, stride, pad), conv_out(W, S, stride, pad)
    dy = dy.double().reshape(N, Ho, Wo, K)
    w = w_krsc.double()
    Hp, Wp = max(H + 2 * pad, (Ho - 1) * stride + R), max(W + 2 * pad, (Wo - 1) * stride + S)
    dxp = dy.new_zeros(N, Hp, Wp, C)
    for r in range(R):
        for s in range(S):
            dxp[:, r:r + stride * Ho:stride, s:s + stride * Wo:stride] += dy @ w[:, r, s, :]
    return dxp[:, pad:pad + H, pad:pad + W].reshape(N * H * W, C).contiguous()


def dgrad_scale(dy, w_krsc, N, H, W, stride, pad):
    """S_acc of dgrad_ref: the same sum over the operands' magnitudes."""
    return dgrad_ref(dy.double().abs(), w_krsc.double().abs(), N, H, W, stride, pad)


def conv_fwd_ref(x, w_krsc, stride, pad):
    """x [N][H][W][C], w_krsc [K][R][S][C] -> float64 [N*Ho*Wo][K], tap by tap over the zero-padded input."""
    N, H, W, C = x.shape
    K, R, S, _ = w_krsc.shape
    Ho, Wo = conv_out(H, R, stride, pad), conv_out(W, S, stride, pad)
    x, w = x.double(), w_krsc.double()
    xp = x.new_zeros(N, max(H + 2 * pad, (Ho - 1) * stride + R), max(W + 2 * pad, (Wo - 1) * stride + S), C)
    xp[:, pad:pad + H, pad:pad + W] = x
    out = x.new_zeros(N, Ho, Wo, K)
    for r in range(R):
        for s in range(S):
            out += xp[:, r:r + stride * Ho:stride, s:s + stride * Wo:stride] @ w[:, r, s, :].t()
    return out.reshape(N * Ho * Wo, K)


def conv_fwd_scale(x, w_krsc, stride, pad):
    return conv_fwd_ref(x.double().abs(), w_krsc.double().abs(), stride, pad)


def unpack_bits(bits, C):
    """uint8 [M][>= C / 8] (bit e of byte (m, c / 8) = mask of column c + e: clite_bn.relu_bits) -> bool [M][C]."""
    b = bits.to(torch.int64)[:, :C // 8]
    e = torch.arange(8, device=bits.device)
    return ((b[:, :, None] >> e) & 1).reshape(b.shape[0], -1).bool()


def pack_bits(mask):
    """bool [M][C] -> uint8 [M][C / 8], the inverse of unpack_bits."""
    w = (2 ** torch.arange(8, device=mask.device)).to(torch.int32)
    return (mask.view(mask.shape[0], -1, 8).to(torch.int32) * w).sum(-1).to(torch.uint8)


def epilogue_ref(acc, S_acc, alpha=1.0, bias=None, bits=None, aux=None, residual=None, mask_after_residual=False):
    """v = (alpha * acc + bias) * m + r (mask before the residual) or (alpha * acc + bias + r) * m (after it). m = the packed `bits`, or aux > 0,
    or 1 without either; r = `residual` [M][C] or nothing. Returns (v, S, m): S = |alpha| * S_acc + |bias| + |r|, m as float64 0 / 1."""
    acc, S = acc.double(), abs(alpha) * S_acc.double()
    a = alpha * acc
    if bias is not None:
        a = a + bias.double()
        S = S + bias.double().abs()
    if bits is not None:
        m = unpack_bits(bits, acc.shape[1]).double()
    elif aux is not None:
        m = (aux.double() > 0).double()
    else:
        m = torch.ones_like(acc)
    if residual is None:
        return Epi(a * m, S, m)
    r = residual.double()
    return Epi((a + r) * m if mask_after_residual else a * m + r, S + r.abs(), m)


def subsample_expand(compact, N, H, W):
    """The compact [N][H/2][W/2][C] gradient of a stride-2 shortcut on the even pixels of the [N][H][W] grid, zero elsewhere: [N*H*W][C]."""
    C = compact.shape[-1]
    full = compact.new_zeros(N, H, W, C, dtype=torch.float64)
    full[:, ::2, ::2] = compact.double().reshape(N, H // 2, W // 2, C)
    return full.reshape(N * H * W, C)


def scatter_rows(N, Ho, Wo, H, W, stride, off_h=0, off_w=0):
    """Rows of the [N*H*W] pixel list that GEMM rows (n, ho, wo) of an [N][Ho][Wo] grid land on: pixel (n, ho*stride + off_h, wo*stride + off_w).
    int64 [N*Ho*Wo], in GEMM-row order (csrc/igemm.h: map_row)."""
    n = torch.arange(N)[:, None, None]
    ho = torch.arange(Ho)[None, :, None]
    wo = torch.arange(Wo)[None, None, :]
    return ((n * H + ho * stride + off_h) * W + wo * stride + off_w).reshape(-1)


def bn_reductions_ref(stored, y=None, stats_f32=None, inv_count_f32=None):
    """The statistics an epilogue accumulates, of the tensor it STORED [M][C]: S1 = sum v; with y (the BatchNorm input, [M][C]) S2 = sum v * (y - mean),
    mean = (float64 sum of row 0 of the f32 replicas stats_f32 [R][3][C]) * (the f32 inv_count); Sq = sum v^2 (the forward form). t1 / t2 / tq are
    the summed terms [M][C]."""
    v = stored.double()
    S2 = mean = t2 = None
    if y is not None:
        assert stats_f32.dtype == torch.float32
        inv = torch.tensor(inv_count_f32, dtype=torch.float32).double()
        mean = stats_f32[:, 0].double().sum(0) * inv
        t2 = v * (y.double() - mean)
        S2 = t2.sum(0)
    tq = v * v
    return BnRed(v.sum(0), S2, tq.sum(0), mean, v, t2, tq)


# ------------------------------------------------------------------------------------------------ bounds
def elem_bound(v, S, Ktot, rho):
    return rho * v.abs() + Ktot * U23 * S


def assert_elements(what, got, e, Ktot, rho):
    """got [M][C] (any float type) against e = Epi(v, S, m): every element inside the bound, finite, and exactly 0 where the mask is 0 and nothing
    was added after it (v == 0 there by construction: those are the elements with m == 0 and v == 0)."""
    g = got.double()
    assert g.shape == e.v.shape, (what, g.shape, e.v.shape)
    assert bool(torch.isfinite(g).all()), f"{what}: non-finite values stored"
    err = (g - e.v).abs()
    bad = err > elem_bound(e.v, e.S, Ktot, rho)
    assert not bool(bad.any()), \
        f"{what}: {int(bad.sum())} of {bad.numel()} elements out of bound; worst err {err.max().item():.3e} at {tuple(int(i) for i in (err == err.max()).nonzero()[0])}"
    dead = (e.m == 0) & (e.v == 0)
    assert bool((g[dead] == 0).all()), f"{what}: a masked element is not exactly 0"


def assert_reductions(what, got, ref, terms):
    """Per channel |got - ref| <= 1e-4 * max|ref|; prints the measured error on the scale of sum|terms| beside a plain torch.float32 sum's."""
    assert got.dtype == torch.float32 and got.shape == ref.shape, (what, got.dtype, got.shape, ref.shape)
    err = (got.double() - ref).abs()
    top = ref.abs().max().item()
    denom = terms.abs().sum(0).clamp_min(1e-300)
    plain = (terms.float().sum(0).double() - terms.sum(0)).abs()
    print(f"REDERR {what}: kernel {(err / denom).max().item():.2e}  torch.float32 {(plain / denom).max().item():.2e}")
    assert bool((err <= 1e-4 * top).all()), f"{what}: max err {err.max().item():.3e} > 1e-4 * {top:.3e}"
