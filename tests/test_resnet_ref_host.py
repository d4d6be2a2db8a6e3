"""The float64 references of tests/resnet_ref.py against independent float64 formulations (torch.nn.functional, autograd). No GPU, no kernel:
this is what makes the references trustworthy before tests/test_gpu_resnet_ops.py holds the HIP kernels to them. Agreement: 1e-12 relative."""
import pytest
import torch
import torch.nn.functional as F

import resnet_ref as R

REL = 1e-12


def _close(got, ref):
    assert got.dtype == torch.float64 and got.shape == ref.shape
    assert (got - ref).abs().max().item() <= REL * max(ref.abs().max().item(), 1e-300), (got - ref).abs().max().item()


def _randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float64)


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("form", ["none", "plain", "dual"])
@pytest.mark.parametrize("M,C", [(70, 8), (33, 64), (2, 16)])
def test_bn_train_and_backward_refs_match_functional_batch_norm_and_autograd(M, C, form, relu):
    g = torch.Generator().manual_seed(M * 7 + C)
    y = (_randn(g, M, C) * 2 + 0.5).requires_grad_(True)
    r = _randn(g, M, C)
    gamma, beta, g2, b2 = (1 + 0.1 * _randn(g, C)).requires_grad_(True), (0.1 * _randn(g, C)).requires_grad_(True), 1 + 0.1 * _randn(g, C), 0.1 * _randn(g, C)
    rm0, rv0, rm1, rv1 = 0.3 * _randn(g, C), 1 + 0.2 * torch.rand(C, generator=g, dtype=torch.float64), 0.3 * _randn(g, C), 0.5 + torch.rand(C, generator=g, dtype=torch.float64)
    eps, mom = 1e-5, 0.1
    rm, rv, rm2, rv2 = rm0.clone(), rv0.clone(), rm1.clone(), rv1.clone()
    z = F.batch_norm(y, rm, rv, gamma, beta, True, mom, eps)
    if form == "plain":
        z = z + r
    elif form == "dual":
        z = z + F.batch_norm(r, rm2, rv2, g2, b2, True, mom, eps)
    want = F.relu(z) if relu else z
    got = R.bn_train_ref(y.detach(), gamma.detach(), beta.detach(), eps, res=None if form == "none" else r,
                         res_bn=(g2, b2, (rm1, rv1)) if form == "dual" else None, relu=relu, momentum=mom, running=(rm0, rv0))
    _close(got.out, want.detach())
    _close(got.mean, y.detach().mean(0))
    _close(got.var, y.detach().var(0, unbiased=False))
    _close(got.running_mean, rm)
    _close(got.running_var, rv)
    if form == "dual":
        _close(got.res_mean, r.mean(0))
        _close(got.res_var, r.var(0, unbiased=False))
        _close(got.res_running_mean, rm2)
        _close(got.res_running_var, rv2)
    else:
        assert got.res_mean is None and got.res_running_var is None
    # defaults of the running statistics: zeros / ones
    d = R.bn_train_ref(y.detach(), gamma.detach(), beta.detach(), eps, momentum=mom)
    _close(d.running_mean, mom * y.detach().mean(0))
    _close(d.running_var, (1 - mom) + mom * y.detach().var(0, unbiased=True))

    dout = _randn(g, M, C)
    want.backward(dout)
    mask = want.detach() if relu else None
    b = R.bn_bwd_ref(dout, mask, y.detach(), gamma.detach(), eps)
    dz = dout * (want.detach() > 0) if relu else dout
    _close(b.dz, dz)
    _close(b.S1, dz.sum(0))
    _close(b.S2, (dz * (y.detach() - y.detach().mean(0))).sum(0))
    # dy is a difference of terms of size gamma * rstd * |dz| (at M = 2 it cancels to almost nothing): 1e-12 of that scale
    scale = (gamma.detach().abs() / torch.sqrt(b.S1.new_tensor(eps) + y.detach().var(0, unbiased=False))).max().item() * dz.abs().max().item()
    assert b.dy.dtype == torch.float64 and (b.dy - y.grad).abs().max().item() <= REL * scale
    _close(b.dgamma, gamma.grad)
    _close(b.dbeta, beta.grad)


def _codes_from_flat(flat, H, W):
    """F.max_pool2d's flat input index h * W + w of [N][C][Ho][Wo] -> window code r * 3 + s, NHWC."""
    N, C, Ho, Wo = flat.shape
    hi, wi = flat // W, flat % W
    ho = torch.arange(Ho).view(1, 1, Ho, 1)
    wo = torch.arange(Wo).view(1, 1, 1, Wo)
    r, s = hi - (2 * ho - 1), wi - (2 * wo - 1)
    assert ((r >= 0) & (r < 3) & (s >= 0) & (s < 3)).all()
    return (r * 3 + s).permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("N,H,W,C", [(2, 9, 8, 16), (1, 12, 13, 8), (3, 7, 7, 24), (1, 1, 1, 8), (1, 2, 3, 8)])
def test_maxpool_refs_match_functional_max_pool_and_autograd(N, H, W, C):
    g = torch.Generator().manual_seed(H * 31 + W)
    x = _randn(g, N, H, W, C)                                  # continuous values: no ties
    xn = x.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    want, flat = F.max_pool2d(xn, 3, 2, 1, return_indices=True)
    val, code = R.maxpool_ref(x)
    assert val.shape == (N, R.pool_out(H), R.pool_out(W), C)
    _close(val, want.detach().permute(0, 2, 3, 1).contiguous())
    assert torch.equal(code, _codes_from_flat(flat, H, W))
    assert torch.equal(R.maxpool_gather(x, code), val)
    dout = _randn(g, *val.shape)
    want.backward(dout.permute(0, 3, 1, 2))
    _close(R.maxpool_bwd_ref(dout, code, H, W), xn.grad.permute(0, 2, 3, 1).contiguous())


def test_maxpool_ref_tie_and_nan_rule_on_a_hand_made_window():
    """One 3 x 3 input, C = 8: the centre window (ho = wo = 0 of a 3 x 3 input covers taps (1,1)..(2,2) = input (0,0)..(1,1)); the second output
    column / row see other taps. Channel by channel: 0 a unique maximum, 1 a tie (first in (r, s) order wins), 2 all equal, 3 one NaN,
    4 two NaNs (the later one is named), 5 NaN before a larger finite value (the NaN stays), 6 -inf everywhere (first valid tap), 7 +-0."""
    x = torch.zeros(1, 3, 3, 8, dtype=torch.float64)
    nan, inf = float("nan"), float("inf")
    x[0, :, :, 0] = torch.tensor([[1., 2., 0.], [3., 9., 0.], [0., 0., 0.]])
    x[0, :, :, 1] = torch.tensor([[5., 7., 0.], [7., 7., 0.], [0., 0., 0.]])
    x[0, :, :, 2] = 4.0
    x[0, :, :, 3] = torch.tensor([[1., nan, 0.], [3., 2., 0.], [0., 0., 0.]])
    x[0, :, :, 4] = torch.tensor([[nan, 1., 0.], [nan, 2., 0.], [0., 0., 0.]])
    x[0, :, :, 5] = torch.tensor([[nan, 1., 0.], [100., 2., 0.], [0., 0., 0.]])
    x[0, :, :, 6] = -inf
    x[0, :, :, 7] = torch.tensor([[-0., 0., 0.], [0., -0., 0.], [0., 0., 0.]])
    val, code = R.maxpool_ref(x)
    assert val.shape == (1, 2, 2, 8)
    v, c = val[0, 0, 0], code[0, 0, 0]
    # window (0, 0): valid taps are (r, s) in {1, 2}^2 -> codes 4, 5, 7, 8 = inputs (0,0), (0,1), (1,0), (1,1)
    assert v[0] == 9 and c[0] == 8
    assert v[1] == 7 and c[1] == 5                 # first of the three 7s in scan order
    assert v[2] == 4 and c[2] == 4
    assert torch.isnan(v[3]) and c[3] == 5
    assert torch.isnan(v[4]) and c[4] == 7         # a NaN always wins, also over an earlier NaN
    assert torch.isnan(v[5]) and c[5] == 4         # 100 > NaN is false: the NaN stays
    assert v[6] == -inf and c[6] == 4              # the first valid tap is taken whatever its value
    assert v[7] == 0 and c[7] == 4                 # -0 == +0: no later tap is strictly greater
    # window (0, 1): taps s = 0, 1 of rows r = 1, 2 -> inputs (0,1), (0,2), (1,1), (1,2); codes 3, 4, 6, 7
    assert val[0, 0, 1, 0] == 9 and code[0, 0, 1, 0] == 6
    assert val[0, 0, 1, 1] == 7 and code[0, 0, 1, 1] == 3
    # the backward sends each window's gradient to the named tap; input (1,1) of channel 0 is the argmax of all four windows
    dout = torch.arange(1., 33.).view(1, 2, 2, 8).double()
    dx = R.maxpool_bwd_ref(dout, code, 3, 3)
    assert dx[0, 1, 1, 0] == dout[0, :, :, 0].sum() and dx[0, :, :, 0].sum() == dout[0, :, :, 0].sum()


@pytest.mark.parametrize("N,HW,C", [(5, 49, 16), (1, 1, 8), (3, 7, 24)])
def test_avgpool_refs_match_adaptive_avg_pool_and_autograd(N, HW, C):
    g = torch.Generator().manual_seed(HW)
    x = _randn(g, N, HW, C).requires_grad_(True)
    want = F.adaptive_avg_pool2d(x.permute(0, 2, 1).reshape(N, C, HW, 1), 1).reshape(N, C)
    _close(R.avgpool_ref(x.detach()), want.detach())
    dout = _randn(g, N, C)
    want.backward(dout)
    _close(R.avgpool_bwd_ref(dout, HW), x.grad)


def test_image_to_nhwc4_ref_matches_functional_pad():
    g = torch.Generator().manual_seed(3)
    N, H, W, pad, Hp, Wp = 2, 6, 5, 3, 13, 16
    img = _randn(g, N, 3, H, W)
    want = F.pad(torch.cat([img, torch.zeros(N, 1, H, W, dtype=torch.float64)], 1), (pad, Wp - W - pad, pad, Hp - H - pad)).permute(0, 2, 3, 1)
    _close(R.image_to_nhwc4_ref(img, pad, Hp, Wp), want.contiguous())
    assert R.image_to_nhwc4_ref(img.float(), pad, Hp, Wp).dtype == torch.float64


def test_colsum_ref_and_round_to():
    g = torch.Generator().manual_seed(5)
    x = _randn(g, 1001, 72)
    _close(R.colsum_ref(x), x.sum(0))
    _close(R.colsum_ref(x.float()), x.float().double().sum(0))
    v = torch.tensor([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -3.14159, 0.0], dtype=torch.float64)
    # bf16 keeps 8 significant bits: ties go to the even neighbour, anything past the half-way point rounds up
    assert torch.equal(R.round_to(v, torch.bfloat16)[:4], torch.tensor([1.0, 1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7], dtype=torch.float64))
    assert R.round_to(v, torch.bfloat16).dtype == torch.float64
    assert torch.equal(R.round_to(v, torch.float32), v.float().double())
    assert torch.equal(R.round_to(v, torch.float64), v)
