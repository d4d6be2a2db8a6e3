"""float64 references of the image encoder's streaming operations, written from their definitions (torchvision ResNet: train-mode BatchNorm2d,
MaxPool2d(3, 2, 1), AdaptiveAvgPool2d(1)) on plain torch tensors. Nothing here calls into clip_lite_amd; tests/test_resnet_ref_host.py checks every
function against an independent formulation (torch.nn.functional / autograd), tests/test_gpu_resnet_ops.py compares the HIP kernels with them.

Layouts are the kernels': activations NHWC (BatchNorm sees them as [M][C], M = N*H*W), images NCHW. Inputs of any float type are upcast; every
result is float64 (window codes: int64) on the inputs' device."""
from collections import namedtuple

import torch

BnTrain = namedtuple("BnTrain", "out mean var running_mean running_var res_mean res_var res_running_mean res_running_var")
BnBwd = namedtuple("BnBwd", "dz S1 S2 dy dgamma dbeta")


def round_to(x, dtype):
    """x rounded through the storage type `dtype` (round to nearest even), back in float64. A float64 reaches bfloat16 by way of float32, as
    the kernels' values do: they hold float32 and round that."""
    return x.to(dtype).double()


def _moments(y):
    mean = y.mean(0)
    return mean, ((y - mean) ** 2).mean(0)


def _running(mean, var, M, momentum, running):
    rm, rv = (running[0].double(), running[1].double()) if running is not None else (torch.zeros_like(mean), torch.ones_like(var))
    unbiased = var * (M / (M - 1)) if M > 1 else var
    return (1 - momentum) * rm + momentum * mean, (1 - momentum) * rv + momentum * unbiased


def bn_train_ref(y, gamma, beta, eps, res=None, res_bn=None, relu=True, momentum=0.1, running=None):
    """Train-mode BatchNorm of y [M][C] with batch statistics: out = relu?((y - mean) / sqrt(var + eps) * gamma + beta [+ res | + BN'(res)]).
    res_bn = (gamma', beta'[, (running_mean', running_var')]): the dual form, a second train-mode BatchNorm on the residual. Returns out, the
    batch mean, the BIASED batch variance and the running statistics after one update from `running` (default zeros / ones) with `momentum`
    and the unbiased variance; the res_* fields hold the same for the residual's BatchNorm (None without one)."""
    y = y.double()
    M = y.shape[0]
    mean, var = _moments(y)
    z = (y - mean) / torch.sqrt(var + eps) * gamma.double() + beta.double()
    rmean = rvar = rrm = rrv = None
    if res is not None and res_bn is not None:
        r = res.double()
        rmean, rvar = _moments(r)
        z = z + (r - rmean) / torch.sqrt(rvar + eps) * res_bn[0].double() + res_bn[1].double()
        rrm, rrv = _running(rmean, rvar, M, momentum, res_bn[2] if len(res_bn) > 2 else None)
    elif res is not None:
        z = z + res.double()
    out = torch.where(z < 0, torch.zeros_like(z), z) if relu else z
    rm, rv = _running(mean, var, M, momentum, running)
    return BnTrain(out, mean, var, rm, rv, rmean, rvar, rrm, rrv)


def bn_bwd_ref(dout, out_mask, y, gamma, eps):
    """Backward of train-mode BatchNorm (+ ReLU) with respect to its input y [M][C]: dz = dout * (out_mask > 0) (out_mask None: no ReLU),
    S1 = sum dz, S2 = sum dz * (y - mean), dy = gamma * rstd * (dz - S1 / M - xhat * sum(dz * xhat) / M), dgamma = sum dz * xhat, dbeta = S1."""
    y, dout = y.double(), dout.double()
    M = y.shape[0]
    mean, var = _moments(y)
    rstd = 1.0 / torch.sqrt(var + eps)
    dz = dout if out_mask is None else torch.where(out_mask > 0, dout, torch.zeros_like(dout))
    yc = y - mean
    S1, S2 = dz.sum(0), (dz * yc).sum(0)
    xhat = yc * rstd
    dgamma = (dz * xhat).sum(0)
    dy = gamma.double() * rstd * (dz - S1 / M - xhat * dgamma / M)
    return BnBwd(dz, S1, S2, dy, dgamma, S1)


def pool_out(n):
    """Output extent of a 3 / stride 2 / pad 1 window over n positions."""
    return (n + 2 - 3) // 2 + 1


def maxpool_ref(x):
    """3x3 / stride 2 / pad 1 max-pool of x [N][H][W][C] as the explicit nine-tap scan over (r, s) in row-major order: padding taps are
    skipped, the first maximum wins (a later tap replaces the running one only if it is strictly greater), and a NaN tap always wins.
    Returns (values [N][Ho][Wo][C] float64, window code r * 3 + s int64)."""
    x = x.double()
    N, H, W, C = x.shape
    Ho, Wo = pool_out(H), pool_out(W)
    xp = x.new_zeros(N, H + 2, W + 2, C)
    xp[:, 1:H + 1, 1:W + 1] = x
    valid = torch.zeros(H + 2, W + 2, dtype=torch.bool, device=x.device)
    valid[1:H + 1, 1:W + 1] = True
    best = x.new_full((N, Ho, Wo, C), float("-inf"))
    code = torch.full((N, Ho, Wo, C), -1, dtype=torch.int64, device=x.device)
    for r in range(3):
        for s in range(3):
            v = xp[:, r:r + 2 * Ho:2, s:s + 2 * Wo:2]
            ok = valid[r:r + 2 * Ho:2, s:s + 2 * Wo:2][None, :, :, None]
            take = ok & ((v > best) | (code < 0) | torch.isnan(v))
            best = torch.where(take, v, best)
            code = torch.where(take, torch.full_like(code, r * 3 + s), code)
    return best, code


def maxpool_taps(x):
    """The nine taps of every window, [9][N][Ho][Wo][C] float64, and their validity [9][1][Ho][Wo][1] (False on padding)."""
    x = x.double()
    N, H, W, C = x.shape
    Ho, Wo = pool_out(H), pool_out(W)
    xp = x.new_zeros(N, H + 2, W + 2, C)
    xp[:, 1:H + 1, 1:W + 1] = x
    valid = torch.zeros(H + 2, W + 2, dtype=torch.bool, device=x.device)
    valid[1:H + 1, 1:W + 1] = True
    taps = torch.stack([xp[:, r:r + 2 * Ho:2, s:s + 2 * Wo:2] for r in range(3) for s in range(3)])
    ok = torch.stack([valid[r:r + 2 * Ho:2, s:s + 2 * Wo:2] for r in range(3) for s in range(3)])
    return taps, ok[:, None, :, :, None]


def maxpool_gather(x, code):
    """x [N][H][W][C] at each window's tap `code`: [N][Ho][Wo][C] float64."""
    taps, _ = maxpool_taps(x)
    return torch.gather(taps, 0, code[None]).squeeze(0)


def maxpool_bwd_ref(dout, idx, H, W):
    """dx [N][H][W][C]: every pooled gradient goes to the input position its window code names; overlapping windows add."""
    dout = dout.double()
    N, Ho, Wo, C = dout.shape
    dxp = dout.new_zeros(N, H + 2, W + 2, C)
    for r in range(3):
        for s in range(3):
            dxp[:, r:r + 2 * Ho:2, s:s + 2 * Wo:2] += torch.where(idx == r * 3 + s, dout, torch.zeros_like(dout))
    return dxp[:, 1:H + 1, 1:W + 1].contiguous()


def avgpool_ref(x):
    """Global average pool of x [N][HW][C] -> [N][C]."""
    return x.double().sum(1) / x.shape[1]


def avgpool_bwd_ref(dout, HW):
    """dx [N][HW][C] = dout [N][C] / HW at every position."""
    return (dout.double() / HW)[:, None, :].expand(-1, HW, -1).contiguous()


def image_to_nhwc4_ref(img, pad, Hp, Wp):
    """img [N][3][H][W] -> [N][Hp][Wp][4]: the image at offset (pad, pad), channel 3 and everything around the image zero."""
    N, _, H, W = img.shape
    out = torch.zeros(N, Hp, Wp, 4, dtype=torch.float64, device=img.device)
    out[:, pad:pad + H, pad:pad + W, :3] = img.double().permute(0, 2, 3, 1)
    return out


def colsum_ref(x):
    """Column sums of x [M][N]."""
    return x.double().sum(0)
