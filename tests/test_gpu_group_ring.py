"""The LDS-DMA rings of the grouped weight-gradient kernels (csrc/gemm_group.hip) on the GPU, checked for EQUALITY.

The ring's DMA is issued in a form the compiler does not order against the transposed fragment reads; the kernels' own counted vmcnt wait + barrier
per K tile is the only ordering. What can go wrong is a fragment read of a stage that has not landed yet or that has been overwritten already, and it
shows only with more K tiles per workgroup than twice the ring depth, plus a ragged last tile. Every member here has that:

  8-wave members (K tile 64, 2 stages):  linear 256 x 256 and 264 x 320 over 333 rows (6 tiles, 13 rows in the last), 1 x 1 conv 256 -> 256 on
                                         2 x 13 x 13 pixels (338 = 6 tiles, 18 in the last)
  4-wave members (K tile 32, 3 stages):  linear 128 x 136 over 229 rows (8 tiles, 5 in the last); on 2 x 11 x 11 pixels (242 = 8 tiles, 18 in the last)
                                         a 3 x 3 conv 64 -> 64 (its halo reads as zeros), a 3 x 3 conv 96 -> 128 (the general tile family), a 1 x 1 conv
                                         128 -> 64 (<= 64 output channels) and a 1 x 1 conv 64 -> 128 (<= 64 columns)
  CLITE_WGRAD_SHORTK members:            1 x 1 convs 64 -> 64 (4-wave) and 256 -> 256 (8-wave) over 3 x 25 x 28 = 2100 pixels: two K chunks each, i.e. two
                                         workgroups per output tile that add with float atomics

Operands are integer-valued bf16 in [-2, 2], so every product and every partial sum is an integer of magnitude <= 4 * 2100 = 8400 < 2^24: exact in
f32 in ANY summation order (the atomics' order included). The result must therefore EQUAL the float64 reference; there is no tolerance for a stale
read to hide in. The group is launched 5 times into re-zeroed buffers (CLITE_WGRAD_ZEROED: single-chunk members store, the others add)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
BF16 = 0
LAUNCHES = 5


def _ints(shape, g):
    return torch.randint(-2, 3, shape, device="cuda", generator=g).to(torch.bfloat16)


def _conv_wgrad_ref(dy, x, R, pad):
    """float64 dW[K][R][S][C] = sum over pixels of dy[n, ho, wo, k] * x[n, ho + r - pad, wo + s - pad, c] (stride 1), by explicit window slices"""
    N, H, W, C = x.shape
    K = dy.shape[-1]
    xp = torch.zeros(N, H + 2 * pad, W + 2 * pad, C, device=x.device, dtype=torch.float64)
    xp[:, pad:pad + H, pad:pad + W] = x.double()
    dy2 = dy.double().reshape(-1, K)
    dw = torch.empty(K, R, R, C, device=x.device, dtype=torch.float64)
    for r in range(R):
        for s in range(R):
            dw[:, r, s] = dy2.t() @ xp[:, r:r + H, s:s + W].reshape(-1, C)
    return dw


@pytest.fixture(scope="module")
def members():
    """[(label, kind, operands, float64 reference)], built once; the tests leave it unchanged"""
    g = torch.Generator(device="cuda").manual_seed(20)
    out = []
    for (M, N, K) in [(256, 256, 333), (264, 320, 333), (128, 136, 229)]:
        A, B = _ints((K, M), g), _ints((K, N), g)
        out.append((f"linear {M}x{N} over {K}", "linear", (A, B, M, N, K), A.double().t() @ B.double()))
    for (N, H, W, C, K, R, pad, short_k) in [(2, 13, 13, 256, 256, 1, 0, False), (2, 11, 11, 64, 64, 3, 1, False), (2, 11, 11, 96, 128, 3, 1, False),
                                            (2, 11, 11, 128, 64, 1, 0, False), (2, 11, 11, 64, 128, 1, 0, False), (3, 25, 28, 64, 64, 1, 0, True),
                                            (3, 25, 28, 256, 256, 1, 0, True)]:
        x, dy = _ints((N, H, W, C), g), _ints((N, H, W, K), g)
        out.append((f"conv {R}x{R} {C}->{K} on {N}x{H}x{W}" + (" short-K" if short_k else ""), "conv", (dy, x, (N, H, W, C, K, R, pad), short_k),
                    _conv_wgrad_ref(dy, x, R, pad)))
    return out


def test_group_ring_results_equal_float64(members):
    from clip_lite_amd import hip
    hip.set_tile_policy(0)
    hip.set_deterministic(False)
    outs = []
    for label, kind, ops, ref in members:
        outs.append(torch.empty(ref.shape, device="cuda", dtype=torch.float32))
    for launch in range(LAUNCHES):
        grp = hip.WgradGroup(BF16, zeroed=True)
        for (label, kind, ops, ref), o in zip(members, outs):
            o.zero_()
            if kind == "linear":
                A, B, M, N, K = ops
                grp.linear(A, B, M, N, K, o)
            else:
                dy, x, (N, H, W, C, K, R, pad), short_k = ops
                grp.conv(dy, x, hip.conv_desc(BF16, N, H, W, C, K, R, R, 1, pad), o, short_k=short_k)
        grp.launch()
        torch.cuda.synchronize()
        for (label, kind, ops, ref), o in zip(members, outs):
            bad = (o.double() != ref).sum().item()
            assert bad == 0, f"launch {launch}: {label}: {bad} of {ref.numel()} elements differ from the float64 reference"
