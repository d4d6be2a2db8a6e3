"""CPU-side (wave simulator) checks of the ViT kernels of csrc/vit_ops.hip through the C ABI, and of the executor (clip-lite_amd/vit.py) on small
towers against tests/vit_ref.py in float64. The same shapes as tests/test_gpu_vit.py uses for the kernels. Runs without a GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

import vit_ref as R
from detfill import det_fill, det_tensor
from simlib import lib, outbuf, prep, ptr, val

BF16, F32 = 0, 1
V, I = C.c_void_p, C.c_int


def _patchify(L, dtype, img, p):
    B, _, H, W = img.shape
    out = outbuf((B * (H // p) * (W // p), 3 * p * p), dtype)
    L.clite_vit_patchify.argtypes = [I, V, V, I, I, I, I, V]
    rc = L.clite_vit_patchify(dtype, ptr(img), ptr(out), B, H, W, p, None)
    return rc, out


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("H,W,p", [(64, 96, 32), (48, 32, 16)])
def test_patchify_is_unfold_in_c_i_j_order(dtype, H, W, p):
    B = 2
    img = np.random.default_rng(H + p).standard_normal((B, 3, H, W), dtype=np.float32)
    rc, out = _patchify(lib(), dtype, img, p)
    assert rc == 0
    want = torch.nn.functional.unfold(torch.from_numpy(img), p, stride=p).permute(0, 2, 1).reshape(out.shape).numpy()      # columns (c, i, j)
    want = prep(want, dtype)[0]
    assert np.array_equal(val(out, dtype), want)          # a copy: exact after the cast
    # a row/column swap or an (i, j, c) order would show: the patch (ph = 0, pw = 1) of sample 0, channel 1, row 2
    assert np.array_equal(val(out, dtype)[1, p * p + 2 * p:p * p + 3 * p], prep(img[0, 1, 2, p:2 * p], dtype)[0])


def test_patchify_refuses_what_it_cannot_cut():
    L = lib()
    img = np.zeros((1, 3, 64, 96), np.float32)
    assert _patchify(L, F32, img, 32)[0] == 0
    L.clite_vit_patchify.argtypes = [I, V, V, I, I, I, I, V]
    out = np.zeros(3 * 64 * 96, np.float32)
    assert L.clite_vit_patchify(F32, ptr(img), ptr(out), 1, 64, 96, 40, None) == -1          # 40 does not divide 64
    assert L.clite_vit_patchify(F32, ptr(img), ptr(out), 1, 64, 96, 4, None) == -1           # patches narrower than one 8-element chunk
    assert L.clite_vit_patchify(2, ptr(img), ptr(out), 1, 64, 96, 32, None) == -1
    assert L.clite_vit_patchify(F32, None, ptr(out), 1, 64, 96, 32, None) == -1


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("Cc", [128, 768])
def test_tokens_forward_and_backward(dtype, Cc):
    L = lib()
    B, P = 3, 6
    Ls = P + 1
    rng = np.random.default_rng(Cc)
    e, eb = prep(rng.standard_normal((B * P, Cc), dtype=np.float32), dtype)
    cls, cb = prep(rng.standard_normal(Cc, dtype=np.float32), dtype)
    pos, pb = prep(rng.standard_normal((Ls, Cc), dtype=np.float32), dtype)
    s0 = outbuf((B * Ls, Cc), dtype)
    L.clite_vit_tokens_fwd.argtypes = [I, V, V, V, V, I, I, I, V]
    assert L.clite_vit_tokens_fwd(dtype, ptr(eb), ptr(cb), ptr(pb), ptr(s0), B, P, Cc, None) == 0
    want = R.tokens(torch.tensor(e, dtype=torch.float64).view(B, P, Cc), torch.tensor(cls, dtype=torch.float64),
                    torch.tensor(pos, dtype=torch.float64)).reshape(B * Ls, Cc).numpy()
    # exact to one rounding of the sum (the f32 sum of two bf16 / f32 values, then the store's rounding)
    assert np.array_equal(val(s0, dtype), prep(want.astype(np.float32), dtype)[0])

    ds0, db = prep(rng.standard_normal((B * Ls, Cc), dtype=np.float32), dtype)
    d3 = ds0.reshape(B, Ls, Cc)
    L.clite_vit_tokens_bwd.argtypes = [I, V, V, V, V, I, I, I, V]
    runs = []
    for _ in range(2):
        de, dpos, dcls = outbuf((B * P, Cc), dtype), np.zeros((Ls, Cc), np.float32), np.zeros(Cc, np.float32)
        assert L.clite_vit_tokens_bwd(dtype, ptr(db), ptr(de), ptr(dpos), ptr(dcls), B, P, Cc, None) == 0
        runs.append((de, dpos, dcls))
    de, dpos, dcls = runs[0]
    assert np.array_equal(val(de, dtype).reshape(B, P, Cc), d3[:, 1:])
    # against float64, to f32 rounding: B - 1 = 2 additions per slot, each within half an ulp of its partial sum
    d64 = d3.astype(np.float64)
    tol = (B - 1) * np.spacing(np.abs(d64).sum(0).astype(np.float32))
    assert (np.abs(dpos - d64.sum(0)) <= tol).all() and (np.abs(dcls - d64.sum(0)[0]) <= tol[0]).all()
    # index order: the f32 sum over b = 0, 1, 2 exactly; bit-equal across two runs
    assert np.array_equal(dpos, (d3[0] + d3[1]) + d3[2]) and np.array_equal(dcls, dpos[0])
    assert all(np.array_equal(a, b) for a, b in zip(runs[0], runs[1]))
    # the accumulators are added to, not overwritten; either may be absent
    start = rng.integers(-3, 4, (Ls, Cc)).astype(np.float32)
    acc, de2 = start.copy(), outbuf((B * P, Cc), dtype)
    assert L.clite_vit_tokens_bwd(dtype, ptr(db), ptr(de2), ptr(acc), None, B, P, Cc, None) == 0
    assert np.array_equal(acc, start + dpos) and np.array_equal(de2, de)
    assert L.clite_vit_tokens_bwd(dtype, ptr(db), ptr(de2), None, None, B, P, Cc, None) == 0


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_tokens_backward_in_unrolled_rounds_and_tail(dtype):
    """B = 19: one round of 16 batch rows with all loads in flight, then 3 rows one by one - the same index order throughout"""
    L = lib()
    B, P, Cc = 19, 2, 128
    Ls = P + 1
    ds0, db = prep(np.random.default_rng(19).standard_normal((B * Ls, Cc), dtype=np.float32), dtype)
    d3 = ds0.reshape(B, Ls, Cc)
    de, dpos, dcls = outbuf((B * P, Cc), dtype), np.zeros((Ls, Cc), np.float32), np.zeros(Cc, np.float32)
    L.clite_vit_tokens_bwd.argtypes = [I, V, V, V, V, I, I, I, V]
    assert L.clite_vit_tokens_bwd(dtype, ptr(db), ptr(de), ptr(dpos), ptr(dcls), B, P, Cc, None) == 0
    assert np.array_equal(val(de, dtype).reshape(B, P, Cc), d3[:, 1:])
    seq = np.zeros((Ls, Cc), np.float32)
    for b in range(B):
        seq = seq + d3[b]
    assert np.array_equal(dpos, seq) and np.array_equal(dcls, seq[0])


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_class_rows_gather_and_scatter(dtype):
    L = lib()
    B, Ls, Cc = 3, 7, 128
    rng = np.random.default_rng(3)
    x, xb = prep(rng.standard_normal((B * Ls, Cc), dtype=np.float32), dtype)
    out = outbuf((B, Cc), dtype)
    L.clite_vit_class_gather.argtypes = L.clite_vit_class_scatter.argtypes = [I, V, V, I, I, I, V]
    assert L.clite_vit_class_gather(dtype, ptr(xb), ptr(out), B, Ls, Cc, None) == 0
    assert np.array_equal(val(out, dtype), x.reshape(B, Ls, Cc)[:, 0])
    dx = outbuf((B * Ls, Cc), dtype)
    assert L.clite_vit_class_scatter(dtype, ptr(out), ptr(dx), B, Ls, Cc, None) == 0
    want = np.zeros((B, Ls, Cc), np.float32)
    want[:, 0] = x.reshape(B, Ls, Cc)[:, 0]
    assert np.array_equal(val(dx, dtype).reshape(B, Ls, Cc), want)


# ---------------------------------------------------------------------------------------------------- the executor on the simulator
class _Holder(torch.nn.Module):
    def __init__(self, enc):
        super().__init__()
        self.image_encoder = enc


@pytest.fixture
def sim_hip(monkeypatch):
    import simlib
    from clip_lite_amd import hip
    simlib.build_sim()
    monkeypatch.setattr(hip, "_lib", hip._bind(C.CDLL(simlib.SIM_SO)))
    monkeypatch.setattr(hip, "_allow_host_tensors", True)
    return hip


@pytest.mark.parametrize("name,H,W,layers", [("vit_b_32", 64, 96, 2), ("vit_b_16", 96, 96, 1)])
def test_executor_matches_reference_in_exact_f32(sim_hip, name, H, W, layers):
    """7 tokens (one-tile attention) and 37 tokens (four key tiles, ragged second tile) on a 64-wide, one-head tower: features and every parameter
    gradient against float64. Bounds: the f32 parity bounds of the GPU tower test."""
    from clip_lite_amd.encoder import ImageEncoder
    from clip_lite_amd.model import attach_runtime
    heads, inner, B = 1, 128, 2
    enc = ImageEncoder(name, image_size=(H, W), num_layers=layers, hidden=64 * heads, heads=heads, mlp_dim=inner)
    det_fill(enc)
    holder = _Holder(enc)
    attach_runtime(holder, torch.device("cpu"), lowp=False)
    sd = {k: v.clone() for k, v in enc.img_encoder.state_dict().items()}
    image = det_tensor("image", (B, 3, H, W), "normal")
    dfeat = det_tensor("dfeat", (B, 64 * heads), "normal")
    feat = enc(image)
    assert feat.shape == (B, 64 * heads) and feat.requires_grad
    feat.backward(dfeat)
    want, grads = R.features_and_grads(sd, image, layers, heads, dfeat)
    assert (feat.detach().double() - want).abs().max() <= 1e-4 * want.abs().max()
    for k, p in enc.img_encoder.named_parameters():
        g = grads[k]
        assert p.grad.shape == g.shape, k
        assert (p.grad.double() - g).abs().max() <= 2e-3 * g.abs().max(), k
    # the no-grad path gives the same features, and another image size is refused
    with torch.no_grad():
        assert torch.equal(enc(image), feat.detach())
    with pytest.raises(RuntimeError, match="was built for"):
        enc(torch.zeros(1, 3, H, W + enc.img_encoder.patch))


def test_fp8_forward_refuses_a_vit(sim_hip):
    """--fp8 (DeviceRuntime.fp8 in bf16 mode) is built for the ResNets and the BERT tower: a ViT image encoder raises before it launches anything"""
    from clip_lite_amd.encoder import ImageEncoder
    from clip_lite_amd.model import attach_runtime
    enc = ImageEncoder("vit_b_32", image_size=64, num_layers=1, hidden=64, heads=1, mlp_dim=64)
    rt = attach_runtime(_Holder(enc), torch.device("cpu"), lowp=True)
    rt.fp8 = True
    with pytest.raises(RuntimeError, match="fp8.*ViT"):
        enc(torch.zeros(1, 3, 64, 64))
    rt.fp8 = False
    with torch.no_grad():
        assert enc(torch.zeros(1, 3, 64, 64)).shape == (1, 64)
