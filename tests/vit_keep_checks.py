"""The checks of the patch-dropout kernels (csrc/vit_ops.hip: clite_vit_keep_indices, _patchify_keep, _tokens_keep_fwd, _tokens_keep_bwd) and of
the tower that runs on them, written once against tests/vit_keep_ref.py and run by tests/test_wavesim_vit_keep.py (wave simulator, numpy
buffers) and tests/test_gpu_vit_keep.py (MI355X, torch tensors) through the backends of tests/loss_backends.py."""
import ctypes as C

import numpy as np
import torch

import vit_keep_ref as K
import vit_ref as R
from detfill import det_fill, det_tensor
from loss_backends import BF16, F32, HipBackend, SimBackend

_V, _I = C.c_void_p, C.c_int
SIGNATURES = {
    "vit_keep_indices": [_V, _V, _I, _I, _I, C.c_uint64, C.c_uint32],
    "vit_patchify_keep": [_I, _V, _V, _V, _I, _I, _I, _I, _I],
    "vit_tokens_keep_fwd": [_I, _V, _V, _V, _V, _V, _I, _I, _I, _I],
    "vit_tokens_keep_bwd": [_I, _V, _V, _V, _V, _V, _I, _I, _I, _I],
}
SEED_INDIRECT = 0x80000000


class Sim(SimBackend):
    def __init__(self):
        super().__init__()
        for n, sig in SIGNATURES.items():
            getattr(self.L, "clite_" + n).argtypes = sig + [_V]

    def addr(self, h):
        return h.ctypes.data


class Hip(HipBackend):
    def addr(self, h):
        return h.data_ptr()

    def set_deterministic(self, on):
        self.hip.set_deterministic(on)


def _cast(x, dtype):
    """float32 values as the kernel stores them in `dtype`"""
    x = np.ascontiguousarray(x, np.float32)
    return torch.from_numpy(x).to(torch.bfloat16).float().numpy() if dtype == BF16 else x


# ------------------------------------------------------------------------------------------------ the index kernel
INDEX_SHAPES = [(1, 1, 1), (3, 4, 1), (5, 49, 24), (2, 127, 95), (4, 100, 100)]


def _indices(be, B, P, Kk, seed, site):
    idx, inv = be.dev(np.full((B, Kk), -7), "i32"), be.dev(np.full((B, P), -7), "i32")
    assert be.call("vit_keep_indices", idx, inv, B, P, Kk, seed, site) == 0
    return be.host(idx), be.host(inv)


def check_indices(be, B, P, Kk):
    seed, site = 0x1234567 * 1000003 + 41 * P, 3
    idx, inv = _indices(be, B, P, Kk, seed, site)
    want_idx, want_inv = K.keep_indices(seed, site, B, P, Kk)
    assert np.array_equal(idx, want_idx) and np.array_equal(inv, want_inv)
    if Kk == P:
        assert np.array_equal(idx, np.tile(np.arange(P), (B, 1)))          # keep all: the identity
    # the seed read through a device address (a captured step's form) is the same seed
    cell = be.dev(np.array([seed, 0]), "i64")
    idx2, inv2 = _indices(be, B, P, Kk, be.addr(cell), site | SEED_INDIRECT)
    assert np.array_equal(idx2, idx) and np.array_equal(inv2, inv)
    # another site (and another seed) is another set, wherever there is a choice
    if Kk < P and B * P >= 12:
        for s2, t2 in ((seed, site + 1), (seed + 1, site)):
            other, _ = _indices(be, B, P, Kk, s2, t2)
            assert np.array_equal(other, K.keep_indices(s2, t2, B, P, Kk)[0]) and not np.array_equal(other, idx)


# ------------------------------------------------------------------------------------------------ the gather patchify
PATCHIFY_SHAPES = [(64, 96, 32, 3), (48, 32, 16, 4)]


def check_patchify(be, dtype, H, W, p, Kk):
    B, P = 2, (H // p) * (W // p)
    img = np.random.default_rng(H + p).standard_normal((B, 3, H, W), dtype=np.float32)
    idx, _ = K.keep_indices(7, 1, B, P, Kk)
    assert not np.array_equal(idx[0], idx[1])          # (the two samples keep different patches)
    out = be.dev(np.full((B * Kk, 3 * p * p), np.nan), dtype)
    assert be.call("vit_patchify_keep", dtype, be.dev(img, F32), be.dev(idx, "i32"), out, B, H, W, p, Kk) == 0
    full = R.patchify(torch.from_numpy(img), p).numpy()          # [B][P][3 p p]
    want = np.stack([full[b, idx[b]] for b in range(B)]).reshape(B * Kk, -1)
    assert np.array_equal(be.host(out), _cast(want, dtype))          # a copy: exact after the cast


# ------------------------------------------------------------------------------------------------ the keep-assembly
TOKEN_SHAPES = [(8, 3, 6, 3), (768, 37, 9, 4)]          # C, B, P, Kk; B = 37: two unrolled rounds of 16 plus a tail of 5


def check_tokens_fwd(be, dtype, Cc, B, P, Kk):
    rng = np.random.default_rng(Cc + B)
    e, cls, pos = (_cast(rng.standard_normal(s, dtype=np.float32), dtype) for s in ((B, Kk, Cc), (Cc,), (P + 1, Cc)))
    idx, _ = K.keep_indices(21, 2, B, P, Kk)
    s0 = be.dev(np.full((B * (Kk + 1), Cc), np.nan), dtype)
    assert be.call("vit_tokens_keep_fwd", dtype, be.dev(e, dtype), be.dev(cls, dtype), be.dev(pos, dtype), be.dev(idx, "i32"), s0, B, P, Kk, Cc) == 0
    # the definition: all tokens assembled, rows gathered - with e scattered to its patches first (dropped patches hold NaN: never gathered)
    full = np.full((B, P, Cc), np.nan)
    for b in range(B):
        full[b, idx[b]] = e[b]
    want = K.gather_tokens(R.tokens(torch.from_numpy(full), torch.from_numpy(cls).double(), torch.from_numpy(pos).double()), idx)
    assert torch.isfinite(want).all()
    # exact to one rounding: the float64 sum of two f32 / bf16 values rounded to f32 is their f32 sum, then the store's rounding
    assert np.array_equal(be.host(s0), _cast(want.reshape(B * (Kk + 1), Cc).numpy().astype(np.float32), dtype))


def covering_table(B, P, Kk, seed=0):
    """(idx, inv) in which patch 0 is kept by every sample and patch P - 1 by none, the rest drawn per sample"""
    assert P - 2 >= Kk - 1
    rng = np.random.default_rng(seed)
    idx = np.stack([np.sort(np.concatenate([[0], 1 + rng.permutation(P - 2)[:Kk - 1]])) for _ in range(B)]).astype(np.int32)
    inv = np.full((B, P), -1, np.int32)
    for b in range(B):
        inv[b, idx[b]] = np.arange(Kk)
    return idx, inv


def check_tokens_bwd(be, dtype, Cc, B, P, Kk):
    Ls = Kk + 1
    rng = np.random.default_rng(Cc + 7 * B)
    ds0 = _cast(rng.standard_normal((B, Ls, Cc), dtype=np.float32), dtype)
    idx, inv = covering_table(B, P, Kk)
    assert (inv[:, 0] == 0).all() and (inv[:, P - 1] == -1).all()
    start_pos, start_cls = rng.integers(-3, 4, (P + 1, Cc)).astype(np.float32), rng.integers(-3, 4, Cc).astype(np.float32)
    start_pos[P] = -0.0          # the row of the patch nobody kept: its bits must come back as they are (a `+= 0` would make them +0)
    d_ds0, d_inv = be.dev(ds0.reshape(B * Ls, Cc), dtype), be.dev(inv, "i32")

    def run(with_pos=True, with_cls=True):
        de = be.dev(np.full((B * Kk, Cc), np.nan), dtype)
        dpos, dcls = be.dev(start_pos, F32) if with_pos else None, be.dev(start_cls, F32) if with_cls else None
        assert be.call("vit_tokens_keep_bwd", dtype, d_ds0, d_inv, de, dpos, dcls, B, P, Kk, Cc) == 0
        return be.host(de), None if dpos is None else be.host(dpos), None if dcls is None else be.host(dcls)

    de, dpos, dcls = run()
    assert np.array_equal(de.reshape(B, Kk, Cc), ds0[:, 1:])
    # the sums in float64, and the bound of an f32 accumulation: each of the n additions (the += included) within half an ulp of its partial sum
    sum64, abs64, n = np.zeros((P + 1, Cc)), np.zeros((P + 1, Cc)), np.zeros(P + 1, int)
    seq = np.zeros((P + 1, Cc), np.float32)          # ... and the same additions in ascending b in f32: what the kernel must give bit for bit
    for b in range(B):
        for t in [0] + [1 + int(i) for i in idx[b]]:
            row = ds0[b, 0 if t == 0 else 1 + inv[b, t - 1]]
            sum64[t] += row
            abs64[t] += np.abs(row)
            n[t] += 1
            seq[t] = seq[t] + row
    assert n[0] == B and n[1] == B and n[P] == 0
    tol = n[:, None] * np.spacing((abs64 + np.abs(start_pos)).astype(np.float32))
    assert (np.abs(dpos.astype(np.float64) - (start_pos + sum64)) <= tol).all()
    assert (np.abs(dcls.astype(np.float64) - (start_cls + sum64[0])) <= n[0] * np.spacing((abs64[0] + np.abs(start_cls)).astype(np.float32))).all()
    kept_rows = n > 0
    assert np.array_equal(dpos[kept_rows], (start_pos + seq)[kept_rows]) and np.array_equal(dcls, start_cls + seq[0])
    assert np.array_equal(dpos[P].view(np.uint32), start_pos[P].view(np.uint32))          # nobody kept it: bit-unchanged
    # either accumulator may be absent
    de2, dpos2, none = run(with_cls=False)
    assert none is None and np.array_equal(de2, de) and np.array_equal(dpos2.view(np.uint32), dpos.view(np.uint32))
    de3, none, dcls3 = run(with_pos=False)
    assert none is None and np.array_equal(de3, de) and np.array_equal(dcls3, dcls)
    assert np.array_equal(run(False, False)[0], de)
    # the same bits again, in both settings of the deterministic switch
    for on in (True, False):
        be.set_deterministic(on)
        try:
            again = run()
        finally:
            be.set_deterministic(False)
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(again, (de, dpos, dcls)))


# ------------------------------------------------------------------------------------------------ refusals
def check_refusals(be, null_pointers):
    """each entry returns -1 for what it cannot do; null_pointers: also with absent operands (the torch wrappers check those themselves)"""
    i32 = lambda *s: be.dev(np.zeros(s), "i32")
    f = lambda *s: be.dev(np.zeros(s), F32)
    assert be.call("vit_keep_indices", i32(2, 64), i32(2, 128), 2, 128, 64, 1, 1) == 0          # the widest it is built for
    assert be.call("vit_keep_indices", i32(2, 64), i32(2, 129), 2, 129, 64, 1, 1) == -1
    assert be.call("vit_keep_indices", i32(2, 5), i32(2, 4), 2, 4, 5, 1, 1) == -1          # more kept than there are
    assert be.call("vit_keep_indices", i32(2, 0), i32(2, 4), 2, 4, 0, 1, 1) == -1
    assert be.call("vit_keep_indices", i32(2, 2), i32(2, 4), 2, 4, 2, 0, 1 | SEED_INDIRECT) == -1          # an indirect seed at address 0
    img = f(1, 3, 64, 96)
    assert be.call("vit_patchify_keep", F32, img, i32(1, 3), f(3, 3 * 32 * 32), 1, 64, 96, 32, 3) == 0
    assert be.call("vit_patchify_keep", F32, img, i32(1, 3), f(3, 3 * 4 * 4), 1, 64, 96, 4, 3) == -1          # patches narrower than one 8-element chunk
    assert be.call("vit_patchify_keep", F32, img, i32(1, 7), f(7, 3 * 32 * 32), 1, 64, 96, 32, 7) == -1          # 7 of 6 patches
    assert be.call("vit_tokens_keep_fwd", F32, f(2 * 3, 12), f(12), f(7, 12), i32(2, 3), f(2 * 4, 12), 2, 6, 3, 12) == -1          # C % 8
    assert be.call("vit_tokens_keep_fwd", F32, f(2 * 7, 8), f(8), f(7, 8), i32(2, 7), f(2 * 8, 8), 2, 6, 7, 8) == -1          # Kk > P
    assert be.call("vit_tokens_keep_bwd", F32, f(2 * 4, 12), i32(2, 6), f(2 * 3, 12), f(7, 12), f(12), 2, 6, 3, 12) == -1
    assert be.call("vit_tokens_keep_bwd", F32, f(2 * 8, 8), i32(2, 6), f(2 * 7, 8), f(7, 8), f(8), 2, 6, 7, 8) == -1
    if null_pointers:
        assert be.call("vit_keep_indices", None, i32(2, 4), 2, 4, 2, 1, 1) == -1
        assert be.call("vit_keep_indices", i32(2, 2), None, 2, 4, 2, 1, 1) == -1
        assert be.call("vit_patchify_keep", F32, img, None, f(3, 3 * 32 * 32), 1, 64, 96, 32, 3) == -1
        assert be.call("vit_patchify_keep", 2, img, i32(1, 3), f(3, 3 * 32 * 32), 1, 64, 96, 32, 3) == -1          # no such dtype
        assert be.call("vit_tokens_keep_fwd", F32, f(6, 8), f(8), f(7, 8), None, f(8, 8), 2, 6, 3, 8) == -1
        assert be.call("vit_tokens_keep_bwd", F32, f(8, 8), None, f(6, 8), f(7, 8), f(8), 2, 6, 3, 8) == -1
        assert be.call("vit_tokens_keep_bwd", F32, f(8, 8), i32(2, 6), None, f(7, 8), f(8), 2, 6, 3, 8) == -1


# ------------------------------------------------------------------------------------------------ the tower
class Holder(torch.nn.Module):
    """Gives a lone ImageEncoder the `image_encoder` slot the runtime looks for."""

    def __init__(self, enc):
        super().__init__()
        self.image_encoder = enc


def build_tower(name, size, layers, r, device, lowp, salt="clite", round_bf16=False, **kw):
    """(holder with .rt, the tower's state dict as filled) of an ImageEncoder on `device` ("cpu": the simulator build must be injected)"""
    from clip_lite_amd.encoder import ImageEncoder
    from clip_lite_amd.model import attach_runtime
    enc = det_fill(ImageEncoder(name, image_size=size, num_layers=layers, patch_dropout=r, **kw), salt)
    if round_bf16:
        with torch.no_grad():
            for q in enc.parameters():
                q.copy_(R.round_to(q, torch.bfloat16))
    sd = {k: v.clone() for k, v in enc.img_encoder.state_dict().items()}
    holder = Holder(enc).to(device)
    dev = torch.device(device, torch.cuda.current_device()) if device == "cuda" else torch.device("cpu")
    holder.rt = attach_runtime(holder, dev, lowp)
    return holder.train(), sd


def saved_ctx(feat):
    """the executor's ctx of the pass that produced `feat` (encoder._ViTFn keeps it on its autograd node)"""
    node = feat.grad_fn
    while not hasattr(node, "saved"):
        node = node.next_functions[0][0]
    return node.saved


def tower_pass(holder, image, dfeat):
    """one training pass from the runtime's current seed: (features, {name: gradient}, idx, inv) on the host"""
    rt, net = holder.rt, holder.image_encoder.img_encoder
    rt.arena.flat_g.zero_()
    dev = rt.device
    feat = holder.image_encoder(image.to(dev))
    ctx = saved_ctx(feat)
    feat.backward(dfeat.to(dev).to(feat.dtype))
    if dev.type == "cuda":
        torch.cuda.synchronize()
    grads = {k: q.grad.detach().cpu().clone() for k, q in net.named_parameters()}
    return feat.detach().cpu(), grads, ctx["idx"].cpu().numpy(), ctx["inv"].cpu().numpy()


def check_tower_f32(holder, sd, layers, heads, image, dfeat, r):
    """exact-f32 mode against float64 on the device's own idx; bounds: the f32 parity bounds of tests/test_gpu_vit.py (features within 1e-4 of
    max |ref|, every parameter's gradient and its norm within 2e-3). Then the same pass on an image whose dropped patches are zeroed: bit-identical
    features and gradients - nothing of a dropped patch reaches conv_proj.weight's gradient or anything else."""
    rt, net = holder.rt, holder.image_encoder.img_encoder
    P, p = net.seq_length - 1, net.patch
    Kk = K.kept(P, r)
    steps0 = rt.steps
    feat, grads, idx, inv = tower_pass(holder, image, dfeat)
    B = image.shape[0]
    assert idx.shape == (B, Kk) and inv.shape == (B, P)
    # the set is the reference's for this pass's seed and first site (runtime.StepState), so the host path hands the kernel what it says it does
    want_idx, want_inv = K.keep_indices(rt.base_seed * 1000003 + steps0 + 1, 1, B, P, Kk)
    assert np.array_equal(idx, want_idx) and np.array_equal(inv, want_inv)
    want, ref = K.features_and_grads(sd, image, layers, heads, dfeat, idx)
    err = ((feat.double() - want).abs().max() / want.abs().max()).item()
    print(f"features max |err| / max |ref| = {err:.3e}")
    assert err <= 1e-4
    assert sorted(grads) == sorted(ref)
    gmax = max(g.norm().item() for g in ref.values())
    for k, got in grads.items():
        got, g = got.double(), ref[k]
        assert got.shape == g.shape and g.abs().max() > 0, k
        assert (got - g).abs().max() <= 2e-3 * g.abs().max(), (k, ((got - g).abs().max() / g.abs().max()).item())
        assert abs(got.norm().item() - g.norm().item()) <= 2e-3 * max(g.norm().item(), 1e-3 * gmax), k
    # position rows nobody kept have no gradient at all
    dpos = grads["encoder.pos_embedding"][0]
    for t in range(P):
        if (inv[:, t] < 0).all():
            assert dpos[1 + t].abs().max() == 0
    # the dropped patches zeroed, the same seed again
    W = image.shape[3]
    zeroed = image.clone()
    for b in range(B):
        for t in np.flatnonzero(inv[b] < 0):
            ph, pw = divmod(int(t), W // p)
            zeroed[b, :, ph * p:(ph + 1) * p, pw * p:(pw + 1) * p] = 0
    assert Kk == P or not torch.equal(zeroed, image)
    rt.steps = steps0
    feat2, grads2, idx2, _ = tower_pass(holder, zeroed, dfeat)
    assert np.array_equal(idx2, idx) and torch.equal(feat2, feat)
    for k in grads:
        assert torch.equal(grads2[k], grads[k]), k
    # ... and the next pass draws another set
    if Kk < P:
        _, _, idx3, _ = tower_pass(holder, image, dfeat)
        assert not np.array_equal(idx3, idx)


def bf16_figures(holder, sd, layers, heads, image, dfeat):
    """(forward error / max |ref|, cosine of the flattened parameter gradient) of a bf16 pass against float64 on the same rounded inputs"""
    feat, grads, idx, _ = tower_pass(holder, image, dfeat)
    want, ref = K.features_and_grads(sd, image, layers, heads, dfeat, idx)
    fwd = ((feat.double() - want).abs().max() / want.abs().max()).item()
    a = torch.cat([grads[k].double().flatten() for k in sorted(grads)])
    b = torch.cat([ref[k].flatten() for k in sorted(grads)])
    return fwd, (a @ b / (a.norm() * b.norm())).item()
