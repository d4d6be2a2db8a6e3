"""Kernel-level GPU checks of the parameter-update kernels (csrc/update_ops.hip, csrc/optim_ops.hip) through clip_lite_amd.hip: sumsq, sgd_step and adamw_step called
directly with a hand-made OptimItem table, cast_bf16, transpose_weights with a five-item table, sum_slices. References: tests/loss_ref.py
(float64 on the stored f32 inputs and the f32 hyper-parameters the kernel reads).

Bounds: sumsq 1e-5 * max(1, sum|terms|) and bit-identical between two runs; SGD p / v / slow 1e-6 * max(1, |ref|) per element
(tests/test_wavesim_ops.py's figure); AdamW p 2e-6 * max(1, max|ref|), moments 1e-5 * max|ref| (tests/test_gpu_optim.py's figures against
torch.optim.AdamW); the bf16 copy equals the round-to-nearest-even of the RETURNED p bit for bit; g is zero inside items; every gap between
items, every tail and every buffer the options switch off come back bit for bit; cast_bf16, transpose_weights, sum_slices: exact. No bound was
replaced through the float32 procedure.

Which device path the shapes take (from the launchers in csrc/update_ops.hip and csrc/optim_ops.hip):
  sumsq 0 / 3 / 5        one workgroup; no 4-element chunk (0, 3: the tail loop of thread 0 alone) | one chunk and a 1-element tail
  sumsq 1027             256 chunks: one full workgroup, 3-element tail; out += over one partial
  sumsq 1048583          262145 chunks ask for 1025 workgroups, the cap of 1024 gives thread 0 of workgroup 0 a second trip; 3-element tail; the
                         final kernel folds 1024 partials, four per thread
  sumsq 8195, 7 slots    8 workgroups asked, the launcher caps the grid at the 7 partial slots: threads 0..255 take a second trip
  sgd / adamw            one workgroup per item, a sweep is 256 threads x 4 elements: 4 -> thread 0 alone; 1020 -> 255 threads; 1024 -> one full
                         sweep; 1028 -> thread 0 takes a second sweep; 8192 (the host's chunk) -> 8 sweeps = two rounds of the 4-fold unrolled
                         loop; 64 -> 16 threads
  cast_bf16 0 / 5 / 8    tail loop only (thread 0), twice | one chunk, no tail; 2051: 256 chunks = one full workgroup, 3-element tail
  cast_bf16 8388621      1048577 chunks on the capped 4096 x 256 threads: thread 0 of workgroup 0 takes a second trip; 5-element tail
  transpose_weights      25 workgroups over 5 items located by binary search (first_tile 0, 1, 2, 8, 16): (8, 8) one tile with 8 x 8 live;
                         (64, 64) one full tile; (72, 136) 2 x 3 tiles with 8-row / 8-column remainders; (200, 72) 4 x 2 tiles; the conv weight
                         K = 16, C = 24, R*S = 9 as 9 batched [16][24] -> [24][16] matrices with row strides 216 / 144 and batch strides 24 / 16
  sum_slices (1, 3)      tail only, no additions; (5, 1027) 256 chunks + 3-element tail; (8, 4096) 4 full workgroups
  sum_slices (2, 2097159) 524289 chunks on the capped 2048 x 256 threads: thread 0 takes a second trip; 3-element tail

Measured on an MI355X (`pytest -s`; maxima over the file's cases; no figure feeds a bound):
  sumsq, error / max(1, sum|terms|), kernel / sequential float32 sum: n = 3 7.7e-08 / 1.7e-08   5 8.5e-08 / 2.6e-08   1027 1.8e-08 / 4.9e-07
          1048583 1.3e-08 / 5.9e-04 (the two-stage tree against a running sum)   8195 on 7 slots 4.0e-08 / 9.4e-07
  sgd     max |got - ref| / max(1, |ref|): p, slow 1.1e-07   v 1.5e-07          (bound 1e-6)
  adamw   max |got - ref|: p, slow 2.3e-07 (bound 2e-6 * max(1, max|ref|) = 9e-06)   m 1.9e-09 (bound 3.6e-07)   v2 1.1e-10 (bound 2.8e-08)
"""
import ctypes as C

import numpy as np
import pytest
import torch

import loss_ref as R
from update_table import OPTIONS, clip_setup as _clip_setup

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = 100.0


def _hip():
    from clip_lite_amd import hip
    return hip


def _dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(DEV)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.uint8).numpy()


def _same(t, a):
    """Device tensor t holds exactly the bytes of numpy array a."""
    return np.array_equal(_bits(t), np.ascontiguousarray(a).view(np.uint8).reshape(-1) if a.ndim else a)


# ------------------------------------------------------------------------------------------------ sumsq
@pytest.mark.parametrize("n,slots", [(0, 1024), (3, 1024), (5, 1024), (1027, 1024), (1048583, 1024), (8195, 7)])
def test_sumsq_matches_float64_and_repeats_bitwise(n, slots):
    hip = _hip()
    rng = np.random.default_rng(n)
    x = np.full(n + 8, SENT, np.float32)          # elements past n must not be counted
    x[:n] = rng.standard_normal(n) * 0.3
    terms = x[:n].astype(np.float64) ** 2
    xd = _dev(x)
    outs = []
    for _ in range(2):
        out, parts = _dev([0.75, SENT]), _dev(np.full(slots + 1, SENT))
        hip.sumsq(xd, n, out, parts[:slots])
        got = out.cpu().numpy()
        R.scalar(f"sumsq n = {n}, {slots} slots", got[0], 0.75 + terms.sum(), terms)
        grid = min(max((n // 4 + 255) // 256, 1), 1024, slots)
        assert got[1] == SENT and (parts[grid:] == SENT).all(), "sentinels behind out / the partial slots the grid does not own"
        outs.append(got)
    assert R.same_bits(outs[0], outs[1]) and _same(xd, x)


# ------------------------------------------------------------------------------------------------ sgd_step / adamw_step
COUNTS = [4, 1020, 1024, 1028, 8192, 64]
PAIRS = [(0.2, 1e-4), (1e-3, 0.0)]              # (lr, wd) of the SGD groups
ADAM_PAIRS = [(3e-3, 1e-2), (1e-3, 0.0)]        # tests/test_gpu_optim.py's AdamW groups


def _items(hip, pairs=PAIRS):
    """The item table (device bytes), [(start, count, lr, wd)], the arena length. Starts are multiples of 64; a gap of >= 64 sentinel elements
    precedes the first item and follows every item."""
    rows, start = [], 64
    for i, c in enumerate(COUNTS):
        lr, wd = pairs[i % 2]
        rows.append((start, c, lr, wd))
        start = (start + c + 63) // 64 * 64 + 64
    arr = (hip.OptimItem * len(rows))(*[hip.OptimItem(s, c, lr, wd, 0) for s, c, lr, wd in rows])
    dev = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(DEV)
    return dev, rows, start


def _inside(rows, n):
    m = np.zeros(n, bool)
    for s, c, _, _ in rows:
        m[s:s + c] = True
    return m


def _per_element(rows, n):
    lr, wd = np.zeros(n), np.zeros(n)
    for s, c, a, b in rows:
        lr[s:s + c], wd[s:s + c] = np.float32(a), np.float32(b)
    return lr, wd


def _check_untouched(name, t, before, keep):
    got = t.cpu().numpy() if t.dtype != torch.bfloat16 else t.view(torch.int16).cpu().numpy()
    ref = before if before.dtype != np.uint16 else before.view(np.int16)
    assert np.array_equal(got.view(np.uint8).reshape(len(got), -1)[keep], ref.view(np.uint8).reshape(len(ref), -1)[keep]), f"{name}: a kept element changed"


@pytest.mark.parametrize("sync,cast,clip,gs", OPTIONS)
def test_sgd_step_matches_float64(sync, cast, clip, gs):
    hip = _hip()
    items, rows, n = _items(hip)
    rng = np.random.default_rng(21)
    inside = _inside(rows, n)
    p, g, v, slow = (np.where(inside, rng.standard_normal(n), SENT).astype(np.float32) for _ in range(4))
    cast0 = R.to_bf16_bits(np.full(n, 3.0, np.float32))
    max_norm, ss = _clip_setup(clip, g, inside, gs)
    hp = np.array([0.5, 0.9, max_norm, float(sync), 0.5, gs], np.float32)
    lr, wd = _per_element(rows, n)
    rp, rv, rs = R.sgd_step_ref(p, g, v, slow, lr * float(hp[0]), wd, float(hp[1]), float(hp[2]), sync, float(hp[4]), float(hp[5]), float(ss))
    pd, gd, vd, sd = _dev(p), _dev(g), _dev(v), _dev(slow)
    cd = _dev(cast0, np.uint16).view(torch.bfloat16)
    hip.sgd_step(pd, gd, vd, sd, cd if cast else None, C.c_void_p(items.data_ptr()), len(rows), _dev(hp), _dev([ss]))
    torch.cuda.synchronize()
    for name, t, ref in (("p", pd, rp), ("v", vd, rv), ("slow", sd, rs)):
        got = t.cpu().numpy().astype(np.float64)
        err = np.abs(got - ref)[inside]
        print(f"UPDERR sgd {name} sync={sync} clip={clip}: max err / max(1, |ref|) = {(err / np.maximum(1, np.abs(ref[inside]))).max():.2e}")
        assert (err <= 1e-6 * np.maximum(1.0, np.abs(ref[inside]))).all(), (name, err.max())
    for name, t, before in (("p", pd, p), ("g", gd, g), ("v", vd, v), ("slow", sd, slow), ("cast", cd, cast0)):
        _check_untouched(name, t, before, ~inside)
    assert not gd.cpu().numpy()[inside].any(), "g must be zero inside items"
    if not sync:
        _check_untouched("slow (no sync)", sd, slow, np.ones(n, bool))
    else:
        assert np.array_equal(sd.cpu().numpy()[inside], pd.cpu().numpy()[inside]), "after a sync the slow weights are the fast ones"
    if cast:
        assert np.array_equal(cd.view(torch.int16).cpu().numpy().view(np.uint16)[inside], R.to_bf16_bits(pd.cpu().numpy())[inside]), \
            "the bf16 copy must be the round-to-nearest-even of the returned p"
    else:
        _check_untouched("cast (not given)", cd, cast0, np.ones(n, bool))


@pytest.mark.parametrize("step", [1, 1000])
@pytest.mark.parametrize("sync,cast,clip,gs", OPTIONS)
def test_adamw_step_matches_float64(sync, cast, clip, gs, step):
    hip = _hip()
    items, rows, n = _items(hip, ADAM_PAIRS)
    rng = np.random.default_rng(22 + step)
    inside = _inside(rows, n)
    p, g, slow = (np.where(inside, rng.standard_normal(n), SENT).astype(np.float32) for _ in range(3))
    g = np.where(inside, g * 0.01, SENT).astype(np.float32)
    if step == 1:          # the state FusedAdamW starts from
        m, v2 = np.where(inside, 0.0, SENT).astype(np.float32), np.where(inside, 0.0, SENT).astype(np.float32)
    else:
        m = np.where(inside, rng.standard_normal(n) * 0.01, SENT).astype(np.float32)
        v2 = np.where(inside, m.astype(np.float64) ** 2 * (1 + rng.random(n)), SENT).astype(np.float32)
    cast0 = R.to_bf16_bits(np.full(n, 3.0, np.float32))
    max_norm, ss = _clip_setup(clip, g, inside, gs)
    b1, b2, eps = 0.9, 0.999, 1e-8
    # as FusedAdamW.upload_hp: formed in double on the host, uploaded as f32
    hp = np.array([0.5, b1, max_norm, float(sync), 0.5, gs, b2, eps, 1.0 - b1 ** step, 1.0 - b2 ** step, 1.0 - b1, 1.0 - b2], np.float32)
    lr, wd = _per_element(rows, n)
    h = [float(x) for x in hp]
    rp, rm, rv2, rs = R.adamw_step_ref(p, g, m, v2, slow, lr * h[0], wd, h[2], sync, h[4], h[5], h[6], h[7], h[8], h[9], h[10], h[11], float(ss))
    pd, gd, md, v2d, sd = _dev(p), _dev(g), _dev(m), _dev(v2), _dev(slow)
    cd = _dev(cast0, np.uint16).view(torch.bfloat16)
    hip.adamw_step(pd, gd, md, v2d, sd, cd if cast else None, C.c_void_p(items.data_ptr()), len(rows), _dev(hp), _dev([ss]))
    torch.cuda.synchronize()
    for name, t, ref, tol in (("p", pd, rp, 2e-6), ("slow", sd, rs, 2e-6), ("m", md, rm, 1e-5), ("v2", v2d, rv2, 1e-5)):
        got = t.cpu().numpy().astype(np.float64)
        err = np.abs(got - ref)[inside].max()
        top = np.abs(ref[inside]).max()
        bound = tol * (max(top, 1.0) if tol == 2e-6 else top)
        print(f"UPDERR adamw {name} step={step} sync={sync} clip={clip}: max err {err:.2e}, bound {bound:.2e}")
        assert err <= bound, (name, err, bound)
    for name, t, before in (("p", pd, p), ("g", gd, g), ("m", md, m), ("v2", v2d, v2), ("slow", sd, slow), ("cast", cd, cast0)):
        _check_untouched(name, t, before, ~inside)
    assert not gd.cpu().numpy()[inside].any(), "g must be zero inside items"
    if not sync:
        _check_untouched("slow (no sync)", sd, slow, np.ones(n, bool))
    if cast:
        assert np.array_equal(cd.view(torch.int16).cpu().numpy().view(np.uint16)[inside], R.to_bf16_bits(pd.cpu().numpy())[inside])
    else:
        _check_untouched("cast (not given)", cd, cast0, np.ones(n, bool))


# ------------------------------------------------------------------------------------------------ cast_bf16
SPECIAL_BITS = [0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x80000001, 0x00012345, 0x007FFFFF, 0x00008000, 0x00018000,
                0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3F808001, 0x3F807FFF, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000, 0x7F7F7FFF]


@pytest.mark.parametrize("n", [0, 5, 8, 2051, 8388621])
def test_cast_bf16_is_torch_round_to_nearest_even(n):
    """+-0, +-inf, f32 denormals, exact ties (0x3F808000 rounds down to even, 0x3F818000 up), the largest finite f32 (rounds to inf); no NaN, whose
    payload may legitimately differ. The specials sit at the head (the 8-element chunks), every 37th element and the tail loop."""
    hip = _hip()
    rng = np.random.default_rng(n)
    x = (rng.standard_normal(n) * np.exp(rng.standard_normal(n) * 8)).astype(np.float32)
    sp = np.array(SPECIAL_BITS, np.uint32).view(np.float32)
    k = min(n, len(sp))
    x[:k] = sp[:k]
    x[::37] = np.resize(sp, len(x[::37]))
    if n >= 5:
        x[n - 5:] = sp[[10, 11, 16, 4, 1]]
    assert not np.isnan(x).any()
    src = torch.from_numpy(x)
    want = src.to(torch.bfloat16).view(torch.int16).numpy()
    assert np.array_equal(want.view(np.uint16), R.to_bf16_bits(x))          # torch's CPU cast is the bit arithmetic of round to nearest even
    tail0 = R.to_bf16_bits(np.full(8, 3.0, np.float32)).view(np.int16)
    dst = torch.from_numpy(np.concatenate([np.full(n, 0x4049, np.int16), tail0])).to(DEV).view(torch.bfloat16)
    sd = torch.cat([src, torch.full((8,), SENT)]).to(DEV)
    hip.cast_bf16(sd, dst, n)
    got = dst.view(torch.int16).cpu().numpy()
    bad = np.nonzero(got[:n] != want)[0]
    assert bad.size == 0, f"n = {n}: {bad.size} differ, first at {bad[:4]}: src bits {x.view(np.uint32)[bad[:4]]}, got {got[bad[:4]]}, want {want[bad[:4]]}"
    assert np.array_equal(got[n:], tail0), "the tail past n must be untouched"
    assert torch.equal(sd.cpu()[:n].view(torch.int32), src.view(torch.int32))


# ------------------------------------------------------------------------------------------------ transpose_weights
def test_transpose_weights_five_item_table():
    hip = _hip()
    shapes = [("linear", 8, 8), ("linear", 64, 64), ("linear", 72, 136), ("linear", 200, 72), ("conv", 16, 24, 9)]
    items, spans, off, tile = [], [], 64, 0
    for s in shapes:          # offsets and first_tile as runtime.register_transposed builds them (src and dst share the arena's offsets)
        if s[0] == "linear":
            _, N, K = s
            items.append(hip.TransposeItem(off, off, N, K, K, N, 1, 0, 0, tile))
            tile += ((N + 63) // 64) * ((K + 63) // 64)
            numel = N * K
        else:
            _, K, Cc, RS = s
            items.append(hip.TransposeItem(off, off, K, Cc, RS * Cc, RS * K, RS, Cc, K, tile))
            tile += RS * ((K + 63) // 64) * ((Cc + 63) // 64)
            numel = K * Cc * RS
        spans.append((off, numel))
        off = (off + numel + 63) // 64 * 64 + 64
    assert tile == 25 and [it.first_tile for it in items] == [0, 1, 2, 8, 16]
    total = off
    g = torch.Generator().manual_seed(3)
    src = torch.randn(total, generator=g).to(torch.bfloat16)
    dst0 = (torch.arange(total) % 251 + 1).to(torch.int16)          # a non-zero pattern, a different value at every neighbour
    arr = (hip.TransposeItem * len(items))(*items)
    idev = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(DEV)
    sd, dd = src.to(DEV), dst0.to(DEV).view(torch.bfloat16)
    hip.transpose_weights(sd, dd, idev, len(items), tile)
    got = dd.view(torch.int16).cpu()
    want = dst0.clone()
    sbits = src.view(torch.int16)
    for s, (o, numel) in zip(shapes, spans):
        if s[0] == "linear":
            want[o:o + numel] = sbits[o:o + numel].view(s[1], s[2]).t().reshape(-1)
        else:
            want[o:o + numel] = sbits[o:o + numel].view(s[1], s[3], s[2]).permute(2, 1, 0).reshape(-1)          # [K][RS][C] -> [C][RS][K]
    assert torch.equal(got, want), f"{int((got != want).sum())} elements differ (items and the bytes outside them alike)"
    assert torch.equal(sd.cpu().view(torch.int16), sbits)


# ------------------------------------------------------------------------------------------------ sum_slices
@pytest.mark.parametrize("slices,n", [(1, 3), (5, 1027), (8, 4096), (2, 2097159)])
def test_sum_slices_is_the_f32_sum_in_slice_order(slices, n):
    hip = _hip()
    stride = (n + 3) // 4 * 4 + 4
    g = torch.Generator().manual_seed(n)
    src = torch.randn(slices * stride, generator=g) * torch.exp(torch.randn(slices * stride, generator=g) * 3)
    want = src[:n].clone()
    for s in range(1, slices):          # additions only: no product, so no FMA contraction can change a bit
        want = want + src[s * stride:s * stride + n]
    dst = torch.full((n + 8,), SENT)
    sd, dd = src.to(DEV), dst.to(DEV)
    hip.sum_slices(sd, slices, stride, n, dd)
    got = dd.cpu()
    assert torch.equal(got[:n].view(torch.int32), want.view(torch.int32)), f"{int((got[:n] != want).sum())} of {n} differ"
    assert (got[n:] == SENT).all() and torch.equal(sd.cpu().view(torch.int32), src.view(torch.int32))
