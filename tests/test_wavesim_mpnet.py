"""CPU-side (wave simulator) checks of the MPNet kernels of csrc/bert_ops.hip against tests/mpnet_ref.py in float64: the embedding with position
ids counted in the kernel, the masked mean pool, the bias build and its gradient reduce, and attention with the relative-position bias in both
kernel families with the bucket sums of dS. The same small shapes as tests/test_gpu_mpnet.py. Runs without a GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

import mpnet_ref as R
from simlib import lib, outbuf, prep, ptr, val

BF16, F32 = 0, 1
V, I, F, U64, U32 = C.c_void_p, C.c_int, C.c_float, C.c_uint64, C.c_uint32


def _close(got, ref, rel):
    ref = np.asarray(ref, np.float64)
    assert np.abs(got - ref).max() <= rel * max(np.abs(ref).max(), 1e-6), np.abs(got - ref).max()


def _table():
    from clip_lite_amd import hip
    return np.array(hip.relative_position_buckets(), np.int32)


IDS = np.array([[5, 1, 1, 1, 1, 1, 1], [0, 11, 12, 2, 1, 1, 1], [0, 21, 1, 23, 24, 25, 2]], np.int64)      # lengths 1, 4, 7; a pad id mid-caption


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_embedding_with_position_ids_counted_in_the_kernel(dtype):
    L = lib()
    B, Ls = IDS.shape
    Cc, vocab, max_pos = 64, 32, 12
    rng = np.random.default_rng(1)
    word, wb = prep(rng.standard_normal((vocab, Cc), dtype=np.float32), dtype)
    pos, pb = prep(rng.standard_normal((max_pos, Cc), dtype=np.float32), dtype)
    pid = R.position_ids(torch.tensor(IDS)).numpy()
    out, pids = outbuf((B * Ls, Cc), dtype), np.full(B * Ls, -7, np.int32)
    L.clite_embed_mpnet_fwd.argtypes = [I, V, V, V, V, V, I, I, I, I, I, I, V]
    assert L.clite_embed_mpnet_fwd(dtype, ptr(IDS), ptr(wb), ptr(pb), ptr(out), ptr(pids), B * Ls, Ls, Cc, vocab, max_pos, 1, None) == 0
    assert pids.reshape(B, Ls).tolist() == pid.tolist() == [[2, 1, 1, 1, 1, 1, 1], [2, 3, 4, 5, 1, 1, 1], [2, 3, 1, 4, 5, 6, 7]]
    _close(val(out, dtype), (word[IDS] + pos[pid]).reshape(B * Ls, Cc), 2.0 ** -8 if dtype == BF16 else 0.0)
    # backward: both padding rows (word id 1, position id 1) stay zero, everything else is the scatter-add
    d, db = prep(rng.standard_normal((B * Ls, Cc), dtype=np.float32), dtype)
    dword, dpos = np.zeros((vocab, Cc), np.float32), np.zeros((max_pos, Cc), np.float32)
    L.clite_embed_mpnet_bwd.argtypes = [I, V, V, V, V, V, I, I, I, I, I, I, V]
    assert L.clite_embed_mpnet_bwd(dtype, ptr(IDS), ptr(pids), ptr(db), ptr(dword), ptr(dpos), B * Ls, Ls, Cc, vocab, max_pos, 1, None) == 0
    rw, rp = np.zeros((vocab, Cc)), np.zeros((max_pos, Cc))
    np.add.at(rw, IDS.reshape(-1), d)
    np.add.at(rp, pid.reshape(-1), d)
    assert np.abs(rw[1]).max() > 0 and np.abs(rp[1]).max() > 0
    rw[1], rp[1] = 0, 0
    assert np.abs(dword[1]).max() == 0 and np.abs(dpos[1]).max() == 0
    _close(dword, rw, 1e-6)
    _close(dpos, rp, 1e-6)


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_masked_mean_pool(dtype):
    L = lib()
    B, Ls, Cc = 4, 7, 64
    rng = np.random.default_rng(2)
    h, hb = prep(rng.standard_normal((B, Ls, Cc), dtype=np.float32), dtype)
    dy, dyb = prep(rng.standard_normal((B, Cc), dtype=np.float32), dtype)
    mask = np.zeros((B, Ls), np.int64)
    for b, n in enumerate((1, 3, 7, 0)):
        mask[b, :n] = 1
    out, inv, dh = outbuf((B, Cc), dtype), np.full(B, np.nan, np.float32), outbuf((B, Ls, Cc), dtype)
    L.clite_mean_pool_fwd.argtypes = [I, V, V, V, V, I, I, I, V]
    L.clite_mean_pool_bwd.argtypes = [I, V, V, V, V, I, I, I, V]
    assert L.clite_mean_pool_fwd(dtype, ptr(hb), ptr(mask), ptr(out), ptr(inv), B, Ls, Cc, None) == 0
    assert L.clite_mean_pool_bwd(dtype, ptr(dyb), ptr(mask), ptr(inv), ptr(dh), B, Ls, Cc, None) == 0
    h64 = torch.tensor(h, dtype=torch.float64, requires_grad=True)
    ref = R.mean_pool(h64, torch.tensor(mask))
    ref.backward(torch.tensor(dy, dtype=torch.float64))
    np.testing.assert_allclose(inv, [1.0, 1.0 / 3.0, 1.0 / 7.0, 1e9], rtol=1e-6)
    tol = 2.0 ** -8 if dtype == BF16 else 1e-6
    got, gdh = val(out, dtype), val(dh, dtype)
    assert np.isfinite(got).all() and np.abs(got[3]).max() == 0 and np.abs(gdh[3]).max() == 0          # the all-zero mask gives 0, not NaN
    _close(got, ref.detach().numpy(), tol)
    _close(gdh, h64.grad.numpy(), tol)


@pytest.mark.parametrize("Ls", [1, 7, 32])
def test_bias_build_and_gradient_reduce(Ls):
    L = lib()
    H = 3
    rng = np.random.default_rng(Ls)
    rel = rng.standard_normal((32, H), dtype=np.float32)
    bias = np.full((H, 32, 32), np.nan, np.float32)
    L.clite_attention_bias_build.argtypes = [V, V, V, I, I, V]
    assert L.clite_attention_bias_build(ptr(rel), ptr(_table()), ptr(bias), H, Ls, None) == 0
    want = np.zeros((H, 32, 32), np.float32)
    want[:, :Ls, :Ls] = R.position_bias(torch.tensor(rel), Ls).numpy()
    assert np.array_equal(bias, want)
    L.clite_attention_bias_grad_reduce.argtypes = [V, V, I, I, V]
    for rows in (1, 37):
        partials = rng.integers(-8, 9, (rows, H, 32)).astype(np.float32)
        drel = rng.integers(-3, 4, (32, H)).astype(np.float32)
        want = drel + partials.sum(0).T
        assert L.clite_attention_bias_grad_reduce(ptr(partials), ptr(drel), rows, H, None) == 0
        assert np.array_equal(drel, want)


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("B,Ls,H", [(3, 7, 1), (2, 30, 2)])
def test_attention_with_bias_and_bucket_sums(dtype, B, Ls, H):
    L = lib()
    rng = np.random.default_rng(10 * B + Ls)
    qkv, qb = prep(0.7 * rng.standard_normal((B * Ls, 3 * H * 64), dtype=np.float32), dtype)
    do, dob = prep(rng.standard_normal((B * Ls, H * 64), dtype=np.float32), dtype)
    bias = rng.standard_normal((H, 32, 32), dtype=np.float32)
    mask = np.ones((B, Ls), np.int64)
    mask[1, Ls - 2:] = 0
    mask[B - 1, 1:] = 0
    fsig = [I, V, V, V, V, I, I, I, F, U64, U32, V]
    L.clite_attention_bias_fwd.argtypes = fsig
    L.clite_attention_bias_bwd.argtypes = [I, V, V, V, V, V, V, V, I, I, I, F, U64, U32, V]
    ctx, dqkv = outbuf((B * Ls, H * 64), dtype), outbuf((B * Ls, 3 * H * 64), dtype)
    partials = np.full((B * H, 32), np.nan, np.float32)
    assert L.clite_attention_bias_fwd(dtype, ptr(qb), ptr(mask), ptr(bias), ptr(ctx), B, Ls, H, 0.0, 0, 0, None) == 0
    assert L.clite_attention_bias_bwd(dtype, ptr(qb), ptr(mask), ptr(bias), ptr(_table()), ptr(dob), ptr(dqkv), ptr(partials), B, Ls, H, 0.0, 0, 0, None) == 0
    q = torch.tensor(qkv, dtype=torch.float64).view(B, Ls, -1).requires_grad_(True)
    b = torch.tensor(bias[:, :Ls, :Ls], dtype=torch.float64).requires_grad_(True)
    ref = R.attention(q, torch.tensor(mask), b, H)
    ref.backward(torch.tensor(do, dtype=torch.float64).view(B, Ls, -1))
    drel = np.zeros((32, H))
    for i in range(Ls):
        for j in range(Ls):
            drel[R.bucket(j - i)] += b.grad[:, i, j].numpy()
    fwd, bwd = (1e-2, 2e-2) if dtype == BF16 else (1e-5, 1e-5)
    _close(val(ctx, dtype), ref.detach().numpy().reshape(B * Ls, -1), fwd)
    _close(val(dqkv, dtype), q.grad.numpy().reshape(B * Ls, -1), bwd)
    _close(partials.reshape(B, H, 32).sum(0).T, drel, bwd)
    # bias = 0: the entry points without bias, bit for bit
    zero = np.zeros_like(bias)
    ctx0, ctx1 = outbuf(ctx.shape, dtype), outbuf(ctx.shape, dtype)
    L.clite_attention_fwd.argtypes = fsig[:3] + fsig[4:]
    assert L.clite_attention_bias_fwd(dtype, ptr(qb), ptr(mask), ptr(zero), ptr(ctx0), B, Ls, H, 0.0, 0, 0, None) == 0
    assert L.clite_attention_fwd(dtype, ptr(qb), ptr(mask), ptr(ctx1), B, Ls, H, 0.0, 0, 0, None) == 0
    assert np.array_equal(ctx0, ctx1)
