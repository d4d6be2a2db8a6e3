"""Host checks of tests/dropout_ref.py and tests/bert_dropout_ref.py, the references the GPU tests of BERT's dropout masks and bf16 epilogues
(tests/test_gpu_bert_linears.py, tests/test_gpu_bert_dropout_tower.py) stand on. Runs without a GPU.

- Philox4x32-10 against the three known-answer vectors published with Random123 (kat_vectors), so the numpy generator is tied to the paper's
  definition and not to csrc/rng.h.
- The numpy masks against the wave-simulator build of the kernel sources, element for element: LayerNorm forward, the GEMM epilogue under every
  forced tile policy, the attention forward of both pitches. This anchors the reference to the source's definition.
- Which kernel the automatic tile policy selects for BERT's four epilogue forms at the shapes the GPU tests use (the GPU tests cannot see it).
- The fast GELU of the bf16 epilogues, emulated in float32, over every finite bf16 input against float64.
- That the tower test's bound would catch a mis-indexed mask: the float64 reference with one site's mask swapped moves the gradients by far more
  than three times the bf16 rounding floor."""
import ctypes as C

import numpy as np
import pytest
import torch

import bert_dropout_ref as T
import dropout_ref as D
import simlib
from simlib import from_bf16, lib, make_ep, outbuf, prep, ptr, to_bf16, val

BF16, F32 = 0, 1
V, I, F, U64, U32 = C.c_void_p, C.c_int, C.c_float, C.c_uint64, C.c_uint32
P_DROP, SEED = 0.1, 1234


# ------------------------------------------------------------------------------------------------ the generator
def _hex(words):
    return " ".join("%08x" % int(w) for w in words)


def test_philox_known_answers():
    assert _hex(D.philox4x32_10((0, 0, 0, 0), (0, 0))) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    ones = 0xFFFFFFFF
    assert _hex(D.philox4x32_10((ones,) * 4, (ones, ones))) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert _hex(D.philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0))) == "d16cfe09 94fdcceb 5001e420 24126ea1"
    # vectorised over the counter: the same answers as one call each
    q = np.arange(5, dtype=np.uint64)
    both = D.philox4x32_10((q, 0, 7, 1), (3, 4))
    assert all((both[i] == D.philox4x32_10((i, 0, 7, 1), (3, 4))).all() for i in range(5))


def test_keep_fraction_and_stream_layout():
    keep = D.hidden_keep(SEED, 5, 200, 136, P_DROP)
    assert abs(keep.mean() - 0.89989) < 5e-6          # (the value of an independent numpy implementation of the same definition)
    # eight elements per call, the low half of a word first
    w = D.philox4x32_10((1, 0, 5, 1), (SEED, 0))
    u = D.dropout_uniform(SEED, 5, 16)[8:]
    assert (u * 65536 == np.array([[x & 0xFFFF, x >> 16] for x in w.tolist()]).reshape(-1)).all()
    # the attention / prior-noise stream: four per call, counter word 3 = 0, the top 24 bits
    w = D.philox4x32_10((2, 0, 9, 0), (SEED, 0))
    assert (D.uniform8(SEED, 9, 12)[8:] * 2.0 ** 24 == (w >> 8)).all()
    assert not (D.hidden_keep(SEED, 5, 8, 8, P_DROP) == D.hidden_keep(SEED, 6, 8, 8, P_DROP)).all()
    # a seed above 2^32 reaches the second key word; bit 31 of the site (the indirect-seed flag) is not part of the counter
    assert not (D.dropout_keep(SEED + (1 << 32), 5, 512, 0.5) == D.dropout_keep(SEED, 5, 512, 0.5)).all()
    assert (D.dropout_keep(SEED, 5 | 0x80000000, 512, 0.5) == D.dropout_keep(SEED, 5, 512, 0.5)).all()


# ------------------------------------------------------------------------------------------------ against the simulator build
@pytest.mark.parametrize("dtype", [BF16, F32])
def test_layernorm_forward_mask_is_the_numpy_mask(dtype):
    L = lib()
    L.clite_layernorm_fwd.argtypes = [I, V, V, V, F, V, V, I, I, F, U64, U32, V]
    M, Cc = 37, 768
    rng = np.random.default_rng(3)
    _, xb = prep(rng.standard_normal((M, Cc), dtype=np.float32), dtype)
    gamma, beta = np.ones(Cc, np.float32), np.full(Cc, 0.1, np.float32)
    out, stats = outbuf((M, Cc), dtype), np.zeros((M, 2), np.float32)
    assert L.clite_layernorm_fwd(dtype, ptr(xb), ptr(gamma), ptr(beta), 1e-12, ptr(out), ptr(stats), M, Cc, P_DROP, SEED, 7, None) == 0
    assert ((val(out, dtype) != 0) == D.hidden_keep(SEED, 7, M, Cc, P_DROP)).all()


@pytest.mark.parametrize("policy", [1, 2, 3, 4], ids=["w128", "w256x128", "w256", "narrow"])
def test_gemm_epilogue_mask_is_the_numpy_mask(policy):
    """A = 0, bias = 1, residual = 0: the output is non-zero exactly where the element was kept. bf16 with a residual is the 8-wave kernels'
    compiled-in dropout form under policies 1 - 3 and the 4-wave kernel's run-time-flag epilogue under policy 4."""
    L = lib()
    M, N, K = 200, 136, 104
    A, B, R = np.zeros((M, K), np.uint16), to_bf16(np.ones((N, K), np.float32)), np.zeros((M, N), np.uint16)
    bias = np.ones(N, np.float32)
    out = np.zeros((M, N), np.uint16)
    ep = make_ep(out, N, bias=bias, drop_p=P_DROP, drop_seed=SEED, drop_site=5, residual=R)
    assert L.clite_set_tile_policy(policy) == 0
    try:
        simlib.clear_launch_log()
        assert L.clite_gemm_nt(ptr(A), K, ptr(B), K, M, N, K, BF16, C.byref(ep), None) == 0
        (kernel,) = [n for n, _, _ in simlib.launch_log()]
    finally:
        L.clite_set_tile_policy(0)
    if policy == 4:
        assert "::igemm_dma_kernel" in kernel
    else:
        assert "::igemm_wide_kernel<" in kernel and kernel.split(">(")[0].endswith(", 5")
    got = from_bf16(out)
    keep = D.hidden_keep(SEED, 5, M, N, P_DROP)
    assert ((got != 0) == keep).all()
    assert (np.abs(got[keep] - 1 / 0.9) <= 2.0 ** -8 * (1 / 0.9)).all()


@pytest.mark.parametrize("B,L,H", [(2, 30, 2), (2, 40, 2)])
def test_attention_forward_mask_is_the_numpy_mask(B, L, H):
    """Exact-f32 forward with V = one-hot rows (ctx[i][j] is then the dropped probability of key j), with and without dropout: the ratio is the
    multiplier. 30 tokens run the 32-pitch kernel, 40 the 128-pitch one."""
    import attention_long_ref as R
    lb = lib()
    lb.clite_attention_fwd.argtypes = [I, V, V, V, I, I, I, F, U64, U32, V]
    g = torch.Generator().manual_seed(L)
    qkv = (torch.randn(B * L, 3 * H * 64, generator=g) * 0.7).bfloat16().float()
    probe = np.ascontiguousarray(R.one_hot_probe(qkv, B, L, H, 0).numpy(), np.float32)
    mask = np.ones((B, L), np.int64)
    mask[1, L - 7:] = 0
    outs = []
    for drop in ((P_DROP, SEED, 9), (0.0, 0, 0)):
        ctx = np.zeros((B * L, H * 64), np.float32)
        assert lb.clite_attention_fwd(F32, ptr(probe), ptr(mask), ptr(ctx), B, L, H, *drop, None) == 0
        outs.append(ctx.reshape(B, L, H, 64)[..., :L].transpose(0, 2, 1, 3))          # [B][H][i][j]
    pd, p0 = outs
    valid = np.broadcast_to(mask[:, None, None, :] != 0, p0.shape)
    assert (p0[valid] > 1e-20).all()          # every attended key is observable
    keep = D.attention_keep(SEED, 9, B, H, L, P_DROP)
    assert ((pd[valid] != 0) == keep[valid]).all()
    assert abs(keep.mean() - 0.9) < 0.01
    assert (np.abs(pd[valid & keep] / p0[valid & keep] - 1 / 0.9) < 1e-5).all()


def test_uniform_fill_is_the_numpy_stream():
    L = lib()
    L.clite_uniform_fill.argtypes = [I, V, U64, U64, U32, V]
    n = 4096
    u = np.zeros(n, np.float32)
    assert L.clite_uniform_fill(F32, ptr(u), n, 42, 1, None) == 0
    ref = D.uniform8(42, 1, n)
    assert (u.view(np.uint32) == ref.view(np.uint32)).all() and (ref >= 0).all() and (ref < 1).all()


# ------------------------------------------------------------------------------------------------ which kernel BERT's four forms select
def _bert_epilogue(form, ptr_):
    return {3: dict(bias=ptr_, preact=ptr_, act=2), 4: dict(dact_aux=ptr_, dact=2, colsum=ptr_, colsum_rows=1),
            5: dict(bias=ptr_, drop_p=P_DROP, drop_seed=SEED, drop_site=5, residual=ptr_), 6: dict(residual=ptr_)}[form]


@pytest.mark.parametrize("form", [3, 4, 5, 6])
@pytest.mark.parametrize("M,N,K", [(180, 768, 768), (180, 3072, 768), (180, 768, 3072)])
def test_automatic_policy_runs_bert_forms_on_the_128_tile(M, N, K, form):
    """Dry run, automatic tile policy: FFN1 forward (3), FFN2's input gradient (4), the output projections (5) and the residual-stream input
    gradients (6) at the one-layer tower's 180 rows each select igemm_wide_kernel<WideCfg<128, 128, ...>> with that form compiled in."""
    L = lib()
    dummy = np.zeros(4096, np.uint8)
    ep = simlib.Epilogue()
    ep.out, ep.ldc, ep.alpha = dummy.ctypes.data, N, 1.0
    for k, v in _bert_epilogue(form, dummy.ctypes.data).items():
        setattr(ep, k, v)
    assert L.clite_set_tile_policy(0) == 0
    simlib.set_dry_run(True)
    simlib.clear_launch_log()
    try:
        assert L.clite_gemm_nt(ptr(dummy), K, ptr(dummy), K, M, N, K, BF16, C.byref(ep), None) == 0
        log = simlib.launch_log()
    finally:
        simlib.set_dry_run(False)
        simlib.clear_launch_log()
    (kernel,) = [n for n, _, _ in log]
    assert "::igemm_wide_kernel<clite::WideCfg<128, 128, " in kernel and kernel.split(">(")[0].endswith(", %d" % form), kernel


# ------------------------------------------------------------------------------------------------ the fast GELU
def test_fast_gelu_emulation_over_every_finite_bf16():
    """gelu_t<bf16> / gelu_grad_t<bf16> in float32 numpy with exact division and exp2, against float64 x Phi(x) and Phi(x) + x phi(x): the
    approximation's own error, before the hardware reciprocal and exp2 add theirs. Bounds: D.GELU_EMU_ERR and D.GELU_GRAD_EMU_ERR (1.35e-7 *
    max(1, |x|) and 2.68e-7, measured for this formula) with 10 % slack; the GPU test allows three times these."""
    x = D.finite_bf16_values()
    assert x.size == 65280
    g, dg = D.gelu_exact(x)
    fg, fdg = D.gelu_fast(x), D.gelu_grad_fast(x)
    assert not np.isnan(fg).any() and not np.isnan(fdg).any()
    e1 = (np.abs(fg - g) / np.maximum(1.0, np.abs(x.astype(np.float64)))).max()
    e2 = np.abs(fdg - dg).max()
    print(f"fast GELU emulation: {e1:.3e} * max(1, |x|); GELU' {e2:.3e}")
    assert e1 <= 1.1 * D.GELU_EMU_ERR
    assert e2 <= 1.1 * D.GELU_GRAD_EMU_ERR


# ------------------------------------------------------------------------------------------------ the tower bound's sensitivity
def test_a_swapped_hidden_mask_is_far_outside_the_tower_bound():
    """One BERT layer in float64 (vocabulary cut to 2000 rows to keep this quick), dropout on. floor_t = |Rbf - R64| / |R64| is what the GPU test
    multiplies by 3. With the attention output projection's mask (d1) replaced by the FFN output projection's (d2) — what a writer and a
    regenerator that index differently amount to — the pooled output and the gradients of everything in front of that site move by much more."""
    from detfill import det_fill
    from oracle.ref_model import OracleBert
    vocab = 2000
    ids, mask, dpooled = T.problem(vocab=vocab)
    Bc, Lc = ids.shape
    sd = det_fill(OracleBert(1, vocab=vocab)).state_dict()
    drops = {name: (P_DROP, 1000004, i + 1) for i, name in enumerate(T.SITES)}
    mults = T.multipliers(drops, Bc, Lc)
    p64, g64 = T.run(T.build(sd, mults, vocab=vocab), ids, mask, dpooled)
    pbf, gbf = T.run(T.build(sd, mults, emulate=True, vocab=vocab), ids, mask, dpooled)
    swapped = dict(mults, d1=mults["d2"])
    psw, gsw = T.run(T.build(sd, swapped, vocab=vocab), ids, mask, dpooled)
    assert g64[T.ZERO_GRAD].norm() < 1e-9 * g64[T.ZERO_GRAD.replace("key", "query")].norm()
    floors = {n: T.rel_l2(gbf[n], g64[n]) for n in g64 if n != T.ZERO_GRAD}
    floors["pooled"] = T.rel_l2(pbf, p64)
    moved = {n: T.rel_l2(gsw[n], g64[n]) for n in g64 if n != T.ZERO_GRAD}
    moved["pooled"] = T.rel_l2(psw, p64)
    worst = max(floors.values())
    print("floors: pooled %.3e, largest %.3e" % (floors["pooled"], worst))
    assert 1e-4 < floors["pooled"] < 2e-2 and worst < 5e-2          # rounding noise of 2^-9 roundings, not a broken emulation
    layer = "encoder.layer.0."
    downstream = ["pooled", layer + "attention.output.dense.weight", layer + "attention.self.query.weight", layer + "attention.self.key.weight",
                  layer + "attention.self.value.weight", "embeddings.word_embeddings.weight", layer + "intermediate.dense.weight",
                  layer + "output.dense.weight"]
    for n in downstream:
        print(f"{n}: swapped mask moves it by {moved[n]:.3e}, floor {floors[n]:.3e}")
        assert moved[n] > 3 * floors[n] and moved[n] > 3 * worst, n
