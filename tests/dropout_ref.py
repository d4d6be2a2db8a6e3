"""The dropout masks and the prior noise of the kernel library as plain numpy (test infrastructure; shared by the host and the GPU tests).

csrc/rng.h defines a mask element as a pure function of (seed, site, element index) through Philox4x32-10 (Salmon et al., "Parallel random
numbers: as easy as 1, 2, 3", SC'11). This file is a second, independent statement of that definition in uint64 arithmetic: it shares no code
with the kernels or with the simulator build, so a kernel that indexes the stream differently from what rng.h describes disagrees with it.

Philox4x32-10: counter (c0, c1, c2, c3), key (k0, k1), multipliers M0 = 0xD2511F53 and M1 = 0xCD9E8D57, key increments (Weyl constants)
W0 = 0x9E3779B9 and W1 = 0xBB67AE85. One round maps the counter to
    (hi(M1 * c2) ^ c1 ^ k0,  lo(M1 * c2),  hi(M0 * c0) ^ c3 ^ k1,  lo(M0 * c0))
and the key is bumped by (W0, W1) after every round; ten rounds.

The three streams, all with key = (seed & 0xffffffff, seed >> 32) and counter words (q & 0xffffffff, q >> 32, site, w3):
    hidden dropout (dropout_uniform8)   w3 = 1, q = idx >> 3: element idx takes 16 bits of output word (idx & 7) >> 1, the low half for an even
                                        idx and the high half for an odd one; u = bits / 65536; kept when u >= p
    attention dropout (rng_uniform4)    w3 = 0, q = idx >> 2: element idx takes output word idx & 3; u = (word >> 8) / 2^24; kept when u >= p
    prior noise (rng_uniform8)          the rng_uniform4 stream, eight elements at a time
Comparisons are made in float32, as the kernels make them (p = 0.1 is 0.100000001490116 as a float32; u is exact in float32)."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
LO = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter: four arrays (or ints) of 32-bit words, key: two 32-bit ints (or arrays) -> uint32 array [..., 4]."""
    c = [np.asarray(w, dtype=np.uint64) & LO for w in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = (np.asarray(w, dtype=np.uint64) & LO for w in key)
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]          # 32 x 32 -> 64 bits: exact in uint64
        c = [(p1 >> S32) ^ c[1] ^ k0, p1 & LO, (p0 >> S32) ^ c[3] ^ k1, p0 & LO]
        k0, k1 = (k0 + np.uint64(W0)) & LO, (k1 + np.uint64(W1)) & LO
    return np.stack(c, axis=-1).astype(np.uint32)


def _words(seed, site, n_calls, w3):
    """Output words [n_calls][4] of the calls q = 0 .. n_calls - 1 of one stream."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    q = np.arange(n_calls, dtype=np.uint64)
    return philox4x32_10((q & LO, q >> S32, int(site) & 0x7FFFFFFF, w3), (seed & 0xFFFFFFFF, seed >> 32))


def dropout_uniform(seed, site, n_elements):
    """float32 [n_elements]: the hidden-dropout uniforms on the 2^-16 grid."""
    w = _words(seed, site, (n_elements + 7) // 8, 1)                     # [calls][4]
    halves = np.stack([w & np.uint32(0xFFFF), w >> np.uint32(16)], axis=-1)      # [calls][4][low, high]
    return (halves.reshape(-1)[:n_elements].astype(np.float32) / np.float32(65536.0)).astype(np.float32)


def dropout_keep(seed, site, n_elements, p):
    """bool [n_elements]: True where the hidden dropout of (seed, site) keeps element idx."""
    return dropout_uniform(seed, site, n_elements) >= np.float32(p)


def hidden_keep(seed, site, M, C, p):
    """bool [M][C] of a dense [M][C] tensor (element index row * C + col)."""
    return dropout_keep(seed, site, M * C, p).reshape(M, C)


def uniform8(seed, site, n):
    """float32 [n] in [0, 1): the prior-noise stream (clite_uniform_fill), 24 bits per element."""
    w = _words(seed, site, (n + 3) // 4, 0).reshape(-1)[:n]
    return ((w >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)).astype(np.float32)


def attention_pitch(L):
    """Row pitch of the attention kernels' mask index: 32 for the one-tile kernels (L <= 32), 128 for the four-key-tile kernels (33 .. 128)."""
    assert 1 <= L <= 128
    return 32 if L <= 32 else 128


def attention_keep(seed, site, B, H, L, p):
    """bool [B][H][L][L]: True where the attention dropout keeps probability (i, j) of head h of sample b; element index
    ((b * H + h) * P + i) * P + j with P = attention_pitch(L)."""
    P = attention_pitch(L)
    u = uniform8(seed, site, B * H * P * P).reshape(B, H, P, P)
    return (u >= np.float32(p))[:, :, :L, :L].copy()


# ------------------------------------------------------------------------------------------------ the bf16 epilogues' fast GELU
# What the float32 emulation below measures over every finite bf16 input against float64 (tests/test_dropout_ref_host.py asserts them with 10 %
# slack): |gelu - x Phi(x)| <= GELU_EMU_ERR * max(1, |x|), |gelu' - (Phi(x) + x phi(x))| <= GELU_GRAD_EMU_ERR.
GELU_EMU_ERR, GELU_GRAD_EMU_ERR = 1.35e-7, 2.68e-7


def _f32(x):
    return np.asarray(x, dtype=np.float32)


GELU_TAIL_X = np.float32(-5.0)          # below it the epilogues take the tail polynomial (csrc/igemm.h GELU_TAIL_X)
_AS = (1.061405429, 1.453152027, 1.421413741, 0.284496736, 0.254829592)          # Abramowitz & Stegun 7.1.26, a5 .. a1 (signs in the Horner form below)
_TAIL = (0.22693126, -0.058025274, 0.13806723, 0.083405286, 0.093033388)         # igemm.h's tail fit of Phi(-a) e^(a^2 / 2), q5 .. q1


def gelu_fast_parts(x, tail=False):
    """float32 emulation of csrc/igemm.h gelu_fast_parts<TAIL> (same constants, same operation order, exact division and exp2; the fused
    multiply-adds are formed in float64 and rounded once): (0.5 erfc(|x| / sqrt 2), exp(-x^2 / 2))."""
    x = _f32(x)
    ax = np.abs(x)
    c = np.float32(np.float32(0.3275911) * np.float32(0.70710678118654752))
    t = (np.float32(1.0) / (c.astype(np.float64) * ax.astype(np.float64) + 1.0).astype(np.float32)).astype(np.float32)
    k = np.float32(np.float32(-0.5) * np.float32(1.4426950408889634))
    with np.errstate(over="ignore", under="ignore"):
        gauss = np.exp2(((x * x).astype(np.float32) * k).astype(np.float64)).astype(np.float32)
        if tail:
            q5, q4, q3, q2, q1 = (np.float32(v) for v in _TAIL)
            poly = ((((q5 * t + q4).astype(np.float32) * t + q3).astype(np.float32) * t + q2).astype(np.float32) * t + q1).astype(np.float32) * t
        else:
            h = np.float32(0.5)
            a5, a4, a3, a2, a1 = (np.float32(h * np.float32(v)) for v in _AS)
            poly = ((((a5 * t - a4).astype(np.float32) * t + a3).astype(np.float32) * t - a2).astype(np.float32) * t + a1).astype(np.float32) * t
        return (poly.astype(np.float32) * gauss).astype(np.float32), gauss


def _gelu_from(x, h):
    return (-np.abs(x).astype(np.float64) * h.astype(np.float64) + np.maximum(x, np.float32(0)).astype(np.float64)).astype(np.float32)


def gelu_fast(x):
    """gelu_t<bf16>: fma(-|x|, h, max(x, 0)), h from the tail polynomial below GELU_TAIL_X."""
    x = _f32(x)
    return np.where(x < GELU_TAIL_X, _gelu_from(x, gelu_fast_parts(x, True)[0]), _gelu_from(x, gelu_fast_parts(x)[0]))


def gelu_grad_fast(x):
    """gelu_grad_t<bf16>: fma(x / sqrt(2 pi), gauss, cdf) with cdf = 0.5 + copysign(0.5 - h, x), and below GELU_TAIL_X cdf = h of the tail
    polynomial (Phi(x) = h for x < 0, without the cancellation)."""
    x = _f32(x)
    h, g = gelu_fast_parts(x)
    ht, _ = gelu_fast_parts(x, True)
    cdf = (np.float32(0.5) + np.copysign((np.float32(0.5) - h).astype(np.float32), x)).astype(np.float32)
    cdf = np.where(x < GELU_TAIL_X, ht, cdf)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        xs = (x * np.float32(0.39894228040143268)).astype(np.float32)
        return (xs.astype(np.float64) * g.astype(np.float64) + cdf.astype(np.float64)).astype(np.float32)


def gelu_exact(x):
    """float64 (x Phi(x), Phi(x) + x phi(x))."""
    from scipy.special import erfc
    x = np.asarray(x, dtype=np.float64)
    cdf = 0.5 * erfc(-x / np.sqrt(2.0))
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        pdf = np.exp(-0.5 * x * x) / np.sqrt(2.0 * np.pi)
        xp = np.where(pdf == 0.0, 0.0, x * pdf)
        # x Phi(x) for very negative x: Phi underflows before x overflows, the product is 0
        g = np.where(cdf == 0.0, 0.0, x * cdf)
    return g, cdf + xp


def finite_bf16_values():
    """float32 [65280]: every finite bf16 value (both zeros and the subnormals included)."""
    bits = np.arange(65536, dtype=np.uint32)
    bits = bits[(bits & 0x7F80) != 0x7F80]
    return (bits << np.uint32(16)).view(np.float32)
