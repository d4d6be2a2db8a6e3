// Kernels of the BERT text encoder outside the GEMMs (reference encoder.py:165-196 -> transformers.BertModel,
// BertConfig defaults: hidden 768, 12 heads x 64, LayerNorm eps 1e-12, dropout 0.1, additive attention mask,
// pooler = tanh(W h_CLS + b)): embedding gather, LayerNorm forward/backward (also nn.LayerNorm of the MI heads,
// loss.py:23), per-head attention forward/backward for captions of <= 32 tokens (config.py:69: 30).
#include "vec.h"
#include "rng.h"
#include "det.h"
#include "clite.h"

using namespace clite;

namespace {

constexpr int LN_MAXCH = 4;   // 8-element chunks per lane: C <= 64*4*8 = 2048

struct Drop { float p; uint64_t seed; uint32_t site; };

DEV void apply_dropout8(const Drop& d, size_t idx, float (&v)[8]) {
  float u[8];
  dropout_uniform8(d.seed, d.site, idx, u);
  float ks = 1.0f / (1.0f - d.p);
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = u[e] >= d.p ? v[e] * ks : 0.f;
}

// one wave per row; out = dropout((x - mean) * rstd * gamma + beta); stats[row] = (mean, rstd)
// Q (bf16, clite_layernorm_fwd_q8): the producer-fused e4m3 quantiser of the fp8 linears that read `out` - the e4m3 copy of the stored value at a
// delayed scale and the call's max |out| (one integer atomic max per workgroup), as bn_apply's (resnet_ops.hip)
struct LnQ8 { uint8_t* out; const float* scale; float* amax; };
template <typename T, int NCH, bool Q = false>      // NCH = 8-element chunks per lane: C <= 64*NCH*8 (2 covers BERT's 768, 4 the 2048-wide heads)
__global__ __launch_bounds__(256) void layernorm_fwd_kernel(const T* x, const float* gamma, const float* beta, float eps, T* out,
                                                            float* stats, int M, int C, Drop drop, LnQ8 q8) {
  float qmax = 0.f;
  bool qnan = false;
  const float qscale = (Q && q8.out) ? q8.scale[0] : 1.f;
  seed_resolve(drop.seed, drop.site);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nchunk = C / 8;
  const float invC = 1.0f / (float)C;
  for (int row = blockIdx.x * 4 + wave; row < M; row += gridDim.x * 4) {
    float v[NCH][8];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      int c = lane + 64 * i;
      if (c < nchunk) {
        load8(x + (size_t)row * C + c * 8, v[i]);
#pragma unroll
        for (int e = 0; e < 8; ++e) s += v[i][e];
      }
    }
    float mean = wave_sum(s) * invC;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      int c = lane + 64 * i;
      if (c < nchunk) {
#pragma unroll
        for (int e = 0; e < 8; ++e) { float d = v[i][e] - mean; q += d * d; }
      }
    }
    float rstd = rsqrtf(wave_sum(q) * invC + eps);
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      int c = lane + 64 * i;
      if (c < nchunk) {
        float g[8], b[8], o[8];
        load8(gamma + c * 8, g);
        load8(beta + c * 8, b);
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (v[i][e] - mean) * rstd * g[e] + b[e];
        size_t idx = (size_t)row * C + c * 8;
        if (drop.p > 0.f) apply_dropout8(drop, idx, o);
        store8(out + idx, o);
        if constexpr (Q) {
          round8_bf16(o);          // quantise / measure the value as stored
#pragma unroll
          for (int e = 0; e < 8; ++e) { qmax = fmaxf(qmax, fabsf(o[e])); qnan = qnan || o[e] != o[e]; }
          if (q8.out) {
            uint32_t w[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const float p0 = o[2 * e] * qscale, q0 = o[2 * e + 1] * qscale;          // (a NaN passes the clamp untouched: fp8_ops.hip)
              const float pp = p0 != p0 ? p0 : fminf(fmaxf(p0, -448.f), 448.f), qq = q0 != q0 ? q0 : fminf(fmaxf(q0, -448.f), 448.f);
              w[e] = cvt2_fp8(pp, qq);
            }
            *(u32x2*)(q8.out + idx) = u32x2{w[0] | (w[1] << 16), w[2] | (w[3] << 16)};
          }
        }
      }
    }
    if (lane == 0 && stats) { stats[row * 2] = mean; stats[row * 2 + 1] = rstd; }
  }
  if constexpr (Q) {
    if (q8.amax) {
      __shared__ uint32_t red[4];
      uint32_t mb = qnan ? 0x7FC00000u : f32_bits(qmax);
#pragma unroll
      for (int sh = 32; sh >= 1; sh >>= 1) { const uint32_t o = (uint32_t)wave_shfl_xor_i((int)mb, sh); mb = o > mb ? o : mb; }
      if (lane == 0) red[wave] = mb;
      __syncthreads();
      if (threadIdx.x == 0) {
        uint32_t b = red[0];
        for (int w = 1; w < 4; ++w) b = red[w] > b ? red[w] : b;
        atomic_max_u32((uint32_t*)q8.amax + (blockIdx.x % CLITE_FP8_AMAX_REPLICAS) * CLITE_FP8_AMAX_STRIDE, b);
      }
    }
  }
}

// dy' = dropout_mask_in(dy); dx = rstd*(g - mean(g) - xhat*mean(g*xhat)), g = dy'*gamma; dgamma += sum dy'*xhat; dbeta += sum dy'
// optional second output dx_masked = dropout_mask_out(dx)
// NW waves per workgroup, one row per wave at a time; one float atomic per column per workgroup for dgamma / dbeta. What the kernel costs at
// M = 3840, C = 768 (tools/probe_ln.py): 11 us without the parameter gradients, 13 with them, 20 with the recomputed input dropout mask and
// 27 with the masked second output as well — the Philox calls, not the atomics, are the expensive part, so the grid keeps one row or two
// per wave (256 workgroups of 8 waves) rather than trading waves for fewer adders.
template <typename T, int NCH, int NW>
__global__ __launch_bounds__(NW * 64) void layernorm_bwd_kernel(const T* dy, const T* x, const float* stats, const float* gamma, T* dx, T* dx_masked,
                                                                float* dgamma, float* dbeta, float* dcolsum, int M, int C, Drop drop_in, Drop drop_out) {
  seed_resolve(drop_in.seed, drop_in.site);
  seed_resolve(drop_out.seed, drop_out.site);
  __shared__ float red[NW][64 * NCH * 8];   // [wave][per-lane partials], used once for dgamma and once for dbeta
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nchunk = C / 8;
  const float invC = 1.0f / (float)C;
  float ag[NCH][8], ab[NCH][8], ax[NCH][8];      // ax: column sums of the stored gradient = bias gradient of the Linear that fed this LayerNorm
#pragma unroll
  for (int i = 0; i < NCH; ++i) { zero8(ag[i]); zero8(ab[i]); zero8(ax[i]); }
  for (int row = blockIdx.x * NW + wave; row < M; row += gridDim.x * NW) {
    float mean = stats[row * 2], rstd = stats[row * 2 + 1];
    float d[NCH][8], xh[NCH][8];          // g = d*gamma is re-formed in the second loop (gamma is L1-resident): 8*NCH fewer live registers
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      int c = lane + 64 * i;
      if (c < nchunk) {
        size_t idx = (size_t)row * C + c * 8;
        load8(dy + idx, d[i]);
        if (drop_in.p > 0.f) apply_dropout8(drop_in, idx, d[i]);
        float xv[8], gm[8];
        load8(x + idx, xv);
        load8(gamma + c * 8, gm);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          xh[i][e] = (xv[e] - mean) * rstd;
          const float ge = d[i][e] * gm[e];
          s1 += ge;
          s2 += ge * xh[i][e];
          ag[i][e] += d[i][e] * xh[i][e];
          ab[i][e] += d[i][e];
        }
      }
    }
    float m1 = wave_sum(s1) * invC, m2 = wave_sum(s2) * invC;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      int c = lane + 64 * i;
      if (c < nchunk) {
        size_t idx = (size_t)row * C + c * 8;
        float o[8], gm[8];
        load8(gamma + c * 8, gm);
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = rstd * (d[i][e] * gm[e] - m1 - xh[i][e] * m2);
        store8(dx + idx, o);
        if (dx_masked) {
          if (drop_out.p > 0.f) apply_dropout8(drop_out, idx, o);
          store8(dx_masked + idx, o);
        }
        if (dcolsum) {      // sums of what the consumer reads: the masked tensor when there is one, rounded to the storage type
          if (sizeof(T) == 2) round8_bf16(o);
#pragma unroll
          for (int e = 0; e < 8; ++e) ax[i][e] += o[e];
        }
      }
    }
  }
  // fold the 4 waves' partial dgamma/dbeta through LDS (two passes to bound LDS), one atomic per column per block
  for (int which = 0; which < 3; ++which) {
    if (which == 2 && !dcolsum) break;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NCH; ++i)
#pragma unroll
      for (int e = 0; e < 8; ++e) red[wave][(i * 64 + lane) * 8 + e] = which == 0 ? ag[i][e] : which == 1 ? ab[i][e] : ax[i][e];
    __syncthreads();
    float* dst = which == 0 ? dgamma : which == 1 ? dbeta : dcolsum;
    if (dst) {
      for (int j = threadIdx.x; j < NCH * 64 * 8; j += NW * 64) {
        int i = j / 512, l = (j / 8) % 64, e = j % 8;
        int c = l + 64 * i;
        float sacc = 0.f;
#pragma unroll
        for (int w = 0; w < NW; ++w) sacc += red[w][j];
        if (c < nchunk) atomic_add_f32(dst + c * 8 + e, sacc);
      }
    }
  }
}

// s0[row] = word[ids[row]] + pos[row % L] + type[0]
template <typename T>
__global__ __launch_bounds__(256) void embed_fwd_kernel(const int64_t* ids, const T* word, const T* pos, const T* type, T* out, int M, int L, int C, int vocab) {
  const int nchunk = C / 8;
  size_t total = (size_t)M * nchunk;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    int c = (int)(i % nchunk);
    int row = (int)(i / nchunk);
    int64_t id = ids[row];
    if (id < 0) id = 0;
    if (id >= vocab) id = vocab - 1;
    float a[8], b[8], t[8];
    load8(word + (size_t)id * C + c * 8, a);
    load8(pos + (size_t)(row % L) * C + c * 8, b);
    load8(type + c * 8, t);
#pragma unroll
    for (int e = 0; e < 8; ++e) a[e] += b[e] + t[e];
    store8(out + (size_t)row * C + c * 8, a);
  }
}

// dword[ids[row]] += d[row] for ids[row] != padding_idx (nn.Embedding(padding_idx) semantics), dpos[l] += sum_b d[b*L + l].
// Workgroup = (position l, batch segment): a thread owns one 8-column chunk and walks the segment's captions at that position, so
// (a) the position sum is a register accumulation, and (b) consecutive rows with the SAME token id — [CLS] at position 0 and [SEP] at the
// last position of every caption — are summed in registers and leave as one atomic set per run instead of one per caption. (A kernel
// with one atomic per row spent 100 us here: thousands of adders on the [CLS] / [SEP] rows serialise at the memory side.)
constexpr int EMB_SEGS = 4, EMB_COLS = 16;      // C <= 128 * EMB_COLS
DEV float ld1(const bf16* p) { return bf2f(*p); }
DEV float ld1(const float* p) { return *p; }
// MP (MPNet): the position row of a token is pids[row] (embed_mpnet_fwd_kernel) instead of l, so the position sums are run-merged like the word
// sums — captions padded at the tail share pid = l + 2 at position l — and rows with pid == pos_pad add nothing (nn.Embedding(padding_idx)).
// The operands come as a trailing argument that is empty for the BERT instantiation, whose code is therefore what it was without the variant.
template <bool MP> struct EmbMp {};
template <> struct EmbMp<true> { const int32_t* pids; int max_pos, pos_pad; };
template <typename T, bool MP = false>
__global__ __launch_bounds__(128) void embed_bwd_kernel(const int64_t* __restrict__ ids, const T* __restrict__ d, float* __restrict__ dword, float* __restrict__ dpos,
                                                        int B, int L, int C, int vocab, int padding_idx, EmbMp<MP> mp) {
  // (position, segment) pairs are walked grid-stride: normally one per workgroup; the deterministic-reduction mode (det.h) launches a single
  // workgroup, whose threads own disjoint columns and add in program order
  for (int blk = blockIdx.x; blk < L * EMB_SEGS; blk += gridDim.x) {
  const int l = blk / EMB_SEGS, seg = blk % EMB_SEGS;
  const int per = (B + EMB_SEGS - 1) / EMB_SEGS;
  const int b0 = seg * per, b1 = b0 + per < B ? b0 + per : B;
  const int t = threadIdx.x;
  // lane t owns columns t, t + 128, ...: a wave's float atomics then cover 256 contiguous bytes (the full-rate shape), and its 2-byte loads
  // 128 contiguous bytes (the rows are small: 6 MB in all)
  float pacc[EMB_COLS], wacc[EMB_COLS];
#pragma unroll
  for (int j = 0; j < EMB_COLS; ++j) { pacc[j] = 0.f; wacc[j] = 0.f; }
  int64_t cur = -1;
  auto flush = [&]() {
    if (dword && cur >= 0 && cur != padding_idx) {
#pragma unroll
      for (int j = 0; j < EMB_COLS; ++j)
        if (t + 128 * j < C) atomic_add_f32(dword + (size_t)cur * C + t + 128 * j, wacc[j]);
    }
#pragma unroll
    for (int j = 0; j < EMB_COLS; ++j) wacc[j] = 0.f;
  };
  int pcur = -1;
  auto pflush = [&]() {
    if constexpr (MP) {
      if (dpos && pcur >= 0 && pcur != mp.pos_pad) {
#pragma unroll
        for (int j = 0; j < EMB_COLS; ++j)
          if (t + 128 * j < C) atomic_add_f32(dpos + (size_t)pcur * C + t + 128 * j, pacc[j]);
      }
#pragma unroll
      for (int j = 0; j < EMB_COLS; ++j) pacc[j] = 0.f;
    }
  };
  // the next caption's row is fetched before this one's atomics are issued (the loop is otherwise one load latency per caption)
  float v[EMB_COLS], vn[EMB_COLS];
  int64_t id = 0, idn = 0;
  int pid = 0, pidn = 0;
  auto fetch = [&](int b, float (&dst)[EMB_COLS], int64_t& di, int& dp) {
    const size_t row = (size_t)b * L + l;
    di = ids[row];
    if constexpr (MP) dp = mp.pids[row];
#pragma unroll
    for (int j = 0; j < EMB_COLS; ++j) dst[j] = t + 128 * j < C ? ld1(d + row * C + t + 128 * j) : 0.f;
  };
  if (b0 < b1) fetch(b0, vn, idn, pidn);
  for (int b = b0; b < b1; ++b) {
    id = idn;
    pid = pidn;
#pragma unroll
    for (int j = 0; j < EMB_COLS; ++j) v[j] = vn[j];
    if (b + 1 < b1) fetch(b + 1, vn, idn, pidn);
    if (id < 0) id = 0;
    if (id >= vocab) id = vocab - 1;
    if (id != cur) { flush(); cur = id; }
    if constexpr (MP) {
      if (pid < 0) pid = 0;
      if (pid >= mp.max_pos) pid = mp.max_pos - 1;
      if (pid != pcur) { pflush(); pcur = pid; }
    }
#pragma unroll
    for (int j = 0; j < EMB_COLS; ++j) { pacc[j] += v[j]; wacc[j] += v[j]; }
  }
  flush();
  if constexpr (MP) {
    pflush();
  } else {
    if (dpos && b1 > b0) {
#pragma unroll
      for (int j = 0; j < EMB_COLS; ++j)
        if (t + 128 * j < C) atomic_add_f32(dpos + (size_t)l * C + t + 128 * j, pacc[j]);
    }
  }
  }
}

// MPNet embeddings: out[row] = word[ids[row]] + pos[pid], pid = pad + (ids[row] != pad ? #{l' <= l : ids[b][l'] != pad} : 0)
// (transformers create_position_ids_from_input_ids; no token types). One wave per row: lane l' < L holds the caption's l'-th id, an inclusive
// prefix count over the lanes gives every row's pid without a host pass. pids (int32 [M]) is kept for the backward.
template <typename T>
__global__ __launch_bounds__(256) void embed_mpnet_fwd_kernel(const int64_t* ids, const T* word, const T* pos, T* out, int32_t* pids, int M, int L, int C,
                                                              int vocab, int max_pos, int pad) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nchunk = C / 8;
  for (int row = blockIdx.x * 4 + wave; row < M; row += gridDim.x * 4) {      // (wave-uniform: the shuffles below are wave-wide)
    const int b = row / L, l = row % L;
    const bool real = lane < L && ids[(size_t)b * L + lane] != pad;
    const float flag = real ? 1.f : 0.f;
    float cnt = flag;
    for (int off = 1; off < 32; off <<= 1) {      // L <= 32
      float up = wave_shfl(cnt, (lane - off) & 63);
      if (lane >= off) cnt += up;
    }
    const float mine = wave_shfl(cnt, l), mreal = wave_shfl(flag, l);
    int pid = pad + (mreal != 0.f ? (int)mine : 0);
    if (pid < 0) pid = 0;
    if (pid >= max_pos) pid = max_pos - 1;
    int64_t id = ids[row];
    if (id < 0) id = 0;
    if (id >= vocab) id = vocab - 1;
    if (lane == 0 && pids) pids[row] = pid;
    for (int c = lane; c < nchunk; c += 64) {
      float a[8], p[8];
      load8(word + (size_t)id * C + c * 8, a);
      load8(pos + (size_t)pid * C + c * 8, p);
#pragma unroll
      for (int e = 0; e < 8; ++e) a[e] += p[e];
      store8(out + (size_t)row * C + c * 8, a);
    }
  }
}

// Masked mean over the tokens (sentence-transformers mean pooling): out[b] = sum_l h[b][l] * mask[b][l] / max(sum_l mask[b][l], 1e-9);
// inv[b] = 1 / that denominator, for the backward. A caption whose mask is all zero gives 0.
template <typename T>
__global__ __launch_bounds__(256) void mean_pool_fwd_kernel(const T* h, const int64_t* mask, T* out, float* inv, int B, int L, int C) {
  const int nchunk = C / 8;
  const size_t total = (size_t)B * nchunk;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int c = (int)(i % nchunk), b = (int)(i / nchunk);
    float acc[8], cnt = 0.f;
    zero8(acc);
    for (int l = 0; l < L; ++l) {
      const float m = (float)mask[(size_t)b * L + l];
      cnt += m;
      if (m != 0.f) {
        float v[8];
        load8(h + ((size_t)b * L + l) * C + c * 8, v);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] += v[e] * m;
      }
    }
    const float den = fmaxf(cnt, 1e-9f);
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] /= den;
    store8(out + (size_t)b * C + c * 8, acc);
    if (c == 0) inv[b] = 1.0f / den;
  }
}
// dh[b][l] = mask[b][l] * inv[b] * dy[b], for every token
template <typename T>
__global__ __launch_bounds__(256) void mean_pool_bwd_kernel(const T* dy, const int64_t* mask, const float* inv, T* dh, int B, int L, int C) {
  const int nchunk = C / 8;
  const size_t total = (size_t)B * L * nchunk;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int c = (int)(i % nchunk);
    const size_t row = i / nchunk;
    const int b = (int)(row / L);
    const float s = (float)mask[row] * inv[b];
    float v[8];
    load8(dy + (size_t)b * C + c * 8, v);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] *= s;
    store8(dh + row * C + c * 8, v);
  }
}

// ------------------------------------------------------------------------------------------------ attention, L <= 32
// One wave per (batch, head). qkv: [B*L][3*H*64] (q | k | v, head h at columns h*64..). ctx: [B*L][H*64].
constexpr int AT_L = 32, AT_D = 64, AT_PQ = AT_D + 1, AT_PP = AT_L + 1;
#define AT_NEG (-3.4028234663852886e38f)

struct AttnSmem {
  float q[AT_L * AT_PQ], k[AT_L * AT_PQ], v[AT_L * AT_PQ], p[AT_L * AT_PP];
  float m[AT_L * AT_PP];   // dropout multiplier of p[i][j]: 0 or 1/(1-p)
};

// m[i][j] for one (batch, head): element index ((bh*32 + i)*32 + j); each lane draws 4 consecutive j per Philox call
DEV void attn_dropmask(AttnSmem& sm, const Drop& drop, int bh, int lane) {
  const float ks = drop.p > 0.f ? 1.0f / (1.0f - drop.p) : 1.f;
  for (int q4 = lane; q4 < AT_L * AT_L / 4; q4 += 64) {
    int i = q4 >> 3, j0 = (q4 & 7) * 4;
    float u[4] = {1.f, 1.f, 1.f, 1.f};
    if (drop.p > 0.f) rng_uniform4(drop.seed, drop.site, ((size_t)bh * AT_L + i) * AT_L + j0, u);
#pragma unroll
    for (int e = 0; e < 4; ++e) sm.m[i * AT_PP + j0 + e] = u[e] >= drop.p ? ks : 0.f;
  }
}

template <typename T>
DEV void attn_load_rows(const T* base, size_t row_stride, int L, float* dst, int lane) {
  // L rows x 64 values; 8 lanes per row, 8 rows per pass
  for (int r0 = 0; r0 < AT_L; r0 += 8) {
    int r = r0 + (lane >> 3), c = (lane & 7) * 8;
    float v[8];
    if (r < L) load8(base + (size_t)r * row_stride + c, v); else zero8(v);
#pragma unroll
    for (int e = 0; e < 8; ++e) dst[r * AT_PQ + c + e] = v[e];
  }
}

// scores + softmax for all rows: p[i][j] (un-dropped probabilities), i,j < 32 (rows/cols >= L are zero)
// BIAS (MPNet): bias_h = this head's [32][32] additive bias (relative_attention_bias), added after the 1/8 scale and before the mask
template <bool BIAS>
DEV void attn_probs(AttnSmem& sm, const int64_t* mask_row, int L, int lane, const float* bias_h) {
  const int j = lane & 31, half = lane >> 5;
  const bool jvalid = j < L;
  float madd = 0.f;
  if (jvalid && mask_row) madd = mask_row[j] != 0 ? 0.f : AT_NEG;
  for (int i0 = 0; i0 < AT_L; i0 += 2) {
    int i = i0 + half;
    float s = 0.f;
#pragma unroll 16
    for (int d = 0; d < AT_D; ++d) s += sm.q[i * AT_PQ + d] * sm.k[j * AT_PQ + d];
    if constexpr (BIAS) s = (s * 0.125f + bias_h[i * AT_L + j]) + madd;
    else s = s * 0.125f + madd;
    if (!jvalid) s = -INFINITY;
    float mx = s;
#pragma unroll
    for (int m = 16; m >= 1; m >>= 1) mx = fmaxf(mx, wave_shfl_xor(mx, m));
    float e = jvalid ? __expf(s - mx) : 0.f;
    float den = e;
#pragma unroll
    for (int m = 16; m >= 1; m >>= 1) den += wave_shfl_xor(den, m);
    sm.p[i * AT_PP + j] = (i < L) ? e / den : 0.f;
  }
}

// The bias operands of the MPNet instantiations (bias [H][32][32]; backward: the 63-entry bucket table and the partials [B*H][32]) come as a
// trailing argument that is empty without BIAS, so the BERT instantiations are compiled from the text they always were.
template <bool BIAS> struct AttnBias {};
template <> struct AttnBias<true> { const float* bias; const int32_t* btab; float* partials; };
template <bool BIAS> DEV const float* attn_bias_head(const AttnBias<BIAS>& ab, int h) {
  if constexpr (BIAS) return ab.bias + (size_t)h * AT_L * AT_L; else return nullptr;
}

template <typename T, bool BIAS = false>
__global__ __launch_bounds__(64) void attention_fwd_kernel(const T* qkv, const int64_t* mask, T* ctx, int B, int L, int H, Drop drop, AttnBias<BIAS> ab) {
  seed_resolve(drop.seed, drop.site);
  __shared__ AttnSmem sm;
  const int lane = threadIdx.x;
  const int b = blockIdx.x / H, h = blockIdx.x % H;
  const size_t ld = (size_t)3 * H * AT_D;
  const T* base = qkv + (size_t)b * L * ld + h * AT_D;
  attn_load_rows(base, ld, L, sm.q, lane);
  attn_load_rows(base + H * AT_D, ld, L, sm.k, lane);
  attn_load_rows(base + 2 * H * AT_D, ld, L, sm.v, lane);
  __syncthreads();
  attn_probs<BIAS>(sm, mask ? mask + (size_t)b * L : nullptr, L, lane, attn_bias_head(ab, h));
  attn_dropmask(sm, drop, b * H + h, lane);
  __syncthreads();
  for (int i = 0; i < L; ++i) {
    float o = 0.f;
    for (int j = 0; j < L; ++j) o += sm.p[i * AT_PP + j] * sm.m[i * AT_PP + j] * sm.v[j * AT_PQ + lane];
    size_t oi = ((size_t)b * L + i) * ((size_t)H * AT_D) + h * AT_D + lane;
    if constexpr (sizeof(T) == 2) ctx[oi] = f2bf(o); else ctx[oi] = o;
  }
}
struct AttnBwdSmem {
  AttnSmem f;
  float dO[AT_L * AT_PQ], dS[AT_L * AT_PP];
};

// Gradient of the relative-position bias, first stage: the 32 bucket sums of one (batch, head)'s f32 dS tile (LDS, [32][pitch]). Lane d < 63 sums
// the diagonal j - i = d - 31 over i, j < L from the top down; lane k < 32 then adds the diagonals whose bucket (btab[d], the 63-entry table of
// relative offsets -31 .. 31) is k, in ascending offset order. No atomics and a fixed order: the same bits on every run. out = NULL: no store.
DEV void attn_bucket_sums(const float* dS, int pitch, int L, const int32_t* btab, float* out, int lane) {
  const int off = lane - 31;
  float diag = 0.f;
  if (lane < 63) {
    const int i0 = off < 0 ? -off : 0, i1 = off > 0 ? L - off : L;      // i in [i0, i1) <=> 0 <= i + off < L
    for (int i = i0; i < i1; ++i) diag += dS[i * pitch + i + off];
  }
  float acc = 0.f;
  for (int d = 0; d < 63; ++d) {
    const float v = wave_shfl(diag, d);
    if (btab[d] == lane) acc += v;
  }
  if (lane < 32 && out) out[lane] = acc;
}

template <typename T, bool BIAS = false>
__global__ __launch_bounds__(64) void attention_bwd_kernel(const T* qkv, const int64_t* mask, const T* dctx, T* dqkv, int B, int L, int H, Drop drop,
                                                           AttnBias<BIAS> ab) {
  seed_resolve(drop.seed, drop.site);
  __shared__ AttnBwdSmem sm;
  const int lane = threadIdx.x;
  const int b = blockIdx.x / H, h = blockIdx.x % H;
  const size_t ld = (size_t)3 * H * AT_D;
  const T* base = qkv + (size_t)b * L * ld + h * AT_D;
  attn_load_rows(base, ld, L, sm.f.q, lane);
  attn_load_rows(base + H * AT_D, ld, L, sm.f.k, lane);
  attn_load_rows(base + 2 * H * AT_D, ld, L, sm.f.v, lane);
  attn_load_rows(dctx + (size_t)b * L * ((size_t)H * AT_D) + h * AT_D, (size_t)H * AT_D, L, sm.dO, lane);
  __syncthreads();
  attn_probs<BIAS>(sm.f, mask ? mask + (size_t)b * L : nullptr, L, lane, attn_bias_head(ab, h));
  attn_dropmask(sm.f, drop, b * H + h, lane);
  __syncthreads();
  const int j = lane & 31, half = lane >> 5;
  // dP[i][j] = keep[i][j]*ks * sum_d dO[i][d] V[j][d];  dS = P * (dP - sum_j dP*P)
  for (int i0 = 0; i0 < AT_L; i0 += 2) {
    int i = i0 + half;
    float dp = 0.f;
#pragma unroll 16
    for (int d = 0; d < AT_D; ++d) dp += sm.dO[i * AT_PQ + d] * sm.f.v[j * AT_PQ + d];
    dp *= sm.f.m[i * AT_PP + j];
    float pij = sm.f.p[i * AT_PP + j];
    float t = dp * pij;
#pragma unroll
    for (int m = 16; m >= 1; m >>= 1) t += wave_shfl_xor(t, m);
    sm.dS[i * AT_PP + j] = pij * (dp - t);
  }
  __syncthreads();
  if constexpr (BIAS) attn_bucket_sums(sm.dS, AT_PP, L, ab.btab, ab.partials + (size_t)blockIdx.x * AT_L, lane);      // d bias = dS
  // lane = d.  dV[j][d] = sum_i Pd[i][j] dO[i][d];  dK[j][d] = sum_i dS[i][j] Q[i][d] / 8;  dQ[i][d] = sum_j dS[i][j] K[j][d] / 8
  T* obase = dqkv + (size_t)b * L * ld + h * AT_D;
  for (int r = 0; r < L; ++r) {
    float dq = 0.f, dk = 0.f, dv = 0.f;
    for (int t = 0; t < L; ++t) {
      dq += sm.dS[r * AT_PP + t] * sm.f.k[t * AT_PQ + lane];
      dk += sm.dS[t * AT_PP + r] * sm.f.q[t * AT_PQ + lane];
      dv += sm.f.p[t * AT_PP + r] * sm.f.m[t * AT_PP + r] * sm.dO[t * AT_PQ + lane];
    }
    dq *= 0.125f; dk *= 0.125f;
    T* o = obase + (size_t)r * ld + lane;
    if constexpr (sizeof(T) == 2) { o[0] = f2bf(dq); o[H * AT_D] = f2bf(dk); o[2 * H * AT_D] = f2bf(dv); }
    else { o[0] = dq; o[H * AT_D] = dk; o[2 * H * AT_D] = dv; }
  }
}
// ------------------------------------------------------------------------------------------------ attention on MFMA (bf16)
// Same math as the VALU kernels above, on v_mfma_f32_32x32x16_bf16: one wave per (batch, head), the whole 32x32 score tile in
// one accumulator. Forward keeps the KEY index in registers (S^T = K Q^T), so the softmax row reduction is over registers plus
// one cross-half shuffle and the probabilities are directly the B operand of O^T = V^T P^T (accumulator-as-operand with its
// permuted k order; V^T fragments come from ds_read_b64_tr_b16 with the same permutation). Backward keeps the key on the LANE
// (S = Q K^T, dP = dO V^T), so P and dS are directly the B operands of dV^T = dO^T P and dK^T = Q^T dS; only dS crosses LDS once
// (transposed) for dQ^T = K^T dS^T. Dropout masks use the same (seed, site, index) convention as the VALU kernels.
constexpr int AM_PI = 192;   // [32][64] bf16 image pitch (128 B row + 64 B pad)
constexpr int AM_PT = 80;    // [32][32] bf16 image pitch

struct AmFwdSmem { char v[32 * AM_PI]; float madd[32]; };
struct AmBwdSmem { char q[32 * AM_PI], k[32 * AM_PI], d[32 * AM_PI], t[32 * AM_PT]; float m[32 * 33]; float madd[32]; };

DEV void am_load_image(const bf16* base, size_t ld, int L, char* img, int lane) {
  for (int c = lane; c < 256; c += 64) {
    int r = c >> 3, ch = c & 7;
    u32x4 v = {0u, 0u, 0u, 0u};
    if (r < L) v = *(const u32x4*)(base + (size_t)r * ld + ch * 8);
    *(u32x4*)(img + r * AM_PI + ch * 16) = v;
  }
}
// row-major fragment straight from global memory: rows x = lane&31 (zero beyond L), k = 16*ks + 8*(lane>>5) + e
DEV bf16x8 am_frag_rows(const bf16* base, size_t ld, int L, int ks, int lane) {
  Chunk16 c;
  c.u = u32x4{0u, 0u, 0u, 0u};
  int r = lane & 31;
  if (r < L) c.u = *(const u32x4*)(base + (size_t)r * ld + ks * 16 + 8 * (lane >> 5));
  return c.h;
}
// transposed fragment from a [k][x] image, natural k order: k = 16*s + 8*(lane>>5) + e
template <int PITCH> DEV bf16x8 am_frag_tr(const char* img, int x0, int s, int lane) {
  int x = x0 + 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
  int k = 16 * s + 8 * (lane >> 5) + ((lane >> 2) & 3);
  const char* p = img + k * PITCH + x * 2;
  union { s16x4 v[2]; bf16x8 h; } u;
  u.v[0] = lds_read_tr16(p);
  u.v[1] = lds_read_tr16(p + 4 * PITCH);
  return u.h;
}
// transposed fragment in the k order of an accumulator used as the other operand: element e of lane-half h <-> k = 16s + 8(e>>2) + 4h + (e&3)
template <int PITCH> DEV bf16x8 am_frag_tr_acc(const char* img, int x0, int s, int lane) {
  int x = x0 + 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
  int k = 16 * s + 4 * (lane >> 5) + ((lane >> 2) & 3);
  const char* p = img + k * PITCH + x * 2;
  union { s16x4 v[2]; bf16x8 h; } u;
  u.v[0] = lds_read_tr16(p);
  u.v[1] = lds_read_tr16(p + 8 * PITCH);
  return u.h;
}
DEV bf16x8 am_acc_frag(const f32x16& a, int s) {
  bf16x8 f;
#pragma unroll
  for (int e = 0; e < 8; ++e) f[e] = f2bf(a[8 * s + e]);
  return f;
}
DEV int am_row(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }
// store an accumulator whose rows are d (32 per block) and whose column is a token (lane&31): 4 consecutive d per register group
DEV void am_store_T(bf16* base, size_t ld, int L, int d0, const f32x16& a, float scale, int lane) {
  int tok = lane & 31;
  if (tok >= L) return;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    union { bf16 e[4]; u32x2 u; } pk;
#pragma unroll
    for (int e = 0; e < 4; ++e) pk.e[e] = f2bf(a[4 * g + e] * scale);
    *(u32x2*)(base + (size_t)tok * ld + d0 + 8 * g + 4 * (lane >> 5)) = pk.u;
  }
}

template <bool BIAS = false>
__global__ __launch_bounds__(256) void attention_mfma_fwd_kernel(const bf16* qkv, const int64_t* mask, bf16* ctx, int B, int L, int H, Drop drop, AttnBias<BIAS> ab) {
  seed_resolve(drop.seed, drop.site);
  __shared__ __attribute__((aligned(16))) AmFwdSmem sm[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int bh = blockIdx.x * 4 + wave;
  const bool live = bh < B * H;
  if (!live) bh = B * H - 1;
  const int b = bh / H, h = bh % H;
  const size_t ld = (size_t)3 * H * 64;
  const bf16* qb = qkv + (size_t)b * L * ld + h * 64;
  AmFwdSmem& S = sm[wave];
  am_load_image(qb + 2 * H * 64, ld, L, S.v, lane);
  if (lane < 32) S.madd[lane] = (lane < L) ? ((mask && mask[(size_t)b * L + lane] == 0) ? AT_NEG : 0.f) : -INFINITY;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
  for (int ks = 0; ks < 4; ++ks)      // S^T[j][i] = sum_d K[j][d] Q[i][d]
    acc = mfma32_bf16(am_frag_rows(qb + H * 64, ld, L, ks, lane), am_frag_rows(qb, ld, L, ks, lane), acc);
  __syncthreads();
  // softmax over j (registers x the two lane halves) for the query i = lane&31
  float mx = -INFINITY;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    // (BIAS: key j = am_row(r, lane) runs over 4 consecutive floats per register group, query i = lane&31)
    if constexpr (BIAS) acc[r] = (acc[r] * 0.125f + ab.bias[((size_t)h * AT_L + (lane & 31)) * AT_L + am_row(r, lane)]) + S.madd[am_row(r, lane)];
    else acc[r] = acc[r] * 0.125f + S.madd[am_row(r, lane)];
    mx = fmaxf(mx, acc[r]);
  }
  mx = fmaxf(mx, wave_shfl_xor(mx, 32));
  float den = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) { acc[r] = __expf(acc[r] - mx); den += acc[r]; }
  den += wave_shfl_xor(den, 32);
  const float inv = 1.0f / den;
  const int i = lane & 31;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    float u[4] = {1.f, 1.f, 1.f, 1.f};
    if (drop.p > 0.f) rng_uniform4(drop.seed, drop.site, ((size_t)bh * AT_L + i) * AT_L + 8 * g + 4 * (lane >> 5), u);
    const float ks = drop.p > 0.f ? 1.0f / (1.0f - drop.p) : 1.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[4 * g + e] *= inv * (u[e] >= drop.p ? ks : 0.f);
  }
  // O^T[d][i] = sum_j V^T[d][j] P^T[j][i]
#pragma unroll
  for (int db = 0; db < 2; ++db) {
    f32x16 o;
#pragma unroll
    for (int r = 0; r < 16; ++r) o[r] = 0.f;
#pragma unroll
    for (int s = 0; s < 2; ++s) o = mfma32_bf16(am_frag_tr_acc<AM_PI>(S.v, db * 32, s, lane), am_acc_frag(acc, s), o);
    if (live) am_store_T(ctx + (size_t)b * L * ((size_t)H * 64) + h * 64, (size_t)H * 64, L, db * 32, o, 1.f, lane);
  }
}
template <bool BIAS = false>
__global__ __launch_bounds__(128) void attention_mfma_bwd_kernel(const bf16* qkv, const int64_t* mask, const bf16* dctx, bf16* dqkv, int B, int L, int H, Drop drop,
                                                                 AttnBias<BIAS> ab) {
  seed_resolve(drop.seed, drop.site);
  __shared__ __attribute__((aligned(16))) AmBwdSmem sm[2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int bh = blockIdx.x * 2 + wave;
  const bool live = bh < B * H;
  if (!live) bh = B * H - 1;
  const int b = bh / H, h = bh % H;
  const size_t ld = (size_t)3 * H * 64, ldc = (size_t)H * 64;
  const bf16* qb = qkv + (size_t)b * L * ld + h * 64;
  const bf16* dob = dctx + (size_t)b * L * ldc + h * 64;
  AmBwdSmem& S = sm[wave];
  am_load_image(qb, ld, L, S.q, lane);
  am_load_image(qb + H * 64, ld, L, S.k, lane);
  am_load_image(dob, ldc, L, S.d, lane);
  if (lane < 32) S.madd[lane] = (lane < L) ? ((mask && mask[(size_t)b * L + lane] == 0) ? AT_NEG : 0.f) : -INFINITY;
  {   // dropout multipliers m[i][j]
    const float ks = drop.p > 0.f ? 1.0f / (1.0f - drop.p) : 1.f;
    for (int q4 = lane; q4 < 256; q4 += 64) {
      int i = q4 >> 3, j0 = (q4 & 7) * 4;
      float u[4] = {1.f, 1.f, 1.f, 1.f};
      if (drop.p > 0.f) rng_uniform4(drop.seed, drop.site, ((size_t)bh * AT_L + i) * AT_L + j0, u);
#pragma unroll
      for (int e = 0; e < 4; ++e) S.m[i * 33 + j0 + e] = u[e] >= drop.p ? ks : 0.f;
    }
  }
  f32x16 p, dp;
#pragma unroll
  for (int r = 0; r < 16; ++r) { p[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    p = mfma32_bf16(am_frag_rows(qb, ld, L, ks, lane), am_frag_rows(qb + H * 64, ld, L, ks, lane), p);            // S[i][j]
    dp = mfma32_bf16(am_frag_rows(dob, ldc, L, ks, lane), am_frag_rows(qb + 2 * H * 64, ld, L, ks, lane), dp);    // dP[i][j] = dO V^T
  }
  __syncthreads();
  const int j = lane & 31;
  const float madd = S.madd[j];
  f32x16 pd, ds;
#pragma unroll
  for (int r = 0; r < 16; ++r) {      // softmax over j = across the 32 lanes of a half, per register row i
    float s;
    if constexpr (BIAS) s = (p[r] * 0.125f + ab.bias[((size_t)h * AT_L + am_row(r, lane)) * AT_L + j]) + madd;
    else s = p[r] * 0.125f + madd;
    float mx = s;
#pragma unroll
    for (int m = 16; m >= 1; m >>= 1) mx = fmaxf(mx, wave_shfl_xor(mx, m));
    float e = __expf(s - mx);
    float den = e;
#pragma unroll
    for (int m = 16; m >= 1; m >>= 1) den += wave_shfl_xor(den, m);
    int i = am_row(r, lane);
    float pr = (i < L) ? e / den : 0.f;
    float mul = S.m[i * 33 + j];
    float dpd = dp[r] * mul;
    float t = dpd * pr;
#pragma unroll
    for (int m = 16; m >= 1; m >>= 1) t += wave_shfl_xor(t, m);
    p[r] = pr;
    pd[r] = pr * mul;
    ds[r] = pr * (dpd - t);
  }
  if constexpr (BIAS) {
    // the f32 dS tile, before it is rounded to bf16 for the three products, over the dropout multipliers: every lane overwrites exactly the
    // elements it read above, so no barrier is needed in front of the stores
#pragma unroll
    for (int r = 0; r < 16; ++r) S.m[am_row(r, lane) * 33 + j] = ds[r];
  }
  // dS^T image for dQ: T[j][i] = dS[i][j]
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    union { bf16 e[4]; u32x2 u; } pk;
#pragma unroll
    for (int e = 0; e < 4; ++e) pk.e[e] = f2bf(ds[4 * g + e]);
    *(u32x2*)(S.t + j * AM_PT + (8 * g + 4 * (lane >> 5)) * 2) = pk.u;
  }
  __syncthreads();
  if constexpr (BIAS) attn_bucket_sums(S.m, 33, L, ab.btab, live ? ab.partials + (size_t)bh * AT_L : nullptr, lane);
  bf16* ob = dqkv + (size_t)b * L * ld + h * 64;
#pragma unroll
  for (int db = 0; db < 2; ++db) {
    f32x16 dv, dk, dq;
#pragma unroll
    for (int r = 0; r < 16; ++r) { dv[r] = 0.f; dk[r] = 0.f; dq[r] = 0.f; }
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      dv = mfma32_bf16(am_frag_tr_acc<AM_PI>(S.d, db * 32, s, lane), am_acc_frag(pd, s), dv);      // dV^T[d][j] = sum_i dO^T[d][i] Pd[i][j]
      dk = mfma32_bf16(am_frag_tr_acc<AM_PI>(S.q, db * 32, s, lane), am_acc_frag(ds, s), dk);      // dK^T[d][j] = sum_i Q^T[d][i] dS[i][j]
      dq = mfma32_bf16(am_frag_tr<AM_PI>(S.k, db * 32, s, lane), am_frag_tr<AM_PT>(S.t, 0, s, lane), dq);   // dQ^T[d][i] = sum_j K^T[d][j] dS^T[j][i]
    }
    if (live) {
      am_store_T(ob + 2 * H * 64, ld, L, db * 32, dv, 1.f, lane);
      am_store_T(ob + H * 64, ld, L, db * 32, dk, 0.125f, lane);
      am_store_T(ob, ld, L, db * 32, dq, 0.125f, lane);
    }
  }
}
// bias[h][i][j] = rel[btab[j - i + 31]][h] for i, j < L, 0 elsewhere in the [32][32] tile: MPNet's relative_attention_bias (Embedding(32, H), shared by
// all layers, trained) expanded once per step into the operand of the attention kernels above
__global__ __launch_bounds__(256) void attention_bias_build_kernel(const float* rel, const int32_t* btab, float* bias, int H, int L) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= H * AT_L * AT_L) return;
  const int h = idx / (AT_L * AT_L), i = (idx / AT_L) % AT_L, j = idx % AT_L;
  float v = 0.f;
  if (i < L && j < L) {
    int k = btab[j - i + AT_L - 1];
    k = k < 0 ? 0 : (k > AT_L - 1 ? AT_L - 1 : k);
    v = rel[k * H + h];
  }
  bias[idx] = v;
}
// Second stage of the bias gradient: drel[k][h] += sum_r partials[r][h][k] over the R = (layers x batch) rows the backward kernels wrote. One
// workgroup per head: 32 row slices x 32 buckets, the slices' sums added in slice order by one thread per bucket (no atomics).
__global__ __launch_bounds__(1024) void attention_bias_grad_reduce_kernel(const float* partials, float* drel, int R, int H) {
  __shared__ float red[32][33];
  const int h = blockIdx.x, k = threadIdx.x & 31, part = threadIdx.x >> 5;
  float acc = 0.f;
  for (int r = part; r < R; r += 32) acc += partials[((size_t)r * H + h) * AT_L + k];
  red[part][k] = acc;
  __syncthreads();
  if (threadIdx.x < 32) {
    float t = 0.f;
    for (int q = 0; q < 32; ++q) t += red[q][k];
    drel[k * H + h] += t;
  }
}

// ------------------------------------------------------------------------------------------------ attention, 32 < L <= 128
// The same definition as the 32-token kernels above on up to four key tiles of 32: one workgroup per (batch, head), two-pass softmax over the whole
// score row (no running maximum), probabilities recomputed in backward, no atomics and a fixed summation order. The dropout multiplier of p[i][j]
// is drawn from element index ((bh*128 + i)*128 + j), four consecutive j per Philox call, in both families and both directions. Rows >= L of a
// sample belong to the next sample (or lie past the buffer): every global access is guarded by row < L.
constexpr int AL_L = 128;

DEV float al_dropmult(const Drop& drop, int bh, int i, int j) {
  if (!(drop.p > 0.f)) return 1.f;
  float u[4];
  rng_uniform4(drop.seed, drop.site, ((size_t)bh * AL_L + i) * AL_L + (j & ~3), u);
  const int e = j & 3;
  const float ue = e == 0 ? u[0] : (e == 1 ? u[1] : (e == 2 ? u[2] : u[3]));
  return ue >= drop.p ? 1.0f / (1.0f - drop.p) : 0.f;
}
DEV float al_madd(const int64_t* mask, int b, int L, int j) {
  return (j < L) ? ((mask && mask[(size_t)b * L + j] == 0) ? AT_NEG : 0.f) : -INFINITY;
}

// ---- exact f32 on the VALU: four waves, wave w takes the query rows (forward, dQ) and then the key rows (dK, dV) w, w + 4, ...; the lanes of a
// wave hold the 128 entries of that score row / column two apiece (j = lane, lane + 64) and hand them to the 64 head columns through LDS
struct AlSmem {
  float q[AL_L * AT_PQ], k[AL_L * AT_PQ], v[AL_L * AT_PQ];
  float madd[AL_L];
  float row[4][2][AL_L];      // [wave][iteration parity]: one barrier per iteration is enough
};
struct AlBwdSmem {
  float q[AL_L * AT_PQ], k[AL_L * AT_PQ], v[AL_L * AT_PQ], dO[AL_L * AT_PQ];
  float madd[AL_L], mx[AL_L], den[AL_L], t[AL_L];      // per query row: softmax maximum and denominator, sum_j dP*P
  float vec[4][2][2][AL_L];                            // [wave][iteration parity][dS | dropped P]
};

template <typename T>
DEV void al_load_rows(const T* base, size_t row_stride, int L, float* dst, int tid) {
  for (int idx = tid; idx < AL_L * 8; idx += 256) {
    int r = idx >> 3, c = (idx & 7) * 8;
    float v[8];
    if (r < L) load8(base + (size_t)r * row_stride + c, v); else zero8(v);
#pragma unroll
    for (int e = 0; e < 8; ++e) dst[r * AT_PQ + c + e] = v[e];
  }
}
DEV float al_dot(const float* a, const float* b) {
  float s = 0.f;
#pragma unroll 16
  for (int d = 0; d < AT_D; ++d) s += a[d] * b[d];
  return s;
}
template <typename T> DEV void al_store(T* p, float v) {
  if constexpr (sizeof(T) == 2) *p = f2bf(v); else *p = v;
}

template <typename T>
__global__ __launch_bounds__(256) void attention_long_fwd_kernel(const T* qkv, const int64_t* mask, T* ctx, int B, int L, int H, Drop drop) {
  seed_resolve(drop.seed, drop.site);
  __shared__ AlSmem sm;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int bh = blockIdx.x, b = bh / H, h = bh % H;
  const size_t ld = (size_t)3 * H * AT_D;
  const T* base = qkv + (size_t)b * L * ld + h * AT_D;
  al_load_rows(base, ld, L, sm.q, tid);
  al_load_rows(base + H * AT_D, ld, L, sm.k, tid);
  al_load_rows(base + 2 * H * AT_D, ld, L, sm.v, tid);
  if (tid < AL_L) sm.madd[tid] = al_madd(mask, b, L, tid);
  __syncthreads();
  for (int it = 0; it < (L + 3) / 4; ++it) {
    const int i = it * 4 + wave;
    float* row = sm.row[wave][it & 1];
    if (i < L) {
      const float s0 = al_dot(sm.q + i * AT_PQ, sm.k + lane * AT_PQ) * 0.125f + sm.madd[lane];
      const float s1 = al_dot(sm.q + i * AT_PQ, sm.k + (lane + 64) * AT_PQ) * 0.125f + sm.madd[lane + 64];
      const float mx = wave_max(fmaxf(s0, s1));
      const float e0 = __expf(s0 - mx), e1 = __expf(s1 - mx);      // keys >= L: exp(-inf) = 0
      const float den = wave_sum(e0 + e1);
      row[lane] = e0 / den * al_dropmult(drop, bh, i, lane);
      row[lane + 64] = e1 / den * al_dropmult(drop, bh, i, lane + 64);
    }
    __syncthreads();
    if (i < L) {
      float o = 0.f;
      for (int j = 0; j < L; ++j) o += row[j] * sm.v[j * AT_PQ + lane];
      al_store(ctx + ((size_t)b * L + i) * ((size_t)H * AT_D) + h * AT_D + lane, o);
    }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void attention_long_bwd_kernel(const T* qkv, const int64_t* mask, const T* dctx, T* dqkv, int B, int L, int H, Drop drop) {
  seed_resolve(drop.seed, drop.site);
  __shared__ AlBwdSmem sm;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int bh = blockIdx.x, b = bh / H, h = bh % H;
  const size_t ld = (size_t)3 * H * AT_D;
  const T* base = qkv + (size_t)b * L * ld + h * AT_D;
  al_load_rows(base, ld, L, sm.q, tid);
  al_load_rows(base + H * AT_D, ld, L, sm.k, tid);
  al_load_rows(base + 2 * H * AT_D, ld, L, sm.v, tid);
  al_load_rows(dctx + (size_t)b * L * ((size_t)H * AT_D) + h * AT_D, (size_t)H * AT_D, L, sm.dO, tid);
  if (tid < AL_L) sm.madd[tid] = al_madd(mask, b, L, tid);
  __syncthreads();
  T* obase = dqkv + (size_t)b * L * ld + h * AT_D;
  const int iters = (L + 3) / 4;
  // query rows: P, dP = m * dO V^T, dS = P * (dP - sum_j dP*P) for one row i; dQ[i] = dS[i] K / 8. The row's softmax statistics stay in LDS.
  for (int it = 0; it < iters; ++it) {
    const int i = it * 4 + wave;
    float* ds = sm.vec[wave][it & 1][0];
    if (i < L) {
      const float s0 = al_dot(sm.q + i * AT_PQ, sm.k + lane * AT_PQ) * 0.125f + sm.madd[lane];
      const float s1 = al_dot(sm.q + i * AT_PQ, sm.k + (lane + 64) * AT_PQ) * 0.125f + sm.madd[lane + 64];
      const float mx = wave_max(fmaxf(s0, s1));
      const float e0 = __expf(s0 - mx), e1 = __expf(s1 - mx);
      const float den = wave_sum(e0 + e1);
      const float p0 = e0 / den, p1 = e1 / den;
      const float dp0 = al_dot(sm.dO + i * AT_PQ, sm.v + lane * AT_PQ) * al_dropmult(drop, bh, i, lane);
      const float dp1 = al_dot(sm.dO + i * AT_PQ, sm.v + (lane + 64) * AT_PQ) * al_dropmult(drop, bh, i, lane + 64);
      const float t = wave_sum(dp0 * p0 + dp1 * p1);
      ds[lane] = p0 * (dp0 - t);
      ds[lane + 64] = p1 * (dp1 - t);
      if (lane == 0) { sm.mx[i] = mx; sm.den[i] = den; sm.t[i] = t; }
    }
    __syncthreads();
    if (i < L) {
      float dq = 0.f;
      for (int j = 0; j < L; ++j) dq += ds[j] * sm.k[j * AT_PQ + lane];
      al_store(obase + (size_t)i * ld + lane, dq * 0.125f);
    }
  }
  __syncthreads();
  // key rows: column j of dS and of the dropped P from the saved statistics (lane = query i, i + 64); dK[j] = dS[:, j]^T Q / 8, dV[j] = Pd[:, j]^T dO,
  // summed over the queries in ascending order
  for (int it = 0; it < iters; ++it) {
    const int j = it * 4 + wave;
    float* ds = sm.vec[wave][it & 1][0];
    float* pd = sm.vec[wave][it & 1][1];
    if (j < L) {
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const int i = lane + 64 * half;
        float dsv = 0.f, pdv = 0.f;
        if (i < L) {
          const float s = al_dot(sm.q + i * AT_PQ, sm.k + j * AT_PQ) * 0.125f + sm.madd[j];
          const float p = __expf(s - sm.mx[i]) / sm.den[i];
          const float mul = al_dropmult(drop, bh, i, j);
          const float dp = al_dot(sm.dO + i * AT_PQ, sm.v + j * AT_PQ) * mul;
          dsv = p * (dp - sm.t[i]);
          pdv = p * mul;
        }
        ds[i] = dsv;
        pd[i] = pdv;
      }
    }
    __syncthreads();
    if (j < L) {
      float dk = 0.f, dv = 0.f;
      for (int i = 0; i < L; ++i) {
        dk += ds[i] * sm.q[i * AT_PQ + lane];
        dv += pd[i] * sm.dO[i * AT_PQ + lane];
      }
      al_store(obase + (size_t)j * ld + H * AT_D + lane, dk * 0.125f);
      al_store(obase + (size_t)j * ld + 2 * H * AT_D + lane, dv);
    }
  }
}

// ---- bf16 on v_mfma_f32_32x32x16_bf16: NT = ceil(L / 32) key tiles (2..4), one workgroup of NT waves per (batch, head), wave w owning query tile w.
// Forward is the S^T = K Q^T / O^T = V^T P^T scheme of attention_mfma_fwd_kernel looped over the key tiles: a query's whole score row sits in NT
// accumulators of its lane pair, so the softmax is the same two passes. Backward keeps the key on the lane (S = Q K^T, dP = dO V^T) for the wave's
// query tile against all key tiles, leaves dS^T and the dropped P^T in LDS as bf16 images ([key][query]), and after one barrier wave w forms dK, dV
// of key tile w (B operand: 8 consecutive queries of one key row; summed over the query tiles in ascending order) and dQ of query tile w (B operand:
// the transposing read of the dS^T image).
template <int NT> struct AlmFwdSmem { char v[32 * NT * AM_PI]; float madd[32 * NT]; };
template <int NT> struct AlmBwdSmem {
  static constexpr int PT = 64 * NT + 16;      // [32 NT][32 NT] bf16 image pitch
  char q[32 * NT * AM_PI], k[32 * NT * AM_PI], d[32 * NT * AM_PI], ts[32 * NT * PT], tp[32 * NT * PT];
  unsigned char keep[32 * NT][8 * NT];         // keep bits of p[i][4 c .. 4 c + 3]: one Philox call each
  float madd[32 * NT];
};
template <int NT> DEV void alm_load_image(const bf16* base, size_t ld, int L, char* img, int tid) {
  for (int c = tid; c < 32 * NT * 8; c += 64 * NT) {
    int r = c >> 3, ch = c & 7;
    u32x4 v = {0u, 0u, 0u, 0u};
    if (r < L) v = *(const u32x4*)(base + (size_t)r * ld + ch * 8);
    *(u32x4*)(img + r * AM_PI + ch * 16) = v;
  }
}

template <int NT>
__global__ __launch_bounds__(64 * NT) void attention_long_mfma_fwd_kernel(const bf16* qkv, const int64_t* mask, bf16* ctx, int B, int L, int H, Drop drop) {
  seed_resolve(drop.seed, drop.site);
  __shared__ __attribute__((aligned(16))) AlmFwdSmem<NT> S;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int bh = blockIdx.x, b = bh / H, h = bh % H;
  const size_t ld = (size_t)3 * H * 64, ldc = (size_t)H * 64;
  const bf16* qb = qkv + (size_t)b * L * ld + h * 64;
  alm_load_image<NT>(qb + 2 * H * 64, ld, L, S.v, tid);
  if (tid < 32 * NT) S.madd[tid] = al_madd(mask, b, L, tid);
  const int Lq = L - 32 * wave;      // rows of this wave's query tile inside the sample (> 0: L > 32 (NT - 1))
  bf16x8 qf[4];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) qf[ks] = am_frag_rows(qb + (size_t)32 * wave * ld, ld, Lq, ks, lane);
  f32x16 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {      // S^T[j][i] = sum_d K[j][d] Q[i][d], key tile t
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) acc[t] = mfma32_bf16(am_frag_rows(qb + H * 64 + (size_t)32 * t * ld, ld, L - 32 * t, ks, lane), qf[ks], acc[t]);
  }
  __syncthreads();
  // softmax over j (NT accumulators x the two lane halves) for the query i = 32 wave + (lane & 31)
  float mx = -INFINITY;
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      acc[t][r] = acc[t][r] * 0.125f + S.madd[32 * t + am_row(r, lane)];
      mx = fmaxf(mx, acc[t][r]);
    }
  mx = fmaxf(mx, wave_shfl_xor(mx, 32));
  float den = 0.f;
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc[t][r] = __expf(acc[t][r] - mx); den += acc[t][r]; }
  den += wave_shfl_xor(den, 32);
  const float inv = 1.0f / den;
  const int i = 32 * wave + (lane & 31);
  const float ksc = drop.p > 0.f ? 1.0f / (1.0f - drop.p) : 1.f;
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      float u[4] = {1.f, 1.f, 1.f, 1.f};
      if (drop.p > 0.f) rng_uniform4(drop.seed, drop.site, ((size_t)bh * AL_L + i) * AL_L + 32 * t + 8 * g + 4 * (lane >> 5), u);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[t][4 * g + e] *= inv * (u[e] >= drop.p ? ksc : 0.f);
    }
  // O^T[d][i] = sum_j V^T[d][j] P^T[j][i], key tiles in ascending order
#pragma unroll
  for (int db = 0; db < 2; ++db) {
    f32x16 o;
#pragma unroll
    for (int r = 0; r < 16; ++r) o[r] = 0.f;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int s = 0; s < 2; ++s) o = mfma32_bf16(am_frag_tr_acc<AM_PI>(S.v + 32 * t * AM_PI, db * 32, s, lane), am_acc_frag(acc[t], s), o);
    am_store_T(ctx + ((size_t)b * L + 32 * wave) * ldc + h * 64, ldc, Lq, db * 32, o, 1.f, lane);
  }
}

template <int NT>
__global__ __launch_bounds__(64 * NT) void attention_long_mfma_bwd_kernel(const bf16* qkv, const int64_t* mask, const bf16* dctx, bf16* dqkv, int B, int L, int H,
                                                                           Drop drop) {
  seed_resolve(drop.seed, drop.site);
  constexpr int PT = AlmBwdSmem<NT>::PT;
  __shared__ __attribute__((aligned(16))) AlmBwdSmem<NT> S;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int bh = blockIdx.x, b = bh / H, h = bh % H;
  const size_t ld = (size_t)3 * H * 64, ldc = (size_t)H * 64;
  const bf16* qb = qkv + (size_t)b * L * ld + h * 64;
  const bf16* dob = dctx + (size_t)b * L * ldc + h * 64;
  alm_load_image<NT>(qb, ld, L, S.q, tid);
  alm_load_image<NT>(qb + H * 64, ld, L, S.k, tid);
  alm_load_image<NT>(dob, ldc, L, S.d, tid);
  if (tid < 32 * NT) S.madd[tid] = al_madd(mask, b, L, tid);
  for (int c = lane; c < 32 * 8 * NT; c += 64) {      // keep bits of this wave's 32 query rows
    const int i = 32 * wave + c / (8 * NT), jq = c % (8 * NT);
    float u[4] = {1.f, 1.f, 1.f, 1.f};
    if (drop.p > 0.f) rng_uniform4(drop.seed, drop.site, ((size_t)bh * AL_L + i) * AL_L + 4 * jq, u);
    unsigned bits = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) bits |= (u[e] >= drop.p ? 1u : 0u) << e;
    S.keep[i][jq] = (unsigned char)bits;
  }
  const int Lq = L - 32 * wave;
  bf16x8 qf[4], dof[4];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    qf[ks] = am_frag_rows(qb + (size_t)32 * wave * ld, ld, Lq, ks, lane);
    dof[ks] = am_frag_rows(dob + (size_t)32 * wave * ldc, ldc, Lq, ks, lane);
  }
  f32x16 p[NT], dp[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
#pragma unroll
    for (int r = 0; r < 16; ++r) { p[t][r] = 0.f; dp[t][r] = 0.f; }
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      p[t] = mfma32_bf16(qf[ks], am_frag_rows(qb + H * 64 + (size_t)32 * t * ld, ld, L - 32 * t, ks, lane), p[t]);            // S[i][j]
      dp[t] = mfma32_bf16(dof[ks], am_frag_rows(qb + 2 * H * 64 + (size_t)32 * t * ld, ld, L - 32 * t, ks, lane), dp[t]);     // dP[i][j] = dO V^T
    }
  }
  __syncthreads();
  const int jl = lane & 31;
  const float ksc = drop.p > 0.f ? 1.0f / (1.0f - drop.p) : 1.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {      // softmax over j = across the 32 lanes of a half and the NT tiles, per register row i
    const int il = am_row(r, lane);
    float e[NT], mx = -INFINITY;
#pragma unroll
    for (int t = 0; t < NT; ++t) { e[t] = p[t][r] * 0.125f + S.madd[32 * t + jl]; mx = fmaxf(mx, e[t]); }
#pragma unroll
    for (int m = 16; m >= 1; m >>= 1) mx = fmaxf(mx, wave_shfl_xor(mx, m));
    float den = 0.f;
#pragma unroll
    for (int t = 0; t < NT; ++t) { e[t] = __expf(e[t] - mx); den += e[t]; }
#pragma unroll
    for (int m = 16; m >= 1; m >>= 1) den += wave_shfl_xor(den, m);
    float tt = 0.f;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      e[t] = (il < Lq) ? e[t] / den : 0.f;
      const float mul = ((S.keep[32 * wave + il][8 * t + (jl >> 2)] >> (jl & 3)) & 1) ? ksc : 0.f;
      dp[t][r] *= mul;
      tt += dp[t][r] * e[t];
      p[t][r] = e[t] * mul;      // dropped P
    }
#pragma unroll
    for (int m = 16; m >= 1; m >>= 1) tt += wave_shfl_xor(tt, m);
#pragma unroll
    for (int t = 0; t < NT; ++t) dp[t][r] = e[t] * (dp[t][r] - tt);      // dS
  }
  // the images: ts[j][i] = dS[i][j], tp[j][i] = Pd[i][j] for this wave's 32 queries (4 consecutive i per register group)
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      union { bf16 e[4]; u32x2 u; } ks, kp;
#pragma unroll
      for (int e = 0; e < 4; ++e) { ks.e[e] = f2bf(dp[t][4 * g + e]); kp.e[e] = f2bf(p[t][4 * g + e]); }
      const int off = (32 * t + jl) * PT + (32 * wave + 8 * g + 4 * (lane >> 5)) * 2;
      *(u32x2*)(S.ts + off) = ks.u;
      *(u32x2*)(S.tp + off) = kp.u;
    }
  __syncthreads();
  bf16* ob = dqkv + ((size_t)b * L + 32 * wave) * ld + h * 64;      // key tile `wave` for dK, dV; query tile `wave` for dQ
#pragma unroll
  for (int db = 0; db < 2; ++db) {
    f32x16 dv, dk, dq;
#pragma unroll
    for (int r = 0; r < 16; ++r) { dv[r] = 0.f; dk[r] = 0.f; dq[r] = 0.f; }
#pragma unroll
    for (int s = 0; s < 2 * NT; ++s) {
      Chunk16 bp, bs;
      const int off = (32 * wave + jl) * PT + (16 * s + 8 * (lane >> 5)) * 2;
      bp.u = *(const u32x4*)(S.tp + off);
      bs.u = *(const u32x4*)(S.ts + off);
      dv = mfma32_bf16(am_frag_tr<AM_PI>(S.d, db * 32, s, lane), bp.h, dv);      // dV^T[d][j] = sum_i dO^T[d][i] Pd[i][j]
      dk = mfma32_bf16(am_frag_tr<AM_PI>(S.q, db * 32, s, lane), bs.h, dk);      // dK^T[d][j] = sum_i Q^T[d][i] dS[i][j]
      dq = mfma32_bf16(am_frag_tr<AM_PI>(S.k, db * 32, s, lane), am_frag_tr<PT>(S.ts, 32 * wave, s, lane), dq);   // dQ^T[d][i] = sum_j K^T[d][j] dS^T[j][i]
    }
    am_store_T(ob + 2 * H * 64, ld, Lq, db * 32, dv, 1.f, lane);
    am_store_T(ob + H * 64, ld, Lq, db * 32, dk, 0.125f, lane);
    am_store_T(ob, ld, Lq, db * 32, dq, 0.125f, lane);
  }
}

// ------------------------------------------------------------------------------------------------ causal attention (CLIP text tower), L <= 128
// The four kernel families above with one more condition on a score: query i sees key j iff j <= i (and the key mask allows it). A key behind the
// diagonal is treated as a key beyond L is: its score is -inf, so it takes no part in the softmax and its probability is an exact zero. Key 0 is
// visible to every query (mask[b][0] == 1 is the entry points' precondition), so no row is empty. There is no dropout and no bias. The kernels
// are separate ones: the text of the non-causal kernels, and so their code, is what it was.
struct AttnCausalSmem { float q[AT_L * AT_PQ], k[AT_L * AT_PQ], v[AT_L * AT_PQ], p[AT_L * AT_PP]; };
struct AttnCausalBwdSmem { AttnCausalSmem f; float dO[AT_L * AT_PQ], dS[AT_L * AT_PP]; };

// attn_probs with the causal test: p[i][j] = 0 for j > i
DEV void attn_probs_causal(AttnCausalSmem& sm, const int64_t* mask_row, int L, int lane) {
  const int j = lane & 31, half = lane >> 5;
  const bool jvalid = j < L;
  float madd = 0.f;
  if (jvalid && mask_row) madd = mask_row[j] != 0 ? 0.f : AT_NEG;
  for (int i0 = 0; i0 < AT_L; i0 += 2) {
    int i = i0 + half;
    const bool seen = jvalid && j <= i;
    float s = 0.f;
#pragma unroll 16
    for (int d = 0; d < AT_D; ++d) s += sm.q[i * AT_PQ + d] * sm.k[j * AT_PQ + d];
    s = s * 0.125f + madd;
    if (!seen) s = -INFINITY;
    float mx = s;
#pragma unroll
    for (int m = 16; m >= 1; m >>= 1) mx = fmaxf(mx, wave_shfl_xor(mx, m));
    float e = seen ? __expf(s - mx) : 0.f;
    float den = e;
#pragma unroll
    for (int m = 16; m >= 1; m >>= 1) den += wave_shfl_xor(den, m);
    sm.p[i * AT_PP + j] = (i < L) ? e / den : 0.f;
  }
}

template <typename T>
__global__ __launch_bounds__(64) void attention_causal_fwd_kernel(const T* qkv, const int64_t* mask, T* ctx, int B, int L, int H) {
  __shared__ AttnCausalSmem sm;
  const int lane = threadIdx.x;
  const int b = blockIdx.x / H, h = blockIdx.x % H;
  const size_t ld = (size_t)3 * H * AT_D;
  const T* base = qkv + (size_t)b * L * ld + h * AT_D;
  attn_load_rows(base, ld, L, sm.q, lane);
  attn_load_rows(base + H * AT_D, ld, L, sm.k, lane);
  attn_load_rows(base + 2 * H * AT_D, ld, L, sm.v, lane);
  __syncthreads();
  attn_probs_causal(sm, mask ? mask + (size_t)b * L : nullptr, L, lane);
  __syncthreads();
  for (int i = 0; i < L; ++i) {
    float o = 0.f;
    for (int j = 0; j <= i; ++j) o += sm.p[i * AT_PP + j] * sm.v[j * AT_PQ + lane];
    al_store(ctx + ((size_t)b * L + i) * ((size_t)H * AT_D) + h * AT_D + lane, o);
  }
}

template <typename T>
__global__ __launch_bounds__(64) void attention_causal_bwd_kernel(const T* qkv, const int64_t* mask, const T* dctx, T* dqkv, int B, int L, int H) {
  __shared__ AttnCausalBwdSmem sm;
  const int lane = threadIdx.x;
  const int b = blockIdx.x / H, h = blockIdx.x % H;
  const size_t ld = (size_t)3 * H * AT_D;
  const T* base = qkv + (size_t)b * L * ld + h * AT_D;
  attn_load_rows(base, ld, L, sm.f.q, lane);
  attn_load_rows(base + H * AT_D, ld, L, sm.f.k, lane);
  attn_load_rows(base + 2 * H * AT_D, ld, L, sm.f.v, lane);
  attn_load_rows(dctx + (size_t)b * L * ((size_t)H * AT_D) + h * AT_D, (size_t)H * AT_D, L, sm.dO, lane);
  __syncthreads();
  attn_probs_causal(sm.f, mask ? mask + (size_t)b * L : nullptr, L, lane);
  __syncthreads();
  const int j = lane & 31, half = lane >> 5;
  // dP[i][j] = sum_d dO[i][d] V[j][d];  dS = P * (dP - sum_j dP*P): zero behind the diagonal, where P is
  for (int i0 = 0; i0 < AT_L; i0 += 2) {
    int i = i0 + half;
    float dp = 0.f;
#pragma unroll 16
    for (int d = 0; d < AT_D; ++d) dp += sm.dO[i * AT_PQ + d] * sm.f.v[j * AT_PQ + d];
    float pij = sm.f.p[i * AT_PP + j];
    float t = dp * pij;
#pragma unroll
    for (int m = 16; m >= 1; m >>= 1) t += wave_shfl_xor(t, m);
    sm.dS[i * AT_PP + j] = pij * (dp - t);
  }
  __syncthreads();
  // lane = d.  dQ[r] sums the keys t <= r, dK[r] and dV[r] the queries t >= r, in ascending order
  T* obase = dqkv + (size_t)b * L * ld + h * AT_D;
  for (int r = 0; r < L; ++r) {
    float dq = 0.f, dk = 0.f, dv = 0.f;
    for (int t = 0; t <= r; ++t) dq += sm.dS[r * AT_PP + t] * sm.f.k[t * AT_PQ + lane];
    for (int t = r; t < L; ++t) {
      dk += sm.dS[t * AT_PP + r] * sm.f.q[t * AT_PQ + lane];
      dv += sm.f.p[t * AT_PP + r] * sm.dO[t * AT_PQ + lane];
    }
    T* o = obase + (size_t)r * ld + lane;
    al_store(o, dq * 0.125f);
    al_store(o + H * AT_D, dk * 0.125f);
    al_store(o + 2 * H * AT_D, dv);
  }
}

// ---- bf16 MFMA, L <= 32: attention_mfma_{fwd,bwd}_kernel with the element-wise test on the one tile
struct AmCausalBwdSmem { char q[32 * AM_PI], k[32 * AM_PI], d[32 * AM_PI], t[32 * AM_PT]; float madd[32]; };

__global__ __launch_bounds__(256) void attention_causal_mfma_fwd_kernel(const bf16* qkv, const int64_t* mask, bf16* ctx, int B, int L, int H) {
  __shared__ __attribute__((aligned(16))) AmFwdSmem sm[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int bh = blockIdx.x * 4 + wave;
  const bool live = bh < B * H;
  if (!live) bh = B * H - 1;
  const int b = bh / H, h = bh % H;
  const size_t ld = (size_t)3 * H * 64;
  const bf16* qb = qkv + (size_t)b * L * ld + h * 64;
  AmFwdSmem& S = sm[wave];
  am_load_image(qb + 2 * H * 64, ld, L, S.v, lane);
  if (lane < 32) S.madd[lane] = al_madd(mask, b, L, lane);
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
  for (int ks = 0; ks < 4; ++ks)      // S^T[j][i] = sum_d K[j][d] Q[i][d]
    acc = mfma32_bf16(am_frag_rows(qb + H * 64, ld, L, ks, lane), am_frag_rows(qb, ld, L, ks, lane), acc);
  __syncthreads();
  // softmax over the keys j = am_row(r, lane) <= i for the query i = lane&31
  const int i = lane & 31;
  float mx = -INFINITY;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    acc[r] = am_row(r, lane) > i ? -INFINITY : acc[r] * 0.125f + S.madd[am_row(r, lane)];
    mx = fmaxf(mx, acc[r]);
  }
  mx = fmaxf(mx, wave_shfl_xor(mx, 32));
  float den = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) { acc[r] = __expf(acc[r] - mx); den += acc[r]; }
  den += wave_shfl_xor(den, 32);
  const float inv = 1.0f / den;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] *= inv;
  // O^T[d][i] = sum_j V^T[d][j] P^T[j][i]
#pragma unroll
  for (int db = 0; db < 2; ++db) {
    f32x16 o;
#pragma unroll
    for (int r = 0; r < 16; ++r) o[r] = 0.f;
#pragma unroll
    for (int s = 0; s < 2; ++s) o = mfma32_bf16(am_frag_tr_acc<AM_PI>(S.v, db * 32, s, lane), am_acc_frag(acc, s), o);
    if (live) am_store_T(ctx + (size_t)b * L * ((size_t)H * 64) + h * 64, (size_t)H * 64, L, db * 32, o, 1.f, lane);
  }
}

__global__ __launch_bounds__(128) void attention_causal_mfma_bwd_kernel(const bf16* qkv, const int64_t* mask, const bf16* dctx, bf16* dqkv, int B, int L, int H) {
  __shared__ __attribute__((aligned(16))) AmCausalBwdSmem sm[2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int bh = blockIdx.x * 2 + wave;
  const bool live = bh < B * H;
  if (!live) bh = B * H - 1;
  const int b = bh / H, h = bh % H;
  const size_t ld = (size_t)3 * H * 64, ldc = (size_t)H * 64;
  const bf16* qb = qkv + (size_t)b * L * ld + h * 64;
  const bf16* dob = dctx + (size_t)b * L * ldc + h * 64;
  AmCausalBwdSmem& S = sm[wave];
  am_load_image(qb, ld, L, S.q, lane);
  am_load_image(qb + H * 64, ld, L, S.k, lane);
  am_load_image(dob, ldc, L, S.d, lane);
  if (lane < 32) S.madd[lane] = al_madd(mask, b, L, lane);
  f32x16 p, dp;
#pragma unroll
  for (int r = 0; r < 16; ++r) { p[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    p = mfma32_bf16(am_frag_rows(qb, ld, L, ks, lane), am_frag_rows(qb + H * 64, ld, L, ks, lane), p);            // S[i][j]
    dp = mfma32_bf16(am_frag_rows(dob, ldc, L, ks, lane), am_frag_rows(qb + 2 * H * 64, ld, L, ks, lane), dp);    // dP[i][j] = dO V^T
  }
  __syncthreads();
  const int j = lane & 31;
  const float madd = S.madd[j];
  f32x16 ds;
#pragma unroll
  for (int r = 0; r < 16; ++r) {      // softmax over j <= i = across the 32 lanes of a half, per register row i
    const int i = am_row(r, lane);
    const float s = j > i ? -INFINITY : p[r] * 0.125f + madd;
    float mx = s;
#pragma unroll
    for (int m = 16; m >= 1; m >>= 1) mx = fmaxf(mx, wave_shfl_xor(mx, m));
    float e = __expf(s - mx);
    float den = e;
#pragma unroll
    for (int m = 16; m >= 1; m >>= 1) den += wave_shfl_xor(den, m);
    float pr = (i < L) ? e / den : 0.f;
    float t = dp[r] * pr;
#pragma unroll
    for (int m = 16; m >= 1; m >>= 1) t += wave_shfl_xor(t, m);
    p[r] = pr;
    ds[r] = pr * (dp[r] - t);
  }
  // dS^T image for dQ: T[j][i] = dS[i][j]
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    union { bf16 e[4]; u32x2 u; } pk;
#pragma unroll
    for (int e = 0; e < 4; ++e) pk.e[e] = f2bf(ds[4 * g + e]);
    *(u32x2*)(S.t + j * AM_PT + (8 * g + 4 * (lane >> 5)) * 2) = pk.u;
  }
  __syncthreads();
  bf16* ob = dqkv + (size_t)b * L * ld + h * 64;
#pragma unroll
  for (int db = 0; db < 2; ++db) {
    f32x16 dv, dk, dq;
#pragma unroll
    for (int r = 0; r < 16; ++r) { dv[r] = 0.f; dk[r] = 0.f; dq[r] = 0.f; }
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      dv = mfma32_bf16(am_frag_tr_acc<AM_PI>(S.d, db * 32, s, lane), am_acc_frag(p, s), dv);       // dV^T[d][j] = sum_i dO^T[d][i] P[i][j]
      dk = mfma32_bf16(am_frag_tr_acc<AM_PI>(S.q, db * 32, s, lane), am_acc_frag(ds, s), dk);      // dK^T[d][j] = sum_i Q^T[d][i] dS[i][j]
      dq = mfma32_bf16(am_frag_tr<AM_PI>(S.k, db * 32, s, lane), am_frag_tr<AM_PT>(S.t, 0, s, lane), dq);   // dQ^T[d][i] = sum_j K^T[d][j] dS^T[j][i]
    }
    if (live) {
      am_store_T(ob + 2 * H * 64, ld, L, db * 32, dv, 1.f, lane);
      am_store_T(ob + H * 64, ld, L, db * 32, dk, 0.125f, lane);
      am_store_T(ob, ld, L, db * 32, dq, 0.125f, lane);
    }
  }
}

// ---- exact f32 on the VALU, 33..128: attention_long_{fwd,bwd}_kernel; a score row ends at its diagonal, a score column begins there. The upper
// half of the lanes' keys (j = lane + 64) is not formed for a query below 64, nor the lower half of the queries for a key from 64 on.
struct AlCausalBwdSmem {
  float q[AL_L * AT_PQ], k[AL_L * AT_PQ], v[AL_L * AT_PQ], dO[AL_L * AT_PQ];
  float madd[AL_L], mx[AL_L], den[AL_L], t[AL_L];
  float vec[4][2][2][AL_L];                            // [wave][iteration parity][dS | P]
};

template <typename T>
__global__ __launch_bounds__(256) void attention_causal_long_fwd_kernel(const T* qkv, const int64_t* mask, T* ctx, int B, int L, int H) {
  __shared__ AlSmem sm;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int bh = blockIdx.x, b = bh / H, h = bh % H;
  const size_t ld = (size_t)3 * H * AT_D;
  const T* base = qkv + (size_t)b * L * ld + h * AT_D;
  al_load_rows(base, ld, L, sm.q, tid);
  al_load_rows(base + H * AT_D, ld, L, sm.k, tid);
  al_load_rows(base + 2 * H * AT_D, ld, L, sm.v, tid);
  if (tid < AL_L) sm.madd[tid] = al_madd(mask, b, L, tid);
  __syncthreads();
  for (int it = 0; it < (L + 3) / 4; ++it) {
    const int i = it * 4 + wave;
    float* row = sm.row[wave][it & 1];
    if (i < L) {
      float s0 = -INFINITY, s1 = -INFINITY;
      if (lane <= i) s0 = al_dot(sm.q + i * AT_PQ, sm.k + lane * AT_PQ) * 0.125f + sm.madd[lane];
      if (i >= 64 && lane + 64 <= i) s1 = al_dot(sm.q + i * AT_PQ, sm.k + (lane + 64) * AT_PQ) * 0.125f + sm.madd[lane + 64];
      const float mx = wave_max(fmaxf(s0, s1));
      const float e0 = __expf(s0 - mx), e1 = __expf(s1 - mx);      // keys > i and keys >= L: exp(-inf) = 0
      const float den = wave_sum(e0 + e1);
      row[lane] = e0 / den;
      row[lane + 64] = e1 / den;
    }
    __syncthreads();
    if (i < L) {
      float o = 0.f;
      for (int j = 0; j <= i; ++j) o += row[j] * sm.v[j * AT_PQ + lane];
      al_store(ctx + ((size_t)b * L + i) * ((size_t)H * AT_D) + h * AT_D + lane, o);
    }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void attention_causal_long_bwd_kernel(const T* qkv, const int64_t* mask, const T* dctx, T* dqkv, int B, int L, int H) {
  __shared__ AlCausalBwdSmem sm;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int bh = blockIdx.x, b = bh / H, h = bh % H;
  const size_t ld = (size_t)3 * H * AT_D;
  const T* base = qkv + (size_t)b * L * ld + h * AT_D;
  al_load_rows(base, ld, L, sm.q, tid);
  al_load_rows(base + H * AT_D, ld, L, sm.k, tid);
  al_load_rows(base + 2 * H * AT_D, ld, L, sm.v, tid);
  al_load_rows(dctx + (size_t)b * L * ((size_t)H * AT_D) + h * AT_D, (size_t)H * AT_D, L, sm.dO, tid);
  if (tid < AL_L) sm.madd[tid] = al_madd(mask, b, L, tid);
  __syncthreads();
  T* obase = dqkv + (size_t)b * L * ld + h * AT_D;
  const int iters = (L + 3) / 4;
  // query rows: P, dP = dO V^T, dS = P * (dP - sum_j dP*P) over the keys j <= i; dQ[i] = dS[i] K / 8. The row's softmax statistics stay in LDS.
  for (int it = 0; it < iters; ++it) {
    const int i = it * 4 + wave;
    float* ds = sm.vec[wave][it & 1][0];
    if (i < L) {
      float s0 = -INFINITY, s1 = -INFINITY, dp0 = 0.f, dp1 = 0.f;
      if (lane <= i) {
        s0 = al_dot(sm.q + i * AT_PQ, sm.k + lane * AT_PQ) * 0.125f + sm.madd[lane];
        dp0 = al_dot(sm.dO + i * AT_PQ, sm.v + lane * AT_PQ);
      }
      if (i >= 64 && lane + 64 <= i) {
        s1 = al_dot(sm.q + i * AT_PQ, sm.k + (lane + 64) * AT_PQ) * 0.125f + sm.madd[lane + 64];
        dp1 = al_dot(sm.dO + i * AT_PQ, sm.v + (lane + 64) * AT_PQ);
      }
      const float mx = wave_max(fmaxf(s0, s1));
      const float e0 = __expf(s0 - mx), e1 = __expf(s1 - mx);
      const float den = wave_sum(e0 + e1);
      const float p0 = e0 / den, p1 = e1 / den;
      const float t = wave_sum(dp0 * p0 + dp1 * p1);
      ds[lane] = p0 * (dp0 - t);
      ds[lane + 64] = p1 * (dp1 - t);
      if (lane == 0) { sm.mx[i] = mx; sm.den[i] = den; sm.t[i] = t; }
    }
    __syncthreads();
    if (i < L) {
      float dq = 0.f;
      for (int j = 0; j <= i; ++j) dq += ds[j] * sm.k[j * AT_PQ + lane];
      al_store(obase + (size_t)i * ld + lane, dq * 0.125f);
    }
  }
  __syncthreads();
  // key rows: column j of dS and of P from the saved statistics for the queries i >= j (lane = query i, i + 64); dK[j] = dS[:, j]^T Q / 8,
  // dV[j] = P[:, j]^T dO, summed over those queries in ascending order
  for (int it = 0; it < iters; ++it) {
    const int j = it * 4 + wave;
    float* ds = sm.vec[wave][it & 1][0];
    float* pd = sm.vec[wave][it & 1][1];
    if (j < L) {
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        if (half == 0 && j >= 64) continue;      // (queries below 64 do not see this key, and the sums below start at j)
        const int i = lane + 64 * half;
        float dsv = 0.f, pv = 0.f;
        if (i < L && i >= j) {
          const float s = al_dot(sm.q + i * AT_PQ, sm.k + j * AT_PQ) * 0.125f + sm.madd[j];
          pv = __expf(s - sm.mx[i]) / sm.den[i];
          dsv = pv * (al_dot(sm.dO + i * AT_PQ, sm.v + j * AT_PQ) - sm.t[i]);
        }
        ds[i] = dsv;
        pd[i] = pv;
      }
    }
    __syncthreads();
    if (j < L) {
      float dk = 0.f, dv = 0.f;
      for (int i = j; i < L; ++i) {
        dk += ds[i] * sm.q[i * AT_PQ + lane];
        dv += pd[i] * sm.dO[i * AT_PQ + lane];
      }
      al_store(obase + (size_t)j * ld + H * AT_D + lane, dk * 0.125f);
      al_store(obase + (size_t)j * ld + 2 * H * AT_D + lane, dv);
    }
  }
}

// ---- bf16 MFMA, 33..128: attention_long_mfma_{fwd,bwd}_kernel on the lower triangle of the NT x NT tile products. Wave w (query tile w) forms the
// scores against the key tiles 0..w only — 3 of 4 products at NT = 2, 6 of 9 at NT = 3, 10 of 16 at NT = 4 — and only the diagonal tile t = w
// applies the element-wise test. Backward: dQ of query tile w sums the key tiles 0..w, dK / dV of key tile w the query tiles w..NT-1 in ascending
// order; the [key][query] images are written and read on that triangle only.
// Every wave runs the matrix products in a body compiled for ITS tile index W (a switch on the wave index around straight-line code): with the tile loops bounded by a
// run-time wave index instead, each product sat in a basic block of its own behind its own loads, and the one wave a SIMD holds here waited out
// every LDS and global latency in turn — that form ran the backward 1.3 - 1.5 x SLOWER than the non-causal kernel. The
// workgroup barriers stay outside the switches, and the first one behind the score products, which read global memory only: the fill of the
// LDS images overlaps them, as in the non-causal kernels.
template <int NT> struct AlmCausalBwdSmem {
  static constexpr int PT = 64 * NT + 16;      // [32 NT][32 NT] bf16 image pitch
  char q[32 * NT * AM_PI], k[32 * NT * AM_PI], d[32 * NT * AM_PI], ts[32 * NT * PT], tp[32 * NT * PT];
  float madd[32 * NT];
};

// forward of query tile W, from global memory alone (it runs while the V image is still on its way into LDS): S^T = K Q^T over the key tiles 0..W
template <int NT, int W>
DEV void almc_fwd_scores(const bf16* qb, f32x16 (&acc)[NT], int L, int H, int lane) {
  const size_t ld = (size_t)3 * H * 64;
  const int Lq = L - 32 * W;      // rows of this query tile inside the sample (> 0: L > 32 (NT - 1))
  bf16x8 qf[4];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) qf[ks] = am_frag_rows(qb + (size_t)32 * W * ld, ld, Lq, ks, lane);
#pragma unroll
  for (int t = 0; t <= W; ++t) {      // S^T[j][i] = sum_d K[j][d] Q[i][d], key tile t
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) acc[t] = mfma32_bf16(am_frag_rows(qb + H * 64 + (size_t)32 * t * ld, ld, L - 32 * t, ks, lane), qf[ks], acc[t]);
  }
}
// ... then the softmax over the keys j <= i (W + 1 accumulators x the two lane halves) for the query i = 32 W + (lane & 31), and O^T = V^T P^T
template <int NT, int W>
DEV void almc_fwd_out(f32x16 (&acc)[NT], bf16* ctx_tile, const AlmFwdSmem<NT>& S, int L, int H, int lane) {
  const size_t ldc = (size_t)H * 64;
  const int Lq = L - 32 * W;
  const int il = lane & 31;
  float mx = -INFINITY;
#pragma unroll
  for (int t = 0; t <= W; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float s = acc[t][r] * 0.125f + S.madd[32 * t + am_row(r, lane)];
      acc[t][r] = (t == W && am_row(r, lane) > il) ? -INFINITY : s;
      mx = fmaxf(mx, acc[t][r]);
    }
  mx = fmaxf(mx, wave_shfl_xor(mx, 32));
  float den = 0.f;
#pragma unroll
  for (int t = 0; t <= W; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc[t][r] = __expf(acc[t][r] - mx); den += acc[t][r]; }
  den += wave_shfl_xor(den, 32);
  const float inv = 1.0f / den;
#pragma unroll
  for (int t = 0; t <= W; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] *= inv;
  // O^T[d][i] = sum_j V^T[d][j] P^T[j][i], key tiles in ascending order
#pragma unroll
  for (int db = 0; db < 2; ++db) {
    f32x16 o;
#pragma unroll
    for (int r = 0; r < 16; ++r) o[r] = 0.f;
#pragma unroll
    for (int t = 0; t <= W; ++t)
#pragma unroll
      for (int s = 0; s < 2; ++s) o = mfma32_bf16(am_frag_tr_acc<AM_PI>(S.v + 32 * t * AM_PI, db * 32, s, lane), am_acc_frag(acc[t], s), o);
    am_store_T(ctx_tile, ldc, Lq, db * 32, o, 1.f, lane);
  }
}

template <int NT>
__global__ __launch_bounds__(64 * NT) void attention_causal_long_mfma_fwd_kernel(const bf16* qkv, const int64_t* mask, bf16* ctx, int B, int L, int H) {
  __shared__ __attribute__((aligned(16))) AlmFwdSmem<NT> S;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int bh = blockIdx.x, b = bh / H, h = bh % H;
  const size_t ld = (size_t)3 * H * 64, ldc = (size_t)H * 64;
  const bf16* qb = qkv + (size_t)b * L * ld + h * 64;
  alm_load_image<NT>(qb + 2 * H * 64, ld, L, S.v, tid);
  if (tid < 32 * NT) S.madd[tid] = al_madd(mask, b, L, tid);
  f32x16 acc[NT];
  switch (wave) {
    case 0: almc_fwd_scores<NT, 0>(qb, acc, L, H, lane); break;
    case 1: almc_fwd_scores<NT, 1>(qb, acc, L, H, lane); break;
    case 2: if constexpr (NT > 2) almc_fwd_scores<NT, 2>(qb, acc, L, H, lane); break;
    default: if constexpr (NT > 3) almc_fwd_scores<NT, 3>(qb, acc, L, H, lane); break;
  }
  __syncthreads();
  bf16* ct = ctx + ((size_t)b * L + 32 * wave) * ldc + h * 64;
  switch (wave) {
    case 0: almc_fwd_out<NT, 0>(acc, ct, S, L, H, lane); break;
    case 1: almc_fwd_out<NT, 1>(acc, ct, S, L, H, lane); break;
    case 2: if constexpr (NT > 2) almc_fwd_out<NT, 2>(acc, ct, S, L, H, lane); break;
    default: if constexpr (NT > 3) almc_fwd_out<NT, 3>(acc, ct, S, L, H, lane); break;
  }
}

// backward, first part, of query tile W, from global memory alone (the images are still on their way into LDS): S = Q K^T and dP = dO V^T
// against the key tiles 0..W
template <int NT, int W>
DEV void almc_bwd_scores(const bf16* qb, const bf16* dob, f32x16 (&p)[NT], f32x16 (&dp)[NT], int L, int H, int lane) {
  const size_t ld = (size_t)3 * H * 64, ldc = (size_t)H * 64;
  const int Lq = L - 32 * W;
  bf16x8 qf[4], dof[4];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    qf[ks] = am_frag_rows(qb + (size_t)32 * W * ld, ld, Lq, ks, lane);
    dof[ks] = am_frag_rows(dob + (size_t)32 * W * ldc, ldc, Lq, ks, lane);
  }
#pragma unroll
  for (int t = 0; t <= W; ++t) {
#pragma unroll
    for (int r = 0; r < 16; ++r) { p[t][r] = 0.f; dp[t][r] = 0.f; }
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      p[t] = mfma32_bf16(qf[ks], am_frag_rows(qb + H * 64 + (size_t)32 * t * ld, ld, L - 32 * t, ks, lane), p[t]);            // S[i][j]
      dp[t] = mfma32_bf16(dof[ks], am_frag_rows(qb + 2 * H * 64 + (size_t)32 * t * ld, ld, L - 32 * t, ks, lane), dp[t]);     // dP[i][j] = dO V^T
    }
  }
}
// ... then the softmax and dS; leaves dS^T and P^T of the tile's 32 queries in the images. ONE body for all waves (four specialised copies of this
// VALU-heavy part made the NT = 4 kernel 63 KB of code, which does not stay in the instruction cache with four waves in four places of it): the
// key tiles are the outer loop of every stage, so a wave-uniform `t <= wave` guards 16 register rows of straight-line code at a time.
template <int NT>
DEV void almc_bwd_softmax(f32x16 (&p)[NT], f32x16 (&dp)[NT], AlmCausalBwdSmem<NT>& S, int L, int wave, int lane) {
  constexpr int PT = AlmCausalBwdSmem<NT>::PT;
  const int Lq = L - 32 * wave;
  const int jl = lane & 31;
  float mx[16], den[16], tt[16];      // per register row i = am_row(r, lane), over j <= i = across the 32 lanes of a half and the tiles t <= wave
#pragma unroll
  for (int r = 0; r < 16; ++r) { mx[r] = -INFINITY; den[r] = 0.f; tt[r] = 0.f; }
#pragma unroll
  for (int t = 0; t < NT; ++t)
    if (t <= wave) {
      const float madd = S.madd[32 * t + jl];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        p[t][r] = (t == wave && jl > am_row(r, lane)) ? -INFINITY : p[t][r] * 0.125f + madd;
        mx[r] = fmaxf(mx[r], p[t][r]);
      }
    }
#pragma unroll
  for (int r = 0; r < 16; ++r)
#pragma unroll
    for (int m = 16; m >= 1; m >>= 1) mx[r] = fmaxf(mx[r], wave_shfl_xor(mx[r], m));
#pragma unroll
  for (int t = 0; t < NT; ++t)
    if (t <= wave) {
#pragma unroll
      for (int r = 0; r < 16; ++r) { p[t][r] = __expf(p[t][r] - mx[r]); den[r] += p[t][r]; }
    }
#pragma unroll
  for (int r = 0; r < 16; ++r)
#pragma unroll
    for (int m = 16; m >= 1; m >>= 1) den[r] += wave_shfl_xor(den[r], m);
#pragma unroll
  for (int t = 0; t < NT; ++t)
    if (t <= wave) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        p[t][r] = (am_row(r, lane) < Lq) ? p[t][r] / den[r] : 0.f;      // P
        tt[r] += dp[t][r] * p[t][r];
      }
    }
#pragma unroll
  for (int r = 0; r < 16; ++r)
#pragma unroll
    for (int m = 16; m >= 1; m >>= 1) tt[r] += wave_shfl_xor(tt[r], m);
  // dS, and the images on the triangle: ts[j][i] = dS[i][j], tp[j][i] = P[i][j] for this tile's 32 queries (4 consecutive i per register group)
#pragma unroll
  for (int t = 0; t < NT; ++t)
    if (t <= wave) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        union { bf16 e[4]; u32x2 u; } ks, kp;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = 4 * g + e;
          ks.e[e] = f2bf(p[t][r] * (dp[t][r] - tt[r]));
          kp.e[e] = f2bf(p[t][r]);
        }
        const int off = (32 * t + jl) * PT + (32 * wave + 8 * g + 4 * (lane >> 5)) * 2;
        *(u32x2*)(S.ts + off) = ks.u;
        *(u32x2*)(S.tp + off) = kp.u;
      }
    }
}

// backward, second part: dK, dV of key tile W (the 16-query steps s >= 2 W) and dQ of query tile W (the 16-key steps s < 2 W + 2)
template <int NT, int W>
DEV void almc_bwd_grads(bf16* ob, const AlmCausalBwdSmem<NT>& S, int L, int H, int lane) {
  constexpr int PT = AlmCausalBwdSmem<NT>::PT;
  const size_t ld = (size_t)3 * H * 64;
  const int Lq = L - 32 * W, jl = lane & 31;
#pragma unroll
  for (int db = 0; db < 2; ++db) {
    f32x16 dv, dk, dq;
#pragma unroll
    for (int r = 0; r < 16; ++r) { dv[r] = 0.f; dk[r] = 0.f; dq[r] = 0.f; }
#pragma unroll
    for (int s = 2 * W; s < 2 * NT; ++s) {
      Chunk16 bp, bs;
      const int off = (32 * W + jl) * PT + (16 * s + 8 * (lane >> 5)) * 2;
      bp.u = *(const u32x4*)(S.tp + off);
      bs.u = *(const u32x4*)(S.ts + off);
      dv = mfma32_bf16(am_frag_tr<AM_PI>(S.d, db * 32, s, lane), bp.h, dv);      // dV^T[d][j] = sum_i dO^T[d][i] P[i][j]
      dk = mfma32_bf16(am_frag_tr<AM_PI>(S.q, db * 32, s, lane), bs.h, dk);      // dK^T[d][j] = sum_i Q^T[d][i] dS[i][j]
    }
#pragma unroll
    for (int s = 0; s < 2 * W + 2; ++s)
      dq = mfma32_bf16(am_frag_tr<AM_PI>(S.k, db * 32, s, lane), am_frag_tr<PT>(S.ts, 32 * W, s, lane), dq);   // dQ^T[d][i] = sum_j K^T[d][j] dS^T[j][i]
    am_store_T(ob + 2 * H * 64, ld, Lq, db * 32, dv, 1.f, lane);
    am_store_T(ob + H * 64, ld, Lq, db * 32, dk, 0.125f, lane);
    am_store_T(ob, ld, Lq, db * 32, dq, 0.125f, lane);
  }
}

template <int NT>
__global__ __launch_bounds__(64 * NT) void attention_causal_long_mfma_bwd_kernel(const bf16* qkv, const int64_t* mask, const bf16* dctx, bf16* dqkv, int B, int L,
                                                                                  int H) {
  __shared__ __attribute__((aligned(16))) AlmCausalBwdSmem<NT> S;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int bh = blockIdx.x, b = bh / H, h = bh % H;
  const size_t ld = (size_t)3 * H * 64, ldc = (size_t)H * 64;
  const bf16* qb = qkv + (size_t)b * L * ld + h * 64;
  const bf16* dob = dctx + (size_t)b * L * ldc + h * 64;
  alm_load_image<NT>(qb, ld, L, S.q, tid);
  alm_load_image<NT>(qb + H * 64, ld, L, S.k, tid);
  alm_load_image<NT>(dob, ldc, L, S.d, tid);
  if (tid < 32 * NT) S.madd[tid] = al_madd(mask, b, L, tid);
  f32x16 p[NT], dp[NT];
  switch (wave) {
    case 0: almc_bwd_scores<NT, 0>(qb, dob, p, dp, L, H, lane); break;
    case 1: almc_bwd_scores<NT, 1>(qb, dob, p, dp, L, H, lane); break;
    case 2: if constexpr (NT > 2) almc_bwd_scores<NT, 2>(qb, dob, p, dp, L, H, lane); break;
    default: if constexpr (NT > 3) almc_bwd_scores<NT, 3>(qb, dob, p, dp, L, H, lane); break;
  }
  __syncthreads();
  almc_bwd_softmax<NT>(p, dp, S, L, wave, lane);
  __syncthreads();
  bf16* ob = dqkv + ((size_t)b * L + 32 * wave) * ld + h * 64;      // key tile `wave` for dK, dV; query tile `wave` for dQ
  switch (wave) {
    case 0: almc_bwd_grads<NT, 0>(ob, S, L, H, lane); break;
    case 1: almc_bwd_grads<NT, 1>(ob, S, L, H, lane); break;
    case 2: if constexpr (NT > 2) almc_bwd_grads<NT, 2>(ob, S, L, H, lane); break;
    default: if constexpr (NT > 3) almc_bwd_grads<NT, 3>(ob, S, L, H, lane); break;
  }
}

// ---- the CLIP text tower's streaming pieces
// x[row] = token_embedding[ids[row]] + positional_embedding[row % L]: embed_fwd_kernel without the token-type row (and no LayerNorm behind it)
template <typename T>
__global__ __launch_bounds__(256) void embed_clip_fwd_kernel(const int64_t* ids, const T* word, const T* pos, T* out, int M, int L, int C, int vocab) {
  const int nchunk = C / 8;
  size_t total = (size_t)M * nchunk;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    int c = (int)(i % nchunk);
    int row = (int)(i / nchunk);
    int64_t id = ids[row];
    if (id < 0) id = 0;
    if (id >= vocab) id = vocab - 1;
    float a[8], b[8];
    load8(word + (size_t)id * C + c * 8, a);
    load8(pos + (size_t)(row % L) * C + c * 8, b);
#pragma unroll
    for (int e = 0; e < 8; ++e) a[e] += b[e];
    store8(out + (size_t)row * C + c * 8, a);
  }
}
// End-of-text pooling by the mask: idx[b] = (ones in mask[b]) - 1, clamped into the caption; out[b] = x[b][idx[b]]. A thread owns one 8-column
// chunk of one sample and counts that sample's mask itself (L <= 128 cached words); the thread of chunk 0 stores idx[b].
template <typename T>
__global__ __launch_bounds__(256) void last_token_gather_kernel(const T* x, const int64_t* mask, T* out, int32_t* idx, int B, int L, int C) {
  const int nchunk = C / 8;
  const size_t total = (size_t)B * nchunk;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int c = (int)(i % nchunk), b = (int)(i / nchunk);
    int n = 0;
    for (int l = 0; l < L; ++l) n += mask[(size_t)b * L + l] != 0 ? 1 : 0;
    int r = n - 1;
    if (r < 0) r = 0;
    float v[8];
    load8(x + ((size_t)b * L + r) * C + c * 8, v);
    store8(out + (size_t)b * C + c * 8, v);
    if (c == 0) idx[b] = r;
  }
}
// dx[b][idx[b]] = d[b]; the other rows of dx are left as they are (the caller zeroes them)
template <typename T>
__global__ __launch_bounds__(256) void last_token_scatter_kernel(const T* d, const int32_t* idx, T* dx, int B, int L, int C) {
  const int nchunk = C / 8;
  const size_t total = (size_t)B * nchunk;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int c = (int)(i % nchunk), b = (int)(i / nchunk);
    int r = idx[b];
    if (r < 0) r = 0;
    if (r >= L) r = L - 1;
    float v[8];
    load8(d + (size_t)b * C + c * 8, v);
    store8(dx + ((size_t)b * L + r) * C + c * 8, v);
  }
}

// BertPooler backward through tanh: out = dy * (1 - y^2)
template <typename T>
__global__ __launch_bounds__(256) void tanh_bwd_kernel(const T* dy, const T* y, T* out, size_t n8) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += (size_t)gridDim.x * 256) {
    float d[8], v[8];
    load8(dy + i * 8, d);
    load8(y + i * 8, v);
#pragma unroll
    for (int e = 0; e < 8; ++e) d[e] *= 1.f - v[e] * v[e];
    store8(out + i * 8, d);
  }
}

int ew_grid(size_t total) {
  size_t g = (total + 255) / 256;
  return (int)(g < 4096 ? (g ? g : 1) : 4096);
}
int ln_ok(int M, int C) { return M > 0 && C % 8 == 0 && C >= 8 && C <= 64 * LN_MAXCH * 8; }

}  // namespace

#define DISPATCH(dtype, CALL_BF16, CALL_F32) \
  if ((dtype) == CLITE_BF16) { CALL_BF16; } else if ((dtype) == CLITE_F32) { CALL_F32; } else return -1;

extern "C" int clite_layernorm_fwd(int dtype, const void* x, const float* gamma, const float* beta, float eps, void* out, float* stats,
                                   int M, int C, float drop_p, uint64_t drop_seed, uint32_t drop_site, void* stream) {
  if (!ln_ok(M, C) || !x || !out) return -1;
  int grid = (M + 3) / 4;
  if (grid > 2048) grid = 2048;
  Drop d{drop_p, drop_seed, drop_site};
  hipStream_t st = (hipStream_t)stream;
  if (C <= 1024) {
    constexpr int NCHV = 2;
    DISPATCH(dtype,
             hipLaunchKernelGGL((layernorm_fwd_kernel<bf16, NCHV>), dim3(grid), dim3(256), 0, st, (const bf16*)x, gamma, beta, eps, (bf16*)out, stats, M, C, d, LnQ8{}),
             hipLaunchKernelGGL((layernorm_fwd_kernel<float, NCHV>), dim3(grid), dim3(256), 0, st, (const float*)x, gamma, beta, eps, (float*)out, stats, M, C, d, LnQ8{}));
  } else {
    constexpr int NCHV = 4;
    DISPATCH(dtype,
             hipLaunchKernelGGL((layernorm_fwd_kernel<bf16, NCHV>), dim3(grid), dim3(256), 0, st, (const bf16*)x, gamma, beta, eps, (bf16*)out, stats, M, C, d, LnQ8{}),
             hipLaunchKernelGGL((layernorm_fwd_kernel<float, NCHV>), dim3(grid), dim3(256), 0, st, (const float*)x, gamma, beta, eps, (float*)out, stats, M, C, d, LnQ8{}));
  }
  return (int)hipGetLastError();
}

extern "C" int clite_layernorm_fwd_q8(int dtype, const void* x, const float* gamma, const float* beta, float eps, void* out, float* stats,
                                      int M, int C, float drop_p, uint64_t drop_seed, uint32_t drop_site, uint8_t* fp8_out, const float* fp8_scale,
                                      float* fp8_amax, void* stream) {
  if (dtype != CLITE_BF16 || !ln_ok(M, C) || C > 1024 || !x || !out || (fp8_out && !fp8_scale)) return -1;
  int grid = (M + 3) / 4;
  if (grid > 2048) grid = 2048;
  Drop d{drop_p, drop_seed, drop_site};
  hipLaunchKernelGGL((layernorm_fwd_kernel<bf16, 2, true>), dim3(grid), dim3(256), 0, (hipStream_t)stream, (const bf16*)x, gamma, beta, eps, (bf16*)out, stats, M, C, d,
                     LnQ8{fp8_out, fp8_scale, fp8_amax});
  return (int)hipGetLastError();
}

extern "C" int clite_layernorm_bwd(int dtype, const void* dy, const void* x, const float* stats, const float* gamma, void* dx, void* dx_masked,
                                   float* dgamma, float* dbeta, float* dcolsum, int M, int C, float in_p, uint64_t in_seed, uint32_t in_site,
                                   float out_p, uint64_t out_seed, uint32_t out_site, void* stream) {
  if (!ln_ok(M, C) || !dy || !x || !stats || !dx) return -1;
  constexpr int NW = 8, LN_BWD_MAX_WG = 256;
  const bool det = clite::deterministic();      // det.h: one workgroup -> one contribution per parameter-gradient address
  int grid = (M + NW - 1) / NW;
  if (grid > LN_BWD_MAX_WG) grid = LN_BWD_MAX_WG;
  if (det) grid = 1;
  Drop di{in_p, in_seed, in_site}, dout{out_p, out_seed, out_site};
  hipStream_t st = (hipStream_t)stream;
  if (C <= 1024) {
    constexpr int NCHV = 2;
    DISPATCH(dtype,
             hipLaunchKernelGGL((layernorm_bwd_kernel<bf16, NCHV, NW>), dim3(grid), dim3(NW * 64), 0, st, (const bf16*)dy, (const bf16*)x, stats, gamma, (bf16*)dx, (bf16*)dx_masked, dgamma, dbeta, dcolsum, M, C, di, dout),
             hipLaunchKernelGGL((layernorm_bwd_kernel<float, NCHV, NW>), dim3(grid), dim3(NW * 64), 0, st, (const float*)dy, (const float*)x, stats, gamma, (float*)dx, (float*)dx_masked, dgamma, dbeta, dcolsum, M, C, di, dout));
  } else {
    constexpr int NCHV = 4, NW4 = 8;      // 4 chunks per lane: 8 waves keep the row state in registers
    grid = (M + NW4 - 1) / NW4;
    if (grid > LN_BWD_MAX_WG) grid = LN_BWD_MAX_WG;
    if (det) grid = 1;
    DISPATCH(dtype,
             hipLaunchKernelGGL((layernorm_bwd_kernel<bf16, NCHV, NW4>), dim3(grid), dim3(NW4 * 64), 0, st, (const bf16*)dy, (const bf16*)x, stats, gamma, (bf16*)dx, (bf16*)dx_masked, dgamma, dbeta, dcolsum, M, C, di, dout),
             hipLaunchKernelGGL((layernorm_bwd_kernel<float, NCHV, NW4>), dim3(grid), dim3(NW4 * 64), 0, st, (const float*)dy, (const float*)x, stats, gamma, (float*)dx, (float*)dx_masked, dgamma, dbeta, dcolsum, M, C, di, dout));
  }
  return (int)hipGetLastError();
}

extern "C" int clite_embed_fwd(int dtype, const int64_t* ids, const void* word, const void* pos, const void* type, void* out,
                               int M, int L, int C, int vocab, void* stream) {
  if (M <= 0 || L <= 0 || C % 8 || !ids || !out) return -1;
  int grid = ew_grid((size_t)M * (C / 8));
  hipStream_t st = (hipStream_t)stream;
  DISPATCH(dtype,
           hipLaunchKernelGGL(embed_fwd_kernel<bf16>, dim3(grid), dim3(256), 0, st, ids, (const bf16*)word, (const bf16*)pos, (const bf16*)type, (bf16*)out, M, L, C, vocab),
           hipLaunchKernelGGL(embed_fwd_kernel<float>, dim3(grid), dim3(256), 0, st, ids, (const float*)word, (const float*)pos, (const float*)type, (float*)out, M, L, C, vocab));
  return (int)hipGetLastError();
}

extern "C" int clite_embed_bwd(int dtype, const int64_t* ids, const void* d, float* dword, float* dpos, int M, int L, int C, int vocab, int padding_idx,
                               void* stream) {
  if (M <= 0 || L <= 0 || M % L || C % 8 || C > 128 * EMB_COLS || !ids || !d) return -1;
  if (!dword && !dpos) return 0;
  hipStream_t st = (hipStream_t)stream;
  const int egrid = clite::deterministic() ? 1 : L * EMB_SEGS;
  DISPATCH(dtype,
           hipLaunchKernelGGL(embed_bwd_kernel<bf16>, dim3(egrid), dim3(128), 0, st, ids, (const bf16*)d, dword, dpos, M / L, L, C, vocab, padding_idx, EmbMp<false>{}),
           hipLaunchKernelGGL(embed_bwd_kernel<float>, dim3(egrid), dim3(128), 0, st, ids, (const float*)d, dword, dpos, M / L, L, C, vocab, padding_idx, EmbMp<false>{}));
  return (int)hipGetLastError();
}

extern "C" int clite_attention_fwd(int dtype, const void* qkv, const int64_t* mask, void* ctx, int B, int L, int H,
                                   float drop_p, uint64_t drop_seed, uint32_t drop_site, void* stream) {
  if (B <= 0 || L <= 0 || L > AL_L || H <= 0 || !qkv || !ctx) return -1;
  Drop d{drop_p, drop_seed, drop_site};
  hipStream_t st = (hipStream_t)stream;
  if (L > AT_L) {      // 33..128: one workgroup per (batch, head), a wave per 32-query tile
#define AL_FWD(NT) hipLaunchKernelGGL(attention_long_mfma_fwd_kernel<NT>, dim3(B * H), dim3(64 * NT), 0, st, (const bf16*)qkv, mask, (bf16*)ctx, B, L, H, d)
    DISPATCH(dtype,
             if (L <= 64) AL_FWD(2); else if (L <= 96) AL_FWD(3); else AL_FWD(4),
             hipLaunchKernelGGL(attention_long_fwd_kernel<float>, dim3(B * H), dim3(256), 0, st, (const float*)qkv, mask, (float*)ctx, B, L, H, d));
#undef AL_FWD
    return (int)hipGetLastError();
  }
  DISPATCH(dtype,
           hipLaunchKernelGGL(attention_mfma_fwd_kernel<false>, dim3((B * H + 3) / 4), dim3(256), 0, st, (const bf16*)qkv, mask, (bf16*)ctx, B, L, H, d, AttnBias<false>{}),
           hipLaunchKernelGGL(attention_fwd_kernel<float>, dim3(B * H), dim3(64), 0, st, (const float*)qkv, mask, (float*)ctx, B, L, H, d, AttnBias<false>{}));
  return (int)hipGetLastError();
}

extern "C" int clite_attention_bwd(int dtype, const void* qkv, const int64_t* mask, const void* dctx, void* dqkv, int B, int L, int H,
                                   float drop_p, uint64_t drop_seed, uint32_t drop_site, void* stream) {
  if (B <= 0 || L <= 0 || L > AL_L || H <= 0 || !qkv || !dctx || !dqkv) return -1;
  Drop d{drop_p, drop_seed, drop_site};
  hipStream_t st = (hipStream_t)stream;
  if (L > AT_L) {
#define AL_BWD(NT) hipLaunchKernelGGL(attention_long_mfma_bwd_kernel<NT>, dim3(B * H), dim3(64 * NT), 0, st, (const bf16*)qkv, mask, (const bf16*)dctx, (bf16*)dqkv, B, L, H, d)
    DISPATCH(dtype,
             if (L <= 64) AL_BWD(2); else if (L <= 96) AL_BWD(3); else AL_BWD(4),
             hipLaunchKernelGGL(attention_long_bwd_kernel<float>, dim3(B * H), dim3(256), 0, st, (const float*)qkv, mask, (const float*)dctx, (float*)dqkv, B, L, H, d));
#undef AL_BWD
    return (int)hipGetLastError();
  }
  DISPATCH(dtype,
           hipLaunchKernelGGL(attention_mfma_bwd_kernel<false>, dim3((B * H + 1) / 2), dim3(128), 0, st, (const bf16*)qkv, mask, (const bf16*)dctx, (bf16*)dqkv, B, L, H, d, AttnBias<false>{}),
           hipLaunchKernelGGL(attention_bwd_kernel<float>, dim3(B * H), dim3(64), 0, st, (const float*)qkv, mask, (const float*)dctx, (float*)dqkv, B, L, H, d, AttnBias<false>{}));
  return (int)hipGetLastError();
}

extern "C" int clite_attention_bias_fwd(int dtype, const void* qkv, const int64_t* mask, const float* bias, void* ctx, int B, int L, int H,
                                        float drop_p, uint64_t drop_seed, uint32_t drop_site, void* stream) {
  if (B <= 0 || L <= 0 || L > AT_L || H <= 0 || !qkv || !ctx || !bias) return -1;
  Drop d{drop_p, drop_seed, drop_site};
  AttnBias<true> ab{bias, nullptr, nullptr};
  hipStream_t st = (hipStream_t)stream;
  DISPATCH(dtype,
           hipLaunchKernelGGL(attention_mfma_fwd_kernel<true>, dim3((B * H + 3) / 4), dim3(256), 0, st, (const bf16*)qkv, mask, (bf16*)ctx, B, L, H, d, ab),
           hipLaunchKernelGGL((attention_fwd_kernel<float, true>), dim3(B * H), dim3(64), 0, st, (const float*)qkv, mask, (float*)ctx, B, L, H, d, ab));
  return (int)hipGetLastError();
}

extern "C" int clite_attention_bias_bwd(int dtype, const void* qkv, const int64_t* mask, const float* bias, const int32_t* bucket_table, const void* dctx,
                                        void* dqkv, float* dbias_partials, int B, int L, int H, float drop_p, uint64_t drop_seed, uint32_t drop_site,
                                        void* stream) {
  if (B <= 0 || L <= 0 || L > AT_L || H <= 0 || !qkv || !dctx || !dqkv || !bias || !bucket_table || !dbias_partials) return -1;
  Drop d{drop_p, drop_seed, drop_site};
  AttnBias<true> ab{bias, bucket_table, dbias_partials};
  hipStream_t st = (hipStream_t)stream;
  DISPATCH(dtype,
           hipLaunchKernelGGL(attention_mfma_bwd_kernel<true>, dim3((B * H + 1) / 2), dim3(128), 0, st, (const bf16*)qkv, mask, (const bf16*)dctx, (bf16*)dqkv, B, L, H, d, ab),
           hipLaunchKernelGGL((attention_bwd_kernel<float, true>), dim3(B * H), dim3(64), 0, st, (const float*)qkv, mask, (const float*)dctx, (float*)dqkv, B, L, H, d, ab));
  return (int)hipGetLastError();
}

extern "C" int clite_attention_bias_build(const float* rel_weight, const int32_t* bucket_table, float* bias, int H, int L, void* stream) {
  if (H <= 0 || L <= 0 || L > AT_L || !rel_weight || !bucket_table || !bias) return -1;
  hipLaunchKernelGGL(attention_bias_build_kernel, dim3((H * AT_L * AT_L + 255) / 256), dim3(256), 0, (hipStream_t)stream, rel_weight, bucket_table, bias, H, L);
  return (int)hipGetLastError();
}

extern "C" int clite_attention_bias_grad_reduce(const float* partials, float* drel, int rows, int H, void* stream) {
  if (rows <= 0 || H <= 0 || !partials || !drel) return -1;
  hipLaunchKernelGGL(attention_bias_grad_reduce_kernel, dim3(H), dim3(1024), 0, (hipStream_t)stream, partials, drel, rows, H);
  return (int)hipGetLastError();
}

extern "C" int clite_embed_mpnet_fwd(int dtype, const int64_t* ids, const void* word, const void* pos, void* out, int32_t* pids, int M, int L, int C,
                                     int vocab, int max_pos, int padding_idx, void* stream) {
  if (M <= 0 || L <= 0 || L > 32 || M % L || C % 8 || vocab <= 0 || max_pos <= 0 || !ids || !word || !pos || !out) return -1;
  int grid = (M + 3) / 4;
  if (grid > 4096) grid = 4096;
  hipStream_t st = (hipStream_t)stream;
  DISPATCH(dtype,
           hipLaunchKernelGGL(embed_mpnet_fwd_kernel<bf16>, dim3(grid), dim3(256), 0, st, ids, (const bf16*)word, (const bf16*)pos, (bf16*)out, pids, M, L, C, vocab, max_pos, padding_idx),
           hipLaunchKernelGGL(embed_mpnet_fwd_kernel<float>, dim3(grid), dim3(256), 0, st, ids, (const float*)word, (const float*)pos, (float*)out, pids, M, L, C, vocab, max_pos, padding_idx));
  return (int)hipGetLastError();
}

extern "C" int clite_embed_mpnet_bwd(int dtype, const int64_t* ids, const int32_t* pids, const void* d, float* dword, float* dpos, int M, int L, int C,
                                     int vocab, int max_pos, int padding_idx, void* stream) {
  if (M <= 0 || L <= 0 || M % L || C % 8 || C > 128 * EMB_COLS || vocab <= 0 || max_pos <= 0 || !ids || !pids || !d) return -1;
  if (!dword && !dpos) return 0;
  hipStream_t st = (hipStream_t)stream;
  const int egrid = clite::deterministic() ? 1 : L * EMB_SEGS;
  EmbMp<true> mp{pids, max_pos, padding_idx};
  DISPATCH(dtype,
           hipLaunchKernelGGL((embed_bwd_kernel<bf16, true>), dim3(egrid), dim3(128), 0, st, ids, (const bf16*)d, dword, dpos, M / L, L, C, vocab, padding_idx, mp),
           hipLaunchKernelGGL((embed_bwd_kernel<float, true>), dim3(egrid), dim3(128), 0, st, ids, (const float*)d, dword, dpos, M / L, L, C, vocab, padding_idx, mp));
  return (int)hipGetLastError();
}

extern "C" int clite_mean_pool_fwd(int dtype, const void* h, const int64_t* mask, void* out, float* inv, int B, int L, int C, void* stream) {
  if (B <= 0 || L <= 0 || C <= 0 || C % 8 || !h || !mask || !out || !inv) return -1;
  int grid = ew_grid((size_t)B * (C / 8));
  hipStream_t st = (hipStream_t)stream;
  DISPATCH(dtype,
           hipLaunchKernelGGL(mean_pool_fwd_kernel<bf16>, dim3(grid), dim3(256), 0, st, (const bf16*)h, mask, (bf16*)out, inv, B, L, C),
           hipLaunchKernelGGL(mean_pool_fwd_kernel<float>, dim3(grid), dim3(256), 0, st, (const float*)h, mask, (float*)out, inv, B, L, C));
  return (int)hipGetLastError();
}

extern "C" int clite_mean_pool_bwd(int dtype, const void* dy, const int64_t* mask, const float* inv, void* dh, int B, int L, int C, void* stream) {
  if (B <= 0 || L <= 0 || C <= 0 || C % 8 || !dy || !mask || !inv || !dh) return -1;
  int grid = ew_grid((size_t)B * L * (C / 8));
  hipStream_t st = (hipStream_t)stream;
  DISPATCH(dtype,
           hipLaunchKernelGGL(mean_pool_bwd_kernel<bf16>, dim3(grid), dim3(256), 0, st, (const bf16*)dy, mask, inv, (bf16*)dh, B, L, C),
           hipLaunchKernelGGL(mean_pool_bwd_kernel<float>, dim3(grid), dim3(256), 0, st, (const float*)dy, mask, inv, (float*)dh, B, L, C));
  return (int)hipGetLastError();
}

extern "C" int clite_attention_causal_fwd(int dtype, const void* qkv, const int64_t* mask, void* ctx, int B, int L, int H, void* stream) {
  if (B <= 0 || L < 1 || L > AL_L || H <= 0 || !qkv || !ctx) return -1;
  hipStream_t st = (hipStream_t)stream;
  if (L > AT_L) {      // 33..128: one workgroup per (batch, head), a wave per 32-query tile over the key tiles up to its own
#define ALC_FWD(NT) hipLaunchKernelGGL(attention_causal_long_mfma_fwd_kernel<NT>, dim3(B * H), dim3(64 * NT), 0, st, (const bf16*)qkv, mask, (bf16*)ctx, B, L, H)
    DISPATCH(dtype,
             if (L <= 64) ALC_FWD(2); else if (L <= 96) ALC_FWD(3); else ALC_FWD(4),
             hipLaunchKernelGGL(attention_causal_long_fwd_kernel<float>, dim3(B * H), dim3(256), 0, st, (const float*)qkv, mask, (float*)ctx, B, L, H));
#undef ALC_FWD
    return (int)hipGetLastError();
  }
  DISPATCH(dtype,
           hipLaunchKernelGGL(attention_causal_mfma_fwd_kernel, dim3((B * H + 3) / 4), dim3(256), 0, st, (const bf16*)qkv, mask, (bf16*)ctx, B, L, H),
           hipLaunchKernelGGL(attention_causal_fwd_kernel<float>, dim3(B * H), dim3(64), 0, st, (const float*)qkv, mask, (float*)ctx, B, L, H));
  return (int)hipGetLastError();
}

extern "C" int clite_attention_causal_bwd(int dtype, const void* qkv, const int64_t* mask, const void* dctx, void* dqkv, int B, int L, int H, void* stream) {
  if (B <= 0 || L < 1 || L > AL_L || H <= 0 || !qkv || !dctx || !dqkv) return -1;
  hipStream_t st = (hipStream_t)stream;
  if (L > AT_L) {
#define ALC_BWD(NT) hipLaunchKernelGGL(attention_causal_long_mfma_bwd_kernel<NT>, dim3(B * H), dim3(64 * NT), 0, st, (const bf16*)qkv, mask, (const bf16*)dctx, (bf16*)dqkv, B, L, H)
    DISPATCH(dtype,
             if (L <= 64) ALC_BWD(2); else if (L <= 96) ALC_BWD(3); else ALC_BWD(4),
             hipLaunchKernelGGL(attention_causal_long_bwd_kernel<float>, dim3(B * H), dim3(256), 0, st, (const float*)qkv, mask, (const float*)dctx, (float*)dqkv, B, L, H));
#undef ALC_BWD
    return (int)hipGetLastError();
  }
  DISPATCH(dtype,
           hipLaunchKernelGGL(attention_causal_mfma_bwd_kernel, dim3((B * H + 1) / 2), dim3(128), 0, st, (const bf16*)qkv, mask, (const bf16*)dctx, (bf16*)dqkv, B, L, H),
           hipLaunchKernelGGL(attention_causal_bwd_kernel<float>, dim3(B * H), dim3(64), 0, st, (const float*)qkv, mask, (const float*)dctx, (float*)dqkv, B, L, H));
  return (int)hipGetLastError();
}

extern "C" int clite_embed_clip_fwd(int dtype, const int64_t* ids, const void* word, const void* pos, void* out, int M, int L, int C, int vocab, void* stream) {
  if (M <= 0 || L <= 0 || M % L || C <= 0 || C % 8 || vocab <= 0 || !ids || !word || !pos || !out) return -1;
  int grid = ew_grid((size_t)M * (C / 8));
  hipStream_t st = (hipStream_t)stream;
  DISPATCH(dtype,
           hipLaunchKernelGGL(embed_clip_fwd_kernel<bf16>, dim3(grid), dim3(256), 0, st, ids, (const bf16*)word, (const bf16*)pos, (bf16*)out, M, L, C, vocab),
           hipLaunchKernelGGL(embed_clip_fwd_kernel<float>, dim3(grid), dim3(256), 0, st, ids, (const float*)word, (const float*)pos, (float*)out, M, L, C, vocab));
  return (int)hipGetLastError();
}

extern "C" int clite_last_token_gather(int dtype, const void* x, const int64_t* mask, void* out, int32_t* idx, int B, int L, int C, void* stream) {
  if (B <= 0 || L <= 0 || C <= 0 || C % 8 || !x || !mask || !out || !idx) return -1;
  int grid = ew_grid((size_t)B * (C / 8));
  hipStream_t st = (hipStream_t)stream;
  DISPATCH(dtype,
           hipLaunchKernelGGL(last_token_gather_kernel<bf16>, dim3(grid), dim3(256), 0, st, (const bf16*)x, mask, (bf16*)out, idx, B, L, C),
           hipLaunchKernelGGL(last_token_gather_kernel<float>, dim3(grid), dim3(256), 0, st, (const float*)x, mask, (float*)out, idx, B, L, C));
  return (int)hipGetLastError();
}

extern "C" int clite_last_token_scatter(int dtype, const void* d, const int32_t* idx, void* dx, int B, int L, int C, void* stream) {
  if (B <= 0 || L <= 0 || C <= 0 || C % 8 || !d || !idx || !dx) return -1;
  int grid = ew_grid((size_t)B * (C / 8));
  hipStream_t st = (hipStream_t)stream;
  DISPATCH(dtype,
           hipLaunchKernelGGL(last_token_scatter_kernel<bf16>, dim3(grid), dim3(256), 0, st, (const bf16*)d, idx, (bf16*)dx, B, L, C),
           hipLaunchKernelGGL(last_token_scatter_kernel<float>, dim3(grid), dim3(256), 0, st, (const float*)d, idx, (float*)dx, B, L, C));
  return (int)hipGetLastError();
}

extern "C" int clite_tanh_bwd(int dtype, const void* dy, const void* y, void* out, uint64_t n, void* stream) {
  if (!dy || !y || !out || n % 8) return -1;
  int grid = ew_grid(n / 8);
  hipStream_t st = (hipStream_t)stream;
  DISPATCH(dtype,
           hipLaunchKernelGGL(tanh_bwd_kernel<bf16>, dim3(grid), dim3(256), 0, st, (const bf16*)dy, (const bf16*)y, (bf16*)out, (size_t)(n / 8)),
           hipLaunchKernelGGL(tanh_bwd_kernel<float>, dim3(grid), dim3(256), 0, st, (const float*)dy, (const float*)y, (float*)out, (size_t)(n / 8)));
  return (int)hipGetLastError();
}
