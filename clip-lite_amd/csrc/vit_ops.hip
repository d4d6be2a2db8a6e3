// Kernels of the ViT image encoder outside the GEMMs, LayerNorm and attention (torchvision.models.vit_b_32 / vit_b_16: conv_proj as a
// patch GEMM, class token + position embedding, class-token read-out): the patch matrix of an NCHW image, the token assembly and its backward,
// and the gather / scatter of the class rows around the final LayerNorm; and patch dropout (FLIP): the per-sample choice of the kept patches
// and the three kernels above restricted to them. All but the choice stream: every element is read and written once,
// 16 bytes per lane and access. No float atomics anywhere: the reductions over the batch are owned by one thread each and run in index order.
#include "vec.h"
#include "rng.h"
#include "clite.h"

using namespace clite;

namespace {

int ew_grid(size_t total, int block = 256) {
  size_t g = (total + block - 1) / block;
  return (int)(g < 8192 ? (g ? g : 1) : 8192);
}

// out[(b * Ph + ph) * Pw + pw][(c * p + i) * p + j] = img[b][c][ph * p + i][pw * p + j]: one thread per 8 consecutive j (p % 8 == 0, so the
// 8 stay inside one image row): 32 contiguous bytes in, 16 (bf16) or 32 (f32) contiguous bytes out; consecutive threads write consecutive chunks
// of the output and read runs of p floats of the image.
template <typename T>
__global__ __launch_bounds__(256) void vit_patchify_kernel(const float* img, T* out, int B, int H, int W, int p) {
  const int Ph = H / p, Pw = W / p, jc = p / 8;
  const int kchunks = 3 * p * jc;                              // 8-element chunks per output row
  const size_t total = (size_t)B * Ph * Pw * kchunks;
  for (size_t i8 = (size_t)blockIdx.x * 256 + threadIdx.x; i8 < total; i8 += (size_t)gridDim.x * 256) {
    const int k = (int)(i8 % kchunks);
    const size_t row = i8 / kchunks;
    const int j0 = (k % jc) * 8, i = (k / jc) % p, c = k / (jc * p);
    const int pw = (int)(row % Pw), ph = (int)((row / Pw) % Ph);
    const size_t b = row / ((size_t)Pw * Ph);
    float v[8];
    load8_nt(img + ((b * 3 + c) * H + (size_t)ph * p + i) * W + (size_t)pw * p + j0, v);
    store8(out + row * ((size_t)kchunks * 8) + (size_t)k * 8, v);
  }
}

// s0[b][0] = cls + pos[0]; s0[b][1 + t] = e[b][t] + pos[1 + t]; rows of C elements, L = P + 1 tokens. One thread per 8 columns of one token.
template <typename T>
__global__ __launch_bounds__(256) void vit_tokens_fwd_kernel(const T* e, const T* cls, const T* pos, T* s0, int B, int P, int C) {
  const int nchunk = C / 8, L = P + 1;
  const size_t total = (size_t)B * L * nchunk;
  for (size_t i8 = (size_t)blockIdx.x * 256 + threadIdx.x; i8 < total; i8 += (size_t)gridDim.x * 256) {
    const int c = (int)(i8 % nchunk);
    const size_t row = i8 / nchunk;
    const int t = (int)(row % L);
    const size_t b = row / L;
    float a[8], q[8];
    if (t == 0) load8(cls + c * 8, a);
    else load8_nt(e + (b * P + (t - 1)) * C + c * 8, a);
    load8(pos + (size_t)t * C + c * 8, q);
#pragma unroll
    for (int k = 0; k < 8; ++k) a[k] += q[k];
    store8(s0 + row * C + c * 8, a);
  }
}

// Backward of the assembly: de[b][t - 1] = ds0[b][t] (t >= 1), dpos[t] += sum_b ds0[b][t], dcls += sum_b ds0[b][0]. One thread owns the slot
// (t, 8 columns) and walks the batch in index order, VT_UNROLL loads in flight (a batch of 128 is 8 rounds of memory latency), so that the sums
// depend neither on the launch nor on the mode.
constexpr int VT_UNROLL = 16;
template <typename T>
__global__ __launch_bounds__(64) void vit_tokens_bwd_kernel(const T* ds0, T* de, float* dpos, float* dcls, int B, int P, int C) {
  const int nchunk = C / 8, L = P + 1;
  const int slot = blockIdx.x * 64 + threadIdx.x;
  if (slot >= L * nchunk) return;
  const int c = slot % nchunk, t = slot / nchunk;
  float acc[8];
  zero8(acc);
  const size_t bstride = (size_t)L * C;
  const T* src = ds0 + (size_t)t * C + c * 8;
  T* dst = t > 0 ? de + (size_t)(t - 1) * C + c * 8 : nullptr;
  int b = 0;
  for (; b + VT_UNROLL <= B; b += VT_UNROLL) {
    Raw8<T> r[VT_UNROLL];
#pragma unroll
    for (int u = 0; u < VT_UNROLL; ++u) r[u].ld(src + (size_t)(b + u) * bstride);
#pragma unroll
    for (int u = 0; u < VT_UNROLL; ++u) {
      float v[8];
      r[u].get(v);
      if (dst) store8(dst + (size_t)(b + u) * P * C, v);
#pragma unroll
      for (int k = 0; k < 8; ++k) acc[k] += v[k];
    }
  }
  for (; b < B; ++b) {
    float v[8];
    load8(src + (size_t)b * bstride, v);
    if (dst) store8(dst + (size_t)b * P * C, v);
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] += v[k];
  }
  if (dpos) {
    float g[8];
    float* o = dpos + (size_t)t * C + c * 8;
    load8(o, g);
#pragma unroll
    for (int k = 0; k < 8; ++k) g[k] += acc[k];
    store8(o, g);
  }
  if (t == 0 && dcls) {
    float g[8];
    load8(dcls + c * 8, g);
#pragma unroll
    for (int k = 0; k < 8; ++k) g[k] += acc[k];
    store8(dcls + c * 8, g);
  }
}

// SCATTER = false: out[b] = x[b * L] (the class rows, for the final LayerNorm); true: x[b * L] = out[b], the other rows of x left as they are
template <typename T, bool SCATTER>
__global__ __launch_bounds__(256) void vit_class_rows_kernel(T* x, T* out, int B, int L, int C) {
  const int nchunk = C / 8;
  const size_t total = (size_t)B * nchunk;
  for (size_t i8 = (size_t)blockIdx.x * 256 + threadIdx.x; i8 < total; i8 += (size_t)gridDim.x * 256) {
    const int c = (int)(i8 % nchunk);
    const size_t b = i8 / nchunk;
    T* full = x + b * L * C + c * 8;
    T* row = out + b * C + c * 8;
    float v[8];
    load8(SCATTER ? row : full, v);
    store8(SCATTER ? full : row, v);
  }
}

// ---------------------------------------------------------------------------------------------------- patch dropout (FLIP)
// The kept patches of one sample: key[t] = the 24-bit uniform of element b * Ppad + t of the (seed, site) stream (Ppad = P rounded up to 4, so a
// sample starts on a Philox call), rank[t] = #{u : key[u] < key[t] or (key[u] == key[t] and u < t)}, kept iff rank < Kk; idx lists the kept t
// ascending, inv[t] = position of t in idx or -1. One wave per sample, lane l owns the patches l and l + 64; keys and keep flags in LDS, read
// as broadcasts (every lane reads the same u). Latency-bound and tiny: P <= 128 is 4 x 2 x 128 LDS reads per lane.
constexpr int VT_MAXP = 128;
__global__ __launch_bounds__(64) void vit_keep_indices_kernel(int32_t* idx, int32_t* inv, int P, int Kk, uint64_t seed, uint32_t site) {
  __shared__ float key[VT_MAXP];
  __shared__ int kept[VT_MAXP];
  seed_resolve(seed, site);
  const int lane = threadIdx.x, b = blockIdx.x;
  const int Ppad = (P + 3) & ~3;
  if (lane * 4 < Ppad) {
    float u[4];
    rng_uniform4(seed, site, (uint64_t)b * Ppad + lane * 4, u);
#pragma unroll
    for (int e = 0; e < 4; ++e) key[lane * 4 + e] = u[e];
  }
  __syncthreads();
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int t = lane + 64 * h;
    if (t < P) {
      const float kt = key[t];
      int rank = 0;
      for (int u = 0; u < P; ++u) {
        const float ku = key[u];
        rank += (ku < kt || (ku == kt && u < t)) ? 1 : 0;
      }
      kept[t] = rank < Kk ? 1 : 0;
    }
  }
  __syncthreads();
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int t = lane + 64 * h;
    if (t < P) {
      int k = 0;
      for (int u = 0; u < t; ++u) k += kept[u];
      const bool mine = kept[t] != 0;
      inv[(size_t)b * P + t] = mine ? k : -1;
      if (mine) idx[(size_t)b * Kk + k] = t;
    }
  }
}

// vit_patchify_kernel on the kept patches: out row b * Kk + k is the patch idx[b][k]; the dropped share of the image is never read
template <typename T>
__global__ __launch_bounds__(256) void vit_patchify_keep_kernel(const float* img, const int32_t* idx, T* out, int B, int H, int W, int p, int Kk) {
  const int Pw = W / p, P = (H / p) * Pw, jc = p / 8;
  const int kchunks = 3 * p * jc;
  const size_t total = (size_t)B * Kk * kchunks;
  for (size_t i8 = (size_t)blockIdx.x * 256 + threadIdx.x; i8 < total; i8 += (size_t)gridDim.x * 256) {
    const int k = (int)(i8 % kchunks);
    const size_t row = i8 / kchunks;
    const int t = idx[row];
    if ((unsigned)t >= (unsigned)P) continue;      // (an index outside the image: the row is left as it is, nothing is read)
    const int j0 = (k % jc) * 8, i = (k / jc) % p, c = k / (jc * p);
    const int pw = t % Pw, ph = t / Pw;
    const size_t b = row / Kk;
    float v[8];
    load8_nt(img + ((b * 3 + c) * H + (size_t)ph * p + i) * W + (size_t)pw * p + j0, v);
    store8(out + row * ((size_t)kchunks * 8) + (size_t)k * 8, v);
  }
}

// s0[b][0] = cls + pos[0]; s0[b][1 + k] = e[b][k] + pos[1 + idx[b][k]]: L' = Kk + 1 tokens, pos has all P + 1 rows
template <typename T>
__global__ __launch_bounds__(256) void vit_tokens_keep_fwd_kernel(const T* e, const T* cls, const T* pos, const int32_t* idx, T* s0, int B, int P, int Kk,
                                                                  int C) {
  const int nchunk = C / 8, L = Kk + 1;
  const size_t total = (size_t)B * L * nchunk;
  for (size_t i8 = (size_t)blockIdx.x * 256 + threadIdx.x; i8 < total; i8 += (size_t)gridDim.x * 256) {
    const int c = (int)(i8 % nchunk);
    const size_t row = i8 / nchunk;
    const int k = (int)(row % L);
    const size_t b = row / L;
    float a[8], q[8];
    int t = 0;
    if (k == 0) load8(cls + c * 8, a);
    else {
      const int ti = idx[b * Kk + (k - 1)];
      if ((unsigned)ti >= (unsigned)P) continue;      // (an index outside the sequence: the row is left as it is)
      t = 1 + ti;
      load8_nt(e + (b * Kk + (k - 1)) * C + c * 8, a);
    }
    load8(pos + (size_t)t * C + c * 8, q);
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] += q[j];
    store8(s0 + row * C + c * 8, a);
  }
}

// Backward of that assembly. One thread owns the slot (position tp of the FULL sequence, 8 columns) and walks the batch in index order, as
// vit_tokens_bwd_kernel does: tp = 0 sums row 0 of every sample into dpos[0] and dcls; tp = 1 + t looks up k = inv[b][t] and, where sample b kept
// the patch, copies ds0[b][1 + k] to de[b][k] and adds it (every row of de has exactly one owner). The inv entries of a round are read one
// round ahead, so the VT_UNROLL row loads of a round go out together, their addresses already in registers. Nothing in a round branches or
// selects: rows go through buffer loads and stores whose offset is out of range for a dropped patch - the load then returns zeros without
// touching memory (adding +0 leaves the f32 sum as it is, bit for bit: it starts at +0 and a sum is -0 only if both terms are), the store is
// dropped. One wave per CU leaves the round's instruction count exposed: with the copy under `if` and the sum under a select it was 21.6 us
// at B = 128, P = 49, Kk = 24, and is 14.4 as it stands. A position nobody kept leaves its dpos row untouched.
template <typename T>
__global__ __launch_bounds__(64) void vit_tokens_keep_bwd_kernel(const T* ds0, const int32_t* inv, T* de, float* dpos, float* dcls, int B, int P, int Kk,
                                                                 int C) {
  const int nchunk = C / 8, L = Kk + 1;
  const int slot = blockIdx.x * 64 + threadIdx.x;
  if (slot >= (P + 1) * nchunk) return;
  const int c = slot % nchunk, tp = slot / nchunk;
  float acc[8];
  zero8(acc);
  bool any = false;
  const size_t bstride = (size_t)L * C;
  const T* src = ds0 + c * 8;
  const rsrc_t srcr = make_rsrc(ds0, (uint32_t)((size_t)B * L * C * sizeof(T)));          // (the launcher refuses tensors of 0xF0000000 bytes or more)
  const rsrc_t dst = make_rsrc(de, (uint32_t)((size_t)B * Kk * C * sizeof(T)));
  const uint32_t dcol = (uint32_t)(c * 8 * sizeof(T)), drow = (uint32_t)(C * sizeof(T));
  // the class position (tp = 0) reads row 0 of every sample and copies nothing; it walks the inv column of patch 0 like its neighbours, unused
  const bool cls = tp == 0;
  const int32_t* iv = inv + (cls ? 0 : tp - 1);          // iv[b * P]
  const int last = B - 1;
  int kn[VT_UNROLL];
#pragma unroll
  for (int u = 0; u < VT_UNROLL; ++u) kn[u] = iv[(size_t)(u < last ? u : last) * P];          // (clamped: entries past the batch are never used)
  int b = 0;
  for (; b + VT_UNROLL <= B; b += VT_UNROLL) {
    int k[VT_UNROLL];
    Raw8<T> r[VT_UNROLL];
    // the round's row loads first, all addresses in registers; then the next round's inv entries, branch-free, behind them in the queue
#pragma unroll
    for (int u = 0; u < VT_UNROLL; ++u) {
      k[u] = cls ? -1 : kn[u];
      const bool kept = (unsigned)k[u] < (unsigned)Kk;
      r[u].ldb(srcr, cls || kept ? (uint32_t)((b + u) * L + 1 + k[u]) * drow + dcol : OOB_OFF);
    }
#pragma unroll
    for (int u = 0; u < VT_UNROLL; ++u) {
      const int bn = b + VT_UNROLL + u;
      kn[u] = iv[(size_t)(bn < last ? bn : last) * P];
    }
    // the copies, straight from the raw registers, and the sums, in index order
#pragma unroll
    for (int u = 0; u < VT_UNROLL; ++u) {
      float v[8];
      r[u].get(v);
      const bool kept = (unsigned)k[u] < (unsigned)Kk;
      r[u].stb(dst, kept ? (uint32_t)((b + u) * Kk + k[u]) * drow + dcol : OOB_OFF);
      any |= cls || kept;
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] += v[j];
    }
  }
#pragma unroll
  for (int u = 0; u < VT_UNROLL - 1; ++u) {          // the tail, one row at a time (unrolled: kn stays in registers)
    const int k = cls ? -1 : kn[u];
    if (b + u >= B || (!cls && (k < 0 || k >= Kk))) continue;
    float v[8];
    load8(src + (size_t)(b + u) * bstride + (size_t)(cls ? 0 : 1 + k) * C, v);
    if (!cls) store8(de + ((size_t)(b + u) * Kk + k) * C + c * 8, v);
    any = true;
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] += v[j];
  }
  if (!any) return;
  if (dpos) {
    float g[8];
    float* o = dpos + (size_t)tp * C + c * 8;
    load8(o, g);
#pragma unroll
    for (int j = 0; j < 8; ++j) g[j] += acc[j];
    store8(o, g);
  }
  if (tp == 0 && dcls) {
    float g[8];
    load8(dcls + c * 8, g);
#pragma unroll
    for (int j = 0; j < 8; ++j) g[j] += acc[j];
    store8(dcls + c * 8, g);
  }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

#define DISPATCH(dtype, CALL_BF16, CALL_F32) \
  if ((dtype) == CLITE_BF16) { CALL_BF16; } else if ((dtype) == CLITE_F32) { CALL_F32; } else return -1;

extern "C" int clite_vit_patchify(int dtype, const float* img, void* out, int B, int H, int W, int p, void* stream) {
  if (B <= 0 || H <= 0 || W <= 0 || p < 8 || p % 8 || H % p || W % p || !img || !out || !aligned16(img) || !aligned16(out)) return -1;
  const size_t chunks = (size_t)B * (H / p) * (W / p) * 3 * p * (p / 8);
  int grid = ew_grid(chunks);
  hipStream_t st = (hipStream_t)stream;
  DISPATCH(dtype,
           hipLaunchKernelGGL(vit_patchify_kernel<bf16>, dim3(grid), dim3(256), 0, st, img, (bf16*)out, B, H, W, p),
           hipLaunchKernelGGL(vit_patchify_kernel<float>, dim3(grid), dim3(256), 0, st, img, (float*)out, B, H, W, p));
  return (int)hipGetLastError();
}

extern "C" int clite_vit_tokens_fwd(int dtype, const void* e, const void* cls, const void* pos, void* s0, int B, int P, int C, void* stream) {
  if (B <= 0 || P <= 0 || C <= 0 || C % 8 || !e || !cls || !pos || !s0 || !aligned16(e) || !aligned16(cls) || !aligned16(pos) || !aligned16(s0))
    return -1;
  int grid = ew_grid((size_t)B * (P + 1) * (C / 8));
  hipStream_t st = (hipStream_t)stream;
  DISPATCH(dtype,
           hipLaunchKernelGGL(vit_tokens_fwd_kernel<bf16>, dim3(grid), dim3(256), 0, st, (const bf16*)e, (const bf16*)cls, (const bf16*)pos, (bf16*)s0, B, P, C),
           hipLaunchKernelGGL(vit_tokens_fwd_kernel<float>, dim3(grid), dim3(256), 0, st, (const float*)e, (const float*)cls, (const float*)pos, (float*)s0, B, P, C));
  return (int)hipGetLastError();
}

extern "C" int clite_vit_tokens_bwd(int dtype, const void* ds0, void* de, float* dpos, float* dcls, int B, int P, int C, void* stream) {
  if (B <= 0 || P <= 0 || C <= 0 || C % 8 || !ds0 || !de || !aligned16(ds0) || !aligned16(de) || !aligned16(dpos) || !aligned16(dcls)) return -1;
  const int slots = (P + 1) * (C / 8);
  int grid = (slots + 63) / 64;
  hipStream_t st = (hipStream_t)stream;
  DISPATCH(dtype,
           hipLaunchKernelGGL(vit_tokens_bwd_kernel<bf16>, dim3(grid), dim3(64), 0, st, (const bf16*)ds0, (bf16*)de, dpos, dcls, B, P, C),
           hipLaunchKernelGGL(vit_tokens_bwd_kernel<float>, dim3(grid), dim3(64), 0, st, (const float*)ds0, (float*)de, dpos, dcls, B, P, C));
  return (int)hipGetLastError();
}

extern "C" int clite_vit_class_gather(int dtype, const void* x, void* out, int B, int L, int C, void* stream) {
  if (B <= 0 || L <= 0 || C <= 0 || C % 8 || !x || !out || !aligned16(x) || !aligned16(out)) return -1;
  int grid = ew_grid((size_t)B * (C / 8));
  hipStream_t st = (hipStream_t)stream;
  DISPATCH(dtype,
           hipLaunchKernelGGL((vit_class_rows_kernel<bf16, false>), dim3(grid), dim3(256), 0, st, (bf16*)x, (bf16*)out, B, L, C),
           hipLaunchKernelGGL((vit_class_rows_kernel<float, false>), dim3(grid), dim3(256), 0, st, (float*)x, (float*)out, B, L, C));
  return (int)hipGetLastError();
}

extern "C" int clite_vit_class_scatter(int dtype, const void* d, void* dx, int B, int L, int C, void* stream) {
  if (B <= 0 || L <= 0 || C <= 0 || C % 8 || !d || !dx || !aligned16(d) || !aligned16(dx)) return -1;
  int grid = ew_grid((size_t)B * (C / 8));
  hipStream_t st = (hipStream_t)stream;
  DISPATCH(dtype,
           hipLaunchKernelGGL((vit_class_rows_kernel<bf16, true>), dim3(grid), dim3(256), 0, st, (bf16*)dx, (bf16*)d, B, L, C),
           hipLaunchKernelGGL((vit_class_rows_kernel<float, true>), dim3(grid), dim3(256), 0, st, (float*)dx, (float*)d, B, L, C));
  return (int)hipGetLastError();
}

extern "C" int clite_vit_keep_indices(int32_t* idx, int32_t* inv, int B, int P, int Kk, uint64_t seed, uint32_t site, void* stream) {
  if (B <= 0 || P <= 0 || P > VT_MAXP || Kk < 1 || Kk > P || !idx || !inv) return -1;
  if ((site & CLITE_SEED_INDIRECT) && (!seed || (seed & 7))) return -1;
  hipLaunchKernelGGL(vit_keep_indices_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, idx, inv, P, Kk, seed, site);
  return (int)hipGetLastError();
}

extern "C" int clite_vit_patchify_keep(int dtype, const float* img, const int32_t* idx, void* out, int B, int H, int W, int p, int Kk, void* stream) {
  if (B <= 0 || H <= 0 || W <= 0 || p < 8 || p % 8 || H % p || W % p || !img || !idx || !out || !aligned16(img) || !aligned16(out)) return -1;
  if (Kk < 1 || Kk > (H / p) * (W / p)) return -1;
  const size_t chunks = (size_t)B * Kk * 3 * p * (p / 8);
  int grid = ew_grid(chunks);
  hipStream_t st = (hipStream_t)stream;
  DISPATCH(dtype,
           hipLaunchKernelGGL(vit_patchify_keep_kernel<bf16>, dim3(grid), dim3(256), 0, st, img, idx, (bf16*)out, B, H, W, p, Kk),
           hipLaunchKernelGGL(vit_patchify_keep_kernel<float>, dim3(grid), dim3(256), 0, st, img, idx, (float*)out, B, H, W, p, Kk));
  return (int)hipGetLastError();
}

extern "C" int clite_vit_tokens_keep_fwd(int dtype, const void* e, const void* cls, const void* pos, const int32_t* idx, void* s0, int B, int P, int Kk,
                                         int C, void* stream) {
  if (B <= 0 || P <= 0 || Kk < 1 || Kk > P || C <= 0 || C % 8 || !e || !cls || !pos || !idx || !s0 || !aligned16(e) || !aligned16(cls) ||
      !aligned16(pos) || !aligned16(s0))
    return -1;
  int grid = ew_grid((size_t)B * (Kk + 1) * (C / 8));
  hipStream_t st = (hipStream_t)stream;
  DISPATCH(dtype,
           hipLaunchKernelGGL(vit_tokens_keep_fwd_kernel<bf16>, dim3(grid), dim3(256), 0, st, (const bf16*)e, (const bf16*)cls, (const bf16*)pos, idx, (bf16*)s0, B, P, Kk, C),
           hipLaunchKernelGGL(vit_tokens_keep_fwd_kernel<float>, dim3(grid), dim3(256), 0, st, (const float*)e, (const float*)cls, (const float*)pos, idx, (float*)s0, B, P, Kk, C));
  return (int)hipGetLastError();
}

extern "C" int clite_vit_tokens_keep_bwd(int dtype, const void* ds0, const int32_t* inv, void* de, float* dpos, float* dcls, int B, int P, int Kk, int C,
                                         void* stream) {
  if (B <= 0 || P <= 0 || Kk < 1 || Kk > P || C <= 0 || C % 8 || !ds0 || !inv || !de || !aligned16(ds0) || !aligned16(de) || !aligned16(dpos) ||
      !aligned16(dcls))
    return -1;
  if ((size_t)B * (Kk + 1) * C * 4 >= RSRC_WHOLE) return -1;          // ds0 and de are addressed through one buffer resource each
  const int slots = (P + 1) * (C / 8);
  int grid = (slots + 63) / 64;
  hipStream_t st = (hipStream_t)stream;
  DISPATCH(dtype,
           hipLaunchKernelGGL(vit_tokens_keep_bwd_kernel<bf16>, dim3(grid), dim3(64), 0, st, (const bf16*)ds0, inv, (bf16*)de, dpos, dcls, B, P, Kk, C),
           hipLaunchKernelGGL(vit_tokens_keep_bwd_kernel<float>, dim3(grid), dim3(64), 0, st, (const float*)ds0, inv, (float*)de, dpos, dcls, B, P, Kk, C));
  return (int)hipGetLastError();
}
