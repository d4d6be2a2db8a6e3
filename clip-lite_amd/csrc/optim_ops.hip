// What surrounds the parameter update (update_ops.hip) in the train step: the squared gradient norm of global-norm clipping
// (torch.nn.utils.clip_grad_norm_, reference train.py:222), the bf16 copy of a whole buffer, the transposed bf16 weight copies of the
// input-gradient GEMMs, and the slice sum of the data-parallel gradient exchange. Pure HBM streaming.
#include "vec.h"
#include "clite.h"

using namespace clite;

namespace {

// Squared gradient norm in two fixed-order stages: every workgroup stores ONE partial (plain store, its own slot), then a single workgroup
// folds the partials in slot order. No float atomics: the result is a pure function of the data, so every data-parallel rank derives the
// same clip factor from the same all-reduced gradients and the replicas stay bit-identical (torch's clip_grad_norm_ has that property;
// an atomically accumulated norm differs in the last bit from rank to rank, and BatchNorm amplifies such differences step after step).
constexpr int SUMSQ_MAX_GRID = 1024;
__global__ __launch_bounds__(256) void sumsq_partial_kernel(const float* x, size_t n, float* partials) {
  __shared__ float red[4];
  float s = 0.f;
  size_t n4 = n / 4;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    f32x4 v = __builtin_nontemporal_load((const f32x4*)(x + i * 4));
    s += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0)
    for (size_t i = n4 * 4; i < n; ++i) s += x[i] * x[i];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}
__global__ __launch_bounds__(256) void sumsq_final_kernel(const float* partials, int n, float* out) {
  __shared__ float red[4];
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) s += partials[i];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) out[0] += (red[0] + red[1]) + (red[2] + red[3]);      // `out` is pre-zeroed by contract; += keeps the accumulate semantics
}

__global__ __launch_bounds__(256) void cast_bf16_kernel(const float* src, bf16* dst, size_t n) {
  size_t n8 = n / 8;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += (size_t)gridDim.x * 256) {
    float v[8];
    load8(src + i * 8, v);
    store8(dst + i * 8, v);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0)
    for (size_t i = n8 * 8; i < n; ++i) dst[i] = f2bf(src[i]);
}

// Transposed bf16 weight copies for the input-gradient GEMMs. A dgrad contracts over the OUTPUT features, the slow index of a weight stored
// [out][in]: its weight operand would be an XC image (k-rows strided, ds_read_b64_tr_b16 fragments), which the 8-wave kernels stage 10-25 %
// slower than the k-contiguous form (tools/probe_tiles.py: 3840 x 768 x 3072 nn 41 us, the same product as nt 31). The weights change once
// per step, so one grouped launch re-derives [in][out] copies (linear: [N][K] -> [K][N]; conv: [K][R][S][C] -> [C][R][S][K], i.e. R*S
// matrices [K][C] -> [C][K] with row strides R*S*C / R*S*K) and every dgrad runs as a forward-form GEMM. 64 x 64 tiles through LDS
// (odd word pitch: conflict-free both ways), 16-byte global accesses on both sides.
__global__ __launch_bounds__(256) void transpose_weights_kernel(const bf16* __restrict__ src, bf16* __restrict__ dst, const clite_transpose_item* __restrict__ items,
                                                                 int n_items) {
  __shared__ uint16_t tile[64][66];
  int lo = 0, hi = n_items - 1;              // item whose [first_tile, first_tile + tiles) holds this workgroup (block-uniform binary search)
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (items[mid].first_tile <= blockIdx.x) lo = mid; else hi = mid - 1;
  }
  const clite_transpose_item it = items[lo];
  const uint32_t t = blockIdx.x - it.first_tile;
  const uint32_t tiles_c = (it.cols + 63) / 64, tiles_r = (it.rows + 63) / 64;
  const uint32_t b = t / (tiles_r * tiles_c), tr = (t / tiles_c) % tiles_r, tc = t % tiles_c;
  const bf16* s0 = src + it.src_off + (size_t)b * it.src_bstride;
  bf16* d0 = dst + it.dst_off + (size_t)b * it.dst_bstride;
  const int tid = threadIdx.x, c8 = (tid & 7) * 8, r0 = tid >> 3;       // 8 chunks of 8 elements per tile row, 32 rows per sweep
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const uint32_t r = tr * 64 + r0 + 32 * h, c = tc * 64 + c8;
    Chunk16 ch;
    ch.u = u32x4{0u, 0u, 0u, 0u};
    if (r < it.rows && c < it.cols) ch.u = *(const u32x4*)(s0 + (size_t)r * it.src_ld + c);        // cols % 8 == 0 (checked by the launcher)
    const uint16_t* e = (const uint16_t*)&ch;
#pragma unroll
    for (int k = 0; k < 8; ++k) tile[r0 + 32 * h][c8 + k] = e[k];
  }
  __syncthreads();
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const uint32_t c = tc * 64 + r0 + 32 * h, r = tr * 64 + c8;          // output row = input column
    if (c < it.cols && r < it.rows) {
      Chunk16 ch;
      uint16_t* e = (uint16_t*)&ch;
#pragma unroll
      for (int k = 0; k < 8; ++k) e[k] = tile[c8 + k][r0 + 32 * h];
      *(u32x4*)(d0 + (size_t)c * it.dst_ld + r) = ch.u;                                             // rows % 8 == 0
    }
  }
}

// dst[i] = src[i] + src[stride + i] + ... + src[(slices - 1) * stride + i], summed in slice order (every rank of a data-parallel job reduces
// ITS chunk of the gradient arena this way, so the order is fixed by construction)
__global__ __launch_bounds__(256) void sum_slices_kernel(const float* __restrict__ src, int slices, size_t stride, size_t n, float* __restrict__ dst) {
  const size_t n4 = n / 4;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    f32x4 a = *(const f32x4*)(src + i * 4);
    for (int s = 1; s < slices; ++s) {
      const f32x4 b = *(const f32x4*)(src + (size_t)s * stride + i * 4);
      a[0] += b[0]; a[1] += b[1]; a[2] += b[2]; a[3] += b[3];
    }
    *(f32x4*)(dst + i * 4) = a;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const size_t i = n4 * 4 + threadIdx.x;
    float a = src[i];
    for (int s = 1; s < slices; ++s) a += src[(size_t)s * stride + i];
    dst[i] = a;
  }
}

}  // namespace

extern "C" int clite_sum_slices(const float* src, int slices, uint64_t stride, uint64_t n, float* dst, void* stream) {
  if (!src || !dst || slices < 1 || stride % 4 || ((uintptr_t)src | (uintptr_t)dst) % 16) return -1;
  if (n == 0) return 0;
  size_t g = (n / 4 + 255) / 256;
  int grid = (int)(g < 2048 ? (g ? g : 1) : 2048);
  hipLaunchKernelGGL(sum_slices_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, src, slices, (size_t)stride, (size_t)n, dst);
  return (int)hipGetLastError();
}

extern "C" int clite_sumsq(const float* x, uint64_t n, float* out, float* partials, int n_partials, void* stream) {
  if (!x || !out || !partials || n_partials < 1) return -1;
  size_t g = (n / 4 + 255) / 256;
  int grid = (int)(g < (size_t)SUMSQ_MAX_GRID ? (g ? g : 1) : SUMSQ_MAX_GRID);
  if (grid > n_partials) grid = n_partials;
  hipLaunchKernelGGL(sumsq_partial_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, (size_t)n, partials);
  hipLaunchKernelGGL(sumsq_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)partials, grid, out);
  return (int)hipGetLastError();
}

extern "C" int clite_cast_bf16(const float* src, void* dst, uint64_t n, void* stream) {
  if (!src || !dst) return -1;
  size_t g = (n / 8 + 255) / 256;
  int grid = (int)(g < 4096 ? (g ? g : 1) : 4096);
  hipLaunchKernelGGL(cast_bf16_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, src, (bf16*)dst, (size_t)n);
  return (int)hipGetLastError();
}

extern "C" int clite_transpose_weights(const void* src, void* dst, const clite_transpose_item* items_dev, int n_items, uint32_t total_tiles, void* stream) {
  if (!src || !dst || !items_dev || n_items <= 0 || total_tiles == 0) return -1;
  hipLaunchKernelGGL(transpose_weights_kernel, dim3(total_tiles), dim3(256), 0, (hipStream_t)stream, (const bf16*)src, (bf16*)dst, items_dev, n_items);
  return (int)hipGetLastError();
}

