// Downstream classification head: softmax cross-entropy over f32 logits with torch's ignore_index (reference linear_clf.py:188,
// nn.CrossEntropyLoss), top-k accuracy counters (reference utils/metrics.py:20-73 TopkAccuracy; zero_shot.py:155 torch.max) and the
// loss gradient w.r.t. the logits. One wave owns one row and streams it with 16-byte loads; reductions are wavefront shuffles (the same
// instruction set as loss_ops.hip). Each kernel reads the logits once and the backward writes dlogits once; at probe sizes (~1 MB) both
// take far longer than those bytes need: latency-bound (measurements in DESIGN.md §3.3b).
#include "vec.h"
#include "det.h"
#include "clite.h"

using namespace clite;

namespace {

constexpr int XU = 4;                       // 4-column chunks in flight per lane per iteration

// Online max / sum-of-exp of one lane's columns: (m, s) with s = sum exp(z - m). A lane starts, and an empty lane stays, at m = LSE_EMPTY, s = 0:
// the most negative FINITE float, not -inf, so that an element at -inf (a masked class, which nn.CrossEntropyLoss accepts anywhere but at the
// label) takes the second branch as exp(-inf - m) = 0 and contributes nothing; from m = -inf that difference was NaN. The first finite
// element replaces the start value through s = 0 * exp(m - v) + 1 = 1, and a logit equal to LSE_EMPTY itself adds exp(0) = 1 as it should.
constexpr float LSE_EMPTY = -3.402823466e+38f;
DEV void lse_merge(float& m, float& s, float v) {
  if (v > m) {
    s = s * expf(m - v) + 1.f;
    m = v;
  } else {
    s += expf(v - m);
  }
}

// lse[i] = logsumexp(z[i][0:C]); for every row whose label y is a class (labels -100, or outside [0, C), count nowhere):
// acc[0] += lse - z[y], acc[1] += [rank == 0], acc[2] += [rank < topk], acc[3] += 1 with rank = #{j: z_j > z_y} + #{j < y: z_j == z_y}
// (ties to the lower class index, as torch.max / topk on a sorted tie). Each wave sums its rows in registers and adds once at the end.
__global__ __launch_bounds__(64) void xent_fwd_kernel(const float* z, int ld, int B, int C, const int64_t* labels, int topk, float* lse, float* acc) {
  const int lane = threadIdx.x & 63;
  float a_loss = 0.f, a_top1 = 0.f, a_topk = 0.f, a_cnt = 0.f;
  for (int i = blockIdx.x; i < B; i += gridDim.x) {
    const float* row = z + (size_t)i * ld;
    const int64_t y64 = labels[i];
    const bool valid = y64 >= 0 && y64 < C;
    const int y = valid ? (int)y64 : 0;
    const float zy = valid ? row[y] : 0.f;
    float m = LSE_EMPTY, s = 0.f, rank = 0.f;
    for (int j0 = lane * 4; j0 < C; j0 += 64 * 4 * XU) {
      f32x4 v[XU];
#pragma unroll
      for (int u = 0; u < XU; ++u) {
        const int j = j0 + u * 256;
        v[u] = j < C ? *(const f32x4*)(row + j) : f32x4{0.f, 0.f, 0.f, 0.f};      // ld % 4 == 0 and j < C <= ld: the chunk is inside the row
      }
#pragma unroll
      for (int u = 0; u < XU; ++u) {
        const int j = j0 + u * 256;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (j + e < C) {
            const float x = v[u][e];
            lse_merge(m, s, x);
            rank += (x > zy || (x == zy && j + e < y)) ? 1.f : 0.f;
          }
        }
      }
    }
    const float M = wave_max(m);
    s = s * expf(m - M);                       // an empty or fully masked lane: s = 0 times a factor in [0, 1]
    const float S = wave_sum(s);
    const float r = wave_sum(rank);
    const float l = M + logf(S);
    if (lane == 0) lse[i] = l;
    if (valid) {
      a_loss += l - zy;
      a_top1 += r == 0.f ? 1.f : 0.f;
      a_topk += r < (float)topk ? 1.f : 0.f;
      a_cnt += 1.f;
    }
  }
  if (lane == 0 && a_cnt > 0.f) {
    atomic_add_f32(acc + 0, a_loss);
    atomic_add_f32(acc + 1, a_top1);
    atomic_add_f32(acc + 2, a_topk);
    atomic_add_f32(acc + 3, a_cnt);
  }
}

// dz[i][j] = gout / count * (exp(z_ij - lse_i) - [j == y_i]) for i < B with a counted label and j < C; zero elsewhere in [Bp][ldd]
template <typename T>
__global__ __launch_bounds__(64) void xent_bwd_kernel(const float* z, int ld, int B, int Bp, int C, const float* lse, const int64_t* labels,
                                                      const float* acc, const float* gout, T* dz, int ldd) {
  const int lane = threadIdx.x & 63;
  const float cnt = acc[3];
  const float g = cnt > 0.f ? gout[0] / cnt : 0.f;
  for (int i = blockIdx.x; i < Bp; i += gridDim.x) {
    int y = -1;
    float l = 0.f;
    if (i < B) {
      const int64_t y64 = labels[i];
      if (y64 >= 0 && y64 < C) {
        y = (int)y64;
        l = lse[i];
      }
    }
    const float* row = z + (size_t)i * ld;
    T* out = dz + (size_t)i * ldd;
    for (int j0 = lane * 8; j0 < ldd; j0 += 64 * 8) {
      float o[8];
      if (y >= 0 && j0 < C) {
        float v[8];
        f32x4 a = *(const f32x4*)(row + j0);
        f32x4 b = j0 + 4 < C ? *(const f32x4*)(row + j0 + 4) : f32x4{0.f, 0.f, 0.f, 0.f};
        v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3]; v[4] = b[0]; v[5] = b[1]; v[6] = b[2]; v[7] = b[3];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int j = j0 + e;
          o[e] = j < C ? g * (expf(v[e] - l) - (j == y ? 1.f : 0.f)) : 0.f;
        }
      } else {
        zero8(o);
      }
      store8(out + j0, o);
    }
  }
}

}  // namespace

#define DISPATCH(dtype, CALL_BF16, CALL_F32) \
  if ((dtype) == CLITE_BF16) { CALL_BF16; } else if ((dtype) == CLITE_F32) { CALL_F32; } else return -1;

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

extern "C" int clite_xent_fwd(const float* logits, int ld, int B, int C, const int64_t* labels, int topk, float* lse, float* acc, void* stream) {
  if (B <= 0 || C < 1 || ld < C || ld % 4 || topk < 1 || !logits || !labels || !lse || !acc || !aligned16(logits)) return -1;
  int grid = B < 8192 ? B : 8192;
  if (clite::deterministic()) grid = 1;          // one wave: every sum in row order, one contribution per accumulator (det.h)
  hipLaunchKernelGGL(xent_fwd_kernel, dim3(grid), dim3(64), 0, (hipStream_t)stream, logits, ld, B, C, labels, topk, lse, acc);
  return (int)hipGetLastError();
}

extern "C" int clite_xent_bwd(int dtype, const float* logits, int ld, int B, int Bp, int C, const float* lse, const int64_t* labels, const float* acc,
                              const float* gout, void* dlogits, int ldd, void* stream) {
  if (B <= 0 || Bp < B || C < 1 || ld < C || ld % 4 || ldd < C || ldd % 8 || !logits || !lse || !labels || !acc || !gout || !dlogits ||
      !aligned16(logits) || !aligned16(dlogits))
    return -1;
  int grid = Bp < 8192 ? Bp : 8192;
  hipStream_t st = (hipStream_t)stream;
  DISPATCH(dtype,
           hipLaunchKernelGGL(xent_bwd_kernel<bf16>, dim3(grid), dim3(64), 0, st, logits, ld, B, Bp, C, lse, labels, acc, gout, (bf16*)dlogits, ldd),
           hipLaunchKernelGGL(xent_bwd_kernel<float>, dim3(grid), dim3(64), 0, st, logits, ld, B, Bp, C, lse, labels, acc, gout, (float*)dlogits, ldd));
  return (int)hipGetLastError();
}
