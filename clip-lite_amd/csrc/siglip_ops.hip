// Pairwise sigmoid loss of SigLIP (Zhai et al. 2023, "Sigmoid Loss for Language Image Pre-Training", Algorithm 1) on the B x B cosine matrix
// C[i][j] = <a_i, b_j> of the L2-normalised projections (one clite_gemm_nt, as for InfoNCE). With t = exp(temperature), z_ij = +1 on the diagonal
// and -1 elsewhere:
//   x_ij = t * C[i][j] + bias        L = 1/B * sum_ij softplus(-z_ij x_ij)        dL/dx_ij = -z_ij * sigmoid(-z_ij x_ij) / B
// Every pair is its own binary problem: nothing is normalised over a row or a column, so forward keeps nothing for backward (backward recomputes
// x from C) and each kernel reads C once. One wave per row, four waves per workgroup; a lane streams eight consecutive columns per trip.
// No float atomics: a wave stores its row's partial sums, and a second one-wave launch adds them in one fixed order (lane-strided, then the wave
// reduction), the two-stage scheme of clite_lars_norms. The result does not depend on the grid, so two runs give the same bits in either mode.
#include "vec.h"
#include "clite.h"

using namespace clite;

// workgroups of the row kernels: 2048 x 4 waves is what 256 CUs hold at once; rows beyond that take another pass of the same waves. The
// wave-simulator build sets a small cap so that a few hundred rows already take a second pass.
#ifndef CLITE_SIGLIP_WGS
#define CLITE_SIGLIP_WGS 2048
#endif

namespace {

// overflow-free forms: e = exp(-|u|) is in (0, 1] for every finite u (|x| reaches 110 at t = 100, bias = -10)
// log(1 + e) for e in (0, 1]: w = 1 + e is rounded, w - 1 is exact (w in [1, 2]), and log(w) * e / (w - 1) takes the rounding back out; the
// hardware log and reciprocal (about 1 ulp each) in place of the library's log1pf, whose range handling made the forward kernel ALU-bound
DEV float rcp_fast(float x) {
#ifdef CLITE_WAVESIM_H
  return 1.f / x;
#else
  return __builtin_amdgcn_rcpf(x);
#endif
}
DEV float log1p_unit(float e) {
  float w = 1.f + e;
  return w == 1.f ? e : __logf(w) * (e * rcp_fast(w - 1.f));
}
DEV float softplus_stable(float u) { return fmaxf(u, 0.f) + log1p_unit(expf(-fabsf(u))); }
DEV float sigmoid_stable(float u) {
  float e = expf(-fabsf(u));
  return (u >= 0.f ? 1.f : e) * rcp_fast(1.f + e);
}

// columns j0 .. j0 + 7 of one row of C; whole 16-byte loads where the row allows them (ld % 4 == 0 keeps every row start aligned, and
// j0 + 8 <= ld keeps the load inside the row: it may take in padding columns, which the callers mask by j < B), single loads otherwise
DEV void load_cos8(const float* row, int j0, int B, int ld, bool vec_ok, float (&c)[8]) {
  if (vec_ok && j0 + 8 <= ld) {
    load8(row + j0, c);
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) c[e] = j0 + e < B ? row[j0 + e] : 0.f;
  }
}

__global__ __launch_bounds__(256) void siglip_fwd_kernel(const float* Cm, int ld, int B, const float* temperature, const float* bias, float* part) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float t = expf(temperature[0]), b = bias[0];
  const bool vec_ok = ld % 4 == 0;
  for (int i = blockIdx.x * (blockDim.x >> 6) + wave; i < B; i += gridDim.x * (blockDim.x >> 6)) {
    const float* row = Cm + (size_t)i * ld;
    float s = 0.f;
    for (int j0 = lane * 8; j0 < B; j0 += 64 * 8) {
      float c[8];
      load_cos8(row, j0, B, ld, vec_ok, c);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        int j = j0 + e;
        float x = t * c[e] + b;
        if (j < B) s += softplus_stable(i == j ? -x : x);
      }
    }
    s = wave_sum(s);
    if (lane == 0) part[i] = s / (float)B;
  }
}

// dC[i][j] = g * t * dL/dx_ij with g = gout * scale; part[i] = row i's share of dtemp (sum_j g dL/dx_ij * t C[i][j]), part[B + i] that of dbias
template <typename T>
__global__ __launch_bounds__(256) void siglip_bwd_kernel(const float* Cm, int ld, int B, const float* temperature, const float* bias, const float* gout,
                                                         float scale, T* dC, int ldd, float* part) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float t = expf(temperature[0]), b = bias[0];
  const float g = gout[0] * scale / (float)B;
  const bool vec_ok = ld % 4 == 0;
  for (int i = blockIdx.x * (blockDim.x >> 6) + wave; i < B; i += gridDim.x * (blockDim.x >> 6)) {
    const float* row = Cm + (size_t)i * ld;
    float st = 0.f, sb = 0.f;
    for (int j0 = lane * 8; j0 < ldd; j0 += 64 * 8) {
      float c[8], o[8];
      load_cos8(row, j0, B, ld, vec_ok, c);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        int j = j0 + e;
        float tc = t * c[e], x = tc + b;
        // -z sigmoid(-z x): -sigmoid(-x) on the diagonal, sigmoid(x) off it
        float d = g * (i == j ? -sigmoid_stable(-x) : sigmoid_stable(x));
        if (j >= B) d = 0.f;
        st += j < B ? d * tc : 0.f;
        sb += d;
        o[e] = d * t;
      }
      store8(dC + (size_t)i * ldd + j0, o);
    }
    st = wave_sum(st);
    sb = wave_sum(sb);
    if (lane == 0) {
      part[i] = st;
      part[B + i] = sb;
    }
  }
}

// one wave: lane l adds part[l], part[l + 64], ... in that order, then the wave reduction; a plain load-add-store onto the accumulator (the only
// writer of that address in the launch)
DEV float fold_wave(const float* part, int n, int lane) {
  float s = 0.f;
  for (int i = lane; i < n; i += 64) s += part[i];
  return wave_sum(s);
}
__global__ __launch_bounds__(64) void siglip_fold_kernel(const float* part, int B, float* out0, float* out1) {
  const int lane = threadIdx.x;
  if (out0) {
    float s = fold_wave(part, B, lane);
    if (lane == 0) out0[0] = out0[0] + s;
  }
  if (out1) {
    float s = fold_wave(part + B, B, lane);
    if (lane == 0) out1[0] = out1[0] + s;
  }
}

int row_grid(int B) {
  int grid = (B + 3) / 4;
  return grid > CLITE_SIGLIP_WGS ? CLITE_SIGLIP_WGS : grid;
}

}  // namespace

extern "C" int clite_siglip_fwd(const float* Cm, int ld, int B, const float* temperature, const float* bias, float* part, float* acc, void* stream) {
  if (B <= 0 || ld < B || !Cm || !temperature || !bias || !part || !acc) return -1;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(siglip_fwd_kernel, dim3(row_grid(B)), dim3(256), 0, st, Cm, ld, B, temperature, bias, part);
  hipLaunchKernelGGL(siglip_fold_kernel, dim3(1), dim3(64), 0, st, (const float*)part, B, acc, (float*)nullptr);
  return (int)hipGetLastError();
}

extern "C" int clite_siglip_bwd(int dtype, const float* Cm, int ld, int B, const float* temperature, const float* bias, const float* gout, float scale,
                                void* dC, int ldd, float* part, float* dtemp, float* dbias, void* stream) {
  if (B <= 0 || ld < B || ldd < B || ldd % 8 || !Cm || !temperature || !bias || !gout || !dC || !part) return -1;
  hipStream_t st = (hipStream_t)stream;
  const int grid = row_grid(B);
  if (dtype == CLITE_BF16) {
    hipLaunchKernelGGL(siglip_bwd_kernel<bf16>, dim3(grid), dim3(256), 0, st, Cm, ld, B, temperature, bias, gout, scale, (bf16*)dC, ldd, part);
  } else if (dtype == CLITE_F32) {
    hipLaunchKernelGGL(siglip_bwd_kernel<float>, dim3(grid), dim3(256), 0, st, Cm, ld, B, temperature, bias, gout, scale, (float*)dC, ldd, part);
  } else {
    return -1;
  }
  if (dtemp || dbias) hipLaunchKernelGGL(siglip_fold_kernel, dim3(1), dim3(64), 0, st, (const float*)part, B, dtemp, dbias);
  return (int)hipGetLastError();
}
