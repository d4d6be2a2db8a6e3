// LARS (layer-wise adaptive rate scaling) on the update path's item table (optim_ops.hip: sgd_step_kernel): SGD whose step for every adapted
// tensor is scaled by the trust ratio q = eta |p| / (|g'| + wd |p| + eps). A torchlars-style wrapper takes two .norm() launches per tensor
// (~720 for ResNet-50 + BERT-base) plus host logic no hipGraph can hold; here the per-tensor norms are two launches over the same table and the
// update is sgd_step_kernel's body with two of its scalars scaled by q. Pure HBM streaming: the norms read p and g once (8 B per element),
// the update moves what the SGD update moves.
#include "vec.h"
#include "clite.h"
#include "norm_fold.h"

using namespace clite;

namespace {

// Stage 1 of the per-tensor squared norms: one workgroup per item (the update kernel's decomposition, so the 30522 x 768 embedding is spread
// over 2862 workgroups, not streamed through one CU). Every workgroup of an adapted item stores ITS pair (sum p^2, sum g^2) with a plain store
// into its own slot of `partials`; no float atomics (sumsq_partial_kernel's reasoning: a pure function of the data keeps data-parallel replicas
// bit-identical). Items that are not adapted read nothing and write nothing.
__global__ __launch_bounds__(256) void lars_partial_kernel(const float* __restrict__ p, const float* __restrict__ g, const clite_optim_item* __restrict__ items,
                                                           float* __restrict__ partials, uint32_t n_slots) {
  __shared__ float red[2][4];
  const clite_optim_item it = items[blockIdx.x];
  if (it.reserved == 0 || it.reserved > n_slots) return;          // block-uniform
  float sp = 0.f, sg = 0.f;
#pragma unroll 4
  for (uint32_t i = threadIdx.x * 4; i < it.count; i += 1024) {
    const size_t o = (size_t)it.start + i;
    const f32x4 pv = *(const f32x4*)(p + o), gv = *(const f32x4*)(g + o);
    sp += pv[0] * pv[0] + pv[1] * pv[1] + pv[2] * pv[2] + pv[3] * pv[3];
    sg += gv[0] * gv[0] + gv[1] * gv[1] + gv[2] * gv[2] + gv[3] * gv[3];
  }
  sp = wave_sum(sp);
  sg = wave_sum(sg);
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = sp; red[1][threadIdx.x >> 6] = sg; }
  __syncthreads();
  if (threadIdx.x == 0) {
    partials[2 * (size_t)blockIdx.x] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
    partials[2 * (size_t)blockIdx.x + 1] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
  }
}

// Stage 2 is norm_fold_kernel (norm_fold.h, shared with lamb_ops.hip): the workgroup of a tensor's first item folds that tensor's pairs in item order.

// hp: as sgd_step_kernel, plus [6] trust coefficient eta, [7] eps. The trust ratio is formed once per workgroup from block-uniform values and
// folded into the two scalars of the gradient term: q (g gmul + wd p) = g (gmul q) + (wd q) p. The loop below is sgd_step_kernel's loop, statement
// for statement, on those scalars; with q = 1 they are sgd_step_kernel's own values, so the results agree bit for bit.
template <typename T, bool CAST>
__global__ __launch_bounds__(256) void lars_step_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ v, float* __restrict__ slow,
                                                        T* __restrict__ cast, const clite_optim_item* __restrict__ items,
                                                        const float* __restrict__ hp, const float* __restrict__ sumsq, const float* __restrict__ norms,
                                                        uint32_t n_slots) {
  const clite_optim_item it = items[blockIdx.x];
  const float lr = it.lr * hp[0], mu = hp[1], max_norm = hp[2], alpha = hp[4], gs = hp[5], eta = hp[6], eps = hp[7];
  const bool sync = hp[3] != 0.f;
  float clip = 1.f;
  if (max_norm > 0.f) {
    float total = sqrtf(sumsq[0]) * gs;
    clip = fminf(max_norm / (total + 1e-6f), 1.f);
  }
  float gmul = gs * clip, wd = it.wd;
  if (it.reserved != 0 && it.reserved <= n_slots) {
    const float pn = sqrtf(norms[2 * (size_t)(it.reserved - 1)]), gn = sqrtf(norms[2 * (size_t)(it.reserved - 1) + 1]) * gmul;
    if (pn > 0.f && gn > 0.f) {
      const float q = eta * pn / (gn + wd * pn + eps);
      gmul *= q;
      wd *= q;
    }
  }
#pragma unroll 4
  for (uint32_t i = threadIdx.x * 4; i < it.count; i += 1024) {
    size_t o = (size_t)it.start + i;
    f32x4 pv = *(const f32x4*)(p + o), gv = *(const f32x4*)(g + o), vv = *(const f32x4*)(v + o);
    f32x4 sv = {0.f, 0.f, 0.f, 0.f};
    if (sync) sv = *(const f32x4*)(slow + o);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float ge = gv[e] * gmul + wd * pv[e];
      vv[e] = mu * vv[e] + ge;
      pv[e] = pv[e] - lr * vv[e];
      if (sync) { pv[e] = alpha * pv[e] + (1.f - alpha) * sv[e]; sv[e] = pv[e]; }
    }
    *(f32x4*)(p + o) = pv;
    *(f32x4*)(v + o) = vv;
    *(f32x4*)(g + o) = f32x4{0.f, 0.f, 0.f, 0.f};      // zero_grad for the next step
    if (sync) *(f32x4*)(slow + o) = sv;
    if (CAST) {
      union { bf16 e[4]; u32x2 u; } pk;
#pragma unroll
      for (int e = 0; e < 4; ++e) pk.e[e] = f2bf(pv[e]);
      *(u32x2*)((bf16*)cast + o) = pk.u;
    }
  }
}

}  // namespace

extern "C" int clite_lars_norms(const float* p, const float* g, const clite_optim_item* items, int n_items, float* partials, float* norms, int n_slots,
                                void* stream) {
  if (!p || !g || !items || n_items <= 0 || !partials || !norms || n_slots < 0) return -1;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(lars_partial_kernel, dim3(n_items), dim3(256), 0, st, p, g, items, partials, (uint32_t)n_slots);
  hipLaunchKernelGGL(norm_fold_kernel, dim3(n_items), dim3(256), 0, st, items, (uint32_t)n_items, (const float*)partials, norms, (uint32_t)n_slots);
  return (int)hipGetLastError();
}

extern "C" int clite_lars_step(float* p, float* g, float* v, float* slow, void* cast_bf16, const clite_optim_item* items, int n_items, const float* hp,
                               const float* sumsq, const float* norms, int n_slots, void* stream) {
  if (!p || !g || !v || !slow || !items || n_items <= 0 || !hp || !sumsq || !norms || n_slots < 0) return -1;
  hipStream_t st = (hipStream_t)stream;
  if (cast_bf16)
    hipLaunchKernelGGL((lars_step_kernel<bf16, true>), dim3(n_items), dim3(256), 0, st, p, g, v, slow, (bf16*)cast_bf16, items, hp, sumsq, norms, (uint32_t)n_slots);
  else
    hipLaunchKernelGGL((lars_step_kernel<bf16, false>), dim3(n_items), dim3(256), 0, st, p, g, v, slow, (bf16*)nullptr, items, hp, sumsq, norms, (uint32_t)n_slots);
  return (int)hipGetLastError();
}
