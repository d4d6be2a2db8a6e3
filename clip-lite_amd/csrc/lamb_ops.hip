// LAMB (You et al. 2020, "Large Batch Optimization for Deep Learning", Algorithm 2) on the update path's item table: AdamW whose step for every
// adapted tensor is scaled by the trust ratio q = |p| / |r|, r = m^ / (sqrt(v^) + eps) + wd p. |r| needs the moments of THIS step, so the update
// is two passes. The first (clite_lamb_moments) reads p, g, m, v2 (16 B per element), writes m, v2 (8 B) and leaves the per-tensor pairs
// (sum p^2, sum r^2) behind, through lars_ops.hip's two fixed-order stages; the second (clite_lamb_step) re-forms r from the stored m, v2 and p
// (12 B), and writes p, the zeroed g and the bf16 copy (10 B): 46 B against clite_adamw_step's 34. r is never stored: parking it in g's slot
// between the launches would move the same 46 B and leave a foreign quantity in the gradient arena.
#include "vec.h"
#include "clite.h"
#include "norm_fold.h"

using namespace clite;

namespace {

// r = (m / bc1) / (sqrt(v2 / bc2) + eps) + wd p, the one place both kernels form it. Every fused multiply-add is spelled out, so that no
// contraction choice of the compiler can make the r that was normed differ from the r that is applied.
DEV float lamb_r(float p, float m, float v2, float wd, float inv_bc1, float inv_sqrt_bc2, float eps) {
  const float u = (m * inv_bc1) / __builtin_fmaf(sqrtf(v2), inv_sqrt_bc2, eps);
  return __builtin_fmaf(wd, p, u);
}

// adamw_step_kernel's arithmetic (optim_ops.hip), which the kernels below must reproduce bit for bit wherever a tensor is not adapted. Its source
// statements leave the compiler free to contract a multiply and an add, and which pairs it contracts depends on the code around them: the same
// statements inside these kernels came out as other instructions (b2 v2 rounded and g' g' fused, where adamw_step_kernel rounds (1 - beta2) g' g'
// and fuses b2 v2). So the device build spells out the operations adamw_step_kernel's gfx950 code performs, read off its ISA - two per element
// of every v_pk_fma / v_pk_mul there; the host build of the wave simulator contracts nothing in either file, and keeps the statements as
// written. tests/test_gpu_lamb_ops.py and tests/test_wavesim_lamb.py hold both to clite_adamw_step's bits.
DEV void adamw_moments(float g, float gmul, float omb1, float b2, float omb2, float& m, float& v2) {
  const float ge = g * gmul;
#ifdef CLITE_WAVESIM_H
  m = m + omb1 * (ge - m);          // exp_avg.lerp_(grad, 1 - beta1)
  v2 = b2 * v2 + omb2 * ge * ge;
#else
  m = __builtin_fmaf(omb1, __builtin_fmaf(g, gmul, -m), m);
  v2 = __builtin_fmaf(b2, v2, (omb2 * ge) * ge);
#endif
}
DEV float adamw_update(float p, float m, float v2, float decay, float step_size, float inv_sqrt_bc2, float eps) {
#ifdef CLITE_WAVESIM_H
  p *= decay;
  p -= step_size * (m / (sqrtf(v2) * inv_sqrt_bc2 + eps));
  return p;
#else
  return __builtin_fmaf(decay, p, -(step_size * (m / __builtin_fmaf(sqrtf(v2), inv_sqrt_bc2, eps))));
#endif
}
DEV float adamw_clip(float max_norm, const float* sumsq, float gs) {          // the global-norm clip factor
  if (!(max_norm > 0.f)) return 1.f;
#ifdef CLITE_WAVESIM_H
  float total = sqrtf(sumsq[0]) * gs;
  return fminf(max_norm / (total + 1e-6f), 1.f);
#else
  return fminf(max_norm / __builtin_fmaf(sqrtf(sumsq[0]), gs, 1e-6f), 1.f);
#endif
}
DEV float adamw_decay(float lr, float wd) {
#ifdef CLITE_WAVESIM_H
  return 1.f - lr * wd;
#else
  return __builtin_fmaf(-lr, wd, 1.f);
#endif
}
DEV float lookahead_sync(float p, float slow, float alpha) {
#ifdef CLITE_WAVESIM_H
  return alpha * p + (1.f - alpha) * slow;
#else
  return __builtin_fmaf(1.f - alpha, slow, alpha * p);
#endif
}

// hp: adamw_step_kernel's twelve floats (optim_ops.hip), then [12] the TRUST_CLIP flag (read by the step kernel only).
// One workgroup per item. Every item: the two moment statements of adamw_step_kernel (adamw_moments) on g' = g * prescale * clip. An adapted item
// also reads p, forms r per element and stores ITS pair (sum p^2, sum r^2) with a plain store into its own slot of `partials`; an item that
// is not adapted reads no p and writes no pair. p and g are only read.
__global__ __launch_bounds__(256) void lamb_moments_kernel(const float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v2,
                                                           const clite_optim_item* __restrict__ items, const float* __restrict__ hp,
                                                           const float* __restrict__ sumsq, float* __restrict__ partials, uint32_t n_slots) {
  __shared__ float red[2][4];
  const clite_optim_item it = items[blockIdx.x];
  const float wd = it.wd, max_norm = hp[2], gs = hp[5], b2 = hp[6], eps = hp[7], bc1 = hp[8], bc2 = hp[9], omb1 = hp[10], omb2 = hp[11];
  const bool adapted = it.reserved != 0 && it.reserved <= n_slots;          // block-uniform
  const float gmul = gs * adamw_clip(max_norm, sumsq, gs), inv_bc1 = 1.f / bc1, inv_sqrt_bc2 = 1.f / sqrtf(bc2);
  float sp = 0.f, sr = 0.f;
#pragma unroll 4
  for (uint32_t i = threadIdx.x * 4; i < it.count; i += 1024) {
    const size_t o = (size_t)it.start + i;
    f32x4 gv = *(const f32x4*)(g + o), mv = *(const f32x4*)(m + o), vv = *(const f32x4*)(v2 + o);
    f32x4 pv = {0.f, 0.f, 0.f, 0.f};
    if (adapted) pv = *(const f32x4*)(p + o);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float me = mv[e], ve = vv[e];
      adamw_moments(gv[e], gmul, omb1, b2, omb2, me, ve);
      mv[e] = me;
      vv[e] = ve;
      if (adapted) {
        const float r = lamb_r(pv[e], mv[e], vv[e], wd, inv_bc1, inv_sqrt_bc2, eps);
        sp += pv[e] * pv[e];
        sr += r * r;
      }
    }
    *(f32x4*)(m + o) = mv;
    *(f32x4*)(v2 + o) = vv;
  }
  if (!adapted) return;
  sp = wave_sum(sp);
  sr = wave_sum(sr);
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = sp; red[1][threadIdx.x >> 6] = sr; }
  __syncthreads();
  if (threadIdx.x == 0) {
    partials[2 * (size_t)blockIdx.x] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
    partials[2 * (size_t)blockIdx.x + 1] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
  }
}

// The update from the stored moments. An adapted item re-forms r with lamb_r from the p the moments kernel read (p has not been written since)
// and moves p by lr q r, q = |p| / |r| formed once per workgroup from block-uniform values (1 where either norm is zero; capped at 1 under
// TRUST_CLIP). An item that is not adapted runs adamw_step_kernel's two p statements (adamw_update) - multiplicative decoupled
// decay, step_size = lr / bc1 - so a table with every reserved word 0 gives clite_adamw_step's bits. The two forms are equal in exact
// arithmetic. Then the Lookahead sync, the bf16 copy and the zeroing of g as in the sibling kernels; g is not read.
template <typename T, bool CAST>
__global__ __launch_bounds__(256) void lamb_step_kernel(float* __restrict__ p, float* __restrict__ g, const float* __restrict__ m, const float* __restrict__ v2,
                                                        float* __restrict__ slow, T* __restrict__ cast, const clite_optim_item* __restrict__ items,
                                                        const float* __restrict__ hp, const float* __restrict__ norms, uint32_t n_slots) {
  const clite_optim_item it = items[blockIdx.x];
  const float lr = it.lr * hp[0], wd = it.wd, alpha = hp[4], eps = hp[7], bc1 = hp[8], bc2 = hp[9];
  const bool sync = hp[3] != 0.f, adapted = it.reserved != 0 && it.reserved <= n_slots;
  const float decay = adamw_decay(lr, wd), step_size = lr / bc1, inv_bc1 = 1.f / bc1, inv_sqrt_bc2 = 1.f / sqrtf(bc2);
  float lrq = lr;
  if (adapted) {
    const float pn = sqrtf(norms[2 * (size_t)(it.reserved - 1)]), rn = sqrtf(norms[2 * (size_t)(it.reserved - 1) + 1]);
    float q = 1.f;
    if (pn > 0.f && rn > 0.f) q = pn / rn;
    if (hp[12] != 0.f) q = fminf(q, 1.f);
    lrq = lr * q;
  }
#pragma unroll 4
  for (uint32_t i = threadIdx.x * 4; i < it.count; i += 1024) {
    size_t o = (size_t)it.start + i;
    f32x4 pv = *(const f32x4*)(p + o), mv = *(const f32x4*)(m + o), vv = *(const f32x4*)(v2 + o);
    f32x4 sv = {0.f, 0.f, 0.f, 0.f};
    if (sync) sv = *(const f32x4*)(slow + o);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (adapted) {
        pv[e] = __builtin_fmaf(-lrq, lamb_r(pv[e], mv[e], vv[e], wd, inv_bc1, inv_sqrt_bc2, eps), pv[e]);
      } else {
        pv[e] = adamw_update(pv[e], mv[e], vv[e], decay, step_size, inv_sqrt_bc2, eps);
      }
      if (sync) { pv[e] = lookahead_sync(pv[e], sv[e], alpha); sv[e] = pv[e]; }
    }
    *(f32x4*)(p + o) = pv;
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

extern "C" int clite_lamb_moments(const float* p, const float* g, float* m, float* v2, const clite_optim_item* items, int n_items, const float* hp,
                                  const float* sumsq, float* partials, float* norms, int n_slots, void* stream) {
  if (!p || !g || !m || !v2 || !items || n_items <= 0 || !hp || !sumsq || !partials || !norms || n_slots < 0) return -1;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(lamb_moments_kernel, dim3(n_items), dim3(256), 0, st, p, g, m, v2, items, hp, sumsq, partials, (uint32_t)n_slots);
  hipLaunchKernelGGL(norm_fold_kernel, dim3(n_items), dim3(256), 0, st, items, (uint32_t)n_items, (const float*)partials, norms, (uint32_t)n_slots);
  return (int)hipGetLastError();
}

extern "C" int clite_lamb_step(float* p, float* g, const float* m, const float* v2, float* slow, void* cast_bf16, const clite_optim_item* items, int n_items,
                               const float* hp, const float* sumsq, const float* norms, int n_slots, void* stream) {
  // sumsq is part of the signature the update entry points share; the clip factor entered the moments, so no kernel here reads it
  if (!p || !g || !m || !v2 || !slow || !items || n_items <= 0 || !hp || !sumsq || !norms || n_slots < 0) return -1;
  hipStream_t st = (hipStream_t)stream;
  if (cast_bf16)
    hipLaunchKernelGGL((lamb_step_kernel<bf16, true>), dim3(n_items), dim3(256), 0, st, p, g, m, v2, slow, (bf16*)cast_bf16, items, hp, norms, (uint32_t)n_slots);
  else
    hipLaunchKernelGGL((lamb_step_kernel<bf16, false>), dim3(n_items), dim3(256), 0, st, p, g, m, v2, slow, (bf16*)nullptr, items, hp, norms, (uint32_t)n_slots);
  return (int)hipGetLastError();
}
