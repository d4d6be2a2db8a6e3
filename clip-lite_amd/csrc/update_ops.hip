// Parameter-update path of the train step (reference train.py:221-226) on the item table: global-norm gradient clipping
// (torch.nn.utils.clip_grad_norm_), then one of four rules with one (lr, wd) pair per parameter tensor (factories.py:464-482) - torch.optim.SGD
// with momentum and weight decay, torch.optim.AdamW (factories.py:439), and their layer-wise forms LARS (You, Gitman, Ginsburg 2017) and LAMB
// (You et al. 2020, Algorithm 2) - then the Lookahead slow/fast interpolation every k-th step (optim/lookahead.py:88-101), the zeroing of the
// gradients and the bf16 weight copy the next forward reads. One workgroup per item, one pass over flat buffers, pure HBM streaming.
//
// The file has one copy of everything the four share:
//   * the arithmetic (clip_factor .. lamb_r): one function per formula, called by every kernel that must agree on its bits;
//   * update_sweep: item -> lr, sync flag, clip factor -> the 4-wide loop (loads, the rule's element function, Lookahead sync, stores);
//     a rule adds its block-uniform scalars, the number of its state arrays and its element function. Three kernels: sgd_step_kernel
//     (SGD and LARS: SGD is LARS with no norm slots), adamw_step_kernel, lamb_step_kernel;
//   * norm_sweep: the same item loop summing a pair per item (LARS: p^2, g^2; LAMB: the moments in place, then p^2, r^2), and
//     store_block_pair, the fixed-order tail of both and of norm_fold_kernel.
#include <type_traits>
#include "vec.h"
#include "clite.h"

using namespace clite;

// From here on a multiply and an add are fused where the source says __builtin_fmaf and nowhere else. LARS that adapts nothing must give SGD's
// bits and LAMB that adapts nothing AdamW's (include/clite.h), and the r LAMB norms must be the r it applies; left free, the compiler fuses
// other pairs of the same statement in one kernel than in the next. Which pairs are fused is part of what the optimizers compute: changing
// one changes their bits (and saved runs no longer resume bit for bit).
#pragma clang fp contract(off)

namespace {

// ---- arithmetic --------------------------------------------------------------------------------------------------------------------------------
// torch's clip_grad_norm_ factor from the squared gradient norm; gs is the gradient pre-scale
DEV float clip_factor(float max_norm, const float* sumsq, float gs) {
  if (!(max_norm > 0.f)) return 1.f;
  return fminf(max_norm / __builtin_fmaf(sqrtf(sumsq[0]), gs, 1e-6f), 1.f);
}
DEV float lookahead_sync(float p, float slow, float alpha) { return __builtin_fmaf(1.f - alpha, slow, alpha * p); }

// g' = g gmul + wd p; v = mu v + g'; p -= lr v
DEV void sgd_update(float g, float gmul, float wd, float mu, float lr, float& p, float& v) {
  v = mu * v + __builtin_fmaf(wd, p, g * gmul);
  p = __builtin_fmaf(-lr, v, p);
}
// LARS: q = eta |p| / (|g'| + wd |p| + eps) from the squared norms of p and the raw g; 1 where either norm is zero
DEV float lars_trust(float p2, float g2, float gmul, float wd, float eta, float eps) {
  const float pn = sqrtf(p2), gn = sqrtf(g2) * gmul;
  if (!(pn > 0.f && gn > 0.f)) return 1.f;
  return (eta * pn) / (__builtin_fmaf(wd, pn, gn) + eps);
}

// m += (1 - beta1)(g' - m), exp_avg.lerp_(grad, 1 - beta1); v2 = beta2 v2 + (1 - beta2) g'^2, g' = g gmul
// (1 - beta formed in double on the host, as torch does: 1.f - 0.999f is off by 1.3e-5)
DEV void adamw_moments(float g, float gmul, float omb1, float b2, float omb2, float& m, float& v2) {
  const float ge = g * gmul;
  m = __builtin_fmaf(omb1, __builtin_fmaf(g, gmul, -m), m);
  v2 = __builtin_fmaf(b2, v2, (omb2 * ge) * ge);
}
DEV float adamw_decay(float lr, float wd) { return __builtin_fmaf(-lr, wd, 1.f); }
// p = decay p - step_size m / (sqrt(v2) / sqrt(bc2) + eps), step_size = lr / bc1
DEV float adamw_update(float p, float m, float v2, float decay, float step_size, float inv_sqrt_bc2, float eps) {
  return __builtin_fmaf(decay, p, -(step_size * (m / __builtin_fmaf(sqrtf(v2), inv_sqrt_bc2, eps))));
}
// LAMB: r = (m / bc1) / (sqrt(v2 / bc2) + eps) + wd p, the one place the moments pass (which norms it) and the step (which applies it) form it
DEV float lamb_r(float p, float m, float v2, float wd, float inv_bc1, float inv_sqrt_bc2, float eps) {
  const float u = (m * inv_bc1) / __builtin_fmaf(sqrtf(v2), inv_sqrt_bc2, eps);
  return __builtin_fmaf(wd, p, u);
}
// a chunk's sum of squares; which square is rounded (x1's) and the order of the rest are part of the norms' bits
DEV float sumsq4(f32x4 x) { return __builtin_fmaf(x[3], x[3], __builtin_fmaf(x[2], x[2], __builtin_fmaf(x[0], x[0], x[1] * x[1]))); }

DEV f32x4 load4(const float* p) { return *(const f32x4*)p; }
DEV void store4(float* p, f32x4 v) { *(f32x4*)p = v; }
DEV bool is_adapted(const clite_optim_item& it, uint32_t n_slots) { return it.reserved != 0 && it.reserved <= n_slots; }      // block-uniform

// ---- the update sweep -----------------------------------------------------------------------------------------------------------------------------
// hp: [0] lr multiplier (schedule), [1] momentum / beta1, [2] max grad norm (<= 0: no clipping), [3] lookahead sync flag, [4] lookahead alpha,
//     [5] gradient pre-scale (1/world_size after a SUM all-reduce, 1/loss_scale, ...); then per rule (the host uploads them with the rest):
//     LARS [6] trust coefficient eta, [7] eps; AdamW and LAMB [6] beta2, [7] eps, [8] 1 - beta1^t, [9] 1 - beta2^t, [10] 1 - beta1,
//     [11] 1 - beta2; LAMB [12] the TRUST_CLIP flag.
// A rule is built once per workgroup from (item, lr, hp, clip factor, the tensor's pair of squared norms or null when the item is not adapted),
// names its STATES flat arrays (1 or 2) and whether it READS_G - a rule that reads g folds it into its states, which are then stored; one that
// does not (the LAMB step: its moments pass has consumed g) only reads them and needs no clip factor - and maps one element.

// SGD, and LARS where the item has a norm pair: the trust ratio scales the two scalars of the gradient term, q (g gmul + wd p) =
// g (gmul q) + (wd q) p, so an item that is not adapted runs SGD's own values through SGD's own statements.
struct SgdRule {
  static constexpr int STATES = 1;          // v
  static constexpr bool READS_G = true;
  float lr, gmul, wd, mu;
  DEV SgdRule(const clite_optim_item& it, float lr_, const float* hp, float clip, const float* pair) : lr(lr_), gmul(hp[5] * clip), wd(it.wd), mu(hp[1]) {
    if (pair) {
      const float q = lars_trust(pair[0], pair[1], gmul, wd, hp[6], hp[7]);
      gmul *= q;
      wd *= q;
    }
  }
  DEV void element(float& p, float g, float& v, float&) const { sgd_update(g, gmul, wd, mu, lr, p, v); }
};

// torch.optim.AdamW: decoupled weight decay, bias-corrected moments
struct AdamwRule {
  static constexpr int STATES = 2;          // m (exp_avg), v2 (exp_avg_sq)
  static constexpr bool READS_G = true;
  float gmul, omb1, b2, omb2, decay, step_size, inv_sqrt_bc2, eps;
  DEV AdamwRule(const clite_optim_item& it, float lr, const float* hp, float clip, const float*)
      : gmul(hp[5] * clip), omb1(hp[10]), b2(hp[6]), omb2(hp[11]), decay(adamw_decay(lr, it.wd)), step_size(lr / hp[8]), inv_sqrt_bc2(1.f / sqrtf(hp[9])),
        eps(hp[7]) {}
  DEV void element(float& p, float g, float& m, float& v2) const {
    adamw_moments(g, gmul, omb1, b2, omb2, m, v2);
    p = adamw_update(p, m, v2, decay, step_size, inv_sqrt_bc2, eps);
  }
};

// The LAMB update from the moments LambMoments stored. An adapted item re-forms r from the p the moments pass read (p has not been written
// since) and moves p by lr q r, q = |p| / |r| (1 where either norm is zero; capped at 1 under TRUST_CLIP). An item that is not adapted runs
// adamw_update. The two forms are equal in exact arithmetic.
struct LambStepRule {
  static constexpr int STATES = 2;
  static constexpr bool READS_G = false;
  bool adapted;
  float wd, lrq, decay, step_size, inv_bc1, inv_sqrt_bc2, eps;
  DEV LambStepRule(const clite_optim_item& it, float lr, const float* hp, float, const float* pair)
      : adapted(pair != nullptr), wd(it.wd), lrq(lr), decay(adamw_decay(lr, it.wd)), step_size(lr / hp[8]), inv_bc1(1.f / hp[8]),
        inv_sqrt_bc2(1.f / sqrtf(hp[9])), eps(hp[7]) {
    if (adapted) {
      const float pn = sqrtf(pair[0]), rn = sqrtf(pair[1]);
      float q = 1.f;
      if (pn > 0.f && rn > 0.f) q = pn / rn;
      if (hp[12] != 0.f) q = fminf(q, 1.f);
      lrq = lr * q;
    }
  }
  DEV void element(float& p, float, float& m, float& v2) const {
    if (adapted) p = __builtin_fmaf(-lrq, lamb_r(p, m, v2, wd, inv_bc1, inv_sqrt_bc2, eps), p);
    else p = adamw_update(p, m, v2, decay, step_size, inv_sqrt_bc2, eps);
  }
};

template <typename Rule, bool CAST>
DEV void update_sweep(float* __restrict__ p, float* __restrict__ g, float* __restrict__ s0, float* __restrict__ s1, float* __restrict__ slow,
                      bf16* __restrict__ cast, const clite_optim_item* __restrict__ items, const float* __restrict__ hp,
                      const float* __restrict__ sumsq, const float* __restrict__ norms, uint32_t n_slots) {
  const clite_optim_item it = items[blockIdx.x];
  const float lr = it.lr * hp[0], alpha = hp[4];
  const bool sync = hp[3] != 0.f;
  const float clip = Rule::READS_G ? clip_factor(hp[2], sumsq, hp[5]) : 1.f;
  const Rule rule(it, lr, hp, clip, is_adapted(it, n_slots) ? norms + 2 * (size_t)(it.reserved - 1) : nullptr);
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  // the flat arrays never overlap (__restrict__), so an iteration's loads are all issued before its first store
#pragma unroll 4
  for (uint32_t i = threadIdx.x * 4; i < it.count; i += 1024) {
    const size_t o = (size_t)it.start + i;
    // (nontemporal loads / stores measured here: 698 -> 734 us inside the step; plain accesses kept)
    f32x4 pv = load4(p + o), gv = zero, av, bv = zero, sv = zero;
    if (Rule::READS_G) gv = load4(g + o);
    av = load4(s0 + o);
    if (Rule::STATES == 2) bv = load4(s1 + o);
    if (sync) sv = load4(slow + o);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float pe = pv[e], ae = av[e], be = bv[e];
      rule.element(pe, gv[e], ae, be);
      if (sync) { pe = lookahead_sync(pe, sv[e], alpha); sv[e] = pe; }
      pv[e] = pe; av[e] = ae; bv[e] = be;
    }
    store4(p + o, pv);
    if (Rule::READS_G) {
      store4(s0 + o, av);
      if (Rule::STATES == 2) store4(s1 + o, bv);
    }
    store4(g + o, zero);      // zero_grad for the next step
    if (sync) store4(slow + o, sv);
    if (CAST) {
      union { bf16 e[4]; u32x2 u; } pk;
#pragma unroll
      for (int e = 0; e < 4; ++e) pk.e[e] = f2bf(pv[e]);
      *(u32x2*)(cast + o) = pk.u;
    }
  }
}

#define UPDATE_PARAMS                                                                                                                           \
  float *__restrict__ p, float *__restrict__ g, float *__restrict__ s0, float *__restrict__ s1, float *__restrict__ slow, bf16 *__restrict__ cast, \
      const clite_optim_item *__restrict__ items, const float *__restrict__ hp, const float *__restrict__ sumsq, const float *__restrict__ norms,   \
      uint32_t n_slots
#define UPDATE_ARGS p, g, s0, s1, slow, cast, items, hp, sumsq, norms, n_slots
template <bool CAST> __global__ __launch_bounds__(256) void sgd_step_kernel(UPDATE_PARAMS) { update_sweep<SgdRule, CAST>(UPDATE_ARGS); }
template <bool CAST> __global__ __launch_bounds__(256) void adamw_step_kernel(UPDATE_PARAMS) { update_sweep<AdamwRule, CAST>(UPDATE_ARGS); }
template <bool CAST> __global__ __launch_bounds__(256) void lamb_step_kernel(UPDATE_PARAMS) { update_sweep<LambStepRule, CAST>(UPDATE_ARGS); }
#undef UPDATE_PARAMS
#undef UPDATE_ARGS

// ---- the per-tensor norms of the layer-wise rules ----------------------------------------------------------------------------------------------------
// Two squared norms per adapted tensor in two fixed-order stages over the item table, no float atomics (sumsq_partial_kernel's reasoning,
// optim_ops.hip: a pure function of the data keeps data-parallel replicas bit-identical). Stage 1, norm_sweep: one workgroup per item (the update's
// decomposition, so the 30522 x 768 embedding is spread over 2862 workgroups, not streamed through one CU); every workgroup of an adapted item
// stores ITS pair with a plain store into its own slot of `partials`. Stage 2, norm_fold_kernel, folds each tensor's pairs.

// The workgroup's pair from every thread's pair: wave sums, one value per wave through LDS, (a + b) + (c + d) - the one order of all three kernels
DEV void store_block_pair(float a, float b, float* __restrict__ out) {
  __shared__ float red[2][4];
  a = wave_sum(a);
  b = wave_sum(b);
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = a; red[1][threadIdx.x >> 6] = b; }
  __syncthreads();
  if (threadIdx.x == 0) {
    out[0] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
    out[1] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
  }
}

// LARS: (sum p^2, sum g^2) of the raw p and g. Items that are not adapted read nothing and write nothing.
struct LarsNorms {
  static constexpr bool EVERY_ITEM = false;
  DEV LarsNorms(const clite_optim_item&, const float*, const float*) {}
  DEV void chunk(const float* p, const float* g, float*, float*, bool, float& sp, float& sg) const {
    const f32x4 pv = load4(p), gv = load4(g);
    sp += sumsq4(pv);
    sg += sumsq4(gv);
  }
};

// LAMB: every item's moments in place (adamw_moments on g' = g prescale clip); an adapted item also reads p and sums (p^2, r^2), an item that is
// not adapted reads no p and writes no pair. p and g are only read. hp as AdamwRule.
struct LambMoments {
  static constexpr bool EVERY_ITEM = true;
  float wd, gmul, omb1, b2, omb2, inv_bc1, inv_sqrt_bc2, eps;
  DEV LambMoments(const clite_optim_item& it, const float* hp, const float* sumsq)
      : wd(it.wd), gmul(hp[5] * clip_factor(hp[2], sumsq, hp[5])), omb1(hp[10]), b2(hp[6]), omb2(hp[11]), inv_bc1(1.f / hp[8]),
        inv_sqrt_bc2(1.f / sqrtf(hp[9])), eps(hp[7]) {}
  DEV void chunk(const float* p, const float* g, float* m, float* v2, bool adapted, float& sp, float& sr) const {
    f32x4 gv = load4(g), mv = load4(m), vv = load4(v2);
    f32x4 pv = {0.f, 0.f, 0.f, 0.f};
    if (adapted) pv = load4(p);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float me = mv[e], ve = vv[e];
      adamw_moments(gv[e], gmul, omb1, b2, omb2, me, ve);
      mv[e] = me;
      vv[e] = ve;
      if (adapted) {
        const float r = lamb_r(pv[e], me, ve, wd, inv_bc1, inv_sqrt_bc2, eps);
        sp = __builtin_fmaf(pv[e], pv[e], sp);
        sr = __builtin_fmaf(r, r, sr);
      }
    }
    store4(m, mv);
    store4(v2, vv);
  }
};

template <typename Rule>
__global__ __launch_bounds__(256) void norm_sweep_kernel(const float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v2,
                                                         const clite_optim_item* __restrict__ items, const float* __restrict__ hp,
                                                         const float* __restrict__ sumsq, float* __restrict__ partials, uint32_t n_slots) {
  const clite_optim_item it = items[blockIdx.x];
  const bool adapted = is_adapted(it, n_slots);
  if (!Rule::EVERY_ITEM && !adapted) return;
  const Rule rule(it, hp, sumsq);
  float a = 0.f, b = 0.f;
#pragma unroll 4
  for (uint32_t i = threadIdx.x * 4; i < it.count; i += 1024) {
    const size_t o = (size_t)it.start + i;
    rule.chunk(p + o, g + o, m + o, v2 + o, adapted, a, b);
  }
  if (adapted) store_block_pair(a, b, partials + 2 * (size_t)blockIdx.x);
}

// The workgroup of a tensor's FIRST item folds that tensor's pairs; every other workgroup leaves at once. Thread t adds the pairs of
// the tensor's items t, t + 256, ... in that order (a tensor's items are contiguous in the table, so a thread stops at the first item of
// another slot), then the fixed wave / workgroup fold. The order depends on the tensor's own items only: a launch of a sub-range of the table
// that holds the tensor whole gives the same bits as a launch of the whole table. The embedding's 2862 pairs take 12 trips.
__global__ __launch_bounds__(256) void norm_fold_kernel(const clite_optim_item* __restrict__ items, uint32_t n_items, const float* __restrict__ partials,
                                                        float* __restrict__ norms, uint32_t n_slots) {
  const uint32_t head = blockIdx.x, slot1 = items[head].reserved;
  if (slot1 == 0 || slot1 > n_slots) return;
  if (head > 0 && items[head - 1].reserved == slot1) return;
  float a = 0.f, b = 0.f;
  for (uint32_t j = head + threadIdx.x; j < n_items && items[j].reserved == slot1; j += 256) {
    a += partials[2 * (size_t)j];
    b += partials[2 * (size_t)j + 1];
  }
  store_block_pair(a, b, norms + 2 * (size_t)(slot1 - 1));
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------------------------------
// launch(std::true_type) where the bf16 copy is wanted, launch(std::false_type) where not: the two instantiations of an update kernel
template <typename F> int with_cast(const void* cast_bf16, F&& launch) {
  if (cast_bf16) launch(std::true_type{});
  else launch(std::false_type{});
  return (int)hipGetLastError();
}

template <typename Rule>
int launch_norms(const float* p, const float* g, float* m, float* v2, const clite_optim_item* items, int n_items, const float* hp, const float* sumsq,
                 float* partials, float* norms, int n_slots, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(norm_sweep_kernel<Rule>, dim3(n_items), dim3(256), 0, st, p, g, m, v2, items, hp, sumsq, partials, (uint32_t)n_slots);
  hipLaunchKernelGGL(norm_fold_kernel, dim3(n_items), dim3(256), 0, st, items, (uint32_t)n_items, (const float*)partials, norms, (uint32_t)n_slots);
  return (int)hipGetLastError();
}

// SGD is LARS with no norm slots: nothing is adapted and `norms` is not read
int launch_sgd(float* p, float* g, float* v, float* slow, void* cast_bf16, const clite_optim_item* items, int n_items, const float* hp, const float* sumsq,
               const float* norms, int n_slots, void* stream) {
  return with_cast(cast_bf16, [&](auto c) {
    hipLaunchKernelGGL(sgd_step_kernel<decltype(c)::value>, dim3(n_items), dim3(256), 0, (hipStream_t)stream, p, g, v, (float*)nullptr, slow, (bf16*)cast_bf16,
                       items, hp, sumsq, norms, (uint32_t)n_slots);
  });
}

}  // namespace

extern "C" int clite_sgd_step(float* p, float* g, float* v, float* slow, void* cast_bf16, const clite_optim_item* items, int n_items,
                              const float* hp, const float* sumsq, void* stream) {
  if (!p || !g || !v || !slow || !items || n_items <= 0 || !hp || !sumsq) return -1;
  return launch_sgd(p, g, v, slow, cast_bf16, items, n_items, hp, sumsq, nullptr, 0, stream);
}

extern "C" int clite_lars_step(float* p, float* g, float* v, float* slow, void* cast_bf16, const clite_optim_item* items, int n_items, const float* hp,
                               const float* sumsq, const float* norms, int n_slots, void* stream) {
  if (!p || !g || !v || !slow || !items || n_items <= 0 || !hp || !sumsq || !norms || n_slots < 0) return -1;
  return launch_sgd(p, g, v, slow, cast_bf16, items, n_items, hp, sumsq, norms, n_slots, stream);
}

extern "C" int clite_adamw_step(float* p, float* g, float* m, float* v2, float* slow, void* cast_bf16, const clite_optim_item* items, int n_items,
                                const float* hp, const float* sumsq, void* stream) {
  if (!p || !g || !m || !v2 || !slow || !items || n_items <= 0 || !hp || !sumsq) return -1;
  return with_cast(cast_bf16, [&](auto c) {
    hipLaunchKernelGGL(adamw_step_kernel<decltype(c)::value>, dim3(n_items), dim3(256), 0, (hipStream_t)stream, p, g, m, v2, slow, (bf16*)cast_bf16, items, hp,
                       sumsq, (const float*)nullptr, 0u);
  });
}

extern "C" int clite_lars_norms(const float* p, const float* g, const clite_optim_item* items, int n_items, float* partials, float* norms_out, int n_slots,
                                void* stream) {
  if (!p || !g || !items || n_items <= 0 || !partials || !norms_out || n_slots < 0) return -1;
  return launch_norms<LarsNorms>(p, g, nullptr, nullptr, items, n_items, nullptr, nullptr, partials, norms_out, n_slots, stream);
}

extern "C" int clite_lamb_moments(const float* p, const float* g, float* m, float* v2, const clite_optim_item* items, int n_items, const float* hp,
                                  const float* sumsq, float* partials, float* norms_out, int n_slots, void* stream) {
  if (!p || !g || !m || !v2 || !items || n_items <= 0 || !hp || !sumsq || !partials || !norms_out || n_slots < 0) return -1;
  return launch_norms<LambMoments>(p, g, m, v2, items, n_items, hp, sumsq, partials, norms_out, n_slots, stream);
}

extern "C" int clite_lamb_step(float* p, float* g, const float* m, const float* v2, float* slow, void* cast_bf16, const clite_optim_item* items, int n_items,
                               const float* hp, const float* sumsq, const float* norms, int n_slots, void* stream) {
  // sumsq is part of the signature the update entry points share; the clip factor entered the moments, so the kernel does not read it
  if (!p || !g || !m || !v2 || !slow || !items || n_items <= 0 || !hp || !sumsq || !norms || n_slots < 0) return -1;
  return with_cast(cast_bf16, [&](auto c) {      // the step only reads the moments (READS_G = false)
    hipLaunchKernelGGL(lamb_step_kernel<decltype(c)::value>, dim3(n_items), dim3(256), 0, (hipStream_t)stream, p, g, const_cast<float*>(m),
                       const_cast<float*>(v2), slow, (bf16*)cast_bf16, items, hp, sumsq, norms, (uint32_t)n_slots);
  });
}
