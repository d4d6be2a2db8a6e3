// The part of a batched Newton-CG solver that does not depend on the objective, shared by svm_ops.hip (squared hinge) and logreg_ops.hip
// (softmax): P independent convex problems, one workgroup per problem over its vector of n floats (row p of [P][ld] arrays), per-problem
// scalars in a device state table f32 [P][STRIDE] whose first columns are the enum below. The kernels are templates over a reduction policy
// and the stride, so each solver keeps the bits it always produced: the SVM sums in float (wave shuffles, 4 floats of LDS), the logreg in
// double through a 256-entry LDS tree. A policy owns its LDS: a kernel declares SCRATCH elements of acc_t and nothing else for the sums.
#ifndef CLITE_NEWTON_CG_H
#define CLITE_NEWTON_CG_H
#include "vec.h"
#include "clite.h"

namespace clite {
namespace ncg {

// columns 0-12 of every state table (clip-lite_amd/hip.py NCG_* mirrors the ones the host reads); a solver continues from NCG_COLS
enum { G0 = 0, GN, REL, RR, CGTOL2, STEP, NEWTON, CGIT, CGTOT, ACTIVE, CGACT, CGLAST, DPHI0, NCG_COLS };

constexpr int NT = 256;                   // threads of a workgroup of these kernels and of the block sums

// sum over the 256 threads of a workgroup in a fixed order; every thread gets the result
DEV float block_sum(float v, float* red) {
  v = wave_sum(v);
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// sum over the 256 threads of a workgroup as a fixed LDS tree in double; every thread gets the result
DEV double block_sum_d(double v, double* red) {
  __syncthreads();
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = NT / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  return red[0];
}

// Reduction policies: the accumulator of the per-thread partial dot products, the LDS the block sum needs, the block sum, and the norm
// sqrt(sum) as a float. Every other conversion to float is a plain cast of the block sum (a no-op for FloatSum).
struct FloatSum {
  using acc_t = float;
  static constexpr int SCRATCH = 4;
  static DEV float sum(float v, float* red) { return block_sum(v, red); }
  static DEV float root(float v) { return sqrtf(v); }
};
struct DoubleTree {
  using acc_t = double;
  static constexpr int SCRATCH = NT;
  static DEV double sum(double v, double* red) { return block_sum_d(v, red); }
  static DEV float root(double v) { return (float)sqrt(v); }
};

// What newton_begin takes |grad f(0)| of the stopping rule to be, and what it does after a line search that did not move.
enum class Rules {
  // The SVM. g0 is the norm of the gradient seen while NEWTON == 0, whatever G0 held: every solve starts at w = 0. g0_only is not read, nor
  // is STEP: a problem whose line search ended at step 0 repeats the iteration until max_newton (freezing it would be a behaviour change).
  FirstGradient,
  // The logreg. A warm start does not pass through w = 0: a g0_only call records |grad f(0)| and does nothing else, a regular call records
  // g0 only if none is recorded yet (a cold start), and a problem whose line search ended at step 0 is frozen: it would repeat the iteration.
  RecordedG0,
};

// One workgroup per problem: the gradient norm, the stopping test and, for a problem that goes on, a fresh CG solve of H x = -g
// (x = 0, r = d = -g, CG tolerance (eta ||g||)^2 with eta = min(eta_max, sqrt(||g|| / ||g0||))). g0_only is read under Rules::RecordedG0 only.
template <class Red, int STRIDE, Rules RULES>
__global__ __launch_bounds__(NT) void newton_begin_kernel(const float* G, int ld, int n, float* X, float* R, float* D, float* st, float tol,
                                                          int max_newton, float eta_max, int g0_only) {
  using acc_t = typename Red::acc_t;
  constexpr bool RECORDED = RULES == Rules::RecordedG0;
  __shared__ acc_t red[Red::SCRATCH];
  __shared__ int go;
  const int p = blockIdx.x;
  float* s = st + (size_t)p * STRIDE;
  const float* g = G + (size_t)p * ld;
  acc_t a = 0;
  for (int k = threadIdx.x; k < n; k += NT) a += (acc_t)g[k] * (acc_t)g[k];
  const acc_t gn2 = Red::sum(a, red);
  if (threadIdx.x == 0) {
    const float gn = Red::root(gn2);
    int act = 0;
    if (RECORDED && g0_only) {
      s[G0] = gn;
    } else {
      act = s[ACTIVE] != 0.f;
      if (act) {
        if (s[NEWTON] == 0.f && (!RECORDED || s[G0] == 0.f)) s[G0] = gn;
        const float g0 = s[G0];
        const float rel = g0 > 0.f ? gn / g0 : 0.f;
        s[GN] = gn;
        s[REL] = rel;
        if (rel <= tol || s[NEWTON] >= (float)max_newton || (RECORDED && s[NEWTON] > 0.f && s[STEP] == 0.f)) act = 0;
        if (act) {
          const float eta = fminf(eta_max, sqrtf(rel));
          s[NEWTON] += 1.f;
          s[RR] = (float)gn2;
          s[CGTOL2] = (eta * gn) * (eta * gn);
          s[CGLAST] = s[CGIT];
          s[CGIT] = 0.f;
        }
        s[ACTIVE] = act ? 1.f : 0.f;
      }
      s[CGACT] = act ? 1.f : 0.f;
    }
    go = act;
  }
  __syncthreads();
  if (!go) return;
  float* x = X + (size_t)p * ld;
  float* r = R + (size_t)p * ld;
  float* d = D + (size_t)p * ld;
  for (int k = threadIdx.x; k < n; k += NT) {
    x[k] = 0.f;
    r[k] = -g[k];
    d[k] = -g[k];
  }
}

// One CG iteration per problem still solving: alpha = r.r / d.Hd, x += alpha d, r -= alpha Hd, then stop (||r||^2 <= tol) or d = r + beta d.
// The two dot products become floats before anything is compared or divided: alpha, beta and the tests are float arithmetic in both policies.
template <class Red, int STRIDE>
__global__ __launch_bounds__(NT) void cg_update_kernel(const float* HD, int ld, int n, float* X, float* R, float* D, float* st) {
  using acc_t = typename Red::acc_t;
  __shared__ acc_t red[Red::SCRATCH];
  const int p = blockIdx.x;
  float* s = st + (size_t)p * STRIDE;
  if (s[CGACT] == 0.f) return;                   // uniform over the workgroup; only this workgroup writes s
  const float rr = s[RR], tol2 = s[CGTOL2];
  const float* hd = HD + (size_t)p * ld;
  float* x = X + (size_t)p * ld;
  float* r = R + (size_t)p * ld;
  float* d = D + (size_t)p * ld;
  acc_t a = 0;
  for (int k = threadIdx.x; k < n; k += NT) a += (acc_t)d[k] * (acc_t)hd[k];
  const float dhd = (float)Red::sum(a, red);
  if (!(dhd > 0.f) || !(rr > 0.f)) {             // H >= I: only a zero direction gets here
    __syncthreads();
    if (threadIdx.x == 0) s[CGACT] = 0.f;
    return;
  }
  const float alpha = rr / dhd;
  a = 0;
  for (int k = threadIdx.x; k < n; k += NT) {
    x[k] += alpha * d[k];
    const float rk = r[k] - alpha * hd[k];
    r[k] = rk;
    a += (acc_t)rk * (acc_t)rk;
  }
  const float rn = (float)Red::sum(a, red);
  const bool stop = rn <= tol2;
  if (!stop) {
    const float beta = rn / rr;
    for (int k = threadIdx.x; k < n; k += NT) d[k] = r[k] + beta * d[k];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    s[CGIT] += 1.f;
    s[CGTOT] += 1.f;
    if (stop) s[CGACT] = 0.f;
    else s[RR] = rn;
  }
}

// One safeguarded Newton step of a line search on phi' inside the bracket [lo, hi] (phi'(lo) < 0 < phi'(hi)), from phi'(t) = g != 0 and
// phi''(t) = h > 0: t becomes the bracket end on its side, and the Newton point t - g / h is taken unless it leaves the bracket; then the
// midpoint, or 2 t while no right end is known (hi infinite). Returns the next t; when to stop is the caller's business.
DEV float bracket_newton_step(float t, float g, float h, float& lo, float& hi) {
  if (g < 0.f) lo = t;
  else hi = t;
  float tn = t - g / h;
  if (!(tn > lo && tn < hi)) tn = hi < INFINITY ? 0.5f * (lo + hi) : 2.f * t;
  return tn;
}

}  // namespace ncg
}  // namespace clite
#endif  // CLITE_NEWTON_CG_H
