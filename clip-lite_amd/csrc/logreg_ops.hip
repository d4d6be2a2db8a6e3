// Logistic-regression probe (clip-lite_amd/logreg.py): the kernels around the GEMMs of a batched Newton-CG solve of P independent L2-regularised
// multinomial logistic regressions that share one feature matrix X~ [N][Dp],
//   f_p(W) = 1/2 |W|_F^2 + c_p sum_i w_ip (logsumexp(W x~_i) - (W x~_i)[y_i]).
//
// Layouts. Logits and every per-row operand: f32 [N][ldz], problem p owning the Cp = ceil8(C) columns from p * Cp (the output of clite_gemm_nt
// X~ W^T); its C real columns form one softmax group per row, its padding columns are written as zeros and take no part. Weights, gradients and
// the CG vectors: f32 [P * Cp][Dp], so a problem's vector is one contiguous span of n = Cp * Dp floats. Per-problem scalars live in a device
// state table f32 [P][CLITE_LOGREG_STATE], so a whole CG loop and a whole line search are enqueued without a host read-back.
//
// Row kernels: one wave owns one (row, problem) group, loads it once with 16-byte loads into registers (LG_R chunks per lane, C <= 4096) and
// reduces with wave shuffles; a workgroup owns CLITE_LOGREG_ROWS rows of one problem. They stream [N][P * Cp] once and are HBM-bound; the GEMMs
// carry the FLOPs. Every sum is formed in one fixed order (shuffle butterflies, LDS trees, partials in block order), no float
// atomics: reruns are bit-identical whatever the deterministic switch says.
#include "newton_cg.h"

using namespace clite;

namespace {

using ncg::block_sum_d;

// the line search's columns, after the shared ones (ncg::G0 ... ncg::DPHI0, newton_cg.h)
enum {
  L_T = ncg::NCG_COLS, L_LO, L_HI, L_WD, L_DD, L_LSDONE, L_SPARE0, L_SPARE1, L_EVALS
};
static_assert(L_T == 13, "include/clite.h documents the columns by number");
static_assert(L_EVALS < CLITE_LOGREG_STATE, "state table too narrow");

constexpr int NT = ncg::NT;                   // threads of every workgroup here
constexpr int ROWS = CLITE_LOGREG_ROWS;       // rows per workgroup of the row kernels
constexpr float LS_TOL = 1e-4f;               // the line search stops at |phi'(t)| <= LS_TOL |phi'(0)|

// column of element e of chunk u of this lane
DEV int col_of(int u, int lane) { return (u * 64 + lane) * 4; }

template <int R> DEV void load_group(const float* g, int Cp, int lane, f32x4 (&v)[R]) {
#pragma unroll
  for (int u = 0; u < R; ++u) {
    const int j = col_of(u, lane);
    v[u] = j < Cp ? *(const f32x4*)(g + j) : f32x4{0.f, 0.f, 0.f, 0.f};        // Cp % 8 == 0: a chunk that starts inside the group ends inside it
  }
}

// v <- exp(v - M) over the C real columns (0 in the padding), M = max, returns S = sum of the exponentials (>= 1)
template <int R> DEV float group_exp(f32x4 (&v)[R], int C, int lane, float& M) {
  float m = -INFINITY;
#pragma unroll
  for (int u = 0; u < R; ++u)
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (col_of(u, lane) + e < C) m = fmaxf(m, v[u][e]);
  M = wave_max(m);
  float s = 0.f;
#pragma unroll
  for (int u = 0; u < R; ++u)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float x = col_of(u, lane) + e < C ? expf(v[u][e] - M) : 0.f;
      v[u][e] = x;
      s += x;
    }
  return wave_sum(s);
}

// Pr = softmax(z), S = c w (Pr - onehot(y)); part[row block][p] = sum over the block's rows of c w (lse - z_y)
template <int R>
__global__ __launch_bounds__(NT) void logreg_softmax_kernel(const float* Z, const int* y, const float* cost, const float* w, int N, int P, int C,
                                                            int Cp, int ldz, float* Pr, float* S, float* part) {
  __shared__ double red[4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int p = blockIdx.y;
  const int r0 = blockIdx.x * ROWS, r1 = N < r0 + ROWS ? N : r0 + ROWS;
  const float c = cost[p];
  double acc = 0.0;
  for (int i = r0 + wv; i < r1; i += 4) {
    const size_t o = (size_t)i * ldz + (size_t)p * Cp;
    f32x4 v[R];
    load_group<R>(Z + o, Cp, lane, v);
    const int yi = y[i];
    const int yy = yi >= 0 && yi < C ? yi : -1;            // the host validates labels; a bad one is never read through
    const float cw = c * w[(size_t)i * P + p];
    const float zy = yy >= 0 ? Z[o + yy] : 0.f;
    float M;
    const float sum = group_exp<R>(v, C, lane, M);
    const float inv = 1.f / sum;
#pragma unroll
    for (int u = 0; u < R; ++u) {
      const int j = col_of(u, lane);
      if (j < Cp) {
        f32x4 pr, s;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          pr[e] = v[u][e] * inv;
          s[e] = j + e < C ? cw * (pr[e] - (j + e == yy ? 1.f : 0.f)) : 0.f;
        }
        *(f32x4*)(Pr + o + j) = pr;
        *(f32x4*)(S + o + j) = s;
      }
    }
    if (yy >= 0 && cw > 0.f) acc += (double)cw * ((double)logf(sum) + (double)(M - zy));
  }
  if (lane == 0) red[wv] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part[(size_t)blockIdx.x * P + p] = (float)((red[0] + red[1]) + (red[2] + red[3]));
}

// out[p] = sum over row blocks of part[b][p], in a fixed order: one workgroup per problem
__global__ __launch_bounds__(NT) void logreg_partsum_kernel(const float* part, int nb, int P, float* out) {
  __shared__ double red[NT];
  const int p = blockIdx.x;
  double a = 0.0;
  for (int b = threadIdx.x; b < nb; b += NT) a += (double)part[(size_t)b * P + p];
  const double t = block_sum_d(a, red);
  if (threadIdx.x == 0) out[p] = (float)t;
}

// q <- c w Pr (q - <Pr, q>) per group, in place; zeros in the padding columns and in a held-out group (nothing of it is read)
template <int R>
__global__ __launch_bounds__(NT) void logreg_hess_kernel(const float* Pr, const float* cost, const float* w, int N, int P, int C, int Cp, int ldz,
                                                         float* Q) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int p = blockIdx.y;
  const int r0 = blockIdx.x * ROWS, r1 = N < r0 + ROWS ? N : r0 + ROWS;
  const float c = cost[p];
  for (int i = r0 + wv; i < r1; i += 4) {
    const size_t o = (size_t)i * ldz + (size_t)p * Cp;
    const float cw = c * w[(size_t)i * P + p];
    f32x4 pr[R], q[R];
    if (cw > 0.f) {                                        // uniform over the wave
      load_group<R>(Pr + o, Cp, lane, pr);
      load_group<R>(Q + o, Cp, lane, q);
      float d = 0.f;
#pragma unroll
      for (int u = 0; u < R; ++u)
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (col_of(u, lane) + e < C) d += pr[u][e] * q[u][e];
      d = wave_sum(d);
#pragma unroll
      for (int u = 0; u < R; ++u)
#pragma unroll
        for (int e = 0; e < 4; ++e) q[u][e] = col_of(u, lane) + e < C ? cw * pr[u][e] * (q[u][e] - d) : 0.f;
    } else {
#pragma unroll
      for (int u = 0; u < R; ++u) q[u] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int u = 0; u < R; ++u) {
      const int j = col_of(u, lane);
      if (j < Cp) *(f32x4*)(Q + o + j) = q[u];
    }
  }
}

// One evaluation of the line search at t_p: with pi = softmax(z + t delta) per group,
//   part1[b][p] = sum_i c w (<pi, delta> - delta[y]),  part2[b][p] = sum_i c w Var_pi(delta)   over the rows of block b.
// A problem whose search is over is skipped (its partials are not read either).
template <int R>
__global__ __launch_bounds__(NT) void logreg_ray_kernel(const float* Z, const float* Dl, const int* y, const float* cost, const float* w, int N,
                                                        int P, int C, int Cp, int ldz, const float* st, float* part1, float* part2) {
  __shared__ double red1[4], red2[4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int p = blockIdx.y;
  const float* s = st + (size_t)p * CLITE_LOGREG_STATE;
  if (s[L_LSDONE] != 0.f) return;                          // uniform over the workgroup
  const float t = s[L_T];
  const int r0 = blockIdx.x * ROWS, r1 = N < r0 + ROWS ? N : r0 + ROWS;
  const float c = cost[p];
  double a1 = 0.0, a2 = 0.0;
  for (int i = r0 + wv; i < r1; i += 4) {
    const float cw = c * w[(size_t)i * P + p];
    if (!(cw > 0.f)) continue;                             // uniform over the wave
    const size_t o = (size_t)i * ldz + (size_t)p * Cp;
    f32x4 v[R], d[R];
    load_group<R>(Z + o, Cp, lane, v);
    load_group<R>(Dl + o, Cp, lane, d);
    const int yi = y[i];
    const float dy = yi >= 0 && yi < C ? Dl[o + yi] : 0.f;
#pragma unroll
    for (int u = 0; u < R; ++u)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (col_of(u, lane) + e >= C) d[u][e] = 0.f;                     // whatever the padding of delta holds takes no part
        v[u][e] += t * d[u][e];
      }
    float M;
    const float sum = group_exp<R>(v, C, lane, M);
    const float inv = 1.f / sum;
    float m1 = 0.f;
#pragma unroll
    for (int u = 0; u < R; ++u)
#pragma unroll
      for (int e = 0; e < 4; ++e) m1 += v[u][e] * d[u][e];             // v and d are 0 in the padding
    m1 = wave_sum(m1) * inv;
    float var = 0.f;
#pragma unroll
    for (int u = 0; u < R; ++u)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float x = d[u][e] - m1;
        var += v[u][e] * x * x;
      }
    var = wave_sum(var) * inv;
    a1 += (double)cw * (double)(m1 - dy);
    a2 += (double)cw * (double)var;
  }
  if (lane == 0) {
    red1[wv] = a1;
    red2[wv] = a2;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    part1[(size_t)blockIdx.x * P + p] = (float)((red1[0] + red1[1]) + (red1[2] + red1[3]));
    part2[(size_t)blockIdx.x * P + p] = (float)((red2[0] + red2[1]) + (red2[2] + red2[3]));
  }
}

// newton_begin and cg_update are the shared Newton-CG kernels (newton_cg.h) over a problem's span of n = Cp * Dp floats, with the dots in
// double through the LDS tree, and with the rule set a warm start needs: |g0| = |grad f(0)| is recorded by a g0_only call at W = 0, or by the
// first call when none was made (a cold start, where W = 0), and a problem whose line search ended at step 0 is frozen.
constexpr auto logreg_newton_begin_kernel = ncg::newton_begin_kernel<ncg::DoubleTree, CLITE_LOGREG_STATE, ncg::Rules::RecordedG0>;
constexpr auto logreg_cg_update_kernel = ncg::cg_update_kernel<ncg::DoubleTree, CLITE_LOGREG_STATE>;

// Start of the line search along D for one problem per workgroup: phi'(0) = <G, D>, <W, D>, |D|^2; t = 1, bracket [0, inf). A problem that is
// not active, or whose D is no descent direction, is done at t = 0.
__global__ __launch_bounds__(NT) void logreg_ray_begin_kernel(const float* G, const float* W, const float* D, int ld, int n, float* st) {
  __shared__ double red[NT];
  const int p = blockIdx.x;
  float* s = st + (size_t)p * CLITE_LOGREG_STATE;
  const float* g = G + (size_t)p * ld;
  const float* w = W + (size_t)p * ld;
  const float* d = D + (size_t)p * ld;
  double gd = 0.0, wd = 0.0, dd = 0.0;
  for (int k = threadIdx.x; k < n; k += NT) {
    const double dk = (double)d[k];
    gd += (double)g[k] * dk;
    wd += (double)w[k] * dk;
    dd += dk * dk;
  }
  gd = block_sum_d(gd, red);
  wd = block_sum_d(wd, red);
  dd = block_sum_d(dd, red);
  if (threadIdx.x == 0) {
    const bool go = s[ncg::ACTIVE] != 0.f && (float)gd < 0.f && (float)dd > 0.f;
    s[ncg::DPHI0] = (float)gd;
    s[L_WD] = (float)wd;
    s[L_DD] = (float)dd;
    s[L_T] = go ? 1.f : 0.f;
    s[L_LO] = 0.f;
    s[L_HI] = INFINITY;
    s[L_EVALS] = 0.f;
    s[ncg::STEP] = 0.f;
    s[L_LSDONE] = go ? 0.f : 1.f;
  }
}

// One workgroup: for every problem still searching, phi'(t) and phi''(t) from the row-block partials (summed in block order), then a safeguarded
// Newton step on phi' inside the bracket [lo, hi] (phi'(lo) < 0 < phi'(hi)); bisection (or doubling while hi is infinite) when the step leaves it.
__global__ __launch_bounds__(NT) void logreg_ray_step_kernel(const float* part1, const float* part2, int nb, int P, float* st, int last) {
  __shared__ double red[NT];
  for (int p = 0; p < P; ++p) {
    float* s = st + (size_t)p * CLITE_LOGREG_STATE;
    if (s[L_LSDONE] != 0.f) continue;            // uniform: s is written below only after the last read of this flag (barriers in block_sum_d)
    double a = 0.0, b = 0.0;
    for (int k = threadIdx.x; k < nb; k += NT) {
      a += (double)part1[(size_t)k * P + p];
      b += (double)part2[(size_t)k * P + p];
    }
    a = block_sum_d(a, red);
    b = block_sum_d(b, red);
    __syncthreads();
    if (threadIdx.x == 0) {
      const float t = s[L_T];
      const float g = (float)((double)s[L_WD] + (double)t * (double)s[L_DD] + a);      // phi'(t)
      const float h = (float)((double)s[L_DD] + b);                                   // phi''(t) >= |D|^2 > 0
      s[L_EVALS] += 1.f;
      if (fabsf(g) <= LS_TOL * fabsf(s[ncg::DPHI0])) {
        s[ncg::STEP] = t;
        s[L_LSDONE] = 1.f;
      } else {
        const float tn = ncg::bracket_newton_step(t, g, h, s[L_LO], s[L_HI]);
        if (tn == t) {
          s[ncg::STEP] = t;
          s[L_LSDONE] = 1.f;
        } else if (last) {                       // out of evaluations: the bracket's left end. phi' < 0 on [0, lo], so phi(lo) <= phi(0); a point
          s[ncg::STEP] = s[L_LO];                // right of the minimiser has no such guarantee, so with no left end found the step is 0
          s[L_LSDONE] = 1.f;
        } else {
          s[L_T] = tn;
        }
      }
    }
    __syncthreads();
  }
}

// W_p += step_p D_p for every problem that took a step
__global__ __launch_bounds__(NT) void logreg_ray_finish_kernel(float* W, const float* D, int ld, int n, const float* st) {
  const int p = blockIdx.y;
  const float* s = st + (size_t)p * CLITE_LOGREG_STATE;
  const float t = s[L_LSDONE] != 0.f ? s[ncg::STEP] : 0.f;
  if (t == 0.f) return;
  float* w = W + (size_t)p * ld;
  const float* d = D + (size_t)p * ld;
  for (int k = blockIdx.x * NT + threadIdx.x; k < n; k += gridDim.x * NT) w[k] += t * d[k];
}

}  // namespace

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
static int ceil8(int n) { return (n + 7) / 8 * 8; }

// 0 when the row-operand shape is valid, else the error code
static int rows_shape(int N, int P, int C, int ldz) {
  if (N <= 0 || P <= 0 || P > 65535 || C < 1 || ldz <= 0 || ldz % 4) return -1;
  if (C > CLITE_LOGREG_MAX_CLASSES) return -2;
  if ((long long)P * ceil8(C) > (long long)ldz) return -1;
  return 0;
}

// chunks of 4 columns per lane that hold a group of Cp columns: 1, 2, 4, 8 or 16
#define LOGREG_DISPATCH(Cp, LAUNCH)            \
  if ((Cp) <= 256) { LAUNCH(1); }              \
  else if ((Cp) <= 512) { LAUNCH(2); }         \
  else if ((Cp) <= 1024) { LAUNCH(4); }        \
  else if ((Cp) <= 2048) { LAUNCH(8); }        \
  else { LAUNCH(16); }

extern "C" int clite_logreg_softmax(const float* Z, const int* y, const float* costs, const float* w, int N, int P, int C, int ldz, float* Pr, float* S,
                                    float* loss, float* work, void* stream) {
  if (!Z || !y || !costs || !w || !Pr || !S || !loss || !work || !aligned16(Z) || !aligned16(Pr) || !aligned16(S)) return -1;
  if (const int rc = rows_shape(N, P, C, ldz)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int Cp = ceil8(C), nb = (N + ROWS - 1) / ROWS;
#define LAUNCH(R) hipLaunchKernelGGL(logreg_softmax_kernel<R>, dim3(nb, P), dim3(NT), 0, st, Z, y, costs, w, N, P, C, Cp, ldz, Pr, S, work)
  LOGREG_DISPATCH(Cp, LAUNCH)
#undef LAUNCH
  hipLaunchKernelGGL(logreg_partsum_kernel, dim3(P), dim3(NT), 0, st, (const float*)work, nb, P, loss);
  return (int)hipGetLastError();
}

extern "C" int clite_logreg_hess_apply(const float* Pr, const float* costs, const float* w, int N, int P, int C, int ldz, float* Q, void* stream) {
  if (!Pr || !costs || !w || !Q || !aligned16(Pr) || !aligned16(Q)) return -1;
  if (const int rc = rows_shape(N, P, C, ldz)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int Cp = ceil8(C), nb = (N + ROWS - 1) / ROWS;
#define LAUNCH(R) hipLaunchKernelGGL(logreg_hess_kernel<R>, dim3(nb, P), dim3(NT), 0, st, Pr, costs, w, N, P, C, Cp, ldz, Q)
  LOGREG_DISPATCH(Cp, LAUNCH)
#undef LAUNCH
  return (int)hipGetLastError();
}

extern "C" int clite_logreg_newton_begin(const float* G, int ld, int n, int P, float* X, float* R, float* D, float* state, float tol, int max_newton,
                                         float eta_max, int g0_only, void* stream) {
  if (!G || !X || !R || !D || !state || P <= 0 || n <= 0 || ld < n || max_newton < 0 || !(eta_max > 0.f) || !(tol >= 0.f)) return -1;
  hipLaunchKernelGGL(logreg_newton_begin_kernel, dim3(P), dim3(NT), 0, (hipStream_t)stream, G, ld, n, X, R, D, state, tol, max_newton, eta_max,
                     g0_only);
  return (int)hipGetLastError();
}

extern "C" int clite_logreg_cg_update(const float* HD, int ld, int n, int P, float* X, float* R, float* D, float* state, void* stream) {
  if (!HD || !X || !R || !D || !state || P <= 0 || n <= 0 || ld < n) return -1;
  hipLaunchKernelGGL(logreg_cg_update_kernel, dim3(P), dim3(NT), 0, (hipStream_t)stream, HD, ld, n, X, R, D, state);
  return (int)hipGetLastError();
}

extern "C" int clite_logreg_ray_begin(const float* G, const float* W, const float* D, int ld, int n, int P, float* state, void* stream) {
  if (!G || !W || !D || !state || P <= 0 || n <= 0 || ld < n) return -1;
  hipLaunchKernelGGL(logreg_ray_begin_kernel, dim3(P), dim3(NT), 0, (hipStream_t)stream, G, W, D, ld, n, state);
  return (int)hipGetLastError();
}

extern "C" int clite_logreg_ray_eval(const float* Z, const float* delta, const int* y, const float* costs, const float* w, int N, int P, int C,
                                     int ldz, const float* state, float* work, void* stream) {
  if (!Z || !delta || !y || !costs || !w || !state || !work || !aligned16(Z) || !aligned16(delta)) return -1;
  if (const int rc = rows_shape(N, P, C, ldz)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int Cp = ceil8(C), nb = (N + ROWS - 1) / ROWS;
  float* part2 = work + (size_t)nb * P;
#define LAUNCH(R) hipLaunchKernelGGL(logreg_ray_kernel<R>, dim3(nb, P), dim3(NT), 0, st, Z, delta, y, costs, w, N, P, C, Cp, ldz, state, work, part2)
  LOGREG_DISPATCH(Cp, LAUNCH)
#undef LAUNCH
  return (int)hipGetLastError();
}

extern "C" int clite_logreg_ray_step(const float* work, int N, int P, float* state, int last, void* stream) {
  if (!work || !state || N <= 0 || P <= 0) return -1;
  const int nb = (N + ROWS - 1) / ROWS;
  hipLaunchKernelGGL(logreg_ray_step_kernel, dim3(1), dim3(NT), 0, (hipStream_t)stream, work, work + (size_t)nb * P, nb, P, state, last);
  return (int)hipGetLastError();
}

extern "C" int clite_logreg_ray_finish(float* W, const float* D, int ld, int n, int P, const float* state, void* stream) {
  if (!W || !D || !state || P <= 0 || P > 65535 || n <= 0 || ld < n) return -1;
  int gx = (n + NT - 1) / NT;
  if (gx > 1024) gx = 1024;
  hipLaunchKernelGGL(logreg_ray_finish_kernel, dim3(gx, P), dim3(NT), 0, (hipStream_t)stream, W, D, ld, n, state);
  return (int)hipGetLastError();
}
