// VOC07 SVM evaluation (reference voc_clf.py:75-121): the kernels around the GEMMs of a batched Newton-CG solve of P independent L2-regularised
// squared-hinge problems that share one feature matrix X~ [N][Dp] (clip-lite_amd/svm.py), and the per-column average precision.
//
// Layouts. Margins, labels, weights, gradient operands: f32 [N][ldp], one column per problem (the output of clite_gemm_nt X~ W^T). Weights,
// gradients and the CG vectors: f32 [ldp][Dp], one row per problem (the output of clite_gemm_tn). Per-problem scalars live in a device
// state table f32 [P][CLITE_SVM_STATE] (include/clite.h), so a whole CG loop is enqueued without a host read-back.
//
// Every reduction here runs in one fixed order (a workgroup owns each sum; partials meet in LDS in index order), so the solver is bitwise
// reproducible whatever the deterministic switch says. Column kernels give a workgroup SVM_CB adjacent problems and split its rows over
// 256 / SVM_CB row groups: a wave reads 64 / SVM_CB rows of SVM_CB * 4 contiguous bytes. Everything is memory- or latency-bound; the GEMMs
// carry the FLOPs.
#include "newton_cg.h"

using namespace clite;

namespace {

static_assert(ncg::DPHI0 < CLITE_SVM_STATE, "state table too narrow");      // the state columns are ncg:: (newton_cg.h), nothing added

constexpr int NT = ncg::NT;               // threads of every workgroup here
constexpr int SVM_CB = 8;                 // problems per workgroup of the column kernels
constexpr int SVM_RG = NT / SVM_CB;       // row groups
constexpr int MARGIN_ROWS = 512;          // rows per workgroup of the margin kernel (grid.y = ceil(N / 512))
constexpr int LS_MAX = 24;                // line-search iterations (safeguarded Newton on a piecewise quadratic; usually 2-4)
constexpr int AP_MAX = CLITE_SVM_AP_MAX_ROWS;

// S = c 1_I (z - y), H = c 1_I with I = {y z < 1}; part[blockIdx.y][p] = sum over this block's rows of c max(0, 1 - y z)^2.
// Columns p in [P, ldp) are written as zeros (they feed the GEMMs).
__global__ __launch_bounds__(NT) void svm_margin_kernel(const float* Z, const float* Y, const float* Cw, int N, int P, int ldp, float* S,
                                                        float* H, float* part) {
  __shared__ float red[SVM_RG][SVM_CB + 1];
  const int c = threadIdx.x % SVM_CB, rg = threadIdx.x / SVM_CB;
  const int p = blockIdx.x * SVM_CB + c;
  const int r0 = blockIdx.y * MARGIN_ROWS, r1 = N < r0 + MARGIN_ROWS ? N : r0 + MARGIN_ROWS;
  float acc = 0.f;
  if (p < ldp) {
    for (int i0 = r0 + rg; i0 < r1; i0 += 4 * SVM_RG) {
      float z[4], y[4], w[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = i0 + u * SVM_RG;
        const size_t o = (size_t)i * ldp + p;
        const bool ok = i < r1 && p < P;
        z[u] = ok ? Z[o] : 0.f;
        y[u] = ok ? Y[o] : 0.f;
        w[u] = ok ? Cw[o] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = i0 + u * SVM_RG;
        if (i >= r1) break;
        const float m = 1.f - y[u] * z[u];
        const bool in = m > 0.f && w[u] > 0.f;
        const size_t o = (size_t)i * ldp + p;
        S[o] = in ? w[u] * (z[u] - y[u]) : 0.f;
        H[o] = in ? w[u] : 0.f;
        if (in) acc += w[u] * m * m;
      }
    }
  }
  red[rg][c] = acc;
  __syncthreads();
  if (rg == 0 && p < ldp) {
    float t = 0.f;
    for (int k = 0; k < SVM_RG; ++k) t += red[k][c];
    part[(size_t)blockIdx.y * ldp + p] = t;
  }
}

// loss[p] = sum over row blocks of part[b][p], in block order
__global__ __launch_bounds__(NT) void svm_colsum_kernel(const float* part, int nb, int P, int ldp, float* loss) {
  const int p = blockIdx.x * NT + threadIdx.x;
  if (p >= P) return;
  float t = 0.f;
  for (int b = 0; b < nb; ++b) t += part[(size_t)b * ldp + p];
  loss[p] = t;
}

// Q *= H elementwise (n % 4 == 0): the Hessian's diagonal applied to X~ d
__global__ __launch_bounds__(NT) void svm_hess_scale_kernel(const float* H, float* Q, size_t n4) {
  for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < n4; i += (size_t)gridDim.x * NT) {
    f32x4 h = ((const f32x4*)H)[i], q = ((f32x4*)Q)[i];
    ((f32x4*)Q)[i] = f32x4{q[0] * h[0], q[1] * h[1], q[2] * h[2], q[3] * h[3]};
  }
}

// newton_begin and cg_update are the shared Newton-CG kernels (newton_cg.h) with float sums over 4 floats of LDS, and with the rule set in which
// g0 is the first gradient seen and a zero step does not freeze a problem.
constexpr auto svm_newton_begin_kernel = ncg::newton_begin_kernel<ncg::FloatSum, CLITE_SVM_STATE, ncg::Rules::FirstGradient>;
constexpr auto svm_cg_update_kernel = ncg::cg_update_kernel<ncg::FloatSum, CLITE_SVM_STATE>;

// Step length along the Newton direction x for SVM_CB problems per workgroup: the minimiser of the convex piecewise quadratic
//   phi(t) = 1/2 |w + t x|^2 + sum_i c_i max(0, 1 - y_i (z_i + t delta_i))^2,   delta = X~ x,
// by Newton's method on phi' inside a bracket [lo, hi] (phi'(lo) < 0 < phi'(hi)), starting from t = 1; bisection when a step leaves it.
// Then w += t x. A problem that is not active, or whose x is no descent direction, takes t = 0.
__global__ __launch_bounds__(NT) void svm_line_search_kernel(const float* Z, const float* Dl, const float* Y, const float* Cw, int N, int P,
                                                            int ldp, float* W, const float* X, int ld, int Dp, float* st) {
  __shared__ float red1[SVM_RG][SVM_CB + 1], red2[SVM_RG][SVM_CB + 1];
  __shared__ float sh_t[SVM_CB], sh_lo[SVM_CB], sh_hi[SVM_CB], sh_wx[SVM_CB], sh_xx[SVM_CB], sh_d0[SVM_CB];
  __shared__ int sh_done[SVM_CB], sh_all;
  const int p0 = blockIdx.x * SVM_CB;
  // w.x and x.x: SVM_RG consecutive threads per problem walk its row
  {
    const int q = threadIdx.x / SVM_RG, part = threadIdx.x % SVM_RG, p = p0 + q;
    float wx = 0.f, xx = 0.f;
    if (p < P) {
      const float* w = W + (size_t)p * ld;
      const float* x = X + (size_t)p * ld;
      for (int k = part; k < Dp; k += SVM_RG) {
        wx += w[k] * x[k];
        xx += x[k] * x[k];
      }
    }
    red1[part][q] = wx;
    red2[part][q] = xx;
    __syncthreads();
    if (threadIdx.x < SVM_CB) {
      const int pp = p0 + threadIdx.x;
      float a = 0.f, b = 0.f;
      for (int k = 0; k < SVM_RG; ++k) {
        a += red1[k][threadIdx.x];
        b += red2[k][threadIdx.x];
      }
      sh_wx[threadIdx.x] = a;
      sh_xx[threadIdx.x] = b;
      const bool act = pp < P && st[(size_t)pp * CLITE_SVM_STATE + ncg::ACTIVE] != 0.f;
      sh_t[threadIdx.x] = 0.f;                   // the first pass evaluates phi'(0) = g.x
      sh_lo[threadIdx.x] = 0.f;
      sh_hi[threadIdx.x] = INFINITY;
      sh_done[threadIdx.x] = act ? 0 : 1;
    }
    __syncthreads();
  }
  const int c = threadIdx.x % SVM_CB, rg = threadIdx.x / SVM_CB;
  const int p = p0 + c;
  for (int it = 0; it <= LS_MAX; ++it) {
    const float t = sh_t[c];
    float d1 = 0.f, d2 = 0.f;
    if (p < P && !sh_done[c]) {
      for (int i0 = rg; i0 < N; i0 += 4 * SVM_RG) {
        float z[4], dl[4], y[4], w[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int i = i0 + u * SVM_RG;
          const size_t o = (size_t)i * ldp + p;
          const bool ok = i < N;
          z[u] = ok ? Z[o] : 0.f;
          dl[u] = ok ? Dl[o] : 0.f;
          y[u] = ok ? Y[o] : 0.f;
          w[u] = ok ? Cw[o] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const float zt = z[u] + t * dl[u];
          if (w[u] > 0.f && y[u] * zt < 1.f) {
            d1 += w[u] * (zt - y[u]) * dl[u];
            d2 += w[u] * dl[u] * dl[u];
          }
        }
      }
    }
    red1[rg][c] = d1;
    red2[rg][c] = d2;
    __syncthreads();
    if (threadIdx.x < SVM_CB && !sh_done[threadIdx.x]) {
      const int q = threadIdx.x;
      float a = 0.f, b = 0.f;
      for (int k = 0; k < SVM_RG; ++k) {
        a += red1[k][q];
        b += red2[k][q];
      }
      const float tq = sh_t[q];
      const float g = sh_wx[q] + tq * sh_xx[q] + 2.f * a;       // phi'(t)
      const float h = sh_xx[q] + 2.f * b;                        // phi''(t) on the current piece, >= |x|^2
      if (it == 0) {
        sh_d0[q] = g;
        if (!(g < 0.f) || !(h > 0.f)) {            // no descent along x: stay
          sh_done[q] = 1;
        } else {
          sh_t[q] = 1.f;
        }
      } else if (fabsf(g) <= 1e-6f * fabsf(sh_d0[q])) {
        sh_done[q] = 1;
      } else {
        const float tn = ncg::bracket_newton_step(tq, g, h, sh_lo[q], sh_hi[q]);
        if (tn == tq) sh_done[q] = 1;
        else if (it == LS_MAX) sh_t[q] = sh_lo[q];   // out of iterations: the last point known to lie left of the minimiser
        else sh_t[q] = tn;
      }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      int all = 1;
      for (int q = 0; q < SVM_CB; ++q) all &= sh_done[q];
      sh_all = all;
    }
    __syncthreads();
    if (sh_all) break;
  }
  // w += t x for the active problems of this workgroup
  for (int q = 0; q < SVM_CB; ++q) {
    const int pp = p0 + q;
    if (pp >= P) break;
    float* s = st + (size_t)pp * CLITE_SVM_STATE;
    if (s[ncg::ACTIVE] == 0.f) continue;
    const float t = sh_t[q];
    float* w = W + (size_t)pp * ld;
    const float* x = X + (size_t)pp * ld;
    if (t != 0.f)
      for (int k = threadIdx.x; k < Dp; k += NT) w[k] += t * x[k];
    if (threadIdx.x == 0) {
      s[ncg::STEP] = t;
      s[ncg::DPHI0] = sh_d0[q];
    }
  }
}

// ------------------------------------------------------------------------------------------------ average precision
// order-preserving map of a float onto uint32 (ascending); -0 and +0 map to one key (they are one threshold)
DEV uint32_t ordered_bits(float f) {
  if (f == 0.f) f = 0.f;
  const uint32_t u = __builtin_bit_cast(uint32_t, f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// One workgroup per column: sklearn.metrics.average_precision_score of (target > 0) against the score over the rows whose target is >= 0.
// Keys (score bits << 32 | valid << 1 | positive) are bitonic-sorted in LDS, descending; ignored and padding rows are key 0 and sort last.
// AP = sum over tie groups (distinct thresholds) of (positives in the group / all positives) * precision at the group's last row.
__global__ __launch_bounds__(NT) void average_precision_kernel(const float* scores, int lds, const float* targets, int ldt, int N, float* ap) {
  __shared__ uint64_t key[AP_MAX];
  __shared__ int tpa[AP_MAX];
  __shared__ int scan_p[NT], scan_s[NT];
  __shared__ double dred[NT];
  const int col = blockIdx.x, tid = threadIdx.x;
  int L = 256;
  while (L < N) L <<= 1;
  for (int j = tid; j < L; j += NT) {
    uint64_t k = 0;
    if (j < N) {
      const float t = targets[(size_t)j * ldt + col];
      if (t >= 0.f) k = ((uint64_t)ordered_bits(scores[(size_t)j * lds + col]) << 32) | 2u | (t > 0.f ? 1u : 0u);
    }
    key[j] = k;
  }
  __syncthreads();
  for (int k = 2; k <= L; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < L; i += NT) {
        const int ixj = i ^ j;
        if (ixj > i) {
          const uint64_t a = key[i], b = key[ixj];
          const bool desc = (i & k) == 0;
          if (desc ? (a < b) : (a > b)) {
            key[i] = b;
            key[ixj] = a;
          }
        }
      }
      __syncthreads();
    }
  }
  // each thread owns C consecutive sorted rows
  const int C = L / NT, j0 = tid * C;
  int np = 0, last_start = -1;
  for (int j = j0; j < j0 + C; ++j) {
    const uint64_t kj = key[j];
    if (!(kj & 2u)) break;
    np += (int)(kj & 1u);
    if (j == 0 || (uint32_t)(key[j - 1] >> 32) != (uint32_t)(kj >> 32) || !(key[j - 1] & 2u)) last_start = j;
  }
  scan_p[tid] = np;
  scan_s[tid] = last_start;
  __syncthreads();
  for (int off = 1; off < NT; off <<= 1) {       // inclusive scans: sum of positives, max of tie-group starts
    const int vp = tid >= off ? scan_p[tid - off] : 0;
    const int vs = tid >= off ? scan_s[tid - off] : -1;
    __syncthreads();
    scan_p[tid] += vp;
    if (vs > scan_s[tid]) scan_s[tid] = vs;
    __syncthreads();
  }
  const int npos = scan_p[NT - 1];
  int tp = tid > 0 ? scan_p[tid - 1] : 0;
  int start = tid > 0 ? scan_s[tid - 1] : -1;
  for (int j = j0; j < j0 + C; ++j) {
    const uint64_t kj = key[j];
    if (!(kj & 2u)) break;
    tp += (int)(kj & 1u);
    tpa[j] = tp;
  }
  __syncthreads();
  double acc = 0.0;
  for (int j = j0; j < j0 + C; ++j) {
    const uint64_t kj = key[j];
    if (!(kj & 2u)) break;
    if (j == 0 || (uint32_t)(key[j - 1] >> 32) != (uint32_t)(kj >> 32)) start = j;
    const bool end = j + 1 == L || !(key[j + 1] & 2u) || (uint32_t)(key[j + 1] >> 32) != (uint32_t)(kj >> 32);
    if (end) {
      const int tpe = tpa[j], tps = start > 0 ? tpa[start - 1] : 0;
      acc += (double)(tpe - tps) * ((double)tpe / (double)(j + 1));
    }
  }
  dred[tid] = acc;
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    for (int k = 0; k < NT; ++k) s += dred[k];
    ap[col] = npos > 0 ? (float)(s / (double)npos) : 0.f;
  }
}

}  // namespace

static bool svm_cols_ok(int N, int P, int ldp) { return N > 0 && P > 0 && ldp >= P && ldp % 8 == 0; }

extern "C" int clite_svm_margin(const float* Z, const float* Y, const float* Cw, int N, int P, int ldp, float* S, float* H, float* loss,
                                float* work, void* stream) {
  if (!svm_cols_ok(N, P, ldp) || !Z || !Y || !Cw || !S || !H || !loss || !work) return -1;
  hipStream_t st = (hipStream_t)stream;
  const int nb = (N + MARGIN_ROWS - 1) / MARGIN_ROWS;
  hipLaunchKernelGGL(svm_margin_kernel, dim3((ldp + SVM_CB - 1) / SVM_CB, nb), dim3(NT), 0, st, Z, Y, Cw, N, P, ldp, S, H, work);
  hipLaunchKernelGGL(svm_colsum_kernel, dim3((P + NT - 1) / NT), dim3(NT), 0, st, (const float*)work, nb, P, ldp, loss);
  return (int)hipGetLastError();
}

extern "C" int clite_svm_hess_scale(const float* H, float* Q, uint64_t n, void* stream) {
  if (!H || !Q || n == 0 || n % 4 || ((uintptr_t)H & 15) || ((uintptr_t)Q & 15)) return -1;
  const size_t n4 = n / 4;
  size_t grid = (n4 + NT - 1) / NT;
  if (grid > 2048) grid = 2048;
  hipLaunchKernelGGL(svm_hess_scale_kernel, dim3((unsigned)grid), dim3(NT), 0, (hipStream_t)stream, H, Q, n4);
  return (int)hipGetLastError();
}

extern "C" int clite_svm_newton_begin(const float* G, int ld, int Dp, int P, float* X, float* R, float* D, float* state, float tol,
                                      int max_newton, float eta_max, void* stream) {
  if (!G || !X || !R || !D || !state || P <= 0 || Dp <= 0 || ld < Dp || max_newton < 0 || !(eta_max > 0.f)) return -1;
  hipLaunchKernelGGL(svm_newton_begin_kernel, dim3(P), dim3(NT), 0, (hipStream_t)stream, G, ld, Dp, X, R, D, state, tol, max_newton, eta_max,
                     0);      // g0_only: not read under Rules::FirstGradient
  return (int)hipGetLastError();
}

extern "C" int clite_svm_cg_update(const float* HD, int ld, int Dp, int P, float* X, float* R, float* D, float* state, void* stream) {
  if (!HD || !X || !R || !D || !state || P <= 0 || Dp <= 0 || ld < Dp) return -1;
  hipLaunchKernelGGL(svm_cg_update_kernel, dim3(P), dim3(NT), 0, (hipStream_t)stream, HD, ld, Dp, X, R, D, state);
  return (int)hipGetLastError();
}

extern "C" int clite_svm_line_search(const float* Z, const float* delta, const float* Y, const float* Cw, int N, int P, int ldp, float* W,
                                     const float* X, int ld, int Dp, float* state, void* stream) {
  if (!svm_cols_ok(N, P, ldp) || !Z || !delta || !Y || !Cw || !W || !X || !state || Dp <= 0 || ld < Dp) return -1;
  hipLaunchKernelGGL(svm_line_search_kernel, dim3((P + SVM_CB - 1) / SVM_CB), dim3(NT), 0, (hipStream_t)stream, Z, delta, Y, Cw, N, P, ldp, W, X,
                     ld, Dp, state);
  return (int)hipGetLastError();
}

extern "C" int clite_average_precision(const float* scores, int lds, const float* targets, int ldt, int N, int P, float* ap, void* stream) {
  if (!scores || !targets || !ap || N <= 0 || P <= 0 || lds < P || ldt < P) return -1;
  if (N > AP_MAX) return -2;
  hipLaunchKernelGGL(average_precision_kernel, dim3(P), dim3(NT), 0, (hipStream_t)stream, scores, lds, targets, ldt, N, ap);
  return (int)hipGetLastError();
}
