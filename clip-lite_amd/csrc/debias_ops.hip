// Bias evaluation (reference bias_eda.py, utils/we.py; driver: clip-lite_amd/debias.py): a direction found in the text embedding space is removed
// from image features.
//
// clite_debias_pca: the principal directions of P <= 64 pair differences d_i = e(a_i) - e(b_i). we.doPCA fits a PCA to the 2 P rows +-d_i / 2,
// whose column mean is zero, so its components are the right singular vectors of diffs [P][D]. They come from the P x P Gram matrix
// G = diffs diffs^T (f32, one wave per entry, a fixed summation order; G[i][j] and G[j][i] are the same sum, bit for bit), which one workgroup
// diagonalises in LDS by cyclic Jacobi: the P (+ a bye when P is odd) indices are paired by the round-robin circle method, the rotations of a
// round act on disjoint rows and columns and are applied together (G J, then J^T (G J); the eigenvector matrix U J alongside). A sweep is
// n - 1 rounds; it stops once the off-diagonal norm is at most FLT_EPSILON x trace, or after 30 sweeps (info[0] = 1). The eigenvalues are
// read off as Rayleigh quotients of G as given, in f64 (the rotations' rounding in the diagonal is first order, this is second). The same workgroup
// then forms components[j] = diffs^T u_j for the R largest eigenvalues, normalises them, runs one modified Gram-Schmidt pass and makes the
// entry of largest magnitude of every row positive. Every reduction is a fixed tree (lane partials, wave butterfly, waves in order): no float
// atomics, the same bits in every run.
//
// clite_debias_rows: the streaming pass over the image bank. One wave per row; the row stays in registers (16-byte loads, lane l owns the
// vectors l, l + 64, ...), the components sit in LDS (loaded once per workgroup, read as the same 16-byte vectors: conflict-free), every dot
// product is four lane accumulators and the wave butterfly of intrin.h. |y| is taken from y itself: |x|^2 - sum coef^2 cancels when x is
// close to a direction. The kernel reads N D floats once and writes at most 2 N D + N R.
#include "vec.h"
#include "clite.h"

using namespace clite;

namespace {

constexpr int NT = 256;
constexpr int NW = NT / WAVE;
constexpr int MAXP = CLITE_DEBIAS_MAX_PAIRS;
constexpr int MAXR = CLITE_DEBIAS_MAX_COMPONENTS;
constexpr int MAXD = CLITE_DEBIAS_MAX_DIM;
constexpr int LDP = MAXP + 1;               // row stride of the LDS matrices: a column walk touches every bank once
constexpr int MAX_SWEEPS = 30;
constexpr float F32_EPS = 1.1920929e-07f;
constexpr float NORM_FLOOR = 1e-12f;        // F.normalize's eps
static_assert(MAXP % 2 == 0 && MAXP <= NT && MAXR <= MAXP, "one thread per index");

// sum of the lane's four accumulators, then over the wave: the same tree in every lane and every run
DEV float lane4_wave_sum(const float (&s)[4]) { return wave_sum((s[0] + s[1]) + (s[2] + s[3])); }

// ------------------------------------------------------------------------------------------------ Gram matrix
// G[i][j] = <diffs[i], diffs[j]>: one wave per entry
__global__ __launch_bounds__(NT) void debias_gram_kernel(const float* diffs, int P, int D, float* G) {
  const int l = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
  const int e = blockIdx.x * NW + w;
  if (e >= P * P) return;                   // wave-uniform; no barrier follows
  const int i = e / P, j = e - i * P;
  const f32x4* a = (const f32x4*)(diffs + (size_t)i * (size_t)D);
  const f32x4* b = (const f32x4*)(diffs + (size_t)j * (size_t)D);
  const int nvec = D >> 2;
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  for (int q = l; q < nvec; q += WAVE) {
    const f32x4 x = a[q], y = b[q];
#pragma unroll
    for (int c = 0; c < 4; ++c) s[c] += x[c] * y[c];
  }
  const float t = lane4_wave_sum(s);
  if (l == 0) G[e] = t;
}

// ------------------------------------------------------------------------------------------------ eigenvectors and components
// Sum of v over the workgroup in a fixed order; every thread gets the same bits. red: float [NW] in LDS that no thread touches again before
// the next barrier (the caller alternates two).
DEV float block_sum(float v, float* red) {
  v = wave_sum(v);
  if ((threadIdx.x & (WAVE - 1)) == 0) red[threadIdx.x / WAVE] = v;
  __syncthreads();
  float t = red[0];
#pragma unroll
  for (int k = 1; k < NW; ++k) t += red[k];
  return t;
}

// (a at index ai) is a better "largest magnitude" entry than (b at bi); index < 0: none
DEV bool bigger(float a, int ai, float b, int bi) { return ai >= 0 && (bi < 0 || fabsf(a) > fabsf(b) || (fabsf(a) == fabsf(b) && ai < bi)); }

__global__ __launch_bounds__(NT) void debias_eig_kernel(const float* diffs, const float* G, int P, int D, int R, float* eigvals, float* comps,
                                                        int* info) {
  __shared__ float A[MAXP * LDP];           // the Gram matrix, driven to diagonal form
  __shared__ float U[MAXP * LDP];           // its eigenvectors, in columns
  __shared__ float rc[MAXP / 2], rs[MAXP / 2];
  __shared__ int rp[MAXP / 2], rq[MAXP / 2];
  __shared__ float rowv[MAXP];
  __shared__ float dg[MAXP], db[MAXP], dz[MAXP];           // the diagonal: working value, value at the sweep's start, the sweep's corrections
  __shared__ int order[MAXP];
  __shared__ float red[2][NW];
  __shared__ int redi[NW];
  const int tid = threadIdx.x, l = tid & (WAVE - 1), w = tid / WAVE;
  for (int e = tid; e < P * P; e += NT) {
    const int i = e / P, j = e - i * P;
    A[i * LDP + j] = G[e];
    U[i * LDP + j] = i == j ? 1.f : 0.f;
  }
  __syncthreads();

  const int n = (P + 1) & ~1;               // players of the round robin; index P is the bye of an odd P
  const int half = n >> 1;
  int sweeps = 0;
  bool done = false;
  if (tid < P) db[tid] = A[tid * LDP + tid], dz[tid] = 0.f;
  while (true) {
    // off-diagonal norm and trace: row sums by one thread per row, then the rows in order by every thread (the same bits everywhere). The
    // diagonal lives in dg; a sweep's corrections t a_pq are summed on their own in dz and meet the diagonal once, here (Rutishauser).
    if (tid < P) {
      float s = 0.f;
      for (int j = 0; j < P; ++j) {
        const float v = A[tid * LDP + j];
        if (j != tid) s += v * v;
      }
      rowv[tid] = s;
      dg[tid] = db[tid] = db[tid] + dz[tid], dz[tid] = 0.f;
    }
    __syncthreads();
    float off = 0.f, tr = 0.f;
    for (int i = 0; i < P; ++i) off += rowv[i], tr += db[i];    // db, not dg: the round below moves dg with no barrier in between
    done = sqrtf(off) <= F32_EPS * tr || !(off == off);          // a NaN Gram matrix cannot improve: stop, the host sees NaN eigenvalues
    if (done || sweeps == MAX_SWEEPS) break;
    ++sweeps;
    for (int r = 0; r < n - 1; ++r) {
      if (tid < half) {                     // the rotation of pair `tid` of round r, from its 2 x 2 block, which no other pair of the round
        int a = tid == 0 ? n - 1 : (r + tid) % (n - 1);          // touches and which is finished here: a_pq = 0, the diagonal moves by t a_pq
        int b = tid == 0 ? r : (r - tid + n - 1) % (n - 1);
        if (a > b) { const int t = a; a = b; b = t; }
        float c = 1.f, s = 0.f;
        if (b < P) {
          const float apq = A[a * LDP + b];
          if (apq != 0.f) {
            const float theta = (dg[b] - dg[a]) / (2.f * apq);
            const float t = (theta < 0.f ? -1.f : 1.f) / (fabsf(theta) + sqrtf(theta * theta + 1.f));
            c = 1.f / sqrtf(t * t + 1.f);
            s = t * c;
            const float h = t * apq;
            dg[a] -= h, dz[a] -= h, dg[b] += h, dz[b] += h;
            A[a * LDP + b] = A[b * LDP + a] = 0.f;
          }
        } else {
          a = b = -1;                       // the bye
        }
        rc[tid] = c, rs[tid] = s, rp[tid] = a, rq[tid] = b;
      }
      __syncthreads();
      for (int it = tid; it < half * P; it += NT) {               // columns: A <- A J (outside the block), U <- U J
        const int k = it / P, i = it - k * P, p = rp[k], q = rq[k];
        if (p < 0) continue;
        const float c = rc[k], s = rs[k];
        const float up = U[i * LDP + p], uq = U[i * LDP + q];
        U[i * LDP + p] = c * up - s * uq, U[i * LDP + q] = s * up + c * uq;
        if (i == p || i == q) continue;
        const float ap = A[i * LDP + p], aq = A[i * LDP + q];
        A[i * LDP + p] = c * ap - s * aq, A[i * LDP + q] = s * ap + c * aq;
      }
      __syncthreads();
      for (int it = tid; it < half * P; it += NT) {               // rows: A <- J^T A (outside the block)
        const int k = it / P, j = it - k * P, p = rp[k], q = rq[k];
        if (p < 0 || j == p || j == q) continue;
        const float c = rc[k], s = rs[k];
        const float ap = A[p * LDP + j], aq = A[q * LDP + j];
        A[p * LDP + j] = c * ap - s * aq, A[q * LDP + j] = s * ap + c * aq;
      }
      __syncthreads();
    }
  }
  if (tid == 0) info[0] = done ? 0 : 1, info[1] = sweeps;

  // The rotations leave about sqrt(P) FLT_EPSILON |G| of rounding in the diagonal. The eigenvalues are therefore read off as the Rayleigh
  // quotients u^T G u / u^T u of the Gram matrix as it was given, summed in f64: their error is second order in the eigenvectors'.
  if (tid < P) {
    double num = 0.0, den = 0.0;
    for (int i = 0; i < P; ++i) {
      double wv = 0.0;
      for (int k = 0; k < P; ++k) wv += (double)G[i * P + k] * (double)U[k * LDP + tid];
      const double u = (double)U[i * LDP + tid];
      num += u * wv, den += u * u;
    }
    dg[tid] = (float)(num / den);
  }
  __syncthreads();
  // descending (index ascending among equal ones, a NaN - an overflowed Gram matrix - behind every number, so that `order` is a
  // permutation whatever the values); a rounding-negative one of the positive semi-definite G reads zero
  if (tid < P) {
    const float lam = dg[tid];
    int rank = 0;
    for (int j = 0; j < P; ++j) {
      const float o = dg[j];
      const bool ahead = lam == lam ? (o > lam || (o == lam && j < tid)) : (o == o || j < tid);
      rank += ahead ? 1 : 0;
    }
    order[rank] = tid;
    eigvals[rank] = lam < 0.f ? 0.f : lam;       // a NaN stays a NaN
  }
  __syncthreads();

  // components[j] = sum_i U[i][order[j]] diffs[i]: thread t owns the vectors t, t + NT, ... of every component, here and below
  const int nvec = D >> 2;
  f32x4* cv = (f32x4*)comps;
  for (int q = tid; q < nvec; q += NT) {
    f32x4 acc[MAXR];
#pragma unroll
    for (int j = 0; j < MAXR; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int i = 0; i < P; ++i) {
      const f32x4 x = ((const f32x4*)(diffs + (size_t)i * (size_t)D))[q];
#pragma unroll
      for (int j = 0; j < MAXR; ++j)
        if (j < R) {
          const float u = U[i * LDP + order[j]];
#pragma unroll
          for (int c = 0; c < 4; ++c) acc[j][c] += u * x[c];
        }
    }
#pragma unroll
    for (int j = 0; j < MAXR; ++j)
      if (j < R) cv[(size_t)j * nvec + q] = acc[j];
  }
  // normalise, one modified Gram-Schmidt pass (row j against the finished rows i < j, then normalised again), sign
  int ph = 0;
  for (int j = 0; j < R; ++j) {
    f32x4* cj = cv + (size_t)j * nvec;
    for (int i = -1; i < j; ++i) {          // i = -1: the first normalisation
      const f32x4* ci = i < 0 ? cj : cv + (size_t)i * nvec;
      float s[4] = {0.f, 0.f, 0.f, 0.f};
      for (int q = tid; q < nvec; q += NT) {
        const f32x4 x = cj[q], y = ci[q];
#pragma unroll
        for (int c = 0; c < 4; ++c) s[c] += x[c] * y[c];
      }
      const float d = block_sum((s[0] + s[1]) + (s[2] + s[3]), red[ph]);
      ph ^= 1;
      if (i < 0) {
        const float inv = 1.f / fmaxf(sqrtf(d), NORM_FLOOR);
        for (int q = tid; q < nvec; q += NT) cj[q] = cj[q] * inv;
      } else {
        for (int q = tid; q < nvec; q += NT) cj[q] = cj[q] - ci[q] * d;
      }
    }
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    float bv = 0.f;
    int bi = -1;
    for (int q = tid; q < nvec; q += NT) {
      const f32x4 x = cj[q];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        s[c] += x[c] * x[c];
        if (bigger(x[c], 4 * q + c, bv, bi)) bv = x[c], bi = 4 * q + c;
      }
    }
    const float d = block_sum((s[0] + s[1]) + (s[2] + s[3]), red[ph]);
    ph ^= 1;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      const float ov = wave_shfl_xor(bv, m);
      const int oi = wave_shfl_xor_i(bi, m);
      if (bigger(ov, oi, bv, bi)) bv = ov, bi = oi;
    }
    if (l == 0) red[ph][w] = bv, redi[w] = bi;
    __syncthreads();
    bv = red[ph][0], bi = redi[0];
#pragma unroll
    for (int k = 1; k < NW; ++k)
      if (bigger(red[ph][k], redi[k], bv, bi)) bv = red[ph][k], bi = redi[k];
    ph ^= 1;
    const float scale = (bv < 0.f ? -1.f : 1.f) / fmaxf(sqrtf(d), NORM_FLOOR);
    for (int q = tid; q < nvec; q += NT) cj[q] = cj[q] * scale;
    __syncthreads();                        // redi is written again by the next row
  }
}

// ------------------------------------------------------------------------------------------------ rows
// NV: 16-byte vectors of the row a lane may hold (64 NV >= D / 4); LDSF: floats of LDS for the components (>= R D).
template <int NV, int LDSF>
__global__ __launch_bounds__(NT) void debias_rows_kernel(const float* x, const float* comps, int N, int D, int R, float* xn, float* xd, float* coef) {
  __shared__ f32x4 V[LDSF / 4];
  const int tid = threadIdx.x, l = tid & (WAVE - 1), w = tid / WAVE;
  const int nvec = D >> 2;
  const bool proj = xd != nullptr || coef != nullptr;
  if (proj)
    for (int q = tid; q < R * nvec; q += NT) V[q] = ((const f32x4*)comps)[q];
  __syncthreads();
  for (int64_t row = (int64_t)blockIdx.x * NW + w; row < (int64_t)N; row += (int64_t)gridDim.x * NW) {      // wave-uniform; no barrier inside
    const f32x4* xr = (const f32x4*)(x + (size_t)row * (size_t)D);
    f32x4 a[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int q = l + i * WAVE;
      a[i] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (q < nvec) a[i] = __builtin_nontemporal_load(xr + q);
    }
    if (xn) {
      float s[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < NV; ++i)
#pragma unroll
        for (int c = 0; c < 4; ++c) s[c] += a[i][c] * a[i][c];
      const float inv = 1.f / fmaxf(sqrtf(lane4_wave_sum(s)), NORM_FLOOR);
      f32x4* o = (f32x4*)(xn + (size_t)row * (size_t)D);
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int q = l + i * WAVE;
        if (q < nvec) __builtin_nontemporal_store(a[i] * inv, o + q);
      }
    }
    if (!proj) continue;
    f32x4 y[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) y[i] = a[i];
    float mine = 0.f;                       // lane j keeps coefficient j
    for (int j = 0; j < R; ++j) {
      const f32x4* vj = V + j * nvec;
      f32x4 v[NV];
      float s[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int q = l + i * WAVE;
        v[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (q < nvec) v[i] = vj[q];
#pragma unroll
        for (int c = 0; c < 4; ++c) s[c] += a[i][c] * v[i][c];
      }
      const float cf = lane4_wave_sum(s);
      if (l == j) mine = cf;
#pragma unroll
      for (int i = 0; i < NV; ++i) y[i] = y[i] - v[i] * cf;
    }
    if (coef && l < R) coef[(size_t)row * (size_t)R + l] = mine;
    if (xd) {
      float s[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < NV; ++i)
#pragma unroll
        for (int c = 0; c < 4; ++c) s[c] += y[i][c] * y[i][c];
      const float inv = 1.f / fmaxf(sqrtf(lane4_wave_sum(s)), NORM_FLOOR);
      f32x4* o = (f32x4*)(xd + (size_t)row * (size_t)D);
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int q = l + i * WAVE;
        if (q < nvec) __builtin_nontemporal_store(y[i] * inv, o + q);
      }
    }
  }
}

constexpr int ROWS_MAX_GRID = 2048;         // 8 workgroups per CU; the rest of a longer bank is reached by the grid stride

template <int NV>
void launch_rows(const float* x, const float* comps, int N, int D, int R, float* xn, float* xd, float* coef, hipStream_t st) {
  const int64_t wgs = ((int64_t)N + NW - 1) / NW;
  const dim3 grid((unsigned)(wgs < ROWS_MAX_GRID ? wgs : ROWS_MAX_GRID));
  const int need = R * D;                   // the LDS tier decides how many workgroups share a CU
  if (need <= 4096)
    hipLaunchKernelGGL((debias_rows_kernel<NV, 4096>), grid, dim3(NT), 0, st, x, comps, N, D, R, xn, xd, coef);
  else if (need <= 16384)
    hipLaunchKernelGGL((debias_rows_kernel<NV, 16384>), grid, dim3(NT), 0, st, x, comps, N, D, R, xn, xd, coef);
  else
    hipLaunchKernelGGL((debias_rows_kernel<NV, MAXR * MAXD>), grid, dim3(NT), 0, st, x, comps, N, D, R, xn, xd, coef);
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int clite_debias_pca(const float* diffs, int P, int D, int R, float* eigvals, float* components, float* work, int* info, void* stream) {
  if (!diffs || !eigvals || !components || !work || !info || P < 1 || P > MAXP || D < 8 || D > MAXD || D % 8 || R < 1 || R > MAXR || R > P ||
      !aligned16(diffs) || !aligned16(components))
    return -1;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(debias_gram_kernel, dim3((P * P + NW - 1) / NW), dim3(NT), 0, st, diffs, P, D, work);
  hipLaunchKernelGGL(debias_eig_kernel, dim3(1), dim3(NT), 0, st, diffs, (const float*)work, P, D, R, eigvals, components, info);
  return (int)hipGetLastError();
}

extern "C" int clite_debias_rows(const float* x, const float* components, int N, int D, int R, float* xn, float* xd, float* coef, void* stream) {
  if (!x || !components || N < 1 || D < 8 || D > MAXD || D % 8 || R < 1 || R > MAXR || !aligned16(x) || !aligned16(components) || !aligned16(xn) ||
      !aligned16(xd))
    return -1;
  if (!xn && !xd && !coef) return 0;        // nothing asked for
  hipStream_t st = (hipStream_t)stream;
  const int nv = (D / 4 + WAVE - 1) / WAVE;
  if (nv <= 2) launch_rows<2>(x, components, N, D, R, xn, xd, coef, st);
  else if (nv <= 8) launch_rows<8>(x, components, N, D, R, xn, xd, coef, st);
  else launch_rows<16>(x, components, N, D, R, xn, xd, coef, st);
  return (int)hipGetLastError();
}
