// Lloyd's k-means of caption embeddings (reference scripts/cluster.py:131-140, faiss.Kmeans(d, k, niter=200).train + index.search; driver:
// clip-lite_amd/kmeans.py). One iteration is  scores = X C^T (clite_gemm_nt, exact f32)  ->  assign  ->  accumulate  ->  update.
//
// assign: per row the argmin over k < K of  v_k = hc[k] - score[n][k]  with hc[k] = 0.5 |c_k|^2 (the |x|^2 term is common to a row), ties to
// the lower k (0.0 == -0.0 is a tie). A NaN value never wins: the row takes the lowest k whose value is not a NaN, or 0 when all are. G lanes
// share a row (G = the power of two >= K / 4, at most a wave), each with 16-byte loads of 4 adjacent columns, merged by a butterfly.
//
// accumulate / update: the per-cluster sums must be bitwise reproducible (a last-bit change of a centroid can move a boundary row), so no float
// atomic is used anywhere. Rows are first grouped by cluster with a stable counting sort (per 256-row block: rank of a row among the block's
// earlier rows of its cluster, and the block's count per cluster; a column scan over the blocks; a scan over the clusters), which yields
// order[] = the row indices of cluster 0 ascending, then those of cluster 1, ...  Every cluster's list is cut into chunks of
// CLITE_KMEANS_CHUNK rows; one workgroup gathers the rows of one chunk from X (each row is read once per iteration, whole 16-byte vectors) and
// adds them in list order into part[chunk][D]; the update kernel adds a cluster's chunks in chunk order, divides by the count and forms the
// new 0.5 |c|^2. Every order is a function of the assignment alone, so the result is the same in every run and in both deterministic modes.
// All integer bookkeeping is exact; the only atomic is the integer add of the changed-row count (order-independent).
#include "vec.h"
#include "clite.h"

using namespace clite;

namespace {

constexpr int NT = 256;                     // threads of every kernel here
constexpr int NW = NT / WAVE;
constexpr int BLK = CLITE_KMEANS_BLOCK;     // rows per block of the counting sort
constexpr int CH = CLITE_KMEANS_CHUNK;      // rows per partial sum
constexpr int UNROLL = 8;                   // rows whose loads a lane issues before it adds any
static_assert(BLK == NT, "one thread per row of a sort block");
static_assert(CLITE_KMEANS_MAX_K <= 4 * NT, "starts_kernel scans four clusters per thread of one workgroup");

#ifdef CLITE_WAVESIM_H
inline void atomic_add_i32(int* p, int v) { std::atomic_ref<int>(*p).fetch_add(v); }
#else
DEV void atomic_add_i32(int* p, int v) { atomicAdd(p, v); }
#endif

DEV int wave_sum_i(int v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += wave_shfl_xor_i(v, m);
  return v;
}

struct Work {                 // carve-up of the workspace (include/clite.h: CLITE_KMEANS_WORK_BYTES)
  int nb, maxchunks;
  int *hist, *rank, *order, *start, *cstart;
  float *dpart, *part;
  size_t bytes;
};

size_t align4(size_t n) { return (n + 3) & ~(size_t)3; }

Work carve(void* base, int N, int D, int K) {
  Work w;
  w.nb = (N + BLK - 1) / BLK;
  w.maxchunks = (N + CH - 1) / CH + K;
  int* ip = (int*)base;
  w.hist = ip;
  w.rank = w.hist + (size_t)w.nb * K;
  w.order = w.rank + N;
  w.start = w.order + N;
  w.cstart = w.start + (K + 1);
  const size_t ints = align4((size_t)w.nb * K + 2 * (size_t)N + 2 * (size_t)(K + 1));
  w.dpart = (float*)(ip + ints);
  w.part = w.dpart + align4(w.nb);
  w.bytes = 4 * (ints + align4(w.nb) + (size_t)w.maxchunks * D);
  return w;
}

// out[n] = scale * sum_d x[n][d]^2: one wave per row, lanes over the 16-byte vectors, a butterfly at the end (one fixed order)
template <bool VEC>
__global__ __launch_bounds__(NT) void row_norms_kernel(const float* X, int ldx, int N, int D, float scale, float* out) {
  const int tid = threadIdx.x, w = tid / WAVE, l = tid & (WAVE - 1);
  const int n = blockIdx.x * NW + w;
  if (n >= N) return;                       // whole wave
  const float* row = X + (size_t)n * (size_t)ldx;
  float acc = 0.f;
  for (int v = l; 4 * v < D; v += WAVE) {
    float x[4];
    if (VEC) {
      const f32x4 t = *(const f32x4*)(row + 4 * v);
      x[0] = t[0], x[1] = t[1], x[2] = t[2], x[3] = t[3];
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) x[e] = row[4 * v + e];
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) acc = fmaf(x[e], x[e], acc);
  }
  acc = wave_sum(acc);
  if (l == 0) out[n] = scale * acc;
}

// (ov, ok) replaces (bv, bk): a candidate exists and is smaller, or equal at a lower k. k < 0: no candidate yet.
DEV bool takes(float ov, int ok, float bv, int bk) { return ok >= 0 && (bk < 0 || ov < bv || (ov == bv && ok < bk)); }

template <bool VEC>
__global__ __launch_bounds__(NT) void assign_kernel(const float* scores, int lds, const float* hc, const float* xnorm, int N, int K, int G, int* assign,
                                                    float* dist, int* changed) {
  const int tid = threadIdx.x, l = tid & (WAVE - 1);
  const int n = blockIdx.x * (NT / G) + tid / G, q = tid & (G - 1);
  const bool valid = n < N;
  const float* row = scores + (size_t)(valid ? n : 0) * (size_t)lds;
  float bv = 0.f;
  int bk = -1;
  if (valid) {
    for (int k0 = 4 * q; k0 < K; k0 += 4 * G) {
      float s[4];
      if (VEC) {                            // columns k >= K of the vector lie inside the row (lds % 4 == 0): loaded, never compared
        const f32x4 t = __builtin_nontemporal_load((const f32x4*)(row + k0));
        s[0] = t[0], s[1] = t[1], s[2] = t[2], s[3] = t[3];
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) s[e] = k0 + e < K ? row[k0 + e] : 0.f;
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int k = k0 + e;
        if (k < K) {
          const float v = hc[k] - s[e];
          if (v == v && (bk < 0 || v < bv)) bv = v, bk = k;       // ascending k inside a lane: < keeps the lower k of a tie
        }
      }
    }
  }
  for (int m = G >> 1; m >= 1; m >>= 1) {
    const float ov = wave_shfl_xor(bv, m);
    const int ok = wave_shfl_xor_i(bk, m);
    if (takes(ov, ok, bv, bk)) bv = ov, bk = ok;
  }
  int ch = 0;
  if (valid && q == 0) {
    const int a = bk < 0 ? 0 : bk;
    ch = assign[n] != a ? 1 : 0;
    assign[n] = a;
    if (dist) {                             // |x|^2 - 2 x.c + |c|^2 = |x|^2 + 2 v, clamped at 0; 0 for a row without a candidate
      const float d = bk < 0 ? 0.f : xnorm[n] + 2.f * bv;
      dist[n] = d > 0.f ? d : 0.f;
    }
  }
  ch = wave_sum_i(ch);
  if (l == 0 && ch) atomic_add_i32(changed, ch);
}

// Block b = rows [256 b, 256 b + 256): rank[n] = #{earlier rows of the block in the same cluster}; the last row of a cluster in the block
// writes the block's count of it into hist[b][k] (pre-zeroed); dpart[b] = sum of the block's distances (wave butterflies, then wave order).
__global__ __launch_bounds__(NT) void hist_kernel(const int* assign, const float* dist, int N, int K, int* rank, int* hist, float* dpart) {
  __shared__ int a[BLK];
  __shared__ float ds[NW];
  const int tid = threadIdx.x, b = blockIdx.x, n = b * BLK + tid;
  int av = n < N ? assign[n] : -1;
  if ((unsigned)av >= (unsigned)K) av = -1;             // the caller's assignment is not trusted: such a row joins no cluster
  a[tid] = av;
  const float d = wave_sum(n < N && dist ? dist[n] : 0.f);
  if ((tid & (WAVE - 1)) == 0) ds[tid / WAVE] = d;
  __syncthreads();
  int r = 0;
  bool later = false;
  for (int j = 0; j < BLK; ++j) {
    const bool same = a[j] == av;
    r += same && j < tid ? 1 : 0;
    later = later || (same && j > tid);
  }
  if (av >= 0) {
    rank[n] = r;
    if (!later) hist[(size_t)b * K + av] = r + 1;
  }
  if (tid == 0) {
    float s = ds[0];
#pragma unroll
    for (int k = 1; k < NW; ++k) s += ds[k];
    dpart[b] = s;
  }
}

// hist[b][k] -> the number of rows of cluster k in blocks before b; counts[k] = the total
__global__ __launch_bounds__(NT) void scan_kernel(int* hist, int nb, int K, int* counts) {
  const int k = blockIdx.x * NT + threadIdx.x;
  if (k >= K) return;
  int run = 0;
  for (int b = 0; b < nb; ++b) {
    const int t = hist[(size_t)b * K + k];
    hist[(size_t)b * K + k] = run;
    run += t;
  }
  counts[k] = run;
}

// One workgroup: start[k] = rows in clusters before k, cstart[k] = chunks before k (k <= K), inertia = sum of dpart in one fixed order (double)
__global__ __launch_bounds__(NT) void starts_kernel(const int* counts, int K, int* start, int* cstart, const float* dpart, int nb, double* inertia) {
  __shared__ int sr[NT], sc[NT];
  __shared__ double sd[NT];
  const int tid = threadIdx.x;
  int c[4], rows = 0, chunks = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int k = 4 * tid + e;
    c[e] = k < K ? counts[k] : 0;
    rows += c[e];
    chunks += (c[e] + CH - 1) / CH;
  }
  double s = 0.0;
  for (int b = tid; b < nb; b += NT) s += (double)dpart[b];
  sr[tid] = rows, sc[tid] = chunks, sd[tid] = s;
  __syncthreads();
  if (tid == 0) {
    int r = 0, q = 0;
    double tot = 0.0;
    for (int t = 0; t < NT; ++t) {
      const int tr = sr[t], tq = sc[t];
      sr[t] = r, sc[t] = q;
      r += tr, q += tq;
      tot += sd[t];
    }
    if (inertia) *inertia = tot;
  }
  __syncthreads();
  int r = sr[tid], q = sc[tid];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int k = 4 * tid + e;
    if (k <= K) start[k] = r, cstart[k] = q;
    r += c[e];
    q += (c[e] + CH - 1) / CH;
  }
  if (tid == NT - 1 && K == 4 * NT) start[K] = r, cstart[K] = q;      // K = CLITE_KMEANS_MAX_K: entry K lies behind the last thread's four
}

__global__ __launch_bounds__(NT) void scatter_kernel(const int* assign, int N, int K, const int* rank, const int* hist, const int* start, int* order) {
  const int n = blockIdx.x * NT + threadIdx.x;
  if (n >= N) return;
  const int av = assign[n];
  if ((unsigned)av >= (unsigned)K) return;
  const int pos = start[av] + hist[(size_t)(n / BLK) * K + av] + rank[n];
  if ((unsigned)pos < (unsigned)N) order[pos] = n;
}

DEV f32x4 load_row4(const float* p, bool vec) {
  if (vec) return *(const f32x4*)p;
  return f32x4{p[0], p[1], p[2], p[3]};
}

// Workgroup (w, y): chunk w of the chunk list (cluster k = the one with cstart[k] <= w < cstart[k + 1]), column vectors [256 y, 256 y + cw).
// R = 256 / cw row groups: group g adds the chunk's rows g, g + R, ... in list order, the groups meet in LDS in group order.
template <bool VEC>
__global__ __launch_bounds__(NT) void sum_kernel(const float* X, int ldx, int N, int D, int K, const int* order, const int* start, const int* cstart, float* part) {
  __shared__ f32x4 red[NT];
  const int tid = threadIdx.x, w = blockIdx.x;
  if (w >= cstart[K]) return;               // whole workgroup
  int lo = 0, hi = K;                       // the last k in [0, K) with cstart[k] <= w (empty clusters before it share its value)
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (cstart[mid] <= w) lo = mid; else hi = mid;
  }
  const int k = lo;
  const int r0 = start[k] + (w - cstart[k]) * CH;
  const int r1 = start[k + 1] < r0 + CH ? start[k + 1] : r0 + CH;
  const int nvec = D >> 2, v0 = blockIdx.y * NT;
  const int cw = nvec - v0 < NT ? nvec - v0 : NT;
  const int R = NT / cw, g = tid / cw, cv = tid - g * cw;
  const bool active = g < R;
  const float* col = X + 4 * (size_t)(v0 + cv);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (active) {
    int i = r0 + g;
    for (; i + (UNROLL - 1) * R < r1; i += UNROLL * R) {
      f32x4 x[UNROLL];
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        const int row = order[i + u * R];
        x[u] = (unsigned)row < (unsigned)N ? load_row4(col + (size_t)row * (size_t)ldx, VEC) : f32x4{0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) acc += x[u];
    }
    for (; i < r1; i += R) {
      const int row = order[i];
      if ((unsigned)row < (unsigned)N) acc += load_row4(col + (size_t)row * (size_t)ldx, VEC);
    }
  }
  if (R > 1) {
    red[tid] = acc;
    __syncthreads();
    if (g == 0)
      for (int o = 1; o < R; ++o) acc += red[o * cw + cv];
  }
  if (g == 0) *(f32x4*)(part + (size_t)w * (size_t)D + 4 * (size_t)(v0 + cv)) = acc;
}

// One workgroup per cluster: c_k = (sum of its chunks, in chunk order) / count_k, hc[k] = 0.5 |c_k|^2. An empty cluster keeps its centroid.
__global__ __launch_bounds__(NT) void update_kernel(const float* part, const int* cstart, const int* counts, int D, float* C, int ldc, float* hc) {
  __shared__ float hs[NW];
  const int tid = threadIdx.x, k = blockIdx.x;
  const int cnt = counts[k], c0 = cstart[k], c1 = cstart[k + 1];
  float* crow = C + (size_t)k * (size_t)ldc;
  float h = 0.f;
  for (int v = tid; 4 * v < D; v += NT) {
    f32x4 c;
    if (cnt > 0) {
      f32x4 s = {0.f, 0.f, 0.f, 0.f};
      for (int ci = c0; ci < c1; ++ci) s += *(const f32x4*)(part + (size_t)ci * (size_t)D + 4 * v);
      const float fc = (float)cnt;
      c = f32x4{s[0] / fc, s[1] / fc, s[2] / fc, s[3] / fc};
      *(f32x4*)(crow + 4 * v) = c;
    } else {
      c = *(const f32x4*)(crow + 4 * v);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) h = fmaf(c[e], c[e], h);
  }
  h = wave_sum(h);
  if ((tid & (WAVE - 1)) == 0) hs[tid / WAVE] = h;
  __syncthreads();
  if (tid == 0) {
    float s = hs[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) s += hs[w];
    hc[k] = 0.5f * s;
  }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
bool shape_ok(int N, int D, int K) { return D > 0 && D % 8 == 0 && K >= 2 && K <= CLITE_KMEANS_MAX_K && N >= K; }

}  // namespace

extern "C" int clite_kmeans_row_norms(const float* X, int ldx, int N, int D, float scale, float* out, void* stream) {
  if (!X || !out || N <= 0 || D <= 0 || D % 8 || ldx < D) return -1;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((N + NW - 1) / NW);
  if (aligned16(X) && ldx % 4 == 0)
    hipLaunchKernelGGL(row_norms_kernel<true>, grid, dim3(NT), 0, st, X, ldx, N, D, scale, out);
  else
    hipLaunchKernelGGL(row_norms_kernel<false>, grid, dim3(NT), 0, st, X, ldx, N, D, scale, out);
  return (int)hipGetLastError();
}

extern "C" int clite_kmeans_assign(const float* scores, int lds, const float* hc, const float* xnorm, int N, int K, int* assign, float* dist, int* changed,
                                   void* stream) {
  if (!scores || !hc || !assign || !changed || (dist && !xnorm) || N <= 0 || K < 2 || K > CLITE_KMEANS_MAX_K || N < K || lds < K) return -1;
  hipStream_t st = (hipStream_t)stream;
  int G = 1;
  while (G < WAVE && 4 * G < K) G <<= 1;
  const dim3 grid((N + NT / G - 1) / (NT / G));
  if (aligned16(scores) && lds % 4 == 0)
    hipLaunchKernelGGL(assign_kernel<true>, grid, dim3(NT), 0, st, scores, lds, hc, xnorm, N, K, G, assign, dist, changed);
  else
    hipLaunchKernelGGL(assign_kernel<false>, grid, dim3(NT), 0, st, scores, lds, hc, xnorm, N, K, G, assign, dist, changed);
  return (int)hipGetLastError();
}

extern "C" int clite_kmeans_accumulate(const float* X, int ldx, const int* assign, const float* dist, int N, int D, int K, int* counts, double* inertia,
                                       void* work, uint64_t work_bytes, void* stream) {
  if (!X || !assign || !counts || !work || !shape_ok(N, D, K) || ldx < D || !aligned16(work)) return -1;
  const Work w = carve(work, N, D, K);
  if (work_bytes < w.bytes) return -2;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(w.hist, 0, sizeof(int) * (size_t)w.nb * K, st) != hipSuccess) return -3;
  hipLaunchKernelGGL(hist_kernel, dim3(w.nb), dim3(NT), 0, st, assign, dist, N, K, w.rank, w.hist, w.dpart);
  hipLaunchKernelGGL(scan_kernel, dim3((K + NT - 1) / NT), dim3(NT), 0, st, w.hist, w.nb, K, counts);
  hipLaunchKernelGGL(starts_kernel, dim3(1), dim3(NT), 0, st, (const int*)counts, K, w.start, w.cstart, (const float*)w.dpart, w.nb, inertia);
  hipLaunchKernelGGL(scatter_kernel, dim3(w.nb), dim3(NT), 0, st, assign, N, K, (const int*)w.rank, (const int*)w.hist, (const int*)w.start, w.order);
  const dim3 grid(w.maxchunks, (D / 4 + NT - 1) / NT);
  if (aligned16(X) && ldx % 4 == 0)
    hipLaunchKernelGGL(sum_kernel<true>, grid, dim3(NT), 0, st, X, ldx, N, D, K, (const int*)w.order, (const int*)w.start, (const int*)w.cstart, w.part);
  else
    hipLaunchKernelGGL(sum_kernel<false>, grid, dim3(NT), 0, st, X, ldx, N, D, K, (const int*)w.order, (const int*)w.start, (const int*)w.cstart, w.part);
  return (int)hipGetLastError();
}

extern "C" int clite_kmeans_update(const void* work, uint64_t work_bytes, const int* counts, int N, int D, int K, float* C, int ldc, float* hc, void* stream) {
  if (!work || !counts || !C || !hc || !shape_ok(N, D, K) || ldc < D || ldc % 4 || !aligned16(C) || !aligned16(work)) return -1;
  const Work w = carve((void*)work, N, D, K);
  if (work_bytes < w.bytes) return -2;
  hipLaunchKernelGGL(update_kernel, dim3(K), dim3(NT), 0, (hipStream_t)stream, (const float*)w.part, (const int*)w.cstart, counts, D, C, ldc, hc);
  return (int)hipGetLastError();
}
