// Weighted k-nearest-neighbour classification on frozen features (Wu et al. 2018; the "k-NN top-1" of DINO and others; driver: clip-lite_amd/knn.py).
// The similarity matrix of all queries against the whole bank never exists: the driver forms it one [query block] x [bank chunk] tile at a time
// (clite_gemm_nt, exact f32) and after every tile the merge kernel folds the tile into each query's running list of its K best bank rows.
//
// Order everywhere: score descending, bank index ascending among equal scores, 0.0 == -0.0 (retrieval_ops.hip's order; the first K of
// np.argsort(-s, kind="stable") over the whole bank row). The order is total on (score, index) pairs with distinct indices, so the merged list
// is a pure function of the old list and the chunk: no atomics, nothing that depends on scheduling. A NaN score is never selected.
//
// merge: one 256-thread workgroup per query row. The list lives in LDS (S / I, entries [0, have)), candidates are appended behind it. While
// the list is full its K-th entry is a threshold: the row is streamed once with 16-byte loads (UNROLL per lane in flight), a lane keeps a bit
// per element that beats the threshold, a workgroup prefix sum of the counts (wave butterflies, then wave totals through LDS) gives every
// survivor its slot in thread order, and when the 256 slots run out (and at the end of the row) the candidates are sorted by a bitonic network
// in LDS and merged into the list, which is cut back to K; that also tightens the threshold. With a full list of random scores a chunk adds
// about K ln((base + Nc) / base) survivors per row, so the kernel is one HBM pass over the tile.
//
// vote: one workgroup per query. weight_r = exp((s_r - s_0) / T); class bins in LDS; thread t owns the classes c with c % 256 == t and adds
// the weights of its classes in rank order, so every bin is one f32 sum in rank order whatever the schedule. After the first k ranks of every
// requested k the five best classes by (score descending, class ascending) are picked by five workgroup arg-max rounds.
#include "vec.h"
#include "clite.h"

using namespace clite;

namespace {

constexpr int NT = 256;                     // threads of both kernels
constexpr int NW = NT / WAVE;
constexpr int MAXK = CLITE_KNN_MAX_K;
constexpr int CAP = MAXK + NT;              // LDS entries of the merge: the list, then up to NT candidates
constexpr int UNROLL = 8;                   // vectors whose loads a lane issues before it compares any
constexpr int MAXC = CLITE_KNN_MAX_CLASSES;
constexpr int TOP = CLITE_KNN_PRED;
constexpr int IDX_NONE = 0x7fffffff;        // index of a list entry that holds nothing: ranks behind every bank row (base + Nc <= INT32_MAX)
static_assert(MAXK <= NT, "one thread per list entry");
static_assert(UNROLL * 4 <= 32, "one survivor bit per element of a batch");

// (a, ai) ranks before (b, bi)
DEV bool before(float a, int ai, float b, int bi) { return a > b || (a == b && ai < bi); }

// off: the sum of c over the threads before this one (thread order), total: over the workgroup. tot: int [NW] in LDS that no thread touches
// again before the next __syncthreads() (the caller alternates two).
struct Scan {
  int off, total;
};
DEV Scan block_scan(int c, int* tot) {
  const int tid = threadIdx.x, l = tid & (WAVE - 1), w = tid / WAVE;
  int sum = c, pre = 0;
#pragma unroll
  for (int m = 1; m < WAVE; m <<= 1) {      // sum: over the lane's aligned group of 2 m lanes; pre: over the lanes of that group below this one
    const int o = wave_shfl_xor_i(sum, m);
    if (l & m) pre += o;
    sum += o;
  }
  if (l == 0) tot[w] = sum;
  __syncthreads();
  Scan r = {pre, 0};
#pragma unroll
  for (int k = 0; k < NW; ++k) {
    const int t = tot[k];
    if (k < w) r.off += t;
    r.total += t;
  }
  return r;
}

// The number of entries of the sorted run (S, I)[0, n) that rank before (x, xi)
DEV int rank_in(const float* S, const int* I, int n, float x, int xi) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (before(S[mid], I[mid], x, xi)) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// Folds the candidates (S, I)[have, have + nbuf), nbuf <= NT, into the list (S, I)[0, have) and keeps the first K: the candidates are sorted by a
// bitonic network over the next power of two (padded with empty entries), then every list entry and every candidate finds its place in the
// merged order by a binary search in the other run (the keys are distinct, so the places are). Ends with a barrier.
DEV void merge_cut(float* S, int* I, int K, int& have, int& nbuf) {
  const int tid = threadIdx.x;
  float* CS = S + have;
  int* CI = I + have;
  int n = 1;
  while (n < nbuf) n <<= 1;
  if (tid >= nbuf && tid < n) CS[tid] = -__builtin_inff(), CI[tid] = IDX_NONE;
  __syncthreads();
  for (int k = 2; k <= n; k <<= 1)
    for (int j = k >> 1; j >= 1; j >>= 1) {
      if (tid < (n >> 1)) {
        const int i = 2 * tid - (tid & (j - 1)), p = i + j;       // bit j of i is clear
        const float a = CS[i], b = CS[p];
        const int ai = CI[i], bi = CI[p];
        const bool up = (i & k) == 0;                             // this run comes out best first
        if (before(b, bi, a, ai) == up) CS[i] = b, CI[i] = bi, CS[p] = a, CI[p] = ai;
      }
      __syncthreads();
    }
  float a = 0.f, c = 0.f;
  int ai = 0, ci = 0, pa = K, pc = K;
  if (tid < have) a = S[tid], ai = I[tid], pa = tid + rank_in(CS, CI, nbuf, a, ai);
  if (tid < nbuf) c = CS[tid], ci = CI[tid], pc = tid + rank_in(S, I, have, c, ci);
  __syncthreads();
  if (pa < K) S[pa] = a, I[pa] = ai;
  if (pc < K) S[pc] = c, I[pc] = ci;
  __syncthreads();
  have = have + nbuf < K ? have + nbuf : K;
  nbuf = 0;
}

// W = 4: 16-byte loads (16-byte aligned base, lds % 4 == 0; the columns >= Nc of the last vector lie inside the row: loaded, never selected);
// W = 1: scalar loads of columns < Nc only.
template <int W>
__global__ __launch_bounds__(NT) void knn_topk_merge_kernel(const float* scores, int lds, int Nc, int base, int K, int have0, float* top_s, int* top_i) {
  __shared__ float S[CAP];
  __shared__ int I[CAP];
  __shared__ int wt[2][NW];
  const int tid = threadIdx.x;
  const float* row = scores + (size_t)blockIdx.x * (size_t)lds;
  float* os = top_s + (size_t)blockIdx.x * (size_t)K;
  int* oi = top_i + (size_t)blockIdx.x * (size_t)K;
  int have = have0, nbuf = 0, ph = 0;       // the same in every thread
  if (tid < have) S[tid] = os[tid], I[tid] = oi[tid];
  __syncthreads();
  bool full = have == K;
  float ts = full ? S[K - 1] : 0.f;         // the threshold: the list's last entry once the list is full
  int ti = full ? I[K - 1] : 0;

  const unsigned nvec = ((unsigned)Nc + W - 1) / W;
  for (unsigned q0 = tid; q0 - tid < nvec; q0 += NT * UNROLL) {
    float v[UNROLL][W];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const unsigned q = q0 + u * NT;
      if (W == 4) {
        f32x4 x = {0.f, 0.f, 0.f, 0.f};
        if (q < nvec) x = __builtin_nontemporal_load((const f32x4*)row + q);
#pragma unroll
        for (int e = 0; e < W; ++e) v[u][e] = x[e];
      } else {
        v[u][0] = q < nvec ? __builtin_nontemporal_load(row + q) : 0.f;
      }
    }
    unsigned msk = 0;                       // bit u W + e: element (u, e) is a column < Nc, not a NaN, and beats the threshold
#pragma unroll
    for (int u = 0; u < UNROLL; ++u)
#pragma unroll
      for (int e = 0; e < W; ++e) {
        const unsigned col = (q0 + u * NT) * W + e;
        const float s = v[u][e];
        const bool ok = col < (unsigned)Nc && s == s && (!full || before(s, base + (int)col, ts, ti));
        msk |= ok ? 1u << (u * W + e) : 0u;
      }
    const Scan sc = block_scan(__builtin_popcount(msk), wt[ph]);
    ph ^= 1;
    if (sc.total == 0) continue;
    if (nbuf + sc.total > NT && nbuf > 0) {                       // make room; survivors of the old threshold that no longer beat the new one
      merge_cut(S, I, K, have, nbuf);                             // are still appended: the next merge drops them
      full = have == K;
      if (full) ts = S[K - 1], ti = I[K - 1];
    }
    if (nbuf + sc.total <= NT) {
      int pos = have + nbuf + sc.off;
#pragma unroll
      for (int u = 0; u < UNROLL; ++u)
#pragma unroll
        for (int e = 0; e < W; ++e)
          if (msk >> (u * W + e) & 1u) {
            S[pos] = v[u][e], I[pos] = base + (int)((q0 + u * NT) * W + e);
            ++pos;
          }
      nbuf += sc.total;
    } else {
      // More survivors than the whole candidate area (a list that is not full yet, or a row that keeps improving): one element per thread
      // at a time, at most NT candidates per round, re-read from the row.
      for (int s = 0; s < UNROLL * W; ++s) {
        const unsigned col = (q0 + (unsigned)(s / W) * NT) * W + (unsigned)(s % W);
        float x = 0.f;
        bool ok = (msk >> s & 1u) != 0;
        if (ok) {
          x = row[col];
          ok = !full || before(x, base + (int)col, ts, ti);
        }
        const Scan s2 = block_scan(ok ? 1 : 0, wt[ph]);
        ph ^= 1;
        if (s2.total == 0) continue;
        if (nbuf + s2.total > NT) {
          merge_cut(S, I, K, have, nbuf);
          full = have == K;
          if (full) ts = S[K - 1], ti = I[K - 1];
        }
        if (ok) S[have + nbuf + s2.off] = x, I[have + nbuf + s2.off] = base + (int)col;
        nbuf += s2.total;
      }
    }
  }
  if (nbuf > 0) merge_cut(S, I, K, have, nbuf);
  const int valid = Nc < K - have0 ? have0 + Nc : K;              // min(K, have0 + Nc): what the caller takes as valid from now on
  if (tid < have) os[tid] = S[tid], oi[tid] = I[tid];
  else if (tid < valid) os[tid] = -__builtin_inff(), oi[tid] = IDX_NONE;      // NaN scores were passed over: entries that hold nothing
}

struct Ks {
  int k[CLITE_KNN_MAX_KS];
};

// (os, oc) replaces (bs, bc): a candidate exists and has the higher score, or the same at a lower class. c < 0: no candidate.
DEV bool takes(float os, int oc, float bs, int bc) { return oc >= 0 && (bc < 0 || os > bs || (os == bs && oc < bc)); }

__global__ __launch_bounds__(NT) void knn_vote_kernel(const float* top_s, const int* top_i, const int* labels, int Q, int K, int N, int C, Ks ks, int nk,
                                                      float inv_T, float* class_scores, int* pred) {
  __shared__ float bins[MAXC];
  __shared__ float wgt[MAXK];
  __shared__ int lab[MAXK];
  __shared__ float rs[NW];
  __shared__ int rc[NW];
  const int tid = threadIdx.x, w = tid / WAVE, q = blockIdx.x;
  const float* s = top_s + (size_t)q * (size_t)K;
  for (int c = tid; c < C; c += NT) bins[c] = 0.f;
  if (tid < K) {
    const int idx = top_i[(size_t)q * (size_t)K + tid];
    int l = -1;
    if ((unsigned)idx < (unsigned)N) {      // validated on the host; an entry outside the bank or the classes votes for nothing
      l = labels[idx];
      if ((unsigned)l >= (unsigned)C) l = -1;
    }
    lab[tid] = l;
    wgt[tid] = expf((s[tid] - s[0]) * inv_T);
  }
  __syncthreads();
  int r0 = 0;
  for (int j = 0; j < nk; ++j) {
    const int k = ks.k[j];
    for (int r = r0; r < k; ++r) {          // class c belongs to thread c % NT: one adder per bin, ranks in order
      const int l = lab[r];
      if (l >= 0 && (l & (NT - 1)) == tid) bins[l] += wgt[r];
    }
    r0 = k;
    __syncthreads();
    const size_t slot = (size_t)j * (size_t)Q + (size_t)q;
    if (class_scores)
      for (int c = tid; c < C; c += NT) class_scores[slot * (size_t)C + c] = bins[c];
    float ps = __builtin_inff();            // the previous pick: the next one ranks strictly behind it
    int pc = -1;
    for (int p = 0; p < TOP; ++p) {
      float bs = 0.f;
      int bc = -1;
      for (int c = tid; c < C; c += NT) {
        const float x = bins[c];
        const bool behind = x < ps || (x == ps && c > pc);
        if (behind && (bc < 0 || x > bs)) bs = x, bc = c;         // ascending c inside a thread: > keeps the lower class of a tie
      }
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) {
        const float os = wave_shfl_xor(bs, m);
        const int oc = wave_shfl_xor_i(bc, m);
        if (takes(os, oc, bs, bc)) bs = os, bc = oc;
      }
      if ((tid & (WAVE - 1)) == 0) rs[w] = bs, rc[w] = bc;
      __syncthreads();
      bs = rs[0], bc = rc[0];
#pragma unroll
      for (int i = 1; i < NW; ++i)
        if (takes(rs[i], rc[i], bs, bc)) bs = rs[i], bc = rc[i];
      __syncthreads();
      if (tid == 0) pred[slot * TOP + p] = bc;                    // -1 once the classes are used up (C < 5)
      if (bc >= 0) ps = bs, pc = bc;
    }
  }
}

}  // namespace

extern "C" int clite_knn_topk_merge(const float* scores, int lds, int Q, int Nc, int base, int K, int have, float* top_s, int* top_i, void* stream) {
  if (!scores || !top_s || !top_i || Q <= 0 || Nc <= 0 || lds < Nc || base < 0 || K < 1 || K > MAXK || have < 0 || have > K ||
      (int64_t)base + (int64_t)Nc > (int64_t)0x7fffffff)
    return -1;
  hipStream_t st = (hipStream_t)stream;
  if (lds % 4 == 0 && ((uintptr_t)scores & 15) == 0)
    hipLaunchKernelGGL(knn_topk_merge_kernel<4>, dim3(Q), dim3(NT), 0, st, scores, lds, Nc, base, K, have, top_s, top_i);
  else
    hipLaunchKernelGGL(knn_topk_merge_kernel<1>, dim3(Q), dim3(NT), 0, st, scores, lds, Nc, base, K, have, top_s, top_i);
  return (int)hipGetLastError();
}

extern "C" int clite_knn_vote(const float* top_s, const int* top_i, const int* labels, int Q, int K, int N, int C, const int* ks, int nk, float inv_T,
                              float* class_scores, int* pred, void* stream) {
  if (!top_s || !top_i || !labels || !ks || !pred || Q <= 0 || K < 1 || K > MAXK || N <= 0 || C < 1 || C > MAXC || nk < 1 || nk > CLITE_KNN_MAX_KS ||
      !(inv_T == inv_T) || inv_T < 0.f || inv_T == __builtin_inff())
    return -1;
  Ks kv = {};
  for (int j = 0; j < nk; ++j) {
    if (ks[j] < 1 || ks[j] > K || (j > 0 && ks[j] <= ks[j - 1])) return -1;
    kv.k[j] = ks[j];
  }
  hipLaunchKernelGGL(knn_vote_kernel, dim3(Q), dim3(NT), 0, (hipStream_t)stream, top_s, top_i, labels, Q, K, N, C, kv, nk, inv_T, class_scores, pred);
  return (int)hipGetLastError();
}
