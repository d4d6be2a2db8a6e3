// Image augmentation on the device (clip-lite_amd/augment.py holds the semantics; reference factories.py:112-160, data/dataloader.py:186-192 on the
// CPU): crop box -> antialiased triangle resample to S x S -> horizontal flip -> colour jitter -> ImageNet normalisation, from the uint8 canvases
// the loader workers pre-sized, straight into f32 NCHW (the batch-dict contract) or into the stem's padded NHWC4 input (what clite_image_to_nhwc4
// would make of the f32 form). A second view of the same canvases is a second plan row: no second decode, no second transfer.
//
// One work-item produces all three channels of one output pixel (gray, saturation and hue need them together); lanes run along x, so a wave's
// NHWC4 stores are contiguous, and the canvas bytes of neighbouring lanes share cache lines. The pixel function `view_pixel` is ONE routine,
// used by the gray pass and by both output forms, and this file is compiled with floating-point contraction off: every instantiation performs
// the same IEEE operations in the same order, so the stem form is bit for bit the rounding of the f32 form.
//
// The contrast op needs the mean gray value of the whole view as it stands in front of it: clite_augment_gray_mean is a first pass that applies
// the ops preceding contrast and reduces the gray values, with no float atomics - each workgroup writes one partial (wave butterfly, then the
// waves in order through LDS) and a small second kernel adds a view's partials in workgroup order: the mean is a pure function of its inputs.
//
// Nothing the tables hold can make a kernel read or write out of bounds: a canvas extent that does not fit its slot blanks the view, taps are
// clipped to the canvas and capped at CLITE_AUGMENT_MAX_TAPS per axis. The launchers additionally validate host mirrors of the tables.
#include "vec.h"
#include "clite.h"

#pragma clang fp contract(off)

using namespace clite;

namespace {

constexpr int NT = 256;
constexpr int NW = NT / WAVE;
constexpr int PW = CLITE_AUGMENT_PLAN_W;
constexpr int TAPS = CLITE_AUGMENT_MAX_TAPS;

// plan row fields (augment.py PLAN_*)
enum { P_X0 = 0, P_Y0, P_CW, P_CH, P_FLIP, P_JIT, P_FB, P_FC, P_FS, P_FH, P_ORD, P_NORM = P_ORD + 4 };

struct Axis {          // taps [lo, hi) of one output coordinate, their centre, 1 / support and the sum of the raw weights
  int lo, hi;
  float centre, inv_ss, wsum;
};

DEV float tri(const Axis& a, int i) {
  const float t = 1.f - fabsf(((float)i - a.centre + 0.5f) * a.inv_ss);
  return t > 0.f ? t : 0.f;
}

// PIL's precompute_coeffs for the triangle filter (Resample.c): scale = c / S, centre = o0 + (o + 0.5) scale, support = max(scale, 1)
DEV Axis make_axis(float o0, float c, int S, int o, int n) {
  Axis a;
  const float scale = c / (float)S;
  const float ss = scale > 1.f ? scale : 1.f;
  a.centre = o0 + ((float)o + 0.5f) * scale;
  a.inv_ss = 1.f / ss;
  int lo = (int)(a.centre - ss + 0.5f), hi = (int)(a.centre + ss + 0.5f);
  lo = lo < 0 ? 0 : lo;
  hi = hi > n ? n : hi;
  lo = lo > n - 1 ? n - 1 : lo;          // a box outside the canvas (refused on the host) still reads inside it
  hi = hi < lo + 1 ? lo + 1 : hi;
  hi = hi > lo + TAPS ? lo + TAPS : hi;
  a.lo = lo, a.hi = hi;
  float s = 0.f;
  for (int i = lo; i < hi; ++i) s += tri(a, i);
  a.wsum = s;
  return a;
}

DEV float clamp255(float v) { return v < 0.f ? 0.f : (v > 255.f ? 255.f : v); }
DEV float gray_of(const float (&v)[3]) { return 0.299f * v[0] + 0.587f * v[1] + 0.114f * v[2]; }

// colorsys' RGB -> HSV -> RGB on [0, 255] values with the hue turned by fh (fraction of the circle)
DEV void hue_shift(float (&v)[3], float fh) {
  const float r = v[0], g = v[1], b = v[2];
  const float maxc = fmaxf(r, fmaxf(g, b)), minc = fminf(r, fminf(g, b));
  const float d = maxc - minc;
  if (d <= 0.f) return;          // gray: no hue
  const float s = d / maxc;
  const float rc = (maxc - r) / d, gc = (maxc - g) / d, bc = (maxc - b) / d;
  float h = r == maxc ? bc - gc : (g == maxc ? 2.f + rc - bc : 4.f + gc - rc);
  h = h / 6.f + fh;
  h = h - floorf(h);
  const float h6 = h * 6.f;
  int i = (int)h6;
  const float f = h6 - (float)i;
  i = i >= 6 ? i - 6 : i;
  const float p = maxc * (1.f - s), q = maxc * (1.f - s * f), t = maxc * (1.f - s * (1.f - f));
  v[0] = i == 0 || i == 5 ? maxc : (i == 1 ? q : (i == 4 ? t : p));
  v[1] = i == 1 || i == 2 ? maxc : (i == 3 ? q : (i == 0 ? t : p));
  v[2] = i == 3 || i == 4 ? maxc : (i == 5 ? q : (i == 2 ? t : p));
}

// Output pixel (oy, ox) of the S x S view that plan row `pl` cuts out of the h x w canvas `cv` (HWC uint8, pitch 3 w). GRAY: stop in front of the
// contrast op and return false when the view has none (jitter off); otherwise v holds the finished pixel, normalisation included.
template <bool GRAY>
DEV bool view_pixel(const uint8_t* cv, int h, int w, const float* pl, int S, int oy, int ox, float mean, float (&v)[3]) {
  const bool jit = pl[P_JIT] != 0.f;
  if (GRAY && !jit) return false;
  if (pl[P_FLIP] != 0.f) ox = S - 1 - ox;
  const Axis ax = make_axis(pl[P_X0], pl[P_CW], S, ox, w), ay = make_axis(pl[P_Y0], pl[P_CH], S, oy, h);
  v[0] = v[1] = v[2] = 0.f;
  for (int y = ay.lo; y < ay.hi; ++y) {
    const uint8_t* row = cv + (size_t)y * (size_t)(3 * w);
    float r[3] = {0.f, 0.f, 0.f};
    for (int x = ax.lo; x < ax.hi; ++x) {
      const float wx = tri(ax, x) / ax.wsum;
#pragma unroll
      for (int c = 0; c < 3; ++c) r[c] += wx * (float)row[3 * x + c];
    }
    const float wy = tri(ay, y) / ay.wsum;
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] += wy * r[c];
  }
  if (jit) {
    for (int k = 0; k < 4; ++k) {
      const int op = (int)pl[P_ORD + k];
      if (op == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = clamp255(v[c] * pl[P_FB]);
      } else if (op == 1) {
        if (GRAY) return true;
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = clamp255(mean + pl[P_FC] * (v[c] - mean));
      } else if (op == 2) {
        const float g = gray_of(v);
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = clamp255(g + pl[P_FS] * (v[c] - g));
      } else {
        hue_shift(v, pl[P_FH]);
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = clamp255(v[c]);
      }
    }
  }
  if (GRAY) return true;          // (a plan without a contrast op: the mean is never used, the gray of the finished ops is as good as any)
  const float mu[3] = {0.485f, 0.456f, 0.406f}, sd[3] = {0.229f, 0.224f, 0.225f};          // reference data/transforms.py:232-235
  const bool norm = pl[P_NORM] != 0.f;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float u = v[c] / 255.f;
    v[c] = norm ? (u - mu[c]) / sd[c] : u;
  }
  return true;
}

// the canvas of view n, or nullptr when its (h, w) entry does not fit a slot
DEV const uint8_t* canvas_of(const uint8_t* canv, const int* hw, long long cap, int n, int& h, int& w) {
  h = hw[2 * n], w = hw[2 * n + 1];
  if (h <= 0 || w <= 0 || (long long)h * (long long)w * 3 > cap) return nullptr;
  return canv + (size_t)n * (size_t)cap;
}

// part[n][b] = sum of the gray values of workgroup b's pixels of view n (jitter on), in a fixed order. grid = (ceil(S S / NT), N).
__global__ __launch_bounds__(NT) void augment_gray_kernel(const uint8_t* canv, const int* hw, long long cap, const float* plan, int S, float* part) {
  __shared__ float red[NW];
  const int n = blockIdx.y, tid = threadIdx.x;
  const float* pl = plan + (size_t)n * PW;
  if (pl[P_JIT] == 0.f) return;          // the whole workgroup: the sum pass writes this view's mean without reading partials
  int h, w;
  const uint8_t* cv = canvas_of(canv, hw, cap, n, h, w);
  const int px = blockIdx.x * NT + tid;
  float g = 0.f;
  if (cv && px < S * S) {
    float v[3];
    view_pixel<true>(cv, h, w, pl, S, px / S, px - (px / S) * S, 0.f, v);
    g = gray_of(v);
  }
  g = wave_sum(g);
  if ((tid & (WAVE - 1)) == 0) red[tid / WAVE] = g;
  __syncthreads();
  if (tid == 0) {
    float s = red[0];
#pragma unroll
    for (int k = 1; k < NW; ++k) s += red[k];
    part[(size_t)n * gridDim.x + blockIdx.x] = s;
  }
}

// mean[n] = (sum of view n's nb partials, in workgroup order) / (S S); 0 for a view without jitter
__global__ __launch_bounds__(NT) void augment_gray_sum_kernel(const float* part, int nb, const float* plan, int N, int S, float* mean) {
  const int n = blockIdx.x * NT + threadIdx.x;
  if (n >= N) return;
  float s = 0.f;
  if (plan[(size_t)n * PW + P_JIT] != 0.f)
    for (int b = 0; b < nb; ++b) s += part[(size_t)n * nb + b];
  mean[n] = s / (float)(S * S);
}

// FORM 0: out f32 [N][3][S][S] (Hp = Wp = S, pad = 0). FORM 1: out T [N][Hp][Wp][4], the S x S view at (pad, pad), zeros everywhere else.
// A work-item per element of the [Hp][Wp] plane; grid = (ceil(Hp Wp / NT), N).
template <int FORM, typename T>
__global__ __launch_bounds__(NT) void augment_apply_kernel(const uint8_t* canv, const int* hw, long long cap, const float* plan, const float* mean,
                                                           int S, int pad, int Hp, int Wp, T* out) {
  const int n = blockIdx.y;
  const int px = blockIdx.x * NT + threadIdx.x;
  if (px >= Hp * Wp) return;
  const int hp = px / Wp, wp = px - hp * Wp;
  const int oy = hp - pad, ox = wp - pad;
  float v[3] = {0.f, 0.f, 0.f};
  int h, w;
  const uint8_t* cv = canvas_of(canv, hw, cap, n, h, w);
  if (cv && (unsigned)oy < (unsigned)S && (unsigned)ox < (unsigned)S)
    view_pixel<false>(cv, h, w, plan + (size_t)n * PW, S, oy, ox, mean[n], v);
  if constexpr (FORM == 0) {
    float* o = (float*)out + (size_t)n * 3 * S * S + px;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[(size_t)c * S * S] = v[c];
  } else {
    T* o = out + ((size_t)n * Hp * Wp + px) * 4;
    if constexpr (sizeof(T) == 2) {          // the conversion of image_to_nhwc4_kernel
      union { bf16 x[4]; u32x2 u; } pk;
      pk.x[0] = f2bf(v[0]); pk.x[1] = f2bf(v[1]); pk.x[2] = f2bf(v[2]); pk.x[3] = f2bf(0.f);
      *(u32x2*)o = pk.u;
    } else {
      *(f32x4*)o = f32x4{v[0], v[1], v[2], 0.f};
    }
  }
}

bool finite_f(float x) { return x == x && x - x == 0.f; }

// host mirrors of the tables (optional): 0, or the error code of the first bad entry
int check_tables(const float* plan_host, const int* hw_host, int N, int S, long long cap) {
  for (int n = 0; n < N; ++n) {
    if (hw_host) {
      const long long h = hw_host[2 * n], w = hw_host[2 * n + 1];
      if (h <= 0 || w <= 0 || h * w * 3 > cap) return -2;
    }
    if (plan_host) {
      const float* pl = plan_host + (size_t)n * PW;
      for (int k = 0; k < PW; ++k)
        if (!finite_f(pl[k])) return -3;
      if (!(pl[P_CW] > 0.f) || !(pl[P_CH] > 0.f)) return -3;
      if (pl[P_CW] > (float)CLITE_AUGMENT_MAX_SCALE * (float)S || pl[P_CH] > (float)CLITE_AUGMENT_MAX_SCALE * (float)S) return -4;
      if (hw_host) {
        const float h = (float)hw_host[2 * n], w = (float)hw_host[2 * n + 1];
        if (pl[P_X0] < 0.f || pl[P_Y0] < 0.f || pl[P_X0] + pl[P_CW] > w || pl[P_Y0] + pl[P_CH] > h) return -3;
      }
      int seen = 0;
      for (int k = 0; k < 4; ++k) {
        const float o = pl[P_ORD + k];
        if (o != 0.f && o != 1.f && o != 2.f && o != 3.f) return -3;
        seen |= 1 << (int)o;
      }
      if (seen != 15) return -3;
    }
  }
  return 0;
}

bool shape_ok(int N, int S, long long cap) {
  return N > 0 && N <= 65535 && S > 0 && S <= 4096 && cap > 0;
}

}  // namespace

extern "C" int clite_augment_gray_mean(const uint8_t* canvases, const int* hw, int64_t cap, const float* plan, int N, int S, float* mean,
                                       float* work, const float* plan_host, const int* hw_host, void* stream) {
  if (!canvases || !hw || !plan || !mean || !work || !shape_ok(N, S, cap)) return -1;
  if (int rc = check_tables(plan_host, hw_host, N, S, cap)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int nb = CLITE_AUGMENT_GRAY_BLOCKS(S);
  hipLaunchKernelGGL(augment_gray_kernel, dim3(nb, N), dim3(NT), 0, st, canvases, hw, (long long)cap, plan, S, work);
  hipLaunchKernelGGL(augment_gray_sum_kernel, dim3((N + NT - 1) / NT), dim3(NT), 0, st, (const float*)work, nb, plan, N, S, mean);
  return (int)hipGetLastError();
}

extern "C" int clite_augment_apply(int form, int dtype, const uint8_t* canvases, const int* hw, int64_t cap, const float* plan, const float* mean,
                                   int N, int S, void* out, int pad, int Hp, int Wp, const float* plan_host, const int* hw_host, void* stream) {
  if (!canvases || !hw || !plan || !mean || !out || !shape_ok(N, S, cap)) return -1;
  if (form == CLITE_AUGMENT_NCHW) {
    if (dtype != CLITE_F32) return -1;
    pad = 0, Hp = Wp = S;
  } else if (form == CLITE_AUGMENT_NHWC4) {
    if ((dtype != CLITE_BF16 && dtype != CLITE_F32) || pad < 0 || Hp < S + 2 * pad || Wp < S + 2 * pad || Hp > 8192 || Wp > 8192) return -1;
  } else {
    return -1;
  }
  if (int rc = check_tables(plan_host, hw_host, N, S, cap)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((Hp * Wp + NT - 1) / NT, N);
  if (form == CLITE_AUGMENT_NCHW)
    hipLaunchKernelGGL((augment_apply_kernel<0, float>), grid, dim3(NT), 0, st, canvases, hw, (long long)cap, plan, mean, S, pad, Hp, Wp, (float*)out);
  else if (dtype == CLITE_BF16)
    hipLaunchKernelGGL((augment_apply_kernel<1, bf16>), grid, dim3(NT), 0, st, canvases, hw, (long long)cap, plan, mean, S, pad, Hp, Wp, (bf16*)out);
  else
    hipLaunchKernelGGL((augment_apply_kernel<1, float>), grid, dim3(NT), 0, st, canvases, hw, (long long)cap, plan, mean, S, pad, Hp, Wp, (float*)out);
  return (int)hipGetLastError();
}
