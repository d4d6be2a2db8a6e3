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
// Gray and blur (augment.py steps 3b / 3c) come from a second table, `post`, through clite_augment_apply_post: blur needs a pixel's neighbours
// AFTER the non-linear colour ops, so that kernel works on a 32 x 32 tile of the view per workgroup - the un-normalised pixels of the tile and a
// 3-pixel halo (at the reflected view coordinates) go to LDS, a horizontal and a vertical 7-tap pass follow. The pixel function is split into
// its colour stage (`view_colour`) and its normalise stage (`view_normalise`); `view_pixel` is the two in a row, so all kernels still share one routine.
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

// Colour stage (steps 1-3) of output pixel (oy, ox) of the S x S view that plan row `pl` cuts out of the h x w canvas `cv` (HWC uint8, pitch 3 w):
// v holds the jittered pixel on [0, 255], not normalised. GRAY: stop in front of the contrast op and return false when the view has none (jitter off).
template <bool GRAY>
DEV bool view_colour(const uint8_t* cv, int h, int w, const float* pl, int S, int oy, int ox, float mean, float (&v)[3]) {
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
  return true;          // (GRAY with a plan without a contrast op: the mean is never used, the gray of the finished ops is as good as any)
}

// Normalise stage (step 4) of a pixel on [0, 255]
DEV void view_normalise(const float* pl, float (&v)[3]) {
  const float mu[3] = {0.485f, 0.456f, 0.406f}, sd[3] = {0.229f, 0.224f, 0.225f};          // reference data/transforms.py:232-235
  const bool norm = pl[P_NORM] != 0.f;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float u = v[c] / 255.f;
    v[c] = norm ? (u - mu[c]) / sd[c] : u;
  }
}

// The whole pixel function: with GRAY what view_colour<true> leaves, otherwise the finished pixel, normalisation included.
template <bool GRAY>
DEV bool view_pixel(const uint8_t* cv, int h, int w, const float* pl, int S, int oy, int ox, float mean, float (&v)[3]) {
  const bool r = view_colour<GRAY>(cv, h, w, pl, S, oy, ox, mean, v);
  if (!GRAY) view_normalise(pl, v);
  return r;
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

// element px of view n's [Hp][Wp] plane. FORM 0: the three channel planes of f32 NCHW. FORM 1: one NHWC4 pixel, channel 3 zero.
template <int FORM, typename T>
DEV void store_pixel(T* out, int n, int S, int Hp, int Wp, int px, const float (&v)[3]) {
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
  store_pixel<FORM>(out, n, S, Hp, Wp, px, v);
}

constexpr int QW = CLITE_AUGMENT_POST_W;
constexpr int TS = 32;                   // side of a workgroup's tile of the view
constexpr int HALO = 3;                  // the 7-tap filter's reach
constexpr int TSH = TS + 2 * HALO;

// post row fields (augment.py POST_*)
enum { Q_GRAY = 0, Q_BLUR, Q_W0 };

// OpenCV's default border (REFLECT_101: -1 -> 1, S -> S - 2), then clamped: no table and no S can make the result leave [0, S - 1]
DEV int reflect101(int q, int S) {
  q = q < 0 ? -q : q;
  q = q >= S ? 2 * S - 2 - q : q;
  return q < 0 ? 0 : (q > S - 1 ? S - 1 : q);
}

// clite_augment_apply with steps 3b / 3c. A workgroup per TS x TS tile of the view, grid = (ceil(S / TS)^2, N): the post flags of view n are
// uniform across the workgroup, so every barrier is reached by all of it or by none. Both LDS arrays hold three f32 per pixel: neighbouring
// lanes are 3 dwords apart, an odd stride, so the 32 lanes of an access group fall on 32 different banks.
template <int FORM, typename T>
__global__ __launch_bounds__(NT) void augment_post_kernel(const uint8_t* canv, const int* hw, long long cap, const float* plan, const float* post,
                                                          const float* mean, int S, int pad, int Hp, int Wp, T* out) {
  __shared__ float a[TSH * TSH * 3];          // colour stage of the tile and its halo
  __shared__ float b[TSH * TS * 3];           // ... after the horizontal pass
  const int n = blockIdx.y, tid = threadIdx.x;
  const int tiles = (S + TS - 1) / TS;
  const int ty = blockIdx.x / tiles, tx = blockIdx.x - ty * tiles;
  const int oy0 = ty * TS, ox0 = tx * TS;
  const int th = S - oy0 < TS ? S - oy0 : TS, tw = S - ox0 < TS ? S - ox0 : TS;
  const float* pl = plan + (size_t)n * PW;
  const float* q = post + (size_t)n * QW;
  const bool gray = q[Q_GRAY] != 0.f, blur = q[Q_BLUR] != 0.f;
  const float m = mean[n];
  int h, w;
  const uint8_t* cv = canvas_of(canv, hw, cap, n, h, w);
  if (!blur) {
    for (int i = tid; i < th * tw; i += NT) {
      const int ly = i / tw, lx = i - ly * tw;
      float v[3] = {0.f, 0.f, 0.f};
      if (cv) {
        view_colour<false>(cv, h, w, pl, S, oy0 + ly, ox0 + lx, m, v);
        if (gray) v[0] = v[1] = v[2] = gray_of(v);
        view_normalise(pl, v);
      }
      store_pixel<FORM>(out, n, S, Hp, Wp, (oy0 + ly + pad) * Wp + ox0 + lx + pad, v);
    }
  } else {
    const float wt[4] = {q[Q_W0], q[Q_W0 + 1], q[Q_W0 + 2], q[Q_W0 + 3]};
    const int aw = tw + 2 * HALO, ah = th + 2 * HALO;
    for (int i = tid; i < ah * aw; i += NT) {
      const int ry = i / aw, rx = i - ry * aw;
      float v[3] = {0.f, 0.f, 0.f};
      if (cv) {
        view_colour<false>(cv, h, w, pl, S, reflect101(oy0 + ry - HALO, S), reflect101(ox0 + rx - HALO, S), m, v);
        if (gray) v[0] = v[1] = v[2] = gray_of(v);
      }
      float* o = a + (ry * TSH + rx) * 3;
      o[0] = v[0], o[1] = v[1], o[2] = v[2];
    }
    __syncthreads();
    for (int i = tid; i < ah * tw; i += NT) {
      const int ry = i / tw, lx = i - ry * tw;
      const float* src = a + (ry * TSH + lx + HALO) * 3;
      float s[3] = {0.f, 0.f, 0.f};
#pragma unroll
      for (int k = -HALO; k <= HALO; ++k) {
        const float wk = wt[k < 0 ? -k : k];
#pragma unroll
        for (int c = 0; c < 3; ++c) s[c] += wk * src[3 * k + c];
      }
      float* o = b + (ry * TS + lx) * 3;
      o[0] = s[0], o[1] = s[1], o[2] = s[2];
    }
    __syncthreads();
    for (int i = tid; i < th * tw; i += NT) {
      const int ly = i / tw, lx = i - ly * tw;
      const float* src = b + ((ly + HALO) * TS + lx) * 3;
      float v[3] = {0.f, 0.f, 0.f};
#pragma unroll
      for (int k = -HALO; k <= HALO; ++k) {
        const float wk = wt[k < 0 ? -k : k];
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] += wk * src[3 * TS * k + c];
      }
      if (cv) view_normalise(pl, v);
      store_pixel<FORM>(out, n, S, Hp, Wp, (oy0 + ly + pad) * Wp + ox0 + lx + pad, v);
    }
  }
  if constexpr (FORM == 1) {          // the plane's border (and its channel 3), shared out over the view's workgroups
    const float z[3] = {0.f, 0.f, 0.f};
    for (int px = blockIdx.x * NT + tid; px < Hp * Wp; px += gridDim.x * NT) {
      const int hp = px / Wp, wp = px - hp * Wp;
      if ((unsigned)(hp - pad) >= (unsigned)S || (unsigned)(wp - pad) >= (unsigned)S) store_pixel<FORM>(out, n, S, Hp, Wp, px, z);
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

// host mirror of the post table (optional): -3 for a flag that is not 0 or 1, a weight that is not finite or negative, and on a blurred row
// for weights that do not sum to 1 or a view smaller than the filter's reflection needs
int check_post(const float* post_host, int N, int S) {
  if (!post_host) return 0;
  for (int n = 0; n < N; ++n) {
    const float* q = post_host + (size_t)n * QW;
    for (int k = Q_GRAY; k <= Q_BLUR; ++k)
      if (q[k] != 0.f && q[k] != 1.f) return -3;
    for (int k = Q_W0; k < Q_W0 + 4; ++k)
      if (!finite_f(q[k]) || q[k] < 0.f) return -3;
    if (q[Q_BLUR] != 0.f) {
      const float d = q[Q_W0] + 2.f * (q[Q_W0 + 1] + q[Q_W0 + 2] + q[Q_W0 + 3]) - 1.f;
      if (!(d <= 1e-3f && d >= -1e-3f) || S < HALO + 1) return -3;
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

extern "C" int clite_augment_apply_post(int form, int dtype, const uint8_t* canvases, const int* hw, int64_t cap, const float* plan, const float* post,
                                        const float* mean, int N, int S, void* out, int pad, int Hp, int Wp, const float* plan_host,
                                        const int* hw_host, const float* post_host, void* stream) {
  if (!canvases || !hw || !plan || !post || !mean || !out || !shape_ok(N, S, cap)) return -1;
  if (form == CLITE_AUGMENT_NCHW) {
    if (dtype != CLITE_F32) return -1;
    pad = 0, Hp = Wp = S;
  } else if (form == CLITE_AUGMENT_NHWC4) {
    if ((dtype != CLITE_BF16 && dtype != CLITE_F32) || pad < 0 || Hp < S + 2 * pad || Wp < S + 2 * pad || Hp > 8192 || Wp > 8192) return -1;
  } else {
    return -1;
  }
  if (int rc = check_tables(plan_host, hw_host, N, S, cap)) return rc;
  if (int rc = check_post(post_host, N, S)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int tiles = (S + TS - 1) / TS;
  const dim3 grid(tiles * tiles, N);
  if (form == CLITE_AUGMENT_NCHW)
    hipLaunchKernelGGL((augment_post_kernel<0, float>), grid, dim3(NT), 0, st, canvases, hw, (long long)cap, plan, post, mean, S, pad, Hp, Wp, (float*)out);
  else if (dtype == CLITE_BF16)
    hipLaunchKernelGGL((augment_post_kernel<1, bf16>), grid, dim3(NT), 0, st, canvases, hw, (long long)cap, plan, post, mean, S, pad, Hp, Wp, (bf16*)out);
  else
    hipLaunchKernelGGL((augment_post_kernel<1, float>), grid, dim3(NT), 0, st, canvases, hw, (long long)cap, plan, post, mean, S, pad, Hp, Wp, (float*)out);
  return (int)hipGetLastError();
}
