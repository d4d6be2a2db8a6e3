/* clite.h — C ABI of libclite_hip.so, the MI355X (gfx950) kernel library behind the CLIP-Lite
 * pretraining step.
 *
 * The reference (4m4n5/CLIP-Lite) has no native layer: its hot path is Python calling ATen/cuDNN/cuBLAS.
 * Every entry point below therefore cites the reference *call site* whose device math it replaces
 * (file:line relative to the reference repository). The host side that mirrors the reference's Python
 * classes lives in clip-lite_amd/ and reaches these functions through ctypes.
 *
 * Conventions
 *   - plain pointers and sizes only; all pointers are device pointers owned by the caller
 *   - bf16 tensors are passed as void*; "f32" means IEEE binary32
 *   - activations are NHWC / row-major [rows][features]; weights are [out][...in], inner dim contiguous
 *   - `stream` is a hipStream_t; kernels are only enqueued, nothing synchronises, nothing allocates
 *   - return value: 0 on success, a hipError_t value or -1 (bad argument) otherwise; nothing throws
 *   - entry points are re-entrant (forward runs on the Python main thread, backward on the autograd engine
 *     thread). The library holds exactly two pieces of process-wide state, both plain atomics set through their
 *     own entry points and never written by a kernel launcher: the deterministic-reduction flag
 *     (clite_set_deterministic) and the tile policy (clite_set_tile_policy). Both are read once per call, when
 *     the kernels are ENQUEUED: a captured hipGraph keeps the mode it was recorded in, an eager step follows the
 *     current value — set them before a step, not during one.
 */
#ifndef CLITE_H
#define CLITE_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CLITE_ABI_VERSION 12
int clite_abi_version(void);

/* Deterministic-reduction mode (process-wide, default off; the counterpart of torch.use_deterministic_algorithms for this library).
 * Off: split-K partial products, BatchNorm / bias / LayerNorm statistics and the loss scalars meet through float atomics, so the
 * summation order — and with it the last bits of every gradient — differs from run to run. On: every launcher picks a decomposition in
 * which each address receives exactly one contribution per launch (unsplit K ranges, one row slab per statistics replica, single-wave
 * loss kernels; clip-lite_amd/csrc/det.h), so two runs of the same step are bit-identical — which is what makes checkpoint-resume
 * equivalence (reference utils/checkpointing.py:169-222, train.py:143-148) testable exactly. Several times slower; a testing aid.
 * The flag is read when a kernel is enqueued (a captured hipGraph keeps the mode it was recorded in). Returns 0. */
int clite_set_deterministic(int on);
int clite_get_deterministic(void);

/* ABI v10 — split-bf16 form of the exact-f32 mode (process-wide, like the deterministic switch). With dtype CLITE_F32 the GEMM / convolution entry
 * points keep f32 storage, f32 accumulation and f32 epilogues, but form every product on three bf16 MFMAs: x = hi + lo with hi = bf16(x),
 * lo = bf16(x - hi), a b ~ lo_a hi_b + hi_a lo_b + hi_a hi_b (bf16 x bf16 products are exact in f32). Relative error ~2^-17 per product — between the
 * bf16 path's 2^-9 and the default f32 path's exact fmaf chain (v_mfma_f32_32x32x2_f32, 1/16 of the bf16 matrix rate) — at 3/16 of the default's
 * matrix-pipe time. The full-size parity test (tests/test_gpu_model.py) holds this form to the same 1e-4 loss bar as the exact form. Off by default;
 * bf16 launches are unaffected. */
int clite_set_f32_split(int on);
int clite_get_f32_split(void);

/* Tile-shape policy of the bf16 GEMM / conv launchers (process-wide, default 0). 0: automatic — per launch, the largest of the 128 x 128,
 * 256 x 128 and 256 x 256 wide-K tiles (K tile 64 = whole 128-byte lines, 8 waves; clip-lite_amd/csrc/igemm_wide.h) that still fills the
 * 256 CUs. 1 / 2 / 3: force that wide tile wherever an instantiation exists. 4: keep every launch on the 4-wave 128 x 128 x 32 kernels.
 * The forced forms exist so that every instantiation can be parity-tested on small problems; results are identical up to the
 * summation order of the K loop. Returns 0, or -1 for an unknown policy. */
int clite_set_tile_policy(int policy);

/* storage type of activations / weights handed to a kernel. CLITE_F32 selects the exact-f32 parity mode
 * (v_mfma_f32_32x32x2_f32, 1/16 of the bf16 MFMA rate). Accumulation is f32 in both. */
enum { CLITE_BF16 = 0, CLITE_F32 = 1 };

/* Dropout / noise seeds. Every (seed, site) pair below is normally passed by value. When CLITE_SEED_INDIRECT is OR-ed into the
 * site, the 64-bit seed argument is instead the DEVICE ADDRESS of a uint64_t holding the seed: the kernel loads it (one scalar
 * load per wave) and masks the flag off the site. A captured hipGraph of the train step uses this form so that every replay
 * draws fresh masks from a device-side counter without re-recording kernel arguments. */
#define CLITE_SEED_INDIRECT 0x80000000u

enum { CLITE_ACT_NONE = 0, CLITE_ACT_RELU = 1, CLITE_ACT_GELU = 2, CLITE_ACT_TANH = 3 };

/* Fused GEMM epilogue. v = alpha*acc + bias; preact <- v; v = act(v); v *= act'(dact_aux);
 * v = dropout(v); v += residual; [mask_after_residual: the act'(dact_aux) factor is applied here instead]; out <- v;
 * colsum += (sum, sum of squares) of the stored values — or, when bn_y is given, (sum v, sum v*(bn_y - mean)): the two
 * reductions of a BatchNorm backward over the tensor this GEMM produces (dz = masked gradient, bn_y = that BN's input,
 * mean_c = sum over replicas of bn_stats[r*bn_rstride + c] * bn_inv_count), which saves the separate reduction pass. */
typedef struct clite_epilogue {
  void* out;            /* [M][ldc] in the call's dtype, or f32 when out_f32 = 1 */
  int32_t ldc;
  int32_t out_f32;
  int32_t atomic;       /* 1: out (f32) += alpha*acc with float atomics (split-K / gradient accumulation) */
  float alpha;
  const float* bias;    /* [N] f32 or NULL */
  int32_t act;          /* CLITE_ACT_* */
  void* preact;         /* [M][ldc] in the call's dtype, or NULL */
  const void* dact_aux; /* [M][ldc] in the call's dtype, or NULL */
  int32_t dact;         /* 1 relu' (aux = forward output), 2 gelu' (aux = pre-activation), 3 tanh' (aux = output) */
  float drop_p;
  uint64_t drop_seed;
  uint32_t drop_site;
  const void* residual; /* [M][ldc] in the call's dtype, or NULL */
  float* colsum;        /* f32 [2][N] or NULL */
  int32_t colsum_replicas;  /* R > 1: workgroup b accumulates into colsum + (b % R) * colsum_stride (spreads same-address atomics) */
  int32_t colsum_stride;    /* elements between replicas */
  int32_t colsum_rows;      /* 0 or 2: both rows [2][N]; 1: the column sums only (row 0) — e.g. straight into a bias gradient, whose neighbour in
                             * memory is another tensor */
  const void* bn_y;         /* [M][ldc] in the call's dtype, or NULL (plain sum of squares) */
  const float* bn_stats;    /* forward statistics of that BatchNorm: replicated [R][3][N] sums (row 0 = sum of y) */
  int32_t bn_replicas;
  int32_t bn_rstride;
  float bn_inv_count;       /* 1 / rows of the BatchNorm */
  int32_t mask_after_residual;
  const uint8_t* relu_bits; /* BatchNorm-backward form only (bn_y / mask_after_residual): the relu' mask as PACKED BITS instead of dact_aux — bit (c & 7)
                             * of byte (row * ldc + c) / 8 is 1 where the forward activation was > 0 (written by clite_bn_apply, clite_bn.relu_bits):
                             * 1/16 of the bytes of reading the bf16 activation for its sign. NULL: dact_aux (if any) supplies the mask. */
  float* splitk_ws;         /* optional f32 [M][N] workspace, ZERO on entry (left dirty): lets clite_gemm_nt / _nn run a GEMM of few output tiles
                             * (the M = 128/256-row GEMMs of the projection heads and prior discriminators) as split-K over all CUs — partial
                             * sums accumulate here with float atomics and a second small kernel applies this epilogue. NULL: never split. */
  int32_t residual_subsample; /* ABI v10. 0 / 1: `residual` has the output's rows. 2: clite_conv_dgrad_wt of a 1 x 1 / stride 1 convolution in the
                             * BatchNorm-backward form only (bn_y + relu_bits + mask_after_residual, bf16): `residual` is the COMPACT tensor
                             * [N][H/2][W/2][ldc] whose pixel (n, h/2, w/2) is added to output pixel (n, h, w) for even h, w and nothing elsewhere —
                             * the input gradient of the block's stride-2 1 x 1 shortcut, kept compact instead of scatter-added into the full-size
                             * gradient (which cost a read-modify-write pass and, before it, a separate BatchNorm-backward reduction pass). */
  /* ABI v11, clite_gemm_nt_fp8 only (every other entry point returns -1 when one of them is set): the producer-fused e4m3 quantiser of the NEXT
   * GEMM's A operand, as clite_bn.fp8_* for clite_bn_apply — BERT's FFN1 launch leaves the e4m3 copy of its GELU output for FFN2.
   *   fp8_out   [M][ldc] bytes: e4m3(clamp(out * fp8_scale[0], +-448)) of the bf16 value as stored (bf16 out only);
   *   fp8_scale device f32[2] = {scale, 1 / scale}, delayed scaling (clite_fp8_scale_update); required with fp8_out;
   *   fp8_amax  one amax slot (CLITE_FP8_AMAX_REPLICAS x CLITE_FP8_AMAX_STRIDE words): max |out| of this call. Any of the three may be NULL. */
  uint8_t* fp8_out;
  const float* fp8_scale;
  float* fp8_amax;
} clite_epilogue;

/* NHWC convolution problem. x: [N][H][W][C], w: [K][R][S][C], y: [N][Ho][Wo][K], all of `dtype`. */
typedef struct clite_conv {
  int32_t dtype;
  int32_t N, H, W, C;
  int32_t K, R, S;
  int32_t stride, pad;
  int32_t Ho, Wo;
} clite_conv;

/* lda / ldb: row strides in elements (multiples of 8), so a strided row subset (BERT's h[:, 0] for the pooler) needs no copy.
 * C[M,N] = A[M,K] * B[N,K]^T  — nn.Linear forward (reference loss.py:16-22,46-48; HF BertModel linears
 * behind encoder.py:193). K % 8 == 0, N % 8 == 0. */
int clite_gemm_nt(const void* A, int lda, const void* B, int ldb, int M, int N, int K, int dtype, const clite_epilogue* ep, void* stream);
/* C[M,N] = A[M,K] * B[K,N]       — nn.Linear input gradient (autograd of the same call sites). */
int clite_gemm_nn(const void* A, int lda, const void* B, int ldb, int M, int N, int K, int dtype, const clite_epilogue* ep, void* stream);
/* C[M,N] (+)= A[K,M]^T * B[K,N]  — nn.Linear weight gradient; ep->atomic selects f32 accumulation. */
int clite_gemm_tn(const void* A, int lda, const void* B, int ldb, int M, int N, int K, int dtype, const clite_epilogue* ep, void* stream);

/* y = conv(x, w): torchvision ResNet nn.Conv2d forward (reference encoder.py:36-38,63; block arithmetic as
 * restated in model_zoo/resnet.py:60-100). Epilogue applies to y viewed as [N*Ho*Wo][K]. */
int clite_conv_fwd(const void* x, const void* w, const clite_conv* cv, const clite_epilogue* ep, void* stream);
/* dx = conv_transpose(dy, w): autograd of the same call. Epilogue applies to dx viewed as [N*H*W][C]. */
int clite_conv_dgrad(const void* dy, const void* w, const clite_conv* cv, const clite_epilogue* ep, void* stream);
/* One parity class (ph, pw in {0,1}) of the dgrad of a 3x3 / stride-2 / pad-1 conv (H, W even; C, K multiples of 64): writes only the
 * input pixels (2*hq + ph, 2*wq + pw). wsub = the taps that reach this class, w[:, r0::2, s0::2, :] with r0 = (ph+1)&1, s0 = (pw+1)&1,
 * packed [K][na][nb][C]. The four classes together equal clite_conv_dgrad at a quarter of the work (no structurally-zero taps). The
 * epilogue (incl. the BatchNorm-backward form) applies to the rows of the class. */
int clite_conv_dgrad_s2class(const void* dy, const void* wsub, const clite_conv* cv, int ph, int pw, const clite_epilogue* ep, void* stream);
/* The same two input gradients with the weight given TRANSPOSED, wt = [C][R][S][K] (wtsub = [C][na][nb][K]): both GEMM operands are then
 * k-contiguous — the forward form of the tile engine — which the 8-wave kernels stage 10-25 % faster than a k-strided weight image. The
 * transposed copies are re-derived once per step by clite_transpose_weights. Same epilogue semantics and results (up to the summation order). */
int clite_conv_dgrad_wt(const void* dy, const void* wt, const clite_conv* cv, const clite_epilogue* ep, void* stream);
int clite_conv_dgrad_s2class_wt(const void* dy, const void* wtsub, const clite_conv* cv, int ph, int pw, const clite_epilogue* ep, void* stream);
/* dw[K][R][S][C] (f32) += dy^T * im2col(x): autograd of the same call; float-atomic split-K. */
int clite_conv_wgrad(const void* dy, const void* x, const clite_conv* cv, float* dw, void* stream);
/* ABI v10 — the same weight gradient for the 3 x 3 / stride 1 / pad 1, 64 -> 64 channel convolutions (torchvision ResNet layer1 conv2; bf16) on the
 * patch-resident kernel: one persistent workgroup per CU owns the whole [64][3][3][64] gradient in registers and reads dy and the input patch of
 * each strip of rows ONCE (the grouped form gathers every input pixel nine times: 97 us against an HBM ideal of 19 at 56 x 56, batch 128).
 * ws: caller-owned scratch of at least clite_conv_wgrad_patch_workspace() bytes (per-workgroup partial sums; contents undefined afterwards).
 * Returns 0 when launched, 1 when the problem is not one it covers (other shape / dtype, workspace too small, deterministic mode, forced tile
 * policy): nothing was launched and the caller takes clite_conv_wgrad or clite_wgrad_group; < 0 on errors. */
int clite_conv_wgrad_patch_workspace(uint64_t* nbytes);
int clite_conv_wgrad_patch(const void* dy, const void* x, const clite_conv* cv, float* dw, void* ws, uint64_t ws_bytes, void* stream);

/* Grouped weight gradients: every member is one independent dW (f32) += A^T B of the backward pass, all enqueued as ONE launch per tile
 * family so that thousands of workgroups exist without splitting the short-K members (a lone weight gradient has a few dozen output tiles
 * and needs split-K + float atomics to fill 256 CUs: 328 vs 666 TF/s on the BERT FFN gradient; clip-lite_amd/csrc/gemm_group.hip).
 *   kind 0: conv weight gradient — a = dy [N][Ho][Wo][K], b = x [N][H][W][C], cv, out = dw [K][R][S][C]   (as clite_conv_wgrad)
 *   kind 1: linear weight gradient — out[M][N] (row stride ldc) += a[K][M]^T b[K][N]                     (as clite_gemm_tn with ep.atomic)
 *   kind 2 (ABI v12; BASELINE configs[4]): conv weight gradient on FP8 operands — a = dy8 [N][Ho][Wo][K] OCP e5m2 (the copy clite_bn_bwd_apply's fused
 *           quantiser leaves for clite_conv_dgrad_fp8), b = x8 [N][H][W][C] OCP e4m3 (the copy clite_bn_apply leaves for clite_conv_fwd_fp8), cv, a_scales /
 *           b_scales; C % 16 == 0, K % 16 == 0. v_mfma_scale_f32_32x32x64_f8f6f4 (A e5m2, B e4m3) at unit block scales on the grouped 256 x 256 tile,
 *           fragments by ds_read_b64_tr_b8, f32 accumulate. Grouped launches only (-1 where the members run one by one).
 * ws_dev / ws_host: device workspace and PINNED host staging of ws_bytes each (clite_wgrad_group_workspace gives a sufficient size); the
 * library fills ws_host, copies it with one hipMemcpyAsync on `stream` and launches — under stream capture that is a memcpy node, so ws_host
 * must stay alive and unchanged for as long as the captured graph is replayed. With dtype = CLITE_F32, in deterministic-reduction mode, or
 * with ws_dev / ws_host NULL the members are launched one by one. Returns 0, -1 (bad member), -2 (workspace too small) or a HIP status. */
#define CLITE_WGRAD_NARROW 0x100   /* OR-ed into `kind`: keep this member on the 4-wave 128 x 128 x 32 tiles (members with >= 256 rows and columns
                                    * otherwise take the 8-wave 256 x 256 tile); for A/B timing and parity tests */
#define CLITE_WGRAD_ZEROED 0x200   /* ABI v10, OR-ed into `kind`: the caller vouches that `out` holds ZEROS on entry (the train step's update kernel leaves the
                                    * gradient arena zeroed and the step visits this weight once). A member whose contraction fits one K chunk — every BERT
                                    * matrix, the 7 x 7-resolution convolutions — then writes its result with plain stores instead of float atomics
                                    * (memory-side, ~1.3 TB/s chip-wide: 437 MB per step for BERT's 109 M parameters). Same values; without the flag `+=`. */
#define CLITE_WGRAD_SHORTK 0x400   /* ABI v12, OR-ed into `kind`: K chunks of a quarter of the usual length — a member with a tiny output and a very long contraction (the
                                    * folded BatchNorm backward's Gram matrix a^T a: 64 x 64 ... 128 x 128 outputs over 100k - 400k pixels), whose few long workgroups
                                    * would otherwise be the tail of the launch; more chunks cost only more float atomics into that tiny output */
typedef struct clite_wgrad_item {
  int32_t kind;
  const void* a;
  const void* b;
  float* out;
  clite_conv cv;                 /* kind 0 */
  int32_t M, N, K, lda, ldb, ldc;  /* kind 1 */
  const float* a_scales;         /* ABI v12, kind 2 only: device f32 {scale, 1 / scale} of a (clite_bn.fp8_scale of the pass that wrote it) ... */
  const float* b_scales;         /* ... and of b; out += a_scales[1] * b_scales[1] * (a^T b) */
  const float* row_scale;        /* ABI v12. NULL, or device f32 [rows of out]: out[r][:] += row_scale[r] * (A^T B)[r][:] — the folded BatchNorm backward's
                                  * per-channel factor ka (clite_bn_fold_prepare) on a weight gradient contracted against dz instead of dy. Grouped
                                  * launches only: -1 where the members run one by one (f32, deterministic mode, no workspace). */
} clite_wgrad_item;
int clite_wgrad_group(int dtype, const clite_wgrad_item* items, int n, void* ws_dev, void* ws_host, uint64_t ws_bytes, void* stream);
int clite_wgrad_group_workspace(int n_items, int64_t total_workgroups, uint64_t* bytes);

/* Batched bf16 matrix transposes inside two flat buffers (the bf16 weight arena and its transposed twin): item i copies `batch` matrices
 * src[src_off + b*src_bstride + r*src_ld + c] -> dst[dst_off + b*dst_bstride + c*dst_ld + r], r < rows, c < cols (rows, cols, the strides
 * and offsets multiples of 8 elements). One launch for all items: workgroup w handles one 64 x 64 tile of the item with first_tile <= w <
 * first_tile + batch * ceil(rows/64) * ceil(cols/64); `items_dev` is a DEVICE array sorted by first_tile, total_tiles the sum. Linear weight
 * [N][K] -> [K][N]: rows N, cols K, batch 1. Conv weight [K][R][S][C] -> [C][R][S][K]: rows K, cols C, src_ld R*S*C, dst_ld R*S*K, batch R*S,
 * src_bstride C, dst_bstride K. (Reference: nothing — autograd's input gradients read the same weight tensor; this is a layout choice.) */
typedef struct clite_transpose_item {
  uint64_t src_off, dst_off;
  uint32_t rows, cols, src_ld, dst_ld, batch, src_bstride, dst_bstride, first_tile;
} clite_transpose_item;
int clite_transpose_weights(const void* src, void* dst, const clite_transpose_item* items_dev, int n_items, uint32_t total_tiles, void* stream);

/* ---- OCP e4m3 forward path (BASELINE.json configs[4]; the reference has no fp8 code — the policy is this library's).
 * Per-tensor current scaling: amax = max|x| (ZERO on entry), scale = 448 / amax, q = e4m3(clamp(x * scale, +-448)) rounded to nearest even;
 * scales (device f32[2]) <- {scale, 1 / scale}. n % 8 == 0. dtype of x: CLITE_BF16 or CLITE_F32. */
int clite_fp8_quantize(int dtype, const void* x, uint64_t n, float* amax, float* scales, void* out_fp8, void* stream);
/* C[M,N] = (A8[M,K] * B8[N,K]^T) * a_scales[1] * b_scales[1] through the fused epilogue (bf16 / f32 output; no split-K, no BatchNorm-backward
 * form): nn.Linear forward on e4m3 operands, v_mfma_f32_32x32x16_fp8_fp8 with f32 accumulation. K, lda, ldb multiples of 16. */
int clite_gemm_nt_fp8(const void* A8, int lda, const void* B8, int ldb, int M, int N, int K, const float* a_scales, const float* b_scales,
                      const clite_epilogue* ep, void* stream);
/* y = conv(x8, w8) * x_scales[1] * w_scales[1]: clite_conv_fwd on e4m3 operands (x8 [N][H][W][C], w8 [K][R][S][C]); C % 16 == 0, and
 * C % 64 == 0 for windowed convs. */
int clite_conv_fwd_fp8(const void* x8, const void* w8, const clite_conv* cv, const float* x_scales, const float* w_scales,
                       const clite_epilogue* ep, void* stream);
/* ABI v11. Input gradient of a stride-1 convolution on fp8 operands, in the one form the bf16 ResNet backward issues for a unit inside a block:
 * dx [N][H][W][C] bf16 = relu'(ep->relu_bits) * (dy (*) w), with the two BatchNorm-backward reductions (ep->bn_y, ep->bn_stats, ep->colsum) - every
 * other clite_epilogue feature is refused. dy8: [N][Ho][Wo][K] OCP e5m2 (written by clite_bn_bwd_apply's producer-fused quantiser: clite_bn.fp8_*
 * of that call; gradients get e5m2's range), wt8: the TRANSPOSED weights [C][R][S][K] in OCP e4m3; dy_scales / w_scales: device f32 {scale, 1 / scale}.
 * K % 64 == 0, C % 8 == 0. v_mfma_scale_f32_32x32x64_f8f6f4 (A e5m2, B e4m3) at unit block scales, f32 accumulate. */
int clite_conv_dgrad_fp8(const void* dy8, const void* wt8, const clite_conv* cv, const float* dy_scales, const float* w_scales,
                         const clite_epilogue* ep, void* stream);
/* Delayed scaling, once per step over all producer-fused tensors: slot i of `amax` (clite_bn.fp8_amax; a = the maximum of its words) with
 * a != 0: scales[2i] = 448 / a, scales[2i + 1] = a / 448 (both NaN when a is not finite); the slot is zeroed. A slot that stayed 0 keeps
 * its scales. */
#define CLITE_FP8_AMAX_REPLICAS 16
#define CLITE_FP8_AMAX_STRIDE 32
int clite_fp8_scale_update(float* amax, float* scales, int n, void* stream);
/* Per-tensor CURRENT scaling of many tensors of one arena in two launches (the conv weights after the optimizer update): item i is the
 * `numel` (% 8 == 0) elements at element offset `offset` (% 8 == 0) of `base`; its e4m3 copy goes to q_base + offset, its scales to
 * scales[2i..2i+1], its amax to amax[i]. wg_table_dev[w] = (item << 12 | chunk): workgroup w handles elements [chunk * 8192, (chunk + 1) * 8192)
 * of its item (chunk < 4096, i.e. tensors up to 32 M elements; items < 2^20), an item's chunks CONSECUTIVE and ascending in the table;
 * `partial` is n_wgs words of scratch. No atomics, nothing to zero: the result is a pure function of the arena. bf16 only. */
typedef struct clite_fp8_item {
  uint64_t offset, numel;
} clite_fp8_item;
int clite_fp8_quantize_group(const void* base, const clite_fp8_item* items_dev, const uint32_t* wg_table_dev, int n_items, int n_wgs,
                             uint32_t* partial, float* amax, float* scales, void* q_base, void* stream);

/* ResNet stem conv1 = nn.Conv2d(3, 64, 7, stride 2, padding 3, bias=False) (torchvision, reference encoder.py:36-38) on the
 * pre-padded NHWC4 image from clite_image_to_nhwc4 (Hp >= 2*(Ho-1)+7, Wp >= 2*(Wo-1)+8, Wp even). wv is the weight packed
 * as [64][7][8][4] (clite_stem_pack from f32 [64][7][7][3]); clite_stem_unpack_grad folds the packed gradient back (+=). */
int clite_stem_fwd(const void* xpad, const void* wv, int dtype, int N, int Hp, int Wp, int Ho, int Wo, const clite_epilogue* ep, void* stream);
int clite_stem_wgrad(const void* dy, const void* xpad, int dtype, int N, int Hp, int Wp, int Ho, int Wo, float* dwv, void* stream);
/* ABI v11. The same weight gradient on a patch-resident kernel (bf16, Wo % 16 == 0, Wo <= 128, Wp <= 254): dw f32 [64][7][7][3] += directly (no
 * packed intermediate), through clite_conv_wgrad_patch_workspace() bytes of scratch. Returns 1 (nothing launched) when the problem is not covered -
 * the caller then takes clite_stem_wgrad + clite_stem_unpack_grad - or in the deterministic mode / under a forced tile policy. */
int clite_stem_wgrad_patch(const void* dy, const void* xpad, int dtype, int N, int Hp, int Wp, int Ho, int Wo, float* dw, void* ws, uint64_t ws_bytes,
                           void* stream);
int clite_stem_pack(const float* w, void* wv, int dtype, void* stream);
int clite_stem_unpack_grad(const float* dwv, float* dw, void* stream);

/* ---- BatchNorm2d / BatchNorm1d, train-mode batch statistics (torchvision ResNet BN behind reference
 * encoder.py:36-65; nn.BatchNorm1d at loss.py:18). Tensors are [M][C] (NHWC flattened), C % 8 == 0, C/8 divides 256.
 * `stats` = per-channel (sum, sum of squares) [2][C] f32 over the M rows, produced by the conv/GEMM epilogue
 * (clite_epilogue.colsum). Biased variance normalises; unbiased variance goes into running_var. */
typedef struct clite_bn {
  int32_t M, C;
  const float* stats;        /* [2][C], or [3][C] when centered = 1 */
  const float* gamma;        /* [C] */
  const float* beta;         /* [C] */
  float* running_mean;       /* [C] */
  float* running_var;        /* [C] */
  int32_t training;          /* 1: batch statistics; 0: running statistics (eval) */
  int32_t update_running;    /* 1: workgroup 0 updates running_* with `momentum` */
  float momentum, eps;
  int32_t relu;              /* apply ReLU at the end */
  int32_t replicas;          /* R >= 1: `stats` (and res_stats) are R partial accumulators `rstride` elements apart; readers sum them */
  int32_t rstride;
  int32_t centered;          /* 1: variance = stats[2][c] / M (two-pass, from clite_bn_centered_var) instead of E[x^2]-E[x]^2 */
  /* optional second BN applied to the residual operand (the 1x1/stride downsample branch of a block) */
  const float* res_stats;
  const float* res_gamma;
  const float* res_beta;
  float* res_running_mean;
  float* res_running_var;
  uint8_t* relu_bits;        /* clite_bn_apply with relu = 1: optional [M][C / 8] bytes, bit e of byte (m * C + c) / 8 = (out[m][c + e] > 0): the
                              * ReLU mask the backward pass needs, at 1/16 of the bytes of re-reading `out` for its sign. NULL: not written. */
  /* clite_bn_apply (e4m3) and, ABI v11, clite_bn_bwd_apply (the same three fields, OCP e5m2 codes of dy for clite_conv_dgrad_fp8: clamp at +-57344, the
   * scale still maps the recorded amax to 448, i.e. 128 x headroom for a gradient that grew since); bf16; any of the three may be NULL:
   *   fp8_out   [M][C] e4m3 copy of `out` for the convs that read it: q = e4m3(clamp(out * fp8_scale[0], +-448)) of the value as stored,
   *             written by the same pass — half a write instead of clite_fp8_quantize's two reads and half a write;
   *   fp8_scale device f32[2] = {scale, 1 / scale}: DELAYED scaling, made from an earlier step's amax (clite_fp8_scale_update);
   *   fp8_amax  one amax SLOT = device f32[CLITE_FP8_AMAX_REPLICAS * CLITE_FP8_AMAX_STRIDE]: max |out| of THIS call folded in by integer
   *             atomic maxima on the bit pattern, workgroup b into word (b % REPLICAS) * STRIDE — same-address atomics retire at ~90 per
   *             microsecond chip-wide, a thousand workgroups on one word cost more than the pass over a small tensor; the slot's value is
   *             the maximum of its words (clite_fp8_scale_update folds and zeroes them). A NaN anywhere makes it the quiet-NaN pattern,
   *             an infinity +inf: both give NaN scales, as clite_fp8_quantize does. */
  uint8_t* fp8_out;
  const float* fp8_scale;
  float* fp8_amax;
  /* ABI v12, clite_bn_apply only (bf16, without the fp8 fields): out_sum[(b % out_sum_replicas) * out_sum_stride + c] += sum over workgroup b's rows of
   * out[m][c] as stored — the column sums of the activation that the folded BatchNorm backward's weight gradient needs (clite_bn_fold_wgrad_finish),
   * taken by the pass that writes it instead of a pass of their own. ZERO on entry. NULL: not accumulated. */
  float* out_sum;
  int32_t out_sum_replicas;
  int32_t out_sum_stride;
} clite_bn;

/* Second pass of a two-pass variance (used by the exact-f32 parity mode): stats[2][c] += sum_m (y[m][c] - stats[0][c]/M)^2;
 * stats[2][*] must be zero on entry. */
int clite_bn_centered_var(int dtype, const void* y, float* stats, int replicas, int rstride, int M, int C, void* stream);
/* out = relu?( bn(y) + [res | bn_res(res)] ) */
int clite_bn_apply(const clite_bn* p, int dtype, const void* y, const void* res, void* out, void* stream);
/* dstats[0][c] += sum dz, dstats[1][c] += sum dz*(y - mean_c), dz = dout * (mask > 0) (mask NULL: dz = dout), mean_c = stats[0][c]/M.
 * The mask is either a tensor of the call's dtype (`mask`) or packed bits as clite_bn.relu_bits writes them (`mask_bits`); at most one of
 * the two. dstats pre-zeroed. */
int clite_bn_bwd_reduce(int dtype, const void* dout, const void* mask, const uint8_t* mask_bits, const void* y, const float* stats, float* dstats,
                        int replicas, int rstride, int M, int C, void* stream);   /* stats and dstats are both replicated (R, rstride) */
/* dy = BN backward of dz through batch statistics; dz (optional) <- masked dout; dgamma/dbeta (optional) += . */
int clite_bn_bwd_apply(const clite_bn* p, int dtype, const void* dout, const void* mask, const uint8_t* mask_bits, const void* y, const float* dstats,
                       void* dy, void* dz, float* dgamma, float* dbeta, void* stream);

/* ---- ABI v12: the block-output BatchNorm backward FOLDED into its consumers (bf16; reference model_zoo/resnet.py:60-100 block arithmetic, autograd of
 * encoder.py:63's torchvision Bottleneck: bn3 backward -> conv3 input gradient + conv3 weight gradient). BatchNorm backward is linear in dz:
 *     dy = ka . dz + kb + kc . (y - mean),   ka = gamma rstd,  kb = -ka S1 / M,  kc = -ka rstd^2 S2 / M     (per channel k; S1 = sum dz, S2 = sum dz (y - mean))
 * so for the 1 x 1 convolution y = a W^T (W [K][Cin]) that produced y
 *     da = dy W          = [dz | y] [diag(ka) W ; diag(kc) W] + (kb - kc . mean) W       one GEMM over the K-concatenation of dz and y, a bias row
 *     dW = dy^T a        = diag(ka) (dz^T a) + kb (x) colsum(a) + diag(kc) W Cov(a),     Cov(a) = a^T a - colsum(a) colsum(a)^T / M   (y = a W^T, mean = colsum(a) W^T / M)
 * and the apply pass (read dz, read y, write dy) with its dy tensor disappears: the dgrad reads dz and y instead of dy, the weight gradient reads dz instead of dy.
 *
 * clite_bn_fold_prepare: from the BatchNorm's forward sums `p->stats`, its two backward reductions `dstats` (same replica layout) and the TRANSPOSED bf16
 * weights wt [Cin][K] (K = p->C) makes, in one launch of Cin workgroups:
 *   w2   bf16 [Cin][2][K]   w2[c][0][k] = bf16(kc[k] wt[c][k]) (multiplies y), w2[c][1][k] = bf16(ka[k] wt[c][k]) (multiplies dz): clite_conv_dgrad_bnfold's weights
 *   bias f32  [Cin]         sum_k kb[k] wt[c][k] - sum_k mean[k] w2[c][0][k]   (with the ROUNDED w2: sum_k (y - mean) w2 then cancels exactly as in y - mean)
 *   coef f32  [3][K]        ka, kb, kc
 *   dgamma[k] += rstd S2, dbeta[k] += S1 (either may be NULL). */
int clite_bn_fold_prepare(const clite_bn* p, const float* dstats, const void* wt, int Cin, void* w2, float* bias, float* coef, float* dgamma, float* dbeta,
                          void* stream);
/* da [M][Cin] = [pair[0] | pair[1]] [w2[:, 1, :] | w2[:, 0, :]]^T + ep->bias through the BatchNorm-backward form of the epilogue (relu_bits + bn_y + colsum:
 * the NEXT BatchNorm backward's mask and reductions), i.e. what clite_bn_bwd_apply followed by clite_conv_dgrad_wt computes. pair = bf16 [2][M][K]: slot 0 the
 * masked gradient dz, slot 1 the BatchNorm input y (the producer of each writes it there). K % 64 == 0, Cin % 8 == 0, 2 M K < 2^31. */
int clite_conv_dgrad_bnfold(const void* pair, const void* w2, int M, int K, int Cin, const clite_epilogue* ep, void* stream);
/* Weight-gradient side: the two correction terms, in f32, with G = a^T a (f32 [Cin][Cin], left by a member of the grouped launch) and the column sums
 * s[c] = sum_r asum[r * asum_stride + c] (clite_bn.out_sum of the clite_bn_apply that wrote a):
 *   dw[k][c] += kb[k] s[c] + kc[k] sum_c' wt[c'][k] (G[c'][c] - s[c'] s[c] / M)                  (float atomics: the member that accumulates ka (dz^T a) may run beside it)
 * The rank-1 term cancels against ka (dz^T a) wherever dz has a mean: nothing here is rounded to bf16. */
int clite_bn_fold_wgrad_finish(const float* G, const float* asum, int asum_replicas, int asum_stride, const float* coef, const void* wt, int M, int K, int Cin,
                               float* dw, void* stream);


/* ---- ABI v12: the MI projection block of the loss heads (reference loss.py:12-40: LayerNorm(W2 relu(BatchNorm1d(W1 x)) + b2 + Ws x + bs)): everything
 * around its six small GEMMs in four kernels, bf16, M <= 128 rows (clip-lite_amd/csrc/heads_fused.hip). The GEMMs stay clite_gemm_nt launches that
 * ACCUMULATE (ep.atomic, f32) into zeroed workspaces; what the step pays for between the encoders' forward and backward is dependent launches, and these
 * four replace fifteen of them:
 *   clite_mi_block_fwd1  sc = f32 [M][2 U] with columns [0, U) = x W1^T and [U, 2 U) = x Ws^T. Per 32-column slab: z <- bf16(sc[:, :U]); stats <- {sum z,
 *                        sum z^2, 0} of the stored values (one replica); the running statistics updated `updates` times (the reference runs the block twice per
 *                        step on the same statistics); a <- relu(bn(z)) with the batch statistics.
 *   clite_mi_block_fwd2  dxs = f32 [M][U] = a W2^T. Per row: t <- bf16(dxs + b2 + sc[:, U:] + bs); out <- LayerNorm(t) (ln_gamma, ln_beta, ln_eps); ln_stats
 *                        <- {mean, rstd} per row (clite_layernorm_bwd's layout).
 *   clite_mi_block_bwd1  dxs = f32 [M][Fin + U] with columns [Fin, Fin + U) = dtt W2 (and [0, Fin) = dtt Ws). Per 32-column slab: da masked by a > 0,
 *                        BatchNorm1d backward -> dz (bf16); dgamma, dbeta +=; db2, dbs += colsum(dtt).
 *   clite_mi_block_bwd2  after dz W1 has been accumulated onto columns [0, Fin): dx <- bf16(dxs[:, :Fin] + dres).
 * Fin % 16 == 0, U % 16 == 0, U <= 4096. -1 for M > 128 or a missing operand (the caller then takes the generic kernels). */
typedef struct clite_mi_block {
  int32_t M, Fin, U, updates;
  float momentum, eps, ln_eps;
  int32_t reserved;
  const float* bs;          /* f32 [U] or NULL (feature_shortcut.bias) */
  const float* b2;          /* f32 [U] or NULL */
  const float* gamma;       /* BatchNorm1d weight / bias, running statistics (updated in place) */
  const float* beta;
  float* running_mean;
  float* running_var;
  void* z;                  /* bf16 [M][U]  pre-BatchNorm, kept for backward */
  void* a;                  /* bf16 [M][U]  relu(bn(z)) */
  float* stats;             /* f32 [3][U] */
  float* sc;                /* f32 [M][2 U] workspace of the first two products */
  void* t;                  /* bf16 [M][U] */
  void* out;                /* bf16 [M][U] */
  const float* ln_gamma;
  const float* ln_beta;
  float* ln_stats;          /* f32 [M][2] */
  const void* dtt;          /* bf16 [M][U] */
  void* dz;                 /* bf16 [M][U] */
  float* dxs;               /* forward: f32 [M][U] = a W2^T; backward: f32 [M][Fin + U] */
  const void* dres;         /* bf16 [M][Fin] or NULL: added to dx (the prior discriminator's gradient w.r.t. the same features) */
  void* dx;                 /* bf16 [M][Fin] */
  float* dgamma;            /* f32 [U], +=; any of the four may be NULL */
  float* dbeta;
  float* db2;
  float* dbs;
} clite_mi_block;
int clite_mi_block_fwd1(const clite_mi_block* p, void* stream);
int clite_mi_block_fwd2(const clite_mi_block* p, void* stream);
int clite_mi_block_bwd1(const clite_mi_block* p, void* stream);
int clite_mi_block_bwd2(const clite_mi_block* p, void* stream);

/* nn.MaxPool2d(3, stride 2, padding 1) of the ResNet stem; idx holds the window position (0..8) of the first maximum. */
int clite_maxpool3x3s2_fwd(int dtype, const void* x, void* out, uint8_t* idx, int N, int H, int W, int C, void* stream);
int clite_maxpool3x3s2_bwd(int dtype, const void* dout, const uint8_t* idx, void* dx, int N, int H, int W, int C, void* stream);
/* The stem's BatchNorm + ReLU + max-pool in one pass each way (torchvision ResNet conv1 -> bn1 -> relu -> maxpool, reference encoder.py:36-38):
 * pooled / idx = clite_maxpool3x3s2_fwd(clite_bn_apply(y)) without the post-BN tensor ever being stored (p->M = N*H*W, p->relu ignored: ReLU is
 * part of the stem; running statistics updated as in clite_bn_apply); and dy = clite_bn_bwd_apply(clite_bn_bwd_reduce(clite_maxpool3x3s2_bwd(dpool)
 * masked by relu'(bn(y)))) with neither the un-pooled gradient nor the mask stored: dstats (replicated like p->stats, ZERO on entry) receives the
 * two reductions, dgamma / dbeta (optional) +=. Bit-identical to the unfused sequence. */
int clite_stem_bn_pool_fwd(const clite_bn* p, int dtype, const void* y, void* pooled, uint8_t* idx, int N, int H, int W, void* stream);
int clite_stem_bn_pool_bwd(const clite_bn* p, int dtype, const void* dpool, const uint8_t* idx, const void* y, float* dstats, void* dy,
                           float* dgamma, float* dbeta, int N, int H, int W, void* stream);
/* ABI v11. The forward pass that also leaves what the backward reductions of this BatchNorm need in POOLED size: ymax [N][Ho][Wo][C] (optional) = the
 * BatchNorm input y at each window's argmax (an exact copy), and p->relu_bits (optional) = the packed relu' bits of the pooled output. Every other
 * position of a window receives no gradient, so sum dz and sum dz (y - mean) over the un-pooled tensor equal the same sums over (pooled gradient *
 * relu', ymax): the kernel that writes the pooled gradient accumulates them in its epilogue (clite_epilogue.bn_y = ymax, relu_bits,
 * mask_after_residual, colsum; bn_inv_count = 1 / (N H W) of the UN-pooled tensor) and clite_stem_bn_pool_bwd_apply takes them as `dstats` -
 * clite_stem_bn_pool_bwd's second half alone, without the pass over y (205 MB at batch 128) that produced them. (The sums skip one rounding of the
 * unfused sequence - the un-pooled gradient of a pixel that is the argmax of several windows was rounded to the storage type before it was summed.) */
int clite_stem_bn_pool_fwd_ex(const clite_bn* p, int dtype, const void* y, void* pooled, uint8_t* idx, void* ymax, int N, int H, int W, void* stream);
int clite_stem_bn_pool_bwd_apply(const clite_bn* p, int dtype, const void* dpool, const uint8_t* idx, const void* y, const float* dstats, void* dy,
                                 float* dgamma, float* dbeta, int N, int H, int W, void* stream);
/* nn.AdaptiveAvgPool2d((1,1)) + view (reference encoder.py:63-65): [N][HW][C] -> [N][C] */
int clite_avgpool_fwd(int dtype, const void* x, void* out, int N, int HW, int C, void* stream);
int clite_avgpool_bwd(int dtype, const void* dout, void* dx, int N, int HW, int C, void* stream);
/* batch["image"] f32 NCHW [N][3][H][W] -> zero-padded NHWC4 [N][Hp][Wp][4] (the layout the 7x7 stem conv gathers from) */
int clite_image_to_nhwc4(int dtype, const float* img, void* out, int N, int H, int W, int pad, int Hp, int Wp, void* stream);
/* out[n] += sum_m x[m][n]  — bias gradients */
int clite_colsum(int dtype, const void* x, float* out, int M, int N, void* stream);

/* ---- BERT text encoder pieces outside the GEMMs (transformers.BertModel behind reference encoder.py:165-196).
 * Dropout masks are a pure function of (seed, site, element index) so backward regenerates them (csrc/rng.h). */
/* out = dropout(LayerNorm(x)); stats[row] = (mean, rstd) f32. C % 8 == 0, C <= 2048. Also nn.LayerNorm at loss.py:23. */
int clite_layernorm_fwd(int dtype, const void* x, const float* gamma, const float* beta, float eps, void* out, float* stats,
                        int M, int C, float drop_p, uint64_t drop_seed, uint32_t drop_site, void* stream);
/* ABI v11. The same pass (bf16 only) that also leaves the e4m3 copy of `out` for the fp8 linears that read it (BERT's QKV projection and FFN1)
 * and / or records max |out|: fp8_out / fp8_scale / fp8_amax as in clite_epilogue (delayed scaling; any may be NULL, fp8_out needs fp8_scale). */
int clite_layernorm_fwd_q8(int dtype, const void* x, const float* gamma, const float* beta, float eps, void* out, float* stats,
                           int M, int C, float drop_p, uint64_t drop_seed, uint32_t drop_site, uint8_t* fp8_out, const float* fp8_scale, float* fp8_amax,
                           void* stream);
/* dx = LayerNorm backward of dropout_in(dy); dx_masked (optional) = dropout_out(dx); dgamma/dbeta (optional) += .
 * dcolsum (optional, f32 [C]) += column sums of dx_masked (of dx when there is no masked output) as stored: the bias gradient of the
 * nn.Linear whose output this LayerNorm normalised (BertSelfOutput.dense / BertOutput.dense; the token-type row of BertEmbeddings). */
int clite_layernorm_bwd(int dtype, const void* dy, const void* x, const float* stats, const float* gamma, void* dx, void* dx_masked,
                        float* dgamma, float* dbeta, float* dcolsum, int M, int C, float in_p, uint64_t in_seed, uint32_t in_site,
                        float out_p, uint64_t out_seed, uint32_t out_site, void* stream);
/* BertEmbeddings sum: out[row] = word[ids[row]] + pos[row % L] + type[0] (token_type_ids = 0, position_ids = arange(L)) */
int clite_embed_fwd(int dtype, const int64_t* ids, const void* word, const void* pos, const void* type, void* out,
                    int M, int L, int C, int vocab, void* stream);
/* dword[ids[row]] += d[row] (float atomics) for ids[row] != padding_idx; dpos[l] += sum_b d[b*L+l]. Either may be NULL.
 * padding_idx: the row nn.Embedding(padding_idx=...) never accumulates a gradient into (HF BertEmbeddings.word_embeddings: pad_token_id = 0,
 * behind reference encoder.py:163-170); -1 = none. */
int clite_embed_bwd(int dtype, const int64_t* ids, const void* d, float* dword, float* dpos, int M, int L, int C, int vocab, int padding_idx,
                    void* stream);
/* BertSelfAttention core for L <= 128, head size 64: qkv [B*L][3*H*64] (q|k|v), mask int64 [B][L] (1 = attend) or NULL,
 * ctx [B*L][H*64] = dropout(softmax(q k^T / 8 + (1-mask)*finfo.min)) v. L <= 32: one wave per (batch, head) on one 32 x 32 score tile;
 * 33 <= L <= 128: one workgroup per (batch, head), a wave per 32-query tile over up to four key tiles (whole score row in registers, two-pass
 * softmax, no atomics: bit-exact reruns). L > 128 returns -1. The dropout multiplier of p[i][j] comes from element index ((bh*32 + i)*32 + j)
 * for L <= 32 and ((bh*128 + i)*128 + j) above; backward recomputes the probabilities and the mask from qkv and the same (seed, site). */
int clite_attention_fwd(int dtype, const void* qkv, const int64_t* mask, void* ctx, int B, int L, int H,
                        float drop_p, uint64_t drop_seed, uint32_t drop_site, void* stream);
int clite_attention_bwd(int dtype, const void* qkv, const int64_t* mask, const void* dctx, void* dqkv, int B, int L, int H,
                        float drop_p, uint64_t drop_seed, uint32_t drop_site, void* stream);

/* ---- MPNet (transformers.MPNetModel) variants of the kernels above; the entry points above are unchanged.
 * Attention with the relative-position bias: bias f32 [H][32][32] (clite_attention_bias_build) is added to q k^T / 8 before the mask.
 * The backward also writes dbias_partials f32 [B*H][32]: the sums of the (batch, head)'s f32 dS tile over the (i, j) of each bucket, with
 * bucket_table int32 [63] = bucket of the relative offsets j - i = -31 .. 31 (host-computed, values 0 .. 31). No float atomics: bit-identical runs. */
int clite_attention_bias_fwd(int dtype, const void* qkv, const int64_t* mask, const float* bias, void* ctx, int B, int L, int H,
                             float drop_p, uint64_t drop_seed, uint32_t drop_site, void* stream);
int clite_attention_bias_bwd(int dtype, const void* qkv, const int64_t* mask, const float* bias, const int32_t* bucket_table, const void* dctx,
                             void* dqkv, float* dbias_partials, int B, int L, int H, float drop_p, uint64_t drop_seed, uint32_t drop_site,
                             void* stream);
/* bias[h][i][j] = rel_weight[bucket_table[j - i + 31]][h] for i, j < L (0 elsewhere); rel_weight f32 [32][H] */
int clite_attention_bias_build(const float* rel_weight, const int32_t* bucket_table, float* bias, int H, int L, void* stream);
/* drel[k][h] += sum_r partials[r][h][k], r < rows (= layers x B slices of clite_attention_bias_bwd's output); fixed summation order */
int clite_attention_bias_grad_reduce(const float* partials, float* drel, int rows, int H, void* stream);
/* MPNetEmbeddings sum: out[row] = word[ids[row]] + pos[pid], pid = padding_idx + (ids[row] != padding_idx ? number of ids != padding_idx among the
 * caption's first l + 1 : 0), computed in the kernel (L <= 32); pids int32 [M] (may be NULL) receives pid for the backward */
int clite_embed_mpnet_fwd(int dtype, const int64_t* ids, const void* word, const void* pos, void* out, int32_t* pids, int M, int L, int C,
                          int vocab, int max_pos, int padding_idx, void* stream);
/* dword[ids[row]] += d[row] for ids[row] != padding_idx; dpos[pids[row]] += d[row] for pids[row] != padding_idx. Either may be NULL. */
int clite_embed_mpnet_bwd(int dtype, const int64_t* ids, const int32_t* pids, const void* d, float* dword, float* dpos, int M, int L, int C,
                          int vocab, int max_pos, int padding_idx, void* stream);
/* Masked mean over tokens: out[b] = sum_l h[b][l] mask[b][l] / max(sum_l mask[b][l], 1e-9), inv[b] = 1 / that denominator; h [B][L][C], C % 8 == 0.
 * Backward: dh[b][l] = mask[b][l] inv[b] dy[b] for every token. */
int clite_mean_pool_fwd(int dtype, const void* h, const int64_t* mask, void* out, float* inv, int B, int L, int C, void* stream);
int clite_mean_pool_bwd(int dtype, const void* dy, const int64_t* mask, const float* inv, void* dh, int B, int L, int C, void* stream);

/* ---- CLIP text transformer (open_clip TextTransformer; clip_lite_amd/cliptext.py). Additive to ABI v12; the entry points above are unchanged and
 * launch what they launched.
 * Causal self-attention: layouts, head size (64) and scaling (/ 8) of clite_attention_fwd; query i sees key j iff j <= i and (mask == NULL or
 * mask[b][j] == 1). A key behind the diagonal takes no part in the softmax (its score is -inf, its probability an exact 0); a masked key in
 * front of it gets clite_attention_fwd's additive finfo.min. PRECONDITION: mask[b][0] == 1 for every sample (every caption has a first token),
 * so that no query's row is empty; with mask[b][0] == 0 the leading masked keys share the row's weight uniformly, as a fully masked row does
 * in clite_attention_fwd. No dropout (the tower has none). L <= 32: the one-tile kernels with the test on the tile; 33 <= L <= 128: one workgroup per
 * (batch, head), a wave per 32-query tile; in bf16 wave w forms only the key tiles 0..w (the products above the diagonal are not computed),
 * dQ of query tile w sums the key tiles 0..w and dK / dV of key tile w the query tiles w..NT-1 in ascending order. No float atomics, every
 * output element written once in a fixed order: the same bits on every run in both settings of clite_set_deterministic. Returns -1 and
 * launches nothing for L > 128, L < 1, a NULL qkv / ctx / dctx / dqkv or an unknown dtype. */
int clite_attention_causal_fwd(int dtype, const void* qkv, const int64_t* mask, void* ctx, int B, int L, int H, void* stream);
int clite_attention_causal_bwd(int dtype, const void* qkv, const int64_t* mask, const void* dctx, void* dqkv, int B, int L, int H, void* stream);
/* Token assembly: out[row] = word[ids[row]] + pos[row % L] (no token types, no LayerNorm); ids clamped into [0, vocab). M = B L rows, C % 8 == 0.
 * The sum is formed in f32 and rounded once. Backward: clite_embed_bwd with padding_idx = -1 (nn.Embedding without a padding row, as in CLIP). */
int clite_embed_clip_fwd(int dtype, const int64_t* ids, const void* word, const void* pos, void* out, int M, int L, int C, int vocab, void* stream);
/* End-of-text pooling by the mask: idx[b] = (number of nonzero mask[b][l]) - 1 (0 for an all-zero mask), out[b] = x[b][idx[b]] of x [B * L][C].
 * Backward: dx[b][idx[b]] = d[b], the other rows of dx left as they are (the caller zeroes them). Exact copies; C % 8 == 0. */
int clite_last_token_gather(int dtype, const void* x, const int64_t* mask, void* out, int32_t* idx, int B, int L, int C, void* stream);
int clite_last_token_scatter(int dtype, const void* d, const int32_t* idx, void* dx, int B, int L, int C, void* stream);

/* BertPooler tanh backward: out = dy * (1 - y^2), n % 8 == 0 */
int clite_tanh_bwd(int dtype, const void* dy, const void* y, void* out, uint64_t n, void* stream);

/* ---- JSD mutual-information loss (reference loss.py). f1 = img_block(image_features), f2 = text_block(text_features),
 * both [B][D], D % 8 == 0, D <= 2048. neg = NULL: negatives are roll-by-one inside the batch, pair (n, n+1 mod B) (loss.py:214-216);
 * otherwise neg[n] (int32, a permutation of 0..B-1) is the row of f2 paired with row n — the cluster hard-negative branch (loss.py:225-252)
 * stacks [batch; hard negatives] and pairs [B/2 + i | (i+1) mod B/2].
 * work: f32 [B][8] per-sample scratch kept for backward. acc: f32 [2] of the step's 8 pre-zeroed accumulators
 * (clite_loss_finalize): acc[0] += mean softplus(-o+) (= -Ej), acc[1] += mean softplus(o-) (= Em). */
int clite_critic_jsd_fwd(int dtype, const void* f1, const void* f2, const float* temperature, int B, int D, const int32_t* neg, float* work,
                         float* acc, void* stream);
/* out[n] = x[n] / max(||x[n]||_2, 1e-12): F.normalize(p=2, dim=-1) of the embedding-extraction / retrieval path that consumes the trained
 * projection heads (reference retrieval.py:108,127; zero_shot.py). [B][D], D % 8 == 0, D <= 2048. */
int clite_l2_normalize(int dtype, const void* x, void* out, int B, int D, void* stream);
int clite_l2_normalize_bwd(int dtype, const void* x, const void* y, const void* dy, void* dx, int B, int D, void* stream);
/* InfoNCE all-pairs variant of the cross-modal term (BASELINE config 4 / SURVEY §8f N4; the reference has no such code): symmetric
 * cross-entropy with diagonal targets over S = exp(temperature) * C, C f32 [B][ld] the cosines of the L2-normalised projections
 * (one clite_gemm_nt). lse_r / lse_c: f32 [B] kept for backward; acc[0] += mean_i(lse_r - S_ii)/2, acc[1] += mean_j(lse_c - S_jj)/2
 * (same slots as the JSD terms, so clite_loss_finalize is shared). */
int clite_infonce_fwd(const float* C, int ld, int B, const float* temperature, float* lse_r, float* lse_c, float* acc, void* stream);
/* dC (call dtype, [B][ldd], ldd % 8 == 0, padding columns zeroed) = dL/dC; dtemp (f32 scalar) += ; scale = (1 - prior_weight). */
int clite_infonce_bwd(int dtype, const float* C, int ld, int B, const float* temperature, const float* lse_r, const float* lse_c,
                      const float* gout, float scale, void* dC, int ldd, float* dtemp, void* stream);
/* SigLIP pairwise sigmoid variant of the cross-modal term (Zhai et al. 2023, Algorithm 1; csrc/siglip_ops.hip) on the same C f32 [B][ld]
 * (columns >= B are padding and enter nothing): x_ij = exp(temperature) * C[i][j] + bias, z_ij = +1 on the diagonal and -1 off it,
 * acc[0] += 1/B sum_ij softplus(-z_ij x_ij); acc[1] is left alone (clite_loss_finalize is shared). Nothing is kept for backward.
 * part: caller-provided f32 scratch of at least 2 B floats. The row kernels store one partial per row there and a one-wave launch folds them in
 * a fixed order: no float atomics, the same bits in every run with or without the deterministic mode. */
int clite_siglip_fwd(const float* C, int ld, int B, const float* temperature, const float* bias, float* part, float* acc, void* stream);
/* dC (call dtype, [B][ldd], ldd % 8 == 0, padding columns zeroed) = dL/dC, recomputed from C; dtemp, dbias (f32 scalars, either may be NULL) += ;
 * scale = (1 - prior_weight). */
int clite_siglip_bwd(int dtype, const float* C, int ld, int B, const float* temperature, const float* bias, const float* gout, float scale,
                     void* dC, int ldd, float* part, float* dtemp, float* dbias, void* stream);
/* gout: device scalar dL/d(total); scale = (1 - prior_weight). df1/df2 in dtype; dtemp (f32 scalar) += . neg as in the forward call,
 * neg_inv its inverse permutation (both NULL = roll by one). */
int clite_critic_jsd_bwd(int dtype, const void* f1, const void* f2, const float* temperature, const float* work, const float* gout, float scale,
                         int B, int D, const int32_t* neg, const int32_t* neg_inv, void* df1, void* df2, float* dtemp, void* stream);
/* PriorDiscriminator.l2 + sigmoid + log terms (loss.py:49-53,189-193) on h1 = relu(l1(relu(l0([u; f])))) stacked [2B][K]:
 * acc += -(mean log D(u) + mean log(1 - D(f))), evaluated as the reference does (log of the f32 sigmoid) when softplus = 0. K % 8 == 0.
 * logit: f32 [2B] kept for backward. With softplus = 1 the same pair of calls is the tail of the `concat` critic GlobalDiscriminator
 * (loss.py:56-68,206-222): rows [0,B) = logits of the positive pairs, acc += mean softplus(-o) (= -Ej); rows [B,2B) = negative pairs,
 * acc += mean softplus(o) (= Em); K = 512. The two forms have the same derivative (clite_prior_tail_bwd). */
int clite_prior_tail_fwd(int dtype, const void* h1, const float* w2, const float* b2, int B, int K, int softplus, float* logit, float* acc,
                         void* stream);
/* dh1 = gradient w.r.t. l1's pre-activation (ReLU mask applied); dw2/db2 (f32) += ; scale = prior_weight. */
int clite_prior_tail_bwd(int dtype, const void* h1, const float* w2, const float* logit, const float* gout, float scale, int B, int K,
                         void* dh1, float* dw2, float* db2, void* stream);
/* acc: f32 [8] = [-Ej, Em | image prior, text prior | visual SSL -Ej, Em | textual SSL -Ej, Em] (loss.py:256-300 for the SSL terms).
 * out: f32 [8]: out[0] = (1-w)*(cross + visual + textual) + w*prior (loss.py:302-305), out[1] = cross = Em - Ej, out[2] = prior,
 * out[3] = visual, out[4] = textual, rest 0. */
int clite_loss_finalize(const float* acc, float prior_weight, float* out, void* stream);
/* out = a + b, n % 8 == 0 elements of `dtype`: feature gradients that arrive from several loss terms (cross-modal + SSL + prior). */
int clite_add(int dtype, const void* a, const void* b, void* out, uint64_t n, void* stream);
/* torch.rand_like replacement for the prior noise (loss.py:189,196): U[0,1) from Philox(seed, site, index). n % 8 == 0. */
int clite_uniform_fill(int dtype, void* out, uint64_t n, uint64_t seed, uint32_t site, void* stream);

/* ---- Downstream classification (reference linear_clf.py, zero_shot.py; clip-lite_amd/classify.py). One wave per row of f32 logits [B][ld]
 * (ld % 4 == 0, ld >= C, 16-byte aligned), C >= 1 real classes; labels int64 [B]. A label of -100 (torch's ignore_index) — or any value outside
 * [0, C) — adds nothing to the loss or the count.
 * lse (f32 [B]) = logsumexp over the C columns, kept for backward. acc (f32 [4], accumulated: zero it first, or keep adding across batches)
 * += { sum (lse - z_y), #[rank == 0], #[rank < topk], #counted rows } with rank = #{j: z_j > z_y} + #{j < y: z_j == z_y} (ties go to the lower index).
 * Replaces nn.CrossEntropyLoss at linear_clf.py:188, TopkAccuracy at utils/metrics.py:20-73 and torch.max at zero_shot.py:155.
 * Deterministic mode: one wave over all rows in order, one contribution per accumulator. */
int clite_xent_fwd(const float* logits, int ld, int B, int C, const int64_t* labels, int topk, float* lse, float* acc, void* stream);
/* dlogits (call dtype, [Bp][ldd], ldd % 8 == 0, ldd >= C, Bp >= B) = gout / acc[3] * (softmax(z_i) - onehot(y_i)) — the gradient of the mean over the
 * counted rows, autograd of linear_clf.py:188; zeros in columns >= C, rows >= B and ignored rows. gout (f32 scalar) and the count are read on the
 * device. A batch with no counted row gets a zero gradient. */
int clite_xent_bwd(int dtype, const float* logits, int ld, int B, int Bp, int C, const float* lse, const int64_t* labels, const float* acc,
                   const float* gout, void* dlogits, int ldd, void* stream);

/* ---- VOC07 SVM evaluation (reference voc_clf.py:75-121, train_test_single_svm; clip-lite_amd/svm.py). P independent problems
 *   min_w f_p(w) = 1/2 |w|^2 + sum_i c_ip max(0, 1 - y_ip w.x~_i)^2    (LinearSVC penalty="l2", loss="squared_hinge", intercept_scaling 1)
 * over one shared f32 matrix X~ [N][Dp] (rows: feature, 1, zeros), solved by batched Newton-CG: every CG iteration is clite_gemm_nt (X~ d^T) and
 * clite_gemm_tn (2 X~^T (h . q) + d) plus the kernels below. Column arrays (margins Z = X~ W^T, labels Y = +-1, weights Cw = c >= 0, gradient
 * operand S, Hessian diagonal H) are f32 [N][ldp], ldp % 8 == 0, ldp >= P; row arrays (W, the gradient G, the CG vectors X, R, D, HD) are
 * f32 [rows >= P][ld], Dp <= ld. Per-problem scalars stay on the device in `state`, f32 [P][CLITE_SVM_STATE], zero-initialised with the
 * active flag (column 9) set: 0 |grad f(0)|, 1 |grad f(w)|, 2 their ratio, 5 last step length, 6 Newton iterations, 8 CG iterations.
 * Every sum is formed in one fixed order (no atomics), so results are bitwise reproducible in either deterministic mode. */
#define CLITE_SVM_STATE 16
#define CLITE_SVM_AP_MAX_ROWS 8192
/* S = c 1_I (Z - Y), H = c 1_I with I = {Y Z < 1}; loss (f32 [P]) = sum_i c max(0, 1 - Y Z)^2, the data term of f_p. Columns in [P, ldp) of S and H
 * are written as zeros. work: f32 [ceil(N / 512)][ldp] scratch. Replaces the per-iteration loss / gradient of LinearSVC.fit (voc_clf.py:100-105). */
int clite_svm_margin(const float* Z, const float* Y, const float* Cw, int N, int P, int ldp, float* S, float* H, float* loss, float* work, void* stream);
/* Q *= H elementwise over n floats (n % 4 == 0, 16-byte aligned): the generalised Hessian's diagonal applied to X~ d (voc_clf.py:100-105). */
int clite_svm_hess_scale(const float* H, float* Q, uint64_t n, void* stream);
/* One workgroup per problem: |G_p|, the stopping test |G_p| <= tol |grad f_p(0)| or max_newton steps taken (the problem then freezes), and for a
 * problem that goes on the start of a CG solve of H x = -g: X = 0, R = D = -G, CG tolerance eta |g| with eta = min(eta_max, sqrt(|g| / |g0|)).
 * G = W + 2 X~^T S (clite_gemm_tn). voc_clf.py:100-105 (LinearSVC.fit). */
int clite_svm_newton_begin(const float* G, int ld, int Dp, int P, float* X, float* R, float* D, float* state, float tol, int max_newton, float eta_max,
                           void* stream);
/* One CG iteration for every problem whose solve is still open: alpha = r.r / d.HD, X += alpha D, R -= alpha HD, then stop when |R| <= the
 * tolerance or D = R + beta D. Problems that are frozen or done are left untouched. voc_clf.py:100-105 (LinearSVC.fit). */
int clite_svm_cg_update(const float* HD, int ld, int Dp, int P, float* X, float* R, float* D, float* state, void* stream);
/* Step length t_p >= 0 minimising f_p(W_p + t X_p) exactly on its piecewise quadratic (safeguarded Newton on f', starting from t = 1), from
 * Z = X~ W^T and delta = X~ X^T ([N][ldp]); then W_p += t_p X_p. Frozen problems take t = 0. voc_clf.py:100-105 (LinearSVC.fit). */
int clite_svm_line_search(const float* Z, const float* delta, const float* Y, const float* Cw, int N, int P, int ldp, float* W, const float* X, int ld,
                          int Dp, float* state, void* stream);
/* ap[p] (f32 [P]) = sklearn.metrics.average_precision_score(targets[:, p] > 0, scores[:, p]) over the rows with targets[i][p] >= 0 (a negative
 * target is "ignore"): tied scores form one threshold, AP = sum_n (R_n - R_n-1) P_n; 0 for a column without positives. scores [N][lds], targets
 * [N][ldt]. One workgroup sorts a column in LDS: N <= CLITE_SVM_AP_MAX_ROWS, else returns -2. Replaces cross_val_score(scoring=
 * "average_precision") and average_precision_score at voc_clf.py:96-98,121. */
int clite_average_precision(const float* scores, int lds, const float* targets, int ldt, int N, int P, float* ap, void* stream);

/* ---- Image-text retrieval ranks (reference retrieval.py:150-207, itm_eval; clip-lite_amd/retrieval.py gpu_ranks). sims: f32 [Ni][ld], ld >= Nt,
 * of which only columns [0, Nt) are read (similarity() pads the text count to a multiple of 8 with zero columns). The rank of an entry is its
 * 0-based position when its row (i2t) or column (t2i) is sorted by score, highest first, ties to the lower index: np.argsort(-s, kind="stable")
 * order, 0.0 == -0.0 a tie. Neither direction sorts: each is one counting pass over Ni x Nt x 4 bytes, with integer counts summed in fixed
 * orders and no atomics (the same result in either deterministic mode). Indices are not checked on the device: the caller validates them. */
/* rank[i] (int32 [Ni]) = min over the captions c in cap_idx[cap_off[i] .. cap_off[i+1]) of the rank of column c in row i; Nt when image i has
 * no caption (the reference's 1e20: a miss at every k). That minimum is the rank of the best caption (highest score, lowest index among ties):
 * one workgroup per row counts the columns that beat it. cap_off: int32 [Ni + 1], cap_idx: int32 [cap_off[Ni]], entries in [0, Nt). */
int clite_retrieval_rank_i2t(const float* sims, int ld, int Ni, int Nt, const int* cap_off, const int* cap_idx, int* rank, void* stream);
/* rank[t] (int32 [Nt]) = rank of row txt2img[t] (in [0, Ni)) within column t. Lanes own columns, and the rows are split into chunks of
 * CLITE_RETRIEVAL_T2I_ROWS over the grid; each chunk's counts go to work (int32 [ceil(Ni / CLITE_RETRIEVAL_T2I_ROWS)][Nt] scratch), and a
 * second pass adds them in chunk order. */
#define CLITE_RETRIEVAL_T2I_ROWS 128
int clite_retrieval_rank_t2i(const float* sims, int ld, int Ni, int Nt, const int* txt2img, int* rank, int* work, void* stream);

/* ---- k-means of caption embeddings for clustered negative sampling (reference scripts/cluster.py:131-140: faiss.Kmeans(d, k, niter=200).train, then
 * index.search(x, 1); clip-lite_amd/kmeans.py). Lloyd's algorithm on f32 points X [N][ldx] (D % 8 == 0, ldx >= D), 2 <= K <= CLITE_KMEANS_MAX_K,
 * N >= K. One iteration: scores = X C^T by clite_gemm_nt with dtype CLITE_F32 (K padded to a multiple of 8), clite_kmeans_assign,
 * clite_kmeans_accumulate, clite_kmeans_update. No float atomics: every sum is formed in an order that depends on the assignment alone, so the
 * centroids are bitwise reproducible from run to run and identical in both settings of clite_set_deterministic. A 16-byte aligned X with
 * ldx % 4 == 0 is read with 16-byte loads, any other through a scalar path. Every entry returns -1 for a null pointer or a shape outside the
 * above, -2 for a workspace that is too small; clite_kmeans_accumulate returns -3 when it cannot enqueue the zero fill of its histogram. */
#define CLITE_KMEANS_MAX_K 1024
#define CLITE_KMEANS_BLOCK 256   /* rows per block of the counting sort that groups the rows by cluster */
#define CLITE_KMEANS_CHUNK 128   /* rows per partial sum: a cluster of n rows is summed as ceil(n / 128) partial rows, added in order */
/* Workspace of clite_kmeans_accumulate / _update in bytes (16-byte aligned base): with nb = ceil(N / 256), int32 hist [nb][K], rank [N],
 * order [N], start [K + 1], chunk start [K + 1]; f32 distance partials [nb]; f32 partial sums [ceil(N / 128) + K][D]; the int32 and the [nb]
 * parts each rounded up to 4 elements. 8 840 128 bytes (8.43 MiB) at N = 118 287, D = 768, K = 1024. */
#define CLITE_KMEANS_ALIGN4(n) (((uint64_t)(n) + 3) & ~(uint64_t)3)
#define CLITE_KMEANS_WORK_BYTES(N, D, K)                                                                                                        \
  (4 * (CLITE_KMEANS_ALIGN4((((uint64_t)(N) + CLITE_KMEANS_BLOCK - 1) / CLITE_KMEANS_BLOCK) * (uint64_t)(K) + 2 * (uint64_t)(N) +               \
                            2 * ((uint64_t)(K) + 1)) +                                                                                          \
        CLITE_KMEANS_ALIGN4(((uint64_t)(N) + CLITE_KMEANS_BLOCK - 1) / CLITE_KMEANS_BLOCK) +                                                    \
        (((uint64_t)(N) + CLITE_KMEANS_CHUNK - 1) / CLITE_KMEANS_CHUNK + (uint64_t)(K)) * (uint64_t)(D)))
/* out[n] (f32 [N]) = scale * |x_n|^2: the row term of the squared distances (scale 1), and 0.5 |c_k|^2 of the initial centroids (scale 0.5).
 * cluster.py:136-139 (the norms faiss's IndexFlatL2 keeps). */
int clite_kmeans_row_norms(const float* X, int ldx, int N, int D, float scale, float* out, void* stream);
/* assign[n] (int32 [N]) = argmin over k < K of hc[k] - scores[n][k], hc[k] = 0.5 |c_k|^2, ties to the lower k (0.0 == -0.0 is a tie); columns in
 * [K, lds) are never compared. A NaN value never wins: the row takes the lowest k whose value is not a NaN, or 0 when every value is one.
 * *changed (int32, device) += the number of rows whose previous assign[n] differs (integer atomic). dist (f32 [N], optional, needs xnorm =
 * |x_n|^2) = max(0, |x_n|^2 - 2 x_n.c + |c|^2) for the chosen centroid, 0 for an all-NaN row. cluster.py:139-140 (the assignment inside train, and index.search(x, 1)). */
int clite_kmeans_assign(const float* scores, int lds, const float* hc, const float* xnorm, int N, int K, int* assign, float* dist, int* changed,
                        void* stream);
/* Groups the rows by cluster (stable: ascending row index inside a cluster) and leaves in `work` the partial sums of every cluster's rows, read
 * once from X; counts[k] (int32 [K]) = rows assigned to k; *inertia (double, device, optional) = sum of dist (optional f32 [N]) in a fixed
 * order. A row whose assign[n] is outside [0, K) joins no cluster. cluster.py:136-139 (the centroid update inside faiss.Kmeans.train). */
int clite_kmeans_accumulate(const float* X, int ldx, const int* assign, const float* dist, int N, int D, int K, int* counts, double* inertia,
                            void* work, uint64_t work_bytes, void* stream);
/* From the `work` and counts that clite_kmeans_accumulate left for the same (N, D, K): C[k] (f32 [K][ldc], 16-byte aligned, ldc % 4 == 0) =
 * sum_k / count_k and hc[k] = 0.5 |c_k|^2; an empty cluster keeps its centroid (the driver relocates before it gets here).
 * cluster.py:136-139. */
int clite_kmeans_update(const void* work, uint64_t work_bytes, const int* counts, int N, int D, int K, float* C, int ldc, float* hc, void* stream);

/* ---- Weighted k-nearest-neighbour classification on frozen features (Wu et al. 2018; clip-lite_amd/knn.py). Additive to ABI v12. The similarity
 * matrix of the queries against the bank is formed one [query block] x [bank chunk] tile at a time (clite_gemm_nt with dtype CLITE_F32) and
 * folded into every query's running list of its K best bank rows. Order: score descending, bank index ascending among equal scores,
 * 0.0 == -0.0: the first K of np.argsort(-s, kind="stable") over the whole bank row. No float atomics and no order that depends on scheduling:
 * every result below is a pure function of its inputs. */
#define CLITE_KNN_MAX_K 256
#define CLITE_KNN_MAX_CLASSES 16384   /* the class bins of the vote live in LDS */
#define CLITE_KNN_MAX_KS 8
#define CLITE_KNN_PRED 5              /* predictions per query and k */
/* scores: f32 [Q][lds], lds >= Nc; row q holds the similarities of query q to bank rows base .. base + Nc - 1. Only columns < Nc take part
 * (padding columns may be loaded, never selected). top_s (f32) / top_i (int32) [Q][K]: the running lists, whose first `have` entries are valid
 * and in order (`have` is the same for all rows: min(K, base) when the chunks are fed in order). On return the first min(K, have + Nc)
 * entries hold the best of the old list and the chunk, in order; bank indices are base + column. A NaN score is never selected (a row with
 * fewer than that many other scores ends in entries of score -inf and index INT32_MAX). One workgroup per row streams it once: a 16-byte
 * aligned scores with lds % 4 == 0 with 16-byte loads, any other through a scalar path. Row offsets are 64-bit. Returns -1 and launches
 * nothing for K outside [1, CLITE_KNN_MAX_K], have outside [0, K], Q <= 0, Nc <= 0, lds < Nc, base < 0, base + Nc > INT32_MAX or a null
 * pointer. */
int clite_knn_topk_merge(const float* scores, int lds, int Q, int Nc, int base, int K, int have, float* top_s, int* top_i, void* stream);
/* The vote over the final lists top_s / top_i [Q][K] (every entry valid: K <= N). labels: int32 [N] (device) in [0, C). ks: int32 [nk] in HOST
 * memory, strictly ascending, 1 <= k <= K, nk <= CLITE_KNN_MAX_KS. For every query and every k:
 * score[c] = sum over the ranks r < k with labels[top_i[r]] == c of exp((top_s[r] - top_s[0]) * inv_T), an f32 sum in rank order (the same
 * bits in every run; subtracting the best similarity changes no ranking and cannot overflow). pred: int32 [nk][Q][CLITE_KNN_PRED], the best
 * classes by (score descending, class ascending); classes without a vote score 0 and take part; positions beyond C hold -1. class_scores:
 * f32 [nk][Q][C], or NULL. The caller validates indices and labels; an index outside [0, N) or a label outside [0, C) is skipped on the
 * device, never read through. Returns -1 and launches nothing for K outside [1, CLITE_KNN_MAX_K], C outside [1, CLITE_KNN_MAX_CLASSES], nk
 * outside [1, CLITE_KNN_MAX_KS], ks not ascending or outside [1, K], Q <= 0, N <= 0, inv_T negative or not finite, or a null pointer. */
int clite_knn_vote(const float* top_s, const int* top_i, const int* labels, int Q, int K, int N, int C, const int* ks, int nk, float inv_T,
                   float* class_scores, int* pred, void* stream);

/* ---- Logistic-regression probe on frozen features (the linear-probe protocol of CLIP; clip-lite_amd/logreg.py). Additive to ABI v12. P independent
 *   min_W f_p(W) = 1/2 |W|_F^2 + c_p sum_i w_ip (logsumexp(W x~_i) - (W x~_i)[y_i]),   W in R^{C x Dp}
 * (sklearn LogisticRegression(C=c_p, fit_intercept=False) on the augmented rows with sample_weight w[:, p]: the bias is the last weight and is
 * regularised) over one shared f32 matrix X~ [N][Dp], solved by batched Newton-CG: every CG iteration is clite_gemm_nt (X~ D^T) and clite_gemm_tn
 * (Q^T X~ + D) plus the kernels below. Row operands (logits Z = X~ W^T, probabilities Pr, gradient operand S, Q, delta) are f32 [N][ldz],
 * 16-byte aligned, ldz % 4 == 0, ldz >= P * Cp with Cp = ceil8(C): problem p owns columns p * Cp .. p * Cp + C - 1, its padding columns are
 * written as zeros and take no part in any softmax, columns from P * Cp on are never touched. y: int32 [N] in [0, C) (validated by the caller;
 * a label outside is never read through). costs: f32 [P]. w: f32 [N][P], w_ip >= 0, 0 holds a row out. Vectors (W, the gradient G, the CG
 * vectors X, R, D, HD) are f32 [P * Cp][Dp]: one contiguous span of n = Cp * Dp floats per problem, `ld` floats apart (ld >= n). Per-problem
 * scalars stay on the device in `state`, f32 [P][CLITE_LOGREG_STATE], zero-initialised with the active flag (column 9) set: 0 |grad f(0)|,
 * 1 |grad f(W)|, 2 their ratio, 5 last step length, 6 Newton iterations, 8 CG iterations, 11 CG iterations of the previous Newton iteration,
 * 12 phi'(0) of the last line search, 21 its evaluations. Every sum is formed in one fixed order (no float atomics): results are bitwise
 * reproducible in either deterministic mode. Row kernels return -2 for C > CLITE_LOGREG_MAX_CLASSES (a group is held in registers) and -1 for
 * any other bad argument (null or misaligned pointer, N, P or C <= 0, P > 65535, ldz too small); nothing is launched then. */
#define CLITE_LOGREG_STATE 24
#define CLITE_LOGREG_ROWS 32            /* rows per row-block partial */
#define CLITE_LOGREG_MAX_CLASSES 4096
#define CLITE_LOGREG_BLOCKS(N) (((N) + CLITE_LOGREG_ROWS - 1) / CLITE_LOGREG_ROWS)
/* Pr = softmax over each group of Z, S = c_p w_ip (Pr - onehot(y_i)), loss (f32 [P]) = sum_i c_p w_ip (lse - z_y), the data term of f_p, from
 * row-block partials summed in block order. Stable for logits of any finite magnitude (the group maximum is subtracted). work: f32
 * [CLITE_LOGREG_BLOCKS(N)][P] scratch. The gradient is G = W + S^T X~ (clite_gemm_tn with the residual epilogue). */
int clite_logreg_softmax(const float* Z, const int* y, const float* costs, const float* w, int N, int P, int C, int ldz, float* Pr, float* S,
                         float* loss, float* work, void* stream);
/* In place on Q = X~ D^T: q <- c_p w_ip (Pr * q - Pr <Pr, q>) per group (zeros in a held-out group, which is not read); then the Hessian-vector
 * product is HD = D + Q^T X~. */
int clite_logreg_hess_apply(const float* Pr, const float* costs, const float* w, int N, int P, int C, int ldz, float* Q, void* stream);
/* One workgroup per problem: |G_p| and the stopping test: |G_p| <= tol |grad f_p(0)|, max_newton steps taken, or a last line search that ended at
 * step 0 (W did not move, so the iteration would only repeat); the problem then freezes, in the last two cases with its ratio above tol. For a
 * problem that goes on the start of a CG solve of H x = -g: X = 0, R = D = -G, CG tolerance eta |g| with eta = min(eta_max, sqrt(|g| / |g0|)).
 * |grad f_p(0)| is what a call with g0_only = 1 recorded (G then being the gradient at W = 0; nothing else is written), else |G_p| of the first
 * call (a cold start). */
int clite_logreg_newton_begin(const float* G, int ld, int n, int P, float* X, float* R, float* D, float* state, float tol, int max_newton,
                              float eta_max, int g0_only, void* stream);
/* One CG iteration for every problem whose solve is still open: alpha = r.r / d.HD, X += alpha D, R -= alpha HD, then stop when |R| <= the
 * tolerance or D = R + beta D. Problems that are frozen or done are left untouched. */
int clite_logreg_cg_update(const float* HD, int ld, int n, int P, float* X, float* R, float* D, float* state, void* stream);
/* The line search along D minimises phi_p(t) = f_p(W + t D) by safeguarded Newton on phi' inside a bracket, starting at t = 1:
 *   phi'(t) = <W + t D, D> + c sum_i w_i (<softmax(z_i + t d_i), d_i> - d_i[y_i]),   phi''(t) = |D|^2 + c sum_i w_i Var_softmax(z_i + t d_i)(d_i).
 * ray_begin: phi'(0) = <G, D>, <W, D>, |D|^2; a problem that is not active, or with phi'(0) >= 0, is done at t = 0. ray_eval: one pass over Z
 * and delta = X~ D^T (the padding columns of both may hold anything) that writes the row-block partials of the two sums at the current t_p into work (f32 [2][CLITE_LOGREG_BLOCKS(N)][P]);
 * finished problems are skipped. ray_step (one workgroup): sums the partials in block order and moves t_p and the bracket; the search of a
 * problem ends at |phi'(t)| <= 1e-4 |phi'(0)|, at a step that no longer moves t, or with last != 0 (then at the bracket's left end lo:
 * phi' < 0 on [0, lo], so phi(lo) <= phi(0); that is t = 0 when no point left of the minimiser was found). ray_finish: W_p += t_p D_p for every finished search. Enqueue ray_begin, a fixed number of
 * (ray_eval, ray_step) pairs with last set on the final one, then ray_finish. */
int clite_logreg_ray_begin(const float* G, const float* W, const float* D, int ld, int n, int P, float* state, void* stream);
int clite_logreg_ray_eval(const float* Z, const float* delta, const int* y, const float* costs, const float* w, int N, int P, int C, int ldz,
                          const float* state, float* work, void* stream);
int clite_logreg_ray_step(const float* work, int N, int P, float* state, int last, void* stream);
int clite_logreg_ray_finish(float* W, const float* D, int ld, int n, int P, const float* state, void* stream);

/* ---- Image augmentation on the device (reference factories.py:112-160 and data/dataloader.py:186-192, which run on the CPU; semantics:
 * clip-lite_amd/augment.py). Additive to ABI v12. canvases: uint8 [N][cap], sample n an HWC image of hw[2n] x hw[2n+1] pixels packed at the front
 * of its slot (pitch 3 w); hw: int32 [N][2]; plan: f32 [N][CLITE_AUGMENT_PLAN_W], one row per view: crop box x0, y0, cw, ch in canvas pixels,
 * flip flag, jitter flag, brightness / contrast / saturation factors, hue shift, the order of the four colour ops (0 brightness, 1 contrast,
 * 2 saturation, 3 hue), normalise flag, one unused column. A view is the box resampled to S x S with PIL's antialiased triangle filter, mirrored,
 * jittered on [0, 255] values and scaled to [0, 1] or ImageNet-normalised; all in f32 with contraction off, identical in every entry below.
 * plan_host / hw_host: optional host mirrors of the two tables, validated before anything is enqueued: -2 for a canvas extent that is not
 * positive or does not fit cap, -3 for a row that is not finite, has an empty box, a box outside its canvas or an order that is no permutation,
 * -4 for a box wider or higher than CLITE_AUGMENT_MAX_SCALE * S (the kernels read at most CLITE_AUGMENT_MAX_TAPS taps per axis). -1: a null
 * pointer or a shape outside N in [1, 65535], S in [1, 4096]. Without the mirrors a bad table cannot fault either: such a view comes out
 * blank (extent) or with clipped taps. */
#define CLITE_AUGMENT_PLAN_W 16
#define CLITE_AUGMENT_MAX_SCALE 4
#define CLITE_AUGMENT_MAX_TAPS 9
#define CLITE_AUGMENT_GRAY_BLOCKS(S) (((S) * (S) + 255) / 256)   /* partial sums per view of clite_augment_gray_mean */
enum { CLITE_AUGMENT_NCHW = 0, CLITE_AUGMENT_NHWC4 = 1 };
/* mean[n] (f32 [N]) = mean over the view of 0.299 R + 0.587 G + 0.114 B as the view stands in front of its contrast op; 0 for a view whose
 * jitter flag is off (nothing of it is read). No float atomics: work (f32 [N][CLITE_AUGMENT_GRAY_BLOCKS(S)] scratch) receives one partial sum per
 * workgroup and a second kernel adds them in order, so the result is bitwise reproducible and the same in both settings of
 * clite_set_deterministic. */
int clite_augment_gray_mean(const uint8_t* canvases, const int* hw, int64_t cap, const float* plan, int N, int S, float* mean, float* work,
                            const float* plan_host, const int* hw_host, void* stream);
/* form CLITE_AUGMENT_NCHW: out f32 [N][3][S][S] (dtype CLITE_F32; pad, Hp, Wp ignored) - the batch dict's "image". form CLITE_AUGMENT_NHWC4:
 * out [N][Hp][Wp][4] in dtype, the view at (pad, pad), every other element (padding, channel 3) written as zero - exactly what
 * clite_image_to_nhwc4 makes of the NCHW form. mean: what clite_augment_gray_mean left for the same tables (read only by views with jitter). */
int clite_augment_apply(int form, int dtype, const uint8_t* canvases, const int* hw, int64_t cap, const float* plan, const float* mean, int N, int S,
                        void* out, int pad, int Hp, int Wp, const float* plan_host, const int* hw_host, void* stream);
/* clite_augment_apply with the two transforms that follow the colour jitter (augment.py steps 3b / 3c). Additive to ABI v12. post: f32
 * [N][CLITE_AUGMENT_POST_W], one row per view: gray flag (R = G = B = 0.299 R + 0.587 G + 0.114 B), blur flag, the weights w0..w3 of a symmetric
 * separable 7-tap filter (w[|i|], horizontal pass then vertical, taps added in ascending offset, border REFLECT_101 on the S x S view), two
 * reserved zeros. The host puts the weights of its kernel size into the row; the kernel holds no table. Gray comes first, then blur, then the
 * normalisation. A row of zeros gives what clite_augment_apply gives, bit for bit. mean is clite_augment_gray_mean's of the same plan: both
 * transforms follow the jitter, so the contrast mean does not see them. post_host: optional host mirror, validated with the other two: -3 for
 * a flag that is not 0 or 1, a weight that is not finite or is negative, and on a blurred row for |w0 + 2 (w1 + w2 + w3) - 1| > 1e-3 or S < 4;
 * -1 for a null post. Without the mirror a bad row cannot fault: a reflected coordinate is also clamped to [0, S - 1]. */
#define CLITE_AUGMENT_POST_W 8
int clite_augment_apply_post(int form, int dtype, const uint8_t* canvases, const int* hw, int64_t cap, const float* plan, const float* post,
                             const float* mean, int N, int S, void* out, int pad, int Hp, int Wp, const float* plan_host, const int* hw_host,
                             const float* post_host, void* stream);

/* ---- Update path (reference train.py:221-226, factories.py:464-482, optim/lookahead.py:88-101) over flat f32 buffers. */
typedef struct clite_optim_item {   /* one workgroup's slice of one parameter tensor (never straddles tensors) */
  uint64_t start;                   /* element offset into the flat buffers, multiple of 4 */
  uint32_t count;                   /* elements, multiple of 4 */
  float lr;                         /* base learning rate of the owning tensor's param group */
  float wd;                         /* weight decay of the owning tensor's param group */
  uint32_t reserved;                /* clite_lars_*, clite_lamb_*: slot of the owning tensor in `norms` + 1; 0 = not adapted. The other kernels ignore it. */
} clite_optim_item;
/* out (f32 scalar, pre-zeroed) += sum x^2 — the global gradient norm of clip_grad_norm_. Two fixed-order stages through `partials`
 * (device f32[n_partials], n_partials >= 1; 1024 slots use the whole chip): no float atomics, so the value is a pure function of x and every
 * data-parallel rank derives the same clip factor from the same all-reduced gradients (replicas stay bit-identical). */
int clite_sumsq(const float* x, uint64_t n, float* out, float* partials, int n_partials, void* stream);
/* dst[i] = sum over s < slices of src[s * stride + i], i < n, in slice order (stride % 4 == 0, 16-byte aligned pointers). The local step of the
 * mesh gradient exchange that replaces DDP's ring all-reduce (reference train.py:174-178): after an all-to-all every rank holds its chunk of
 * the gradients from all `slices` = world_size ranks and sums them before the all-gather. */
int clite_sum_slices(const float* src, int slices, uint64_t stride, uint64_t n, float* dst, void* stream);
/* hp (device f32[6]): lr multiplier, momentum, max grad norm (<=0 off), lookahead-sync flag, lookahead alpha, grad pre-scale.
 * g' = g*prescale*clip + wd*p; v = mu*v + g'; p -= lr*mult*v; on sync steps p = alpha*p + (1-alpha)*slow, slow = p.
 * g is zeroed; cast_bf16 (optional) receives the bf16 copy of p at the same offsets. */
int clite_sgd_step(float* p, float* g, float* v, float* slow, void* cast_bf16, const clite_optim_item* items, int n_items,
                   const float* hp, const float* sumsq, void* stream);
/* ABI v11. torch.optim.AdamW (reference factories.py:439: OPTIMIZER_NAME "adamw", torch's defaults) in the same one-pass form, with the same clipping,
 * Lookahead synchronisation, gradient zeroing and bf16 copy. hp (device f32[12]): as clite_sgd_step, with [1] = beta1, [6] = beta2, [7] = eps,
 * [8] = 1 - beta1^t, [9] = 1 - beta2^t of this step, [10] = 1 - beta1, [11] = 1 - beta2 (formed in double by the host). p *= 1 - lr wd; m += (1 - beta1)(g' - m); v2 = beta2 v2 + (1 - beta2) g'^2;
 * p -= lr / hp[8] * m / (sqrt(v2) / sqrt(hp[9]) + eps), g' = g * prescale * clip. */
int clite_adamw_step(float* p, float* g, float* m, float* v2, float* slow, void* cast_bf16, const clite_optim_item* items, int n_items,
                     const float* hp, const float* sumsq, void* stream);
int clite_cast_bf16(const float* src, void* dst, uint64_t n, void* stream);
/* LARS (You, Gitman, Ginsburg 2017: layer-wise adaptive rate scaling; the update SimCLR-style recipes run at batch sizes of 1k .. 32k) on the
 * same item table: SGD whose step for every ADAPTED tensor is scaled by a trust ratio. An item's `reserved` word holds the owning tensor's slot
 * + 1 (0: not adapted — biases, normalisation scales); a tensor's items are contiguous in the table and in arena order.
 *
 * clite_lars_norms: norms[2 slot] = sum p^2, norms[2 slot + 1] = sum g^2 over the raw p and g of every adapted tensor whose items lie in the
 * launched table (a tensor is launched whole or not at all); slots of other tensors are untouched. Two fixed-order stages, no float atomics:
 * every item's workgroup stores its pair into partials[2 i], partials[2 i + 1] (i: index in the launched table; device f32[2 n_items]), then
 * the workgroup of a tensor's FIRST item folds that tensor's pairs in item order. The result is a pure function of the data (bit-identical
 * between runs and between data-parallel ranks) and does not depend on which other tensors share the launch. Items whose reserved word
 * exceeds n_slots are treated as not adapted by both entry points.
 *
 * clite_lars_step: clite_sgd_step with, per adapted tensor, pn = sqrt(norms[2 slot]), gn = prescale clip sqrt(norms[2 slot + 1]),
 * q = eta pn / (gn + wd pn + eps) if pn > 0 and gn > 0, else 1 (q = 1 for items that are not adapted, which never read norms):
 * u = q (g prescale clip + wd p); v = mu v + u; p -= lr mult v; then the Lookahead sync, the zeroing of g and the bf16 copy as there.
 * hp (device f32[8]): as clite_sgd_step, with [6] = eta (trust coefficient), [7] = eps. With every q = 1 the result is clite_sgd_step's bit for bit. */
int clite_lars_norms(const float* p, const float* g, const clite_optim_item* items, int n_items, float* partials, float* norms, int n_slots,
                     void* stream);
int clite_lars_step(float* p, float* g, float* v, float* slow, void* cast_bf16, const clite_optim_item* items, int n_items, const float* hp,
                    const float* sumsq, const float* norms, int n_slots, void* stream);
/* LAMB (You et al. 2020, "Large Batch Optimization for Deep Learning", Algorithm 2) on the same item table, with clite_lars_*'s marking of adapted
 * tensors through `reserved` and its two fixed-order norm stages. Additive to ABI v12. hp (device f32[13]): clite_adamw_step's twelve floats, then
 * [12] = TRUST_CLIP flag. Per tensor, with g' = g prescale clip:
 *   m += (1 - beta1)(g' - m); v2 = beta2 v2 + (1 - beta2) g'^2          (clite_adamw_step's statements)
 *   r = (m / hp[8]) / (sqrt(v2 / hp[9]) + eps) + wd p
 *   adapted: q = |p| / |r| if both norms > 0, else 1; with TRUST_CLIP q = min(q, 1); p -= lr mult q r
 *   not adapted: p *= 1 - lr wd; p -= lr / hp[8] * m / (sqrt(v2) / sqrt(hp[9]) + eps), clite_adamw_step's arithmetic: with every reserved word 0
 *   the two calls together give clite_adamw_step's p, m, v2, slow and bf16 copy bit for bit.
 * |p| is taken before the update, |r| from the moments after it. There is no eps in q and no trust coefficient.
 *
 * clite_lamb_moments: updates m and v2 of every launched item in place and leaves norms[2 slot] = sum p^2, norms[2 slot + 1] = sum r^2 of every
 * adapted tensor whose items lie in the launched table (partials: device f32[2 n_items], as clite_lars_norms; the same fold, so the same
 * guarantees: no float atomics, bit-identical between runs, independent of which other tensors share the launch). p and g are not written.
 *
 * clite_lamb_step: re-forms r from the stored m, v2 and the unchanged p with the same device function (the r that was normed is the r that is
 * applied, bit for bit), updates p, then the Lookahead sync, the zeroing of g and the bf16 copy as clite_adamw_step. Must follow clite_lamb_moments
 * over the same items on the same stream. sumsq is not read (the clip factor entered the moments); it must not be null. */
int clite_lamb_moments(const float* p, const float* g, float* m, float* v2, const clite_optim_item* items, int n_items, const float* hp,
                       const float* sumsq, float* partials, float* norms, int n_slots, void* stream);
int clite_lamb_step(float* p, float* g, const float* m, const float* v2, float* slow, void* cast_bf16, const clite_optim_item* items, int n_items,
                    const float* hp, const float* sumsq, const float* norms, int n_slots, void* stream);

/* ---- Bias evaluation: a direction found in the text embedding space, removed from image features (reference bias_eda.py, utils/we.py;
 * clip-lite_amd/debias.py). Additive to ABI v12. No float atomics: every result below is a pure function of its inputs, bit for bit. */
#define CLITE_DEBIAS_MAX_PAIRS 64
#define CLITE_DEBIAS_MAX_COMPONENTS 8
#define CLITE_DEBIAS_MAX_DIM 4096
/* The principal directions of the pair differences diffs, f32 [P][D] (row i = e(a_i) - e(b_i); 16-byte aligned): what we.doPCA's
 * sklearn PCA of the 2 P rows +-d_i / 2 returns, whose column mean is zero, i.e. the right singular vectors of diffs. The P x P Gram matrix is
 * formed in f32 with a fixed summation order (work: f32 [P * P]) and diagonalised in LDS by one workgroup (cyclic Jacobi, round-robin pairing,
 * a bye for an odd P) until the off-diagonal norm is at most FLT_EPSILON x trace. eigvals: f32 [P], descending (the squared singular values
 * of diffs; a rounding-negative one reads 0; not finite, and last, when the f32 Gram matrix overflowed). components: f32 [R][D] = normalised diffs^T u_j of the R largest, after one modified
 * Gram-Schmidt pass (orthonormal rows to f32 rounding), each row signed so that its entry of largest magnitude (the lowest index among equal
 * ones) is positive. A direction whose eigenvalue is below ~P FLT_EPSILON eigvals[0] is rounding noise of the Gram matrix; the caller judges
 * (debias.directions refuses below 1e-4). info: device int32 [2], written by the kernel like every other result (the call does not wait):
 * info[0] = 0, or the error code 1 when 30 sweeps did not reach the bound (eigvals and components then hold the unconverged state);
 * info[1] = sweeps run. Returns -1 and launches nothing for P outside [1, CLITE_DEBIAS_MAX_PAIRS], D not a positive multiple of 8 or above
 * CLITE_DEBIAS_MAX_DIM, R outside [1, min(P, CLITE_DEBIAS_MAX_COMPONENTS)], a misaligned or a null pointer. */
int clite_debias_pca(const float* diffs, int P, int D, int R, float* eigvals, float* components, float* work, int* info, void* stream);
/* The streaming pass over x, f32 [N][D] (D as above; 16-byte aligned), with components f32 [R][D] (orthonormal rows; R in
 * [1, CLITE_DEBIAS_MAX_COMPONENTS], held in LDS). Any of the outputs may be NULL:
 *   coef [N][R] = <x, v_j>;   xn [N][D] = x / max(|x|, 1e-12);   xd [N][D] = y / max(|y|, 1e-12), y = x - sum_j <x, v_j> v_j
 * (F.normalize's rule; |y| is the norm of y itself). One wave per row, the row in registers, 16-byte accesses; x is read once. With all three
 * NULL nothing is launched (returns 0). Returns -1 and launches nothing for N < 1, a D or R outside the limits, a null x or components, or a
 * misaligned x, components, xn or xd. */
int clite_debias_rows(const float* x, const float* components, int N, int D, int R, float* xn, float* xd, float* coef, void* stream);

/* ---- ViT image encoder (torchvision.models.vit_b_32 / vit_b_16 as the reference's ImageEncoder would build them; clip-lite_amd/vit.py):
 * what the tower needs beside the GEMMs, clite_layernorm_* and clite_attention_*. Additive to ABI v12. Streaming kernels, 16-byte accesses, no
 * float atomics: each result is a pure function of its inputs in both settings of clite_set_deterministic. Every pointer 16-byte aligned;
 * a violated precondition returns -1 and launches nothing. */
/* The patch matrix of an image batch: img f32 NCHW [B][3][H][W] (H % p == 0, W % p == 0, p % 8 == 0) ->
 * out [B * (H/p) * (W/p)][3 * p * p] in `dtype`, row (b, ph, pw) row-major, column (c, i, j) = img[b][c][ph p + i][pw p + j]: the column order
 * of nn.Conv2d(3, C, p, stride = p).weight.view(C, 3 p p), which is then clite_gemm_nt's B operand as it is. The image has no gradient. */
int clite_vit_patchify(int dtype, const float* img, void* out, int B, int H, int W, int p, void* stream);
/* Token assembly, L = P + 1 tokens of C elements (C % 8 == 0): s0[b][0] = cls + pos[0], s0[b][1 + t] = e[b][t] + pos[1 + t]; e [B * P][C] is the
 * patch GEMM's output (conv_proj.bias added by its epilogue), cls [C], pos [L][C], all of `dtype`; the sum is formed in f32 and rounded once. */
int clite_vit_tokens_fwd(int dtype, const void* e, const void* cls, const void* pos, void* s0, int B, int P, int C, void* stream);
/* Its backward: de[b][t] = ds0[b][1 + t] (`dtype`), dpos[t] += sum_b ds0[b][t] and dcls += sum_b ds0[b][0] (f32, either may be NULL). One
 * thread owns a (token, 8 columns) slot and adds over b in index order. */
int clite_vit_tokens_bwd(int dtype, const void* ds0, void* de, float* dpos, float* dcls, int B, int P, int C, void* stream);
/* The class rows around the final LayerNorm (which acts row by row, so only they need it): out[b] = x[b * L] of x [B * L][C]; and the
 * backward, dx[b * L] = d[b], the other rows of dx left as they are (the caller zeroes them). */
int clite_vit_class_gather(int dtype, const void* x, void* out, int B, int L, int C, void* stream);
int clite_vit_class_scatter(int dtype, const void* d, void* dx, int B, int L, int C, void* stream);

/* ---- Patch dropout (FLIP, Li et al. 2023; open_clip's PatchDropout): in training each image keeps Kk of its P patches plus the class token, and
 * the tower runs at L' = Kk + 1 tokens. Additive to ABI v12. No float atomics; the same bits in both settings of clite_set_deterministic.
 * The kept set of sample b: key[t] = the 24-bit uniform of element b * Ppad + t of the (seed, site) stream of rng_uniform4 (csrc/rng.h),
 * Ppad = P rounded up to a multiple of 4; rank[t] = the number of u with key[u] < key[t], or key[u] == key[t] and u < t; patch t is kept iff
 * rank[t] < Kk. idx int32 [B][Kk] lists the kept patches in ascending order, inv int32 [B][P] holds the position of t in idx[b] or -1.
 * (seed, site) as for every dropout site (CLITE_SEED_INDIRECT). Returns -1 for B < 1, P outside 1 .. 128, Kk outside 1 .. P or a null pointer. */
int clite_vit_keep_indices(int32_t* idx, int32_t* inv, int B, int P, int Kk, uint64_t seed, uint32_t site, void* stream);
/* clite_vit_patchify on the kept patches only: out [B * Kk][3 * p * p], row (b, k) = the patch idx[b][k] of image b; the rest of the image is
 * not read. -1 also for Kk outside 1 .. (H/p)(W/p). An idx entry outside 0 .. P - 1 leaves its row unwritten. */
int clite_vit_patchify_keep(int dtype, const float* img, const int32_t* idx, void* out, int B, int H, int W, int p, int Kk, void* stream);
/* Token assembly at L' = Kk + 1: s0[b][0] = cls + pos[0], s0[b][1 + k] = e[b][k] + pos[1 + idx[b][k]]; e [B * Kk][C], pos [P + 1][C],
 * s0 [B * L'][C]; f32 sum, one rounding. Equal to clite_vit_tokens_fwd followed by a gather of the rows 0 and 1 + idx[b]. */
int clite_vit_tokens_keep_fwd(int dtype, const void* e, const void* cls, const void* pos, const int32_t* idx, void* s0, int B, int P, int Kk, int C,
                              void* stream);
/* Its backward, through inv: de[b][k] = ds0[b][1 + k]; dpos[1 + t] += the sum over the samples that kept t of their row, in ascending b;
 * dpos[0] and dcls += the sum over b of row 0 (f32 [P + 1][C] and [C], either may be NULL). One thread owns a (position, 8 columns) slot. The
 * dpos row of a position no sample kept is not touched. -1 also for a ds0 of 0xF0000000 bytes or more in f32 (ds0 and de are addressed through one buffer resource each). */
int clite_vit_tokens_keep_bwd(int dtype, const void* ds0, const int32_t* inv, void* de, float* dpos, float* dcls, int B, int P, int Kk, int C,
                              void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CLITE_H */
