// gfx950 (CDNA4) intrinsic wrappers used by every kernel in csrc/.
//
// Kernels never spell __builtin_amdgcn_* directly; they go through these thin
// inline wrappers so that the wavefront simulator used by the CPU-side kernel
// tests (tests/wavesim/, test infrastructure only) can supply lane-accurate
// emulations of the same names. This header is the ONLY definition the shipped
// library is built with.
#ifndef CLITE_INTRIN_H
#define CLITE_INTRIN_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#define DEV __device__ __forceinline__

typedef __bf16 bf16;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;
typedef __attribute__((ext_vector_type(2))) uint32_t u32x2;

#define WAVE 64

typedef __amdgpu_buffer_rsrc_t rsrc_t;

// Buffer resource over [ptr, ptr+bytes): loads past the end return 0, stores
// past the end are dropped by hardware (raw buffer, stride 0).
DEV rsrc_t make_rsrc(const void* ptr, uint32_t bytes) {
  return __builtin_amdgcn_make_buffer_rsrc((void*)ptr, 0, (int)bytes, 0x00020000);
}
// Byte offset that is out of range for every buffer (<4 GiB): reads as zero.
#define OOB_OFF 0xFFFFFFF0u

DEV u32x4 buf_load16(rsrc_t r, uint32_t off) { return __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 0); }
DEV u32x2 buf_load8(rsrc_t r, uint32_t off) { return __builtin_amdgcn_raw_buffer_load_b64(r, off, 0, 0); }
DEV uint32_t buf_load4(rsrc_t r, uint32_t off) { return __builtin_amdgcn_raw_buffer_load_b32(r, off, 0, 0); }
DEV uint32_t buf_load1(rsrc_t r, uint32_t off) { return (uint32_t)__builtin_amdgcn_raw_buffer_load_b8(r, off, 0, 0); }   // one byte, zero-extended
DEV void buf_store16(rsrc_t r, uint32_t off, u32x4 v) { __builtin_amdgcn_raw_buffer_store_b128(v, r, off, 0, 0); }
DEV void buf_store8(rsrc_t r, uint32_t off, u32x2 v) { __builtin_amdgcn_raw_buffer_store_b64(v, r, off, 0, 0); }
DEV void buf_store4(rsrc_t r, uint32_t off, uint32_t v) { __builtin_amdgcn_raw_buffer_store_b32(v, r, off, 0, 0); }

// LDS-DMA: buffer_load_dwordx4 ... lds — 16 bytes per lane from its own global offset straight into LDS at
// lds_wave_base + lane*16 (the LDS destination is wave-uniform base + lane slot; out-of-range sources write zeros).
// Counts on vmcnt like any other load; data is visible to ds_read only after the issuing wave's vmcnt wait + a barrier.
DEV void buf_load16_lds(rsrc_t r, uint32_t off, void* lds_wave_base) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (__attribute__((address_space(3))) void*)lds_wave_base, 16, off, 0, 0, 0);
}
// ... with the non-temporal cache policy (aux = 2, `nt`): for bytes that ONE CU reads once (MI355X_MICROARCH.md, nt-weights)
DEV void buf_load16_lds_nt(rsrc_t r, uint32_t off, void* lds_wave_base) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (__attribute__((address_space(3))) void*)lds_wave_base, 16, off, 0, 0, 2);
}
// The same instruction as one assembly statement, which the compiler neither counts on vmcnt nor models as an LDS write. The builtin form is an
// LDS write of unknown extent to the compiler: it drains vmcnt(0) in front of the first ds_read_b64_tr_* that follows it (it cannot tell that the
// read is of another ring stage), which serialises a K tile's DMA with its fragment reads. With this form the ONLY ordering between the DMA and
// the LDS reads is the kernel's own wait_vmcnt<N>() + barrier_raw(); N counts these loads by hand. M0 (the wave-uniform LDS destination) is
// written in the statement that reads it; `s_nop 3` covers M0 -> LDS-DMA (1 state) and a descriptor SGPR fresh from a VALU write (5 with the s_mov).
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"          // "clobber list contains reserved registers: m0" — the clobber is the point
DEV void buf_load16_lds_untracked(rsrc_t r, uint32_t off, void* lds_wave_base) {
  const uint32_t dst = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) void*)lds_wave_base;
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 3\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds" ::"s"(dst), "v"(off), "s"(r) : "memory", "m0");
}
#pragma clang diagnostic pop
template <int N> DEV void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
// Makes a value opaque to the optimiser at this point (no instruction): everything derived from it afterwards is computed where it is used
// instead of being hoisted out of an enclosing loop into dozens of live registers.
DEV void opaque_i(int& v) { asm volatile("" : "+v"(v)); }
DEV void barrier_raw() { __builtin_amdgcn_s_barrier(); }   // no implied vmcnt(0): LDS-DMA may stay in flight across it
// Workgroup barrier that orders LDS traffic only: waits for this wave's LDS operations (lgkmcnt), NOT for its global loads / stores.
// __syncthreads() also drains vmcnt, i.e. every epilogue barrier would wait for the stores just issued to reach L2 (~1.5 us each).
DEV void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
}

// v_mfma_f32_32x32x16_bf16: lane l holds A[row l&31][k 8*(l>>5)+j], B[k 8*(l>>5)+j][col l&31];
// D reg i of lane l = D[row (i&3)+8*(i>>2)+4*(l>>5)][col l&31].
DEV f32x16 mfma32_bf16(bf16x8 a, bf16x8 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
// v_mfma_f32_32x32x2_f32 (exact f32): lane l holds A[row l&31][k l>>5], B[k l>>5][col l&31].
DEV f32x16 mfma32_f32(float a, float b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

// v_mfma_f32_32x32x16_fp8_fp8 (OCP e4m3 operands, f32 accumulate; the bf16 MFMA rate at half the operand bytes): lane l holds 8 consecutive
// k of A[row l&31] / B[col l&31] (k = 8*(l>>5) + j) in one 64-bit register pair, byte j = element j; C/D as the bf16 form.
DEV f32x16 mfma32_fp8(uint64_t a, uint64_t b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_fp8_fp8((long)a, (long)b, c, 0, 0, 0);
}
// v_mfma_scale_f32_32x32x64_f8f6f4 on OCP e4m3 operands with unit block scales (E8M0 byte 127 = 1.0; the per-tensor scales stay in the epilogue):
// 64 k per instruction in twice the cycles of the bf16 32x32x16 form, i.e. twice its rate per k (tools/micro/mfma_scale_probe.hip: 4.87 PFLOP/s
// chip-wide against 2.13 for bf16 and 2.25 for the non-scaled fp8 form). Operand map, pinned by that probe on exact integer data (the guides
// give none): lane l = (r = l & 31, h = l >> 5) holds row r of A / column r of B at k = 16 h + j in bytes j = 0..15 and k = 32 + 16 h + (j - 16)
// in bytes 16..31 - two 16-byte runs, `lo` and `hi` below. C/D as every 32x32 form.
typedef __attribute__((ext_vector_type(8))) int i32x8;
DEV f32x16 mfma32x64_fp8(u32x4 a_lo, u32x4 a_hi, u32x4 b_lo, u32x4 b_hi, f32x16 c) {
  const i32x8 a = {(int)a_lo[0], (int)a_lo[1], (int)a_lo[2], (int)a_lo[3], (int)a_hi[0], (int)a_hi[1], (int)a_hi[2], (int)a_hi[3]};
  const i32x8 b = {(int)b_lo[0], (int)b_lo[1], (int)b_lo[2], (int)b_lo[3], (int)b_hi[0], (int)b_hi[1], (int)b_hi[2], (int)b_hi[3]};
  return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, c, 0, 0, 0, 0x7F7F7F7F, 0, 0x7F7F7F7F);
}
// The same instruction with an e5m2 (bf8) A operand (cbsz = 1) and an e4m3 B operand: gradients x weights in the fp8 input gradient. Same operand map
// (the probe's "e5m2 (A, cbsz 1) x e4m3" case).
DEV f32x16 mfma32x64_bf8_fp8(u32x4 a_lo, u32x4 a_hi, u32x4 b_lo, u32x4 b_hi, f32x16 c) {
  const i32x8 a = {(int)a_lo[0], (int)a_lo[1], (int)a_lo[2], (int)a_lo[3], (int)a_hi[0], (int)a_hi[1], (int)a_hi[2], (int)a_hi[3]};
  const i32x8 b = {(int)b_lo[0], (int)b_lo[1], (int)b_lo[2], (int)b_lo[3], (int)b_hi[0], (int)b_hi[1], (int)b_hi[2], (int)b_hi[3]};
  return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, c, 1, 0, 0, 0x7F7F7F7F, 0, 0x7F7F7F7F);
}
// v_cvt_pk_bf8_f32: two f32 -> two OCP e5m2 bytes (round to nearest even), low byte = a.
DEV uint32_t cvt2_bf8(float a, float b) { return (uint32_t)__builtin_amdgcn_cvt_pk_bf8_f32(a, b, 0, false) & 0xFFFFu; }
// v_cvt_pk_fp8_f32: two f32 -> two OCP e4m3 bytes (round to nearest even), low byte = a. The caller clamps to +-448 first.
DEV uint32_t cvt2_fp8(float a, float b) { return (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false) & 0xFFFFu; }

// ds_read_b64_tr_b16: per 16-lane group, lane 4q+p supplies the address of row q,
// columns 4p..4p+3 of a 4x16 block of 16-bit elements; lane i receives column i
// (rows 0..3 in elements 0..3). Address must be 8-byte aligned, EXEC all ones.
DEV s16x4 lds_read_tr16(const void* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)p);
}

// ds_read_b64_tr_b8 (layout measured on the hardware: tools/micro/tr8_probe.hip, profiles/r5_tr8_probe.txt — the guides name the instruction only): inside
// each group of 16 consecutive lanes, lane s supplies the address of an 8-byte chunk; lane i receives, in byte j, byte (i & 7) of the chunk supplied
// by lane 2 j + (i >> 3). With lane s pointing at k-row (s >> 1), column chunk (s & 1) of a [k][x] byte image, lane i ends up with column i of the
// 16 and rows 0..7 in bytes 0..7: eight consecutive k of one column — an fp8 MFMA operand fragment out of an image whose contraction index is the slow one.
DEV u32x2 lds_read_tr8(const void* p) {
  typedef int i32x2_ __attribute__((ext_vector_type(2)));
  const i32x2_ v = __builtin_amdgcn_ds_read_tr8_b64_v2i32((__attribute__((address_space(3))) i32x2_*)p);
  return u32x2{(uint32_t)v[0], (uint32_t)v[1]};
}

DEV float bf2f(bf16 x) { return (float)x; }
DEV bf16 f2bf(float x) { return (bf16)x; }   // round-to-nearest-even (v_cvt_pk_bf16_f32)

// A value that is the same in every lane of the wave (e.g. the wave index): moved to an SGPR so that everything derived from it
// (LDS-DMA destinations, tile offsets) is scalar arithmetic instead of VALU + v_readfirstlane at every use.
DEV int wave_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

DEV float wave_shfl_xor(float v, int m) { return __shfl_xor(v, m, WAVE); }
DEV int wave_shfl_xor_i(int v, int m) { return __shfl_xor(v, m, WAVE); }
DEV float wave_shfl(float v, int src) { return __shfl(v, src, WAVE); }

DEV float wave_sum(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += wave_shfl_xor(v, m);
  return v;
}
DEV float wave_max(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, wave_shfl_xor(v, m));
  return v;
}

DEV void atomic_add_f32(float* p, float v) { atomicAdd(p, v); }
DEV void atomic_max_u32(uint32_t* p, uint32_t v) { atomicMax(p, v); }
DEV uint32_t f32_bits(float f) { return __float_as_uint(f); }
DEV float bits_f32(uint32_t u) { return __uint_as_float(u); }

DEV uint32_t umulhi32(uint32_t a, uint32_t b) { return __umulhi(a, b); }

// pack / unpack helpers on 16-byte chunks of 8 bf16
union Chunk16 {
  u32x4 u;
  bf16x8 h;
  bf16 e[8];
};

#endif  // CLITE_INTRIN_H
