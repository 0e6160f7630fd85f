// Shared helpers for the MI355X (gfx950) kernel library.  Internal header: the public
// C ABI lives in include/sgl_mi355.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/sgl_mi355.h"

// Opt-in fusions that were built, measured bit-identical and NO FASTER: decode attention off the qkv
// GEMM's partial sums, the o_proj input quant folded into the attention epilogue + the GEMM's staging, the per-token
// quant by a request's last workgroup.  Their kernels are compiled only with -DSGLM_OPTIN_FUSIONS=1
// (python -m sglang_npu_amd.build_ext --variant fusions --flag=-DSGLM_OPTIN_FUSIONS=1); in the default library their
// entry points return SGL_MI355_ERR_UNSUPPORTED, which every caller already treats as "make the separate calls"
// (round 4, VERDICT r3 hygiene d).
#ifndef SGLM_OPTIN_FUSIONS
#define SGLM_OPTIN_FUSIONS 0
#endif

namespace sglm {

// Thread-local error message, returned through sgl_mi355_last_error().
void set_error(const char* fmt, ...);

inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

int check_hip(hipError_t e, const char* what);

// What sgl_mi355_fp8_last_kernel() reports (gemm_fp8.hip owns the thread-local; gemm_fp8_block.hip names its kernels too).
void set_fp8_last_kernel(const char* name);

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(4))) _Float16 f16x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) int i32x4;
typedef __attribute__((ext_vector_type(2))) int i32x2;

// Per-dtype traits: the 16-bit storage type, its MFMA fragment types and intrinsics.
template <int DTYPE>
struct Half16;

template <>
struct Half16<SGL_MI355_BF16> {
  using T = __bf16;
  using x8 = bf16x8;
  using x4 = bf16x4;
  static __device__ __forceinline__ f32x4 mfma16(x8 a, x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ f32x16 mfma32(x8 a, x8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ x4 ds_read_tr(const void* lds_ptr) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) x4*)(lds_ptr));
  }
  static __device__ __forceinline__ float to_f32(T v) { return (float)v; }
  static __device__ __forceinline__ T from_f32(float v) { return (T)v; }
};

template <>
struct Half16<SGL_MI355_FP16> {
  using T = _Float16;
  using x8 = f16x8;
  using x4 = f16x4;
  static __device__ __forceinline__ f32x4 mfma16(x8 a, x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ f32x16 mfma32(x8 a, x8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ x4 ds_read_tr(const void* lds_ptr) {
    typedef __attribute__((__vector_size__(4 * sizeof(__fp16)))) __fp16 raw4;
    raw4 r = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) raw4*)(lds_ptr));
    return __builtin_bit_cast(x4, r);
  }
  static __device__ __forceinline__ float to_f32(T v) { return (float)v; }
  static __device__ __forceinline__ T from_f32(float v) { return (T)v; }
};

// s_waitcnt vmcnt(N) with a compile-time N (the immediate must be a literal).
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  static_assert(N >= 0 && N <= 63, "vmcnt is a 6-bit field");
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
__device__ __forceinline__ void wait_lgkmcnt0() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// One LDS-DMA piece: 64 lanes x 16 B, per-lane global source, LDS destination
// lds_addr + lane*16 (lds_addr = wave-uniform LDS byte address).
//
// Issued through inline asm on purpose: hipcc's waitcnt pass, when it can see an LDS-DMA in
// flight, puts `s_waitcnt vmcnt(0)` in front of every later LDS read it cannot prove
// disjoint (all of ours), which would drain the whole prefetch queue once per tile.  Hidden
// in asm the DMA is invisible to that pass; completion is tracked by hand with counted
// wait_vmcnt<N>() (vmcnt retires in issue order), and every LDS read of DMA-written bytes
// sits behind such a wait.  M0 (the DMA's LDS base) is written and restored inside the
// statement because the compiler owns it.
__device__ __forceinline__ void lds_dma16(const void* gsrc, uint32_t lds_addr) {
  lds_addr = __builtin_amdgcn_readfirstlane(lds_addr);  // make wave-uniformity provable ("s" operand)
  uint32_t keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\t"
      "s_mov_b32 m0, %2\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %1, off\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(gsrc), "s"(lds_addr)
      : "memory");
}

// The same piece addressed as a wave-uniform 64-bit base (SGPR pair, scalar ALU) + a per-lane 32-bit byte offset: no 64-bit
// vector arithmetic per piece (round 4; the extend kernel's contiguous new-token rows).
__device__ __forceinline__ void lds_dma16_s(const void* sbase, uint32_t voff, uint32_t lds_addr) {
  lds_addr = __builtin_amdgcn_readfirstlane(lds_addr);
  const uint64_t b = (uint64_t)(uintptr_t)sbase;
  // (the builtin returns int: through uint32_t, or the low half is SIGN-extended over the high one)
  const uint32_t blo = (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)b);
  const uint32_t bhi = (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(b >> 32));
  const uint64_t bs = ((uint64_t)bhi << 32) | (uint64_t)blo;
  uint32_t keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\t"
      "s_mov_b32 m0, %3\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %1, %2\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(voff), "s"(bs), "s"(lds_addr)
      : "memory");
}

// The same piece with the non-temporal cache policy: for bytes that ONE CU reads once (the KV stream of a decode
// step): they should not displace what other kernels of the step keep in L2 / Infinity Cache.
__device__ __forceinline__ void lds_dma16_nt(const void* gsrc, uint32_t lds_addr) {
  lds_addr = __builtin_amdgcn_readfirstlane(lds_addr);
  uint32_t keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\t"
      "s_mov_b32 m0, %2\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %1, off nt\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(gsrc), "s"(lds_addr)
      : "memory");
}

__device__ __forceinline__ uint32_t lds_addr_of(const void* p) {
  return (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const char*)p;
}

__device__ __forceinline__ int ceil_div(int a, int b) { return (a + b - 1) / b; }

// float -> float8_e4m3fn exactly as torch's `.to(torch.float8_e4m3fn)` (c10/util/Float8_e4m3fn.h), which is what the
// reference's FP8 KV-pool write runs (memory_pool.py:385-394): round to nearest even, NO saturation -- NaN and every
// value that would round past 448 (|x| > 464) become NaN with the sign kept (0x7f / 0xff), so a numerical fault
// upstream stays visible in the cache instead of being stored as a finite +-448.  Two values -> two bytes.
__device__ __forceinline__ uint32_t e4m3_byte_fix(float x, uint32_t byte) {
  return (fabsf(x) <= 464.0f) ? byte : (0x7fu | ((__float_as_uint(x) >> 24) & 0x80u));
}
__device__ __forceinline__ uint32_t cvt_pk_e4m3_torch(float a, float b) {
  const int pk = __builtin_amdgcn_cvt_pk_fp8_f32(fminf(fmaxf(a, -448.0f), 448.0f), fminf(fmaxf(b, -448.0f), 448.0f), 0, false);
  return e4m3_byte_fix(a, (uint32_t)pk & 0xffu) | (e4m3_byte_fix(b, ((uint32_t)pk >> 8) & 0xffu) << 8);
}

// The same for `--kv-cache-dtype fp8_e5m2` (server_args.py:829-833): torch's .to(torch.float8_e5m2) of a 16-bit value.
// e5m2 is the upper byte of an IEEE half: round to nearest even on the half's bits, overflow goes to +-inf (0x7c / 0xfc,
// no saturation), NaN -> 0x7f | sign.  Exact for every fp16 and every bf16 input (the bf16 -> half step never rounds
// in a way that changes the e5m2 result; checked exhaustively against torch in tests/test_fp8kv_gpu.py).
__device__ __forceinline__ uint32_t cvt_e5m2_torch(float x) {
  const uint32_t h = __builtin_bit_cast(uint16_t, (_Float16)x);
  const uint32_t r = (h + 0x7Fu + ((h >> 8) & 1u)) >> 8;
  return ((h & 0x7FFFu) > 0x7C00u) ? (0x7Fu | ((h >> 8) & 0x80u)) : (r & 0xFFu);
}
__device__ __forceinline__ uint32_t cvt_pk_e5m2_torch(float a, float b) { return cvt_e5m2_torch(a) | (cvt_e5m2_torch(b) << 8); }

// KV-pool byte formats: 1 = e4m3fn, 2 = e5m2 ("bf8" in the ISA).  Two 16-bit-representable values -> two pool bytes.
template <int FMT>
__device__ __forceinline__ uint32_t cvt_pk_kv_torch(float a, float b) {
  if constexpr (FMT == 2) return cvt_pk_e5m2_torch(a, b);
  else return cvt_pk_e4m3_torch(a, b);
}
typedef float sglm_f32x2 __attribute__((ext_vector_type(2)));
// pool bytes -> fp32 (exact), fp32 -> pool bytes in hardware rounding (RNE; callers pass values inside the finite range:
// softmax weights in [0, 1]), and the byte x byte MFMA
template <bool E5, bool HI>
__device__ __forceinline__ sglm_f32x2 cvt_pk_f32_kv(int v) {
  if constexpr (E5) return __builtin_amdgcn_cvt_pk_f32_bf8(v, HI);
  else return __builtin_amdgcn_cvt_pk_f32_fp8(v, HI);
}
template <bool E5, bool HI>
__device__ __forceinline__ int cvt_pk_kv_f32(float a, float b, int old) {
  if constexpr (E5) return __builtin_amdgcn_cvt_pk_bf8_f32(a, b, old, HI);
  else return __builtin_amdgcn_cvt_pk_fp8_f32(a, b, old, HI);
}
template <bool E5>
__device__ __forceinline__ f32x4 mfma_kv8(long a, long b, f32x4 c) {
  if constexpr (E5) return __builtin_amdgcn_mfma_f32_16x16x32_bf8_bf8(a, b, c, 0, 0, 0);
  else return __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(a, b, c, 0, 0, 0);
}

}  // namespace sglm

#define SGLM_CHECK_ARG(cond, ...)            \
  do {                                       \
    if (!(cond)) {                           \
      ::sglm::set_error(__VA_ARGS__);        \
      return SGL_MI355_ERR_INVALID_ARGUMENT; \
    }                                        \
  } while (0)

#define SGLM_CHECK_HIP(expr)                           \
  do {                                                 \
    int _rc = ::sglm::check_hip((expr), #expr);        \
    if (_rc != 0) return _rc;                          \
  } while (0)
