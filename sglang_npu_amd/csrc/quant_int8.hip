// Dynamic per-token symmetric INT8 activation quantiser of the w8a8_int8 linear path, MI355X / gfx950.
//
// Replaces:
//   * per_token_quant_int8(x) -> (x_q int8 [T, K], scale fp32 [T, 1])
//       called by W8A8Int8LinearMethod.apply, python/sglang/srt/layers/quantization/w8a8_int8.py:390; the reference imports it
//       from an int8_kernel.py it does not carry -- its only definition in the tree is test/srt/cpu/utils.py:23-31, followed
//       here to the rounding, all in fp32:
//         absmax = max(max_k |x|, 1e-10)      scale = absmax / 127      q = (int8) rint(x * (127 / absmax))
//       both divisions correctly rounded, rint = round half to even (v_rndne_f32).
//
// A byte mover (2 B in, 1 B out per element) with a row-owner shape: one workgroup per token, 16-byte loads, the row kept
// in registers between the absmax reduction (wave shuffle, then four words of LDS) and the 8-byte stores.  Rows longer
// than the registers hold (K > 8192) are read a second time instead.
#include "common.h"

namespace sglm {
namespace {

constexpr int kQThreads = 256;

template <int DTYPE>
__device__ __forceinline__ void load8(const void* base, int64_t elem, float* f) {
  using H = Half16<DTYPE>;
  const typename H::x8 v = *reinterpret_cast<const typename H::x8*>(reinterpret_cast<const typename H::T*>(base) + elem);
#pragma unroll
  for (int j = 0; j < 8; ++j) f[j] = H::to_f32(v[j]);
}

// eight quantised values -> eight bytes; |x * inv| <= 127 (+ one rounding), so the conversion never saturates
__device__ __forceinline__ uint2 quant8(const float* f, float inv) {
  uint32_t w[2] = {0u, 0u};
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int q = (int)rintf(__fmul_rn(f[j], inv));
    w[j >> 2] |= ((uint32_t)q & 0xffu) << (8 * (j & 3));
  }
  return uint2{w[0], w[1]};
}

// VPL > 0: 8-element vectors per thread held in registers (K <= 2048 VPL); VPL == 0: any K, the row is read twice
template <int DTYPE, int VPL>
__global__ __launch_bounds__(kQThreads) void per_token_quant_int8_kernel(const void* __restrict__ x, int8_t* __restrict__ q,
                                                                         float* __restrict__ s, int K) {
  __shared__ float red[kQThreads / 64];
  const int64_t row = blockIdx.x;
  const int nvec = K >> 3;
  constexpr int HELD = VPL > 0 ? VPL : 1;
  float v[HELD][8];
  float amax = 1e-10f;  // the reference's clamp_min
  if constexpr (VPL > 0) {
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      const int vi = threadIdx.x + kQThreads * i;
      if (vi < nvec) {
        load8<DTYPE>(x, row * K + 8 * vi, v[i]);
#pragma unroll
        for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(v[i][j]));
      }
    }
  } else {
    for (int vi = threadIdx.x; vi < nvec; vi += kQThreads) {
      load8<DTYPE>(x, row * K + 8 * vi, v[0]);
#pragma unroll
      for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(v[0][j]));
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) amax = fmaxf(amax, __shfl_xor(amax, off));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = amax;
  __syncthreads();
  amax = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  if (threadIdx.x == 0) s[row] = __fdiv_rn(amax, 127.0f);
  const float inv = __fdiv_rn(127.0f, amax);
  if constexpr (VPL > 0) {
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      const int vi = threadIdx.x + kQThreads * i;
      if (vi < nvec) *reinterpret_cast<uint2*>(q + row * K + 8 * vi) = quant8(v[i], inv);
    }
  } else {
    for (int vi = threadIdx.x; vi < nvec; vi += kQThreads) {
      load8<DTYPE>(x, row * K + 8 * vi, v[0]);
      *reinterpret_cast<uint2*>(q + row * K + 8 * vi) = quant8(v[0], inv);
    }
  }
}

template <int DTYPE>
int launch_quant(const void* x, void* q, float* s, int64_t T, int K, hipStream_t st) {
  const int vpl = (K / 8 + kQThreads - 1) / kQThreads;
#define QK(V)                                                                                                           \
  hipLaunchKernelGGL((per_token_quant_int8_kernel<DTYPE, V>), dim3((unsigned)T), dim3(kQThreads), 0, st, x, (int8_t*)q, s, K)
  if (vpl <= 1) QK(1);
  else if (vpl <= 2) QK(2);
  else if (vpl <= 4) QK(4);
  else QK(0);
#undef QK
  return check_hip(hipGetLastError(), "per_token_quant_int8 launch");
}

}  // namespace
}  // namespace sglm

using namespace sglm;

extern "C" int sgl_mi355_per_token_quant_int8(const void* input, void* output_q, float* output_s, int64_t num_tokens,
                                              int64_t hidden_dim, int dtype, void* stream) {
  SGLM_CHECK_ARG(dtype == SGL_MI355_BF16 || dtype == SGL_MI355_FP16, "per_token_quant_int8: input must be Half or BFloat16");
  SGLM_CHECK_ARG(num_tokens >= 0 && num_tokens < (1ll << 31) && hidden_dim > 0 && hidden_dim < (1ll << 31),
                 "per_token_quant_int8: bad shape");
  SGLM_CHECK_ARG(hidden_dim % 16 == 0, "per_token_quant_int8: hidden_dim %% 16 == 0 required (got %ld)", (long)hidden_dim);
  if (num_tokens == 0) return 0;
  SGLM_CHECK_ARG(input && output_q && output_s, "per_token_quant_int8: null tensor pointer");
  SGLM_CHECK_ARG(((uintptr_t)input & 15) == 0 && ((uintptr_t)output_q & 7) == 0, "per_token_quant_int8: unaligned tensor");
  hipStream_t st = as_stream(stream);
  return dtype == SGL_MI355_BF16 ? launch_quant<SGL_MI355_BF16>(input, output_q, output_s, num_tokens, (int)hidden_dim, st)
                                 : launch_quant<SGL_MI355_FP16>(input, output_q, output_s, num_tokens, (int)hidden_dim, st);
}
