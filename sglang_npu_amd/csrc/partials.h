// Helpers shared by the kernels that consume a split-K GEMM while it is still partial sums (elementwise.hip,
// attention_decode.hip): the fp8_scaled_mm epilogue applied on the fly, and the RoPE rotation every RoPE kernel uses.
#pragma once
#include "common.h"

namespace sglm {

// Source of a row that is still a split-K GEMM in flight (sgl_mi355_fp8_scaled_mm_partials): the consumer applies the
// fp8_scaled_mm epilogue itself -- slices summed in slice order, x w_scale[col], x x_scale[row], + bias, ONE rounding to
// the 16-bit dtype (fp8_gemm_finalize_kernel, gemm_fp8.hip) -- and continues with the rounded value, so the result is
// bit-identical to running the GEMM to completion first.  Saves the finalize launch and one activation round trip.
struct PartialSrc {
  const float* partials;  // [num_slices][M][N] fp32
  int num_slices;
  int64_t slice_stride;   // M * N
  const float* sa;        // x_scale [M]
  const float* sb;        // w_scale [N]
  const void* bias;       // 16-bit [N] or null
  int N;
};

// U slices' loads in flight at a time.  U = 8: the down_proj GEMM of a decode step leaves 6-8 slices, so the whole reduction
// is one memory round trip (a plain slice loop serialises one per slice; four at a time made it two).  U = 4: what the
// launchers pick when there are at most four slices (decode qkv / o_proj: K = 4096 leaves exactly four) -- the eight-wide form
// clamps the slice index, so half of its loads would be duplicates of the last slice queued in front of the real ones.
// U is a template parameter, not a branch in here: a branch per call would put each call's sums between its loads and the
// next call's.  Either U is right for any slice count; the sums always run in slice order, as in fp8_gemm_finalize_kernel.
template <int DTYPE, int U = 8>
__device__ __forceinline__ typename Half16<DTYPE>::x8 gemm_row8(const PartialSrc& ps, int64_t row, int col) {
  using Hh = Half16<DTYPE>;
  static_assert(U == 4 || U == 8, "slice batch of 4 or 8");
  float v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const float* src = ps.partials + row * ps.N + col;
  const float sa = ps.sa[row];
  const f32x4 sb0 = *reinterpret_cast<const f32x4*>(ps.sb + col), sb1 = *reinterpret_cast<const f32x4*>(ps.sb + col + 4);
  for (int s0 = 0; s0 < ps.num_slices; s0 += U) {
    f32x4 a[U], b[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int si = s0 + u < ps.num_slices ? s0 + u : ps.num_slices - 1;
      a[u] = *reinterpret_cast<const f32x4*>(src + si * ps.slice_stride);
      b[u] = *reinterpret_cast<const f32x4*>(src + si * ps.slice_stride + 4);
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (s0 + u < ps.num_slices) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          v[j] += a[u][j];
          v[4 + j] += b[u][j];
        }
      }
  }
  typename Hh::x8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
#pragma clang fp contract(off)  // explicit roundings (no fma contraction): must match fp8_gemm_finalize_kernel bit for bit
    float r = (v[j] * (j < 4 ? sb0[j] : sb1[j - 4])) * sa;
    if (ps.bias) r = r + Hh::to_f32(reinterpret_cast<const typename Hh::T*>(ps.bias)[col + j]);
    o[j] = Hh::from_f32(r);
  }
  return o;
}

// One element, in two halves so that a consumer can issue the loads of all its elements before it uses (or stores) any:
// elem_issue starts the first U slices' loads and the column scale, elem_finish sums in slice order (fetching the slices past
// the first U, if any) and applies the epilogue.  Every load is unconditional (a load under `if` costs a wait right behind it,
// docs/history 4.3.1 c-d), so the caller fetches the bias itself (elem_bias) inside ONE `if (ps.bias)` after all other loads,
// and the row scale ps.sa[row] (one per wave) where it suits its other per-row loads.
template <int U>
struct ElemLoads {
  const float* src;
  float a[U];
  float sb;
};
template <int U>
__device__ __forceinline__ ElemLoads<U> elem_issue(const PartialSrc& ps, int64_t row, int col) {
  static_assert(U == 4 || U == 8, "slice batch of 4 or 8");
  ElemLoads<U> l;
  l.src = ps.partials + row * ps.N + col;
#pragma unroll
  for (int u = 0; u < U; ++u) l.a[u] = l.src[(u < ps.num_slices ? u : ps.num_slices - 1) * ps.slice_stride];
  l.sb = ps.sb[col];
  return l;
}
template <int DTYPE>
__device__ __forceinline__ float elem_bias(const PartialSrc& ps, int col) {  // ps.bias != null
  return Half16<DTYPE>::to_f32(reinterpret_cast<const typename Half16<DTYPE>::T*>(ps.bias)[col]);
}
template <int DTYPE, int U>
__device__ __forceinline__ typename Half16<DTYPE>::T elem_finish(const PartialSrc& ps, const ElemLoads<U>& l, float sa, float bias) {
  using Hh = Half16<DTYPE>;
  float v = 0.f;
#pragma unroll
  for (int u = 0; u < U; ++u)
    if (u < ps.num_slices) v += l.a[u];
  for (int s0 = U; s0 < ps.num_slices; s0 += U) {
    float a[U];
#pragma unroll
    for (int u = 0; u < U; ++u) a[u] = l.src[(s0 + u < ps.num_slices ? s0 + u : ps.num_slices - 1) * ps.slice_stride];
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (s0 + u < ps.num_slices) v += a[u];
  }
  float r;
  {
#pragma clang fp contract(off)
    r = (v * l.sb) * sa;
    if (ps.bias) r = r + bias;
  }
  return Hh::from_f32(r);
}

// One rotation, every product and sum rounded on its own (no fma contraction): the four RoPE kernels below must agree
// bit for bit -- the fused paths are tested against the unfused sequence with torch.equal.
__device__ __forceinline__ void rope_pair(float x1, float x2, float c, float s, float& o1, float& o2) {
#pragma clang fp contract(off)  // __fmul_rn & co. are plain operators in the HIP headers and DO get fused otherwise
  const float a = x1 * c, b = x2 * s, d = x2 * c, e = x1 * s;
  o1 = a - b;
  o2 = d + e;
}

}  // namespace sglm
