// NVFP4 weight-only linear for MI355X / gfx950 (`petit_nvfp4`): e2m1 weights, one e4m3 scale per 16 k, one fp32 global scale,
// 16-bit activations, fp32 accumulation.
//
// Replaces:
//   * petit_kernel.repack_nvfp4 / process_nvfp4_scales / mul_nvfp4_a16 (an external package, written for gfx90a / gfx942) as
//     called by prepare_nvfp4_layer_for_petit and apply_petit_nvfp4_linear
//       python/sglang/srt/layers/quantization/petit_utils.py:61-104
//   reached from PetitNvFp4LinearMethod (python/sglang/srt/layers/quantization/petit.py:134-252).
//
//   W[n][k] = e2m1(weight[n][k]) * float(weight_scale[n][k / 16])      exact in fp16 AND in bf16: at most 6 significant
//                                                                      bits, |W| <= 6 * 448, smallest non-zero 2^-10
//   acc     = sum_k x[m][k] W[n][k]                                    fp32, the whole K range
//   r       = round16(fl32(weight_scale_2 * acc))
//   out     = bias ? round16(fl32(r) + fl32(bias[n])) : r              the reference's output.add_(bias): AFTER the rounding
//
// Because W is exact in the activation type, the hot kernels dequantise in registers to that type and feed the 16-bit
// MFMA; weight_scale_2 is applied once, in fp32, in the epilogue.  Dequantisation of one dword (8 codes, k ascending from
// the low nibble) is four v_cvt_scalef32_pk_{f16,f32}_fp4 with the scale operand 1.0 -- that operand is an E8M0 scale, only
// the exponent of the float is used, so it cannot carry the e4m3 scale's mantissa -- each followed by a multiply with the
// group scale: v_pk_mul_f16 for fp16 (8 VALU per dword, 32 per 128-k step and column block = 8 per MFMA at 16 rows);
// bf16 has no packed multiply, so it goes through fp32 pairs: v_cvt_scalef32_pk_f32_fp4, v_pk_mul_f32, v_cvt_pk_bf16_f32
// (12 VALU per dword, 48 per step = 12 per MFMA at 16 rows).
//
// Prepared layout (nvfp4_repack; N % 16 == 0, K % 128 == 0).  Per 16-column block nb the checkpoint's [16 rows][K / 32
// units] is transposed to [K / 32 units][16 rows], a unit being 32 consecutive k of one row:
//   weight byte of (n, k):  ((nb * (K / 32) + k / 32) * 16 + n % 16) * 16 + (k % 32) / 2       nb = n / 16
//   scale  byte of (n, k):  ((nb * (K / 32) + k / 32) * 16 + n % 16) * 2  + (k % 32) / 16
// One 128-k step of a block is then a contiguous 1-KiB weight piece and a 128-byte scale piece in which lane
// (n = lane % 16, q = lane / 16) owns 16 bytes at lane * 16 -- the four dwords k = 128 s + 32 q + 8 j .. + 7, j = 0..3 --
// and the two scales of exactly those 32 k at lane * 2: one global_load_dwordx4 and one global_load_ushort per lane, no
// scale is stored twice (0.5625 B per weight).  The MFMAs run with the WEIGHT as the A operand: MFMA j of a step takes
// dword j, i.e. its k slot (q, e) is the actual k = 128 s + 32 q + 8 j + e, and the activation operand is read from LDS at
// the same k (any bijection between slots and k is a valid dot product).  A lane's four accumulators are token lane % 16 x
// columns 4 (lane / 16) .. + 3, as in gemm_int8.hip: one 8-byte store.
//
//   * M <= 64: `nvfp4_stream`.  A workgroup stages its K slice of the activations row-major in LDS (rows padded by 16
//     bytes); each of its eight waves owns 16-column blocks and pulls their weight and scale pieces global -> VGPR with
//     non-temporal loads, the whole slice (8 KiB + 1 KiB per wave) in flight, the first block's before the staging
//     barrier; no LDS and no barrier for weights.  K is cut into slices of 1024: one slice runs the epilogue, more leave
//     fp32 slabs workspace[slice][M][N] that `nvfp4_finalize` sums in slice order.
//   * M > 64: `nvfp4_tiled`, 128 x 128 tiles, four waves of 64 x 64, k-step 128.  A wave loads its four weight pieces and
//     scale pieces of the NEXT k-step into VGPRs while the 64 MFMAs of this one run and dequantises each dword right into
//     an MFMA operand: no 16-bit copy of the weight exists anywhere.  Activations go register-staged through
//     double-buffered LDS in the fragment order, one barrier per k-step.
//   * `nvfp4_generic`: the checkpoint layout, any N, any K % 16 == 0, any M.  One wave per column and eight rows, lanes
//     split K, fp32 FMA on the VALU, a wave reduction, the same epilogue.  It exists so that no shape falls back to torch;
//     it is not tuned.
#include "common.h"

namespace sglm {
namespace {

struct Nvfp4Args {
  const void* x;
  int64_t x_sm;  // elements between rows of x
  const uint8_t* w;
  const uint8_t* ws;
  const float* ws2;  // device scalar
  const void* bias;
  void* out;
  float* slabs;  // streamer, split-K: [slices][M][N] fp32
  int M, N, K;
  int blocks_per_wg;  // streamer: 16-column blocks per workgroup (blockIdx.x)
};

thread_local const char* g_nvfp4_last_kernel = "";

typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

// e2m1 -> 16 bit.  S is a group scale in the form the multiply wants it; pair() turns the two e4m3 bytes of a 32-k unit
// into two of them; deq() is one dword -> the eight values of an MFMA operand (exact, see the header).
template <int DTYPE>
struct Dq;

template <>
struct Dq<SGL_MI355_FP16> {
  using S = f16x2;
  static __device__ __forceinline__ void pair(uint32_t two_e4m3, S& lo, S& hi) {
    const sglm_f32x2 s = __builtin_amdgcn_cvt_pk_f32_fp8((int)two_e4m3, false);
    lo = S{(_Float16)s[0], (_Float16)s[0]};
    hi = S{(_Float16)s[1], (_Float16)s[1]};
  }
  static __device__ __forceinline__ f16x8 deq(uint32_t w, S s) {
    const f16x2 p0 = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, 1.0f, 0) * s;
    const f16x2 p1 = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, 1.0f, 1) * s;
    const f16x2 p2 = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, 1.0f, 2) * s;
    const f16x2 p3 = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, 1.0f, 3) * s;
    return f16x8{p0[0], p0[1], p1[0], p1[1], p2[0], p2[1], p3[0], p3[1]};
  }
};

template <>
struct Dq<SGL_MI355_BF16> {
  using S = float;
  static __device__ __forceinline__ void pair(uint32_t two_e4m3, S& lo, S& hi) {
    const sglm_f32x2 s = __builtin_amdgcn_cvt_pk_f32_fp8((int)two_e4m3, false);
    lo = s[0];
    hi = s[1];
  }
  static __device__ __forceinline__ bf16x8 deq(uint32_t w, S s) {
    const sglm_f32x2 p0 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, 1.0f, 0) * s;
    const sglm_f32x2 p1 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, 1.0f, 1) * s;
    const sglm_f32x2 p2 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, 1.0f, 2) * s;
    const sglm_f32x2 p3 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, 1.0f, 3) * s;
    return bf16x8{(__bf16)p0[0], (__bf16)p0[1], (__bf16)p1[0], (__bf16)p1[1],
                  (__bf16)p2[0], (__bf16)p2[1], (__bf16)p3[0], (__bf16)p3[1]};
  }
};

// the epilogue of the header comment for columns n .. n + 3 of one token; every operation rounds on its own
template <int DTYPE>
__device__ __forceinline__ typename Half16<DTYPE>::x4 finish4(f32x4 acc, float ws2, const void* bias, int n) {
  using H = Half16<DTYPE>;
  typename H::x4 o;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    typename H::T h = H::from_f32(__fmul_rn(acc[r], ws2));
    if (bias) h = H::from_f32(__fadd_rn(H::to_f32(h), H::to_f32(reinterpret_cast<const typename H::T*>(bias)[n + r])));
    o[r] = h;
  }
  return o;
}

// ------------------------------------------------------------------------------------------
// nvfp4_repack: the transpose of the header comment on units of 16 bytes (weights) and 2 bytes (scales).
template <typename U>
__global__ __launch_bounds__(256) void nvfp4_repack_kernel(const U* __restrict__ in, U* __restrict__ out, int64_t total,
                                                           int units_per_row, int inverse) {
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
    const int n = (int)(t & 15);
    const int64_t bu = t >> 4, nb = bu / units_per_row, u = bu - nb * units_per_row;
    const int64_t r = (nb * 16 + n) * units_per_row + u;  // the same unit in the checkpoint layout
    if (inverse) out[r] = in[t];
    else out[t] = in[r];
  }
}

// ------------------------------------------------------------------------------------------
// weight streamer: M <= 16 MB rows.  grid (column-block groups, K slices), 8 waves.
// Neither number below is a tuned crossover: 64 rows x (2 x 1024 + 16) bytes = 129 KiB is what one workgroup can stage
// of the CU's 160 KiB of LDS, so the streamer ends at 64 rows and a K slice at 1024.
constexpr int kStreamWaves = 8;
constexpr int kStreamMaxRows = 64;
constexpr int kSliceK = 1024;
constexpr int kSliceSteps = kSliceK / 128;  // weight pieces per block and slice: all in flight
// LDS row stride = slice bytes + 16: a multiple of 256 bytes plus 16, so the 16 tokens x 16 bytes that one lane group
// reads with ds_read_b128 fall on 16 different groups of four banks
constexpr int kRowPad = 16;

template <int DTYPE, int MB, bool DIRECT>
__global__ __launch_bounds__(64 * kStreamWaves) void nvfp4_stream_kernel(Nvfp4Args p) {
  using H = Half16<DTYPE>;
  using D = Dq<DTYPE>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int R = 16 * MB;
  constexpr int NT = 64 * kStreamWaves;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r16 = lane & 15, g = lane >> 4;
  const int slice = blockIdx.y;
  const int k0 = slice * kSliceK;
  const int klen = p.K - k0 < kSliceK ? p.K - k0 : kSliceK;
  const int ns = klen >> 7;  // 128-k steps of this slice (K % 128 == 0)
  const int row_stride = klen * 2 + kRowPad;
  const int64_t ksteps = p.K >> 7;

  const int nblocks = p.N >> 4;
  const int nb_begin = blockIdx.x * p.blocks_per_wg;
  const int nb_end = nb_begin + p.blocks_per_wg < nblocks ? nb_begin + p.blocks_per_wg : nblocks;

  // piece i of block nb: this lane's 16 weight bytes and 2 scale bytes of step i of the slice (64-bit offsets: a weight
  // may be larger than 2 GiB).  A step beyond the slice re-reads its last one and is never consumed.
  i32x4 q[kSliceSteps];
  uint32_t sc[kSliceSteps];
  auto fetch = [&](int nb, int i) __attribute__((always_inline)) {
    const int64_t piece = (int64_t)nb * ksteps + (k0 >> 7) + (i < ns ? i : ns - 1);
    q[i] = __builtin_nontemporal_load(reinterpret_cast<const i32x4*>(p.w + piece * 1024 + lane * 16));
    sc[i] = __builtin_nontemporal_load(reinterpret_cast<const uint16_t*>(p.ws + piece * 128 + lane * 2));
  };
  int nb = nb_begin + wave;
  if (nb < nb_end) {
#pragma unroll
    for (int i = 0; i < kSliceSteps; ++i) fetch(nb, i);
  }

  // rows beyond M are staged as zeros: they reach accumulators that are never stored
  const int chunks = ns * 16;  // 16-byte pieces per row
  for (int i = tid; i < R * chunks; i += NT) {
    const int m = i / chunks, c = i - m * chunks;
    i32x4 v = i32x4{0, 0, 0, 0};
    if (m < p.M) v = *reinterpret_cast<const i32x4*>(reinterpret_cast<const char*>(p.x) + ((int64_t)m * p.x_sm + k0 + c * 8) * 2);
    *reinterpret_cast<i32x4*>(smem + m * row_stride + c * 16) = v;
  }
  __syncthreads();

  const char* abase = smem + r16 * row_stride + g * 64;  // token r16, k = 32 g of a step
  const float ws2 = *p.ws2;
  for (; nb < nb_end; nb += kStreamWaves) {
    const bool more = nb + kStreamWaves < nb_end;  // wave-uniform
    f32x4 acc[MB];
#pragma unroll
    for (int mi = 0; mi < MB; ++mi) acc[mi] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < kSliceSteps; ++i) {
      const i32x4 w = q[i];
      const uint32_t s = sc[i];
      if (more) fetch(nb + kStreamWaves, i);  // the next block's piece takes the registers just freed
      if (i < ns) {
        typename D::S slo, shi;
        D::pair(s, slo, shi);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const typename H::x8 wf = D::deq((uint32_t)w[j], j < 2 ? slo : shi);
#pragma unroll
          for (int mi = 0; mi < MB; ++mi)
            acc[mi] = H::mfma16(wf, *reinterpret_cast<const typename H::x8*>(abase + 16 * mi * row_stride + i * 256 + j * 16),
                                acc[mi]);
        }
      }
    }
    // acc[mi][r] = C[token 16 mi + r16][column 16 nb + 4 g + r]
    const int n = nb * 16 + 4 * g;
#pragma unroll
    for (int mi = 0; mi < MB; ++mi) {
      const int m = 16 * mi + r16;
      if (m < p.M) {
        if constexpr (DIRECT) {
          *reinterpret_cast<typename H::x4*>(reinterpret_cast<typename H::T*>(p.out) + (int64_t)m * p.N + n) =
              finish4<DTYPE>(acc[mi], ws2, p.bias, n);
        } else {
          *reinterpret_cast<f32x4*>(p.slabs + ((int64_t)slice * p.M + m) * p.N + n) = acc[mi];
        }
      }
    }
  }
}

// completion of the split-K streamer: the slices are summed in fp32, in slice order, then the one epilogue
template <int DTYPE>
__global__ __launch_bounds__(256) void nvfp4_finalize_kernel(const float* __restrict__ slabs, int SK, int64_t MN, int N,
                                                             const float* __restrict__ ws2, const void* bias, void* out) {
  using H = Half16<DTYPE>;
  const int64_t total = MN >> 2;
  const float s2 = *ws2;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    f32x4 v = *reinterpret_cast<const f32x4*>(slabs + i * 4);
    for (int s = 1; s < SK; ++s) v += *reinterpret_cast<const f32x4*>(slabs + s * MN + i * 4);
    const int n = (int)((i * 4) % N);  // N % 16 == 0: the four columns share a row
    *reinterpret_cast<typename H::x4*>(reinterpret_cast<typename H::T*>(out) + i * 4) = finish4<DTYPE>(v, s2, bias, n);
  }
}

// ------------------------------------------------------------------------------------------
// tiles: 128 x 128 outputs, k-step 128, four waves as 2 x 2, each 64 x 64 = 4 x 4 fragments.
// LDS image of an activation tile: [16-row block rb][j][q][r16][16 B] = 8 x 4 KiB, so that the operand of MFMA j for row
// block rb is one conflict-free 1-KiB read at rb * 4096 + j * 1024 + lane * 16 holding k = 32 q + 8 j .. + 7 of token r16:
// the k order of the weight pieces.
constexpr int kTileStage = 8 * 4096;

template <int DTYPE>
__global__ __launch_bounds__(256) void nvfp4_tiled_kernel(Nvfp4Args p) {
  using H = Half16<DTYPE>;
  using D = Dq<DTYPE>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int r16 = lane & 15, g = lane >> 4;
  const int tiles_m = (p.M + 127) >> 7;
  // M fastest: the workgroups of a column panel of W run together and share it in L2
  const int m0 = ((int)blockIdx.x % tiles_m) << 7, n0 = ((int)blockIdx.x / tiles_m) << 7;
  const int ksteps = p.K >> 7;

  // staging map: thread t moves, for i = 0..7, the 16 bytes k = 8 c .. 8 c + 7 (c = t % 16) of row 16 i + t / 16: a row's
  // 256 bytes are read by 16 neighbouring lanes.  c = 4 q + j.  Rows past M re-read the last one, never stored.
  const int c = tid & 15, srow = tid >> 4;
  const int lds_off = (c & 3) * 1024 + ((c >> 2) * 16 + srow) * 16;
  const char* a_ptr[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int row = m0 + 16 * i + srow;
    a_ptr[i] = reinterpret_cast<const char*>(p.x) + ((int64_t)(row < p.M ? row : p.M - 1) * p.x_sm + 8 * c) * 2;
  }
  // the wave's four column blocks (a block past N shadows the last one, never stored)
  const uint8_t* w_ptr[4];
  const uint8_t* s_ptr[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int nb = (n0 >> 4) + wn * 4 + i < (p.N >> 4) ? (n0 >> 4) + wn * 4 + i : (p.N >> 4) - 1;
    w_ptr[i] = p.w + (int64_t)nb * ksteps * 1024 + lane * 16;
    s_ptr[i] = p.ws + (int64_t)nb * ksteps * 128 + lane * 2;
  }

  i32x4 ra[8];
  auto gload = [&](int ks) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < 8; ++i) ra[i] = *reinterpret_cast<const i32x4*>(a_ptr[i] + (int64_t)ks * 256);
  };
  auto lstore = [&](int stage) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < 8; ++i) *reinterpret_cast<i32x4*>(smem + stage * kTileStage + i * 4096 + lds_off) = ra[i];
  };
  auto wload = [&](int ks, i32x4 (&w)[4], uint32_t (&s)[4]) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      w[i] = *reinterpret_cast<const i32x4*>(w_ptr[i] + (int64_t)ks * 1024);
      s[i] = *reinterpret_cast<const uint16_t*>(s_ptr[i] + (int64_t)ks * 128);
    }
  };

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // one k-step: the next step's global loads are issued first and land under this step's 64 MFMAs (the last step re-reads
  // itself into the idle stage: branch-free, so that the staging registers stay registers)
  auto step = [&](int kt, i32x4 (&wc)[4], uint32_t (&sc)[4], i32x4 (&wnext)[4], uint32_t (&snext)[4]) __attribute__((always_inline)) {
    const int st = kt & 1;
    const int nxt = kt + 1 < ksteps ? kt + 1 : kt;
    gload(nxt);
    wload(nxt, wnext, snext);
    const char* sA = smem + st * kTileStage + wm * 4 * 4096 + lane * 16;
    typename D::S slo[4], shi[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) D::pair(sc[i], slo[i], shi[i]);
#pragma unroll
    for (int j = 0; j < 4; ++j) {  // MFMA j of the step: dword j of every piece
      typename H::x8 af[4];
#pragma unroll
      for (int rb = 0; rb < 4; ++rb) af[rb] = *reinterpret_cast<const typename H::x8*>(sA + rb * 4096 + j * 1024);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const typename H::x8 wf = D::deq((uint32_t)wc[i][j], j < 2 ? slo[i] : shi[i]);
#pragma unroll
        for (int rb = 0; rb < 4; ++rb) acc[i][rb] = H::mfma16(wf, af[rb], acc[i][rb]);
      }
    }
    lstore(st ^ 1);
    __syncthreads();
  };

  i32x4 w0[4], w1[4];
  uint32_t s0[4], s1[4];
  gload(0);
  lstore(0);
  wload(0, w0, s0);
  __syncthreads();
  for (int kt = 0; kt < ksteps; kt += 2) {
    step(kt, w0, s0, w1, s1);
    if (kt + 1 < ksteps) step(kt + 1, w1, s1, w0, s0);
  }

  // acc[i][rb][r] = C[m0 + 64 wm + 16 rb + r16][n0 + 64 wn + 16 i + 4 g + r]; N % 16 == 0: a lane's columns are all in or out
  const float ws2 = *p.ws2;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int n = n0 + wn * 64 + 16 * i + 4 * g;
    if (n < p.N) {
#pragma unroll
      for (int rb = 0; rb < 4; ++rb) {
        const int m = m0 + wm * 64 + 16 * rb + r16;
        if (m < p.M)
          *reinterpret_cast<typename H::x4*>(reinterpret_cast<typename H::T*>(p.out) + (int64_t)m * p.N + n) =
              finish4<DTYPE>(acc[i][rb], ws2, p.bias, n);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------
// generic: the checkpoint layout.  A workgroup is four waves = four columns x eight rows; lane l of a wave takes the
// dwords l, l + 64, ... of its column's weight row (8 k each) and the rows' matching 16 bytes, all in fp32 on the VALU.
constexpr int kGenericRows = 8;

template <int DTYPE>
__global__ __launch_bounds__(256) void nvfp4_generic_kernel(Nvfp4Args p, int col_groups) {
  using H = Half16<DTYPE>;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int n = ((int)blockIdx.x % col_groups) * 4 + wave;
  const int m0 = ((int)blockIdx.x / col_groups) * kGenericRows;
  if (n >= p.N) return;
  const uint32_t* wrow = reinterpret_cast<const uint32_t*>(p.w + (int64_t)n * (p.K >> 1));
  const uint8_t* srow = p.ws + (int64_t)n * (p.K >> 4);
  float acc[kGenericRows];
#pragma unroll
  for (int r = 0; r < kGenericRows; ++r) acc[r] = 0.f;
  for (int c = lane; c < (p.K >> 3); c += 64) {
    const uint32_t w = wrow[c];
    const float s = __builtin_amdgcn_cvt_pk_f32_fp8((int)srow[c >> 1], false)[0];
    const sglm_f32x2 p0 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, 1.0f, 0) * s;
    const sglm_f32x2 p1 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, 1.0f, 1) * s;
    const sglm_f32x2 p2 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, 1.0f, 2) * s;
    const sglm_f32x2 p3 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, 1.0f, 3) * s;
    const float wv[8] = {p0[0], p0[1], p1[0], p1[1], p2[0], p2[1], p3[0], p3[1]};
#pragma unroll
    for (int r = 0; r < kGenericRows; ++r) {
      if (m0 + r < p.M) {  // wave-uniform
        const typename H::x8 xv = *reinterpret_cast<const typename H::x8*>(
            reinterpret_cast<const char*>(p.x) + ((int64_t)(m0 + r) * p.x_sm + 8 * c) * 2);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[r] = fmaf(H::to_f32(xv[e]), wv[e], acc[r]);
      }
    }
  }
  const float ws2 = *p.ws2;
#pragma unroll
  for (int r = 0; r < kGenericRows; ++r) {
    float v = acc[r];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if (lane == 0 && m0 + r < p.M) {
      typename H::T h = H::from_f32(__fmul_rn(v, ws2));
      if (p.bias) h = H::from_f32(__fadd_rn(H::to_f32(h), H::to_f32(reinterpret_cast<const typename H::T*>(p.bias)[n])));
      reinterpret_cast<typename H::T*>(p.out)[(int64_t)(m0 + r) * p.N + n] = h;
    }
  }
}

// ------------------------------------------------------------------------------------------
inline int stream_slices(int64_t K) { return (int)((K + kSliceK - 1) / kSliceK); }

template <int DTYPE, int MB>
int launch_stream(Nvfp4Args p, float* ws, int64_t ws_floats, hipStream_t s) {
  const int SK = stream_slices(p.K);
  SGLM_CHECK_ARG(SK == 1 || (ws != nullptr && ws_floats >= (int64_t)SK * p.M * p.N),
                 "nvfp4_gemm: workspace of %ld floats required for %d K slices (got %ld)", (long)((int64_t)SK * p.M * p.N), SK,
                 (long)(ws ? ws_floats : 0));
  p.slabs = ws;
  // one 16-column block per wave, more where that would be more workgroups than 1024 (four rounds of the chip).  A narrow
  // layer leaves CUs idle: N = 4096, K = 4096 is 32 x 4 = 128 workgroups on 256 CUs.
  const int nblocks = p.N >> 4;
  p.blocks_per_wg = kStreamWaves;
  while ((int64_t)((nblocks + p.blocks_per_wg - 1) / p.blocks_per_wg) * SK > 1024) p.blocks_per_wg *= 2;
  constexpr int kMaxLds = 16 * MB * (kSliceK * 2 + kRowPad);
  const int klen = p.K < kSliceK ? p.K : kSliceK;
  const int lds = 16 * MB * (klen * 2 + kRowPad);
  static int attr_rc = [] {
    int rc = check_hip(hipFuncSetAttribute(reinterpret_cast<const void*>(nvfp4_stream_kernel<DTYPE, MB, true>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLds),
                       "hipFuncSetAttribute");
    return rc ? rc
              : check_hip(hipFuncSetAttribute(reinterpret_cast<const void*>(nvfp4_stream_kernel<DTYPE, MB, false>),
                                              hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLds),
                          "hipFuncSetAttribute");
  }();
  if (attr_rc) return attr_rc;
  g_nvfp4_last_kernel = "nvfp4_stream";
  const dim3 grid((unsigned)((nblocks + p.blocks_per_wg - 1) / p.blocks_per_wg), (unsigned)SK);
  if (SK == 1) {
    hipLaunchKernelGGL((nvfp4_stream_kernel<DTYPE, MB, true>), grid, dim3(64 * kStreamWaves), lds, s, p);
    return check_hip(hipGetLastError(), "nvfp4_stream launch");
  }
  hipLaunchKernelGGL((nvfp4_stream_kernel<DTYPE, MB, false>), grid, dim3(64 * kStreamWaves), lds, s, p);
  int rc = check_hip(hipGetLastError(), "nvfp4_stream launch");
  if (rc) return rc;
  const int64_t MN = (int64_t)p.M * p.N;
  hipLaunchKernelGGL((nvfp4_finalize_kernel<DTYPE>), dim3((unsigned)((MN / 4 + 255) / 256)), dim3(256), 0, s, (const float*)ws,
                     SK, MN, p.N, p.ws2, p.bias, p.out);
  return check_hip(hipGetLastError(), "nvfp4_finalize launch");
}

// The form is picked on the host.  The thresholds are NOT tuned crossovers: 64 rows is the streamer's LDS capacity, and
// above it only the tiled kernel reads the prepared layout.
template <int DTYPE>
int launch_nvfp4(const Nvfp4Args& p, int prepared, float* ws, int64_t ws_floats, hipStream_t s) {
  if (!prepared) {
    const int col_groups = (p.N + 3) >> 2;
    const int64_t wgs = (int64_t)col_groups * ((p.M + kGenericRows - 1) / kGenericRows);
    SGLM_CHECK_ARG(wgs < (1ll << 31), "nvfp4_gemm: M x N of %d x %d has too many workgroups", p.M, p.N);
    g_nvfp4_last_kernel = "nvfp4_generic";
    hipLaunchKernelGGL((nvfp4_generic_kernel<DTYPE>), dim3((unsigned)wgs), dim3(256), 0, s, p, col_groups);
    return check_hip(hipGetLastError(), "nvfp4_generic launch");
  }
  if (p.M <= 16) return launch_stream<DTYPE, 1>(p, ws, ws_floats, s);
  if (p.M <= 32) return launch_stream<DTYPE, 2>(p, ws, ws_floats, s);
  if (p.M <= kStreamMaxRows) return launch_stream<DTYPE, 4>(p, ws, ws_floats, s);
  const int64_t tiles = (int64_t)((p.M + 127) >> 7) * ((p.N + 127) >> 7);
  SGLM_CHECK_ARG(tiles < (1ll << 31), "nvfp4_gemm: M x N of %d x %d has too many tiles", p.M, p.N);
  constexpr int lds = 2 * kTileStage;
  static int attr_rc = check_hip(hipFuncSetAttribute(reinterpret_cast<const void*>(nvfp4_tiled_kernel<DTYPE>),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, lds),
                                 "hipFuncSetAttribute");
  if (attr_rc) return attr_rc;
  g_nvfp4_last_kernel = "nvfp4_tiled";
  hipLaunchKernelGGL((nvfp4_tiled_kernel<DTYPE>), dim3((unsigned)tiles), dim3(256), lds, s, p);
  return check_hip(hipGetLastError(), "nvfp4_tiled launch");
}

inline bool has_prepared_form(int64_t N, int64_t K) { return N > 0 && K > 0 && N % 16 == 0 && K % 128 == 0; }

}  // namespace
}  // namespace sglm

using namespace sglm;

extern "C" int sgl_mi355_nvfp4_repack(const void* weight, const void* weight_scale, void* weight_out, void* scale_out,
                                      int64_t N, int64_t K, int inverse, void* stream) {
  SGLM_CHECK_ARG(N > 0 && K > 0 && N < (1ll << 31) && K < (1ll << 31), "nvfp4_repack: bad shape");
  if (!has_prepared_form(N, K)) {
    set_error("nvfp4_repack: the prepared layout needs N %% 16 == 0 and K %% 128 == 0 (N=%ld K=%ld)", (long)N, (long)K);
    return SGL_MI355_ERR_UNSUPPORTED;
  }
  SGLM_CHECK_ARG(weight && weight_scale && weight_out && scale_out, "nvfp4_repack: null tensor pointer");
  SGLM_CHECK_ARG(weight != weight_out && weight_scale != scale_out, "nvfp4_repack: cannot run in place");
  SGLM_CHECK_ARG(reinterpret_cast<uintptr_t>(weight) % 16 == 0 && reinterpret_cast<uintptr_t>(weight_out) % 16 == 0 &&
                     reinterpret_cast<uintptr_t>(weight_scale) % 2 == 0 && reinterpret_cast<uintptr_t>(scale_out) % 2 == 0,
                 "nvfp4_repack: weights must be 16-byte aligned and scales 2-byte aligned");
  hipStream_t s = as_stream(stream);
  const int64_t total = N * (K / 32);  // units of either tensor
  const unsigned grid = (unsigned)((total + 255) / 256 < 65536 ? (total + 255) / 256 : 65536);
  hipLaunchKernelGGL((nvfp4_repack_kernel<i32x4>), dim3(grid), dim3(256), 0, s, (const i32x4*)weight, (i32x4*)weight_out, total,
                     (int)(K / 32), inverse);
  int rc = check_hip(hipGetLastError(), "nvfp4_repack launch");
  if (rc) return rc;
  hipLaunchKernelGGL((nvfp4_repack_kernel<uint16_t>), dim3(grid), dim3(256), 0, s, (const uint16_t*)weight_scale,
                     (uint16_t*)scale_out, total, (int)(K / 32), inverse);
  return check_hip(hipGetLastError(), "nvfp4_repack launch");
}

extern "C" int sgl_mi355_nvfp4_gemm(const void* x, const void* weight, const void* weight_scale, const float* weight_scale_2,
                                    const void* bias, void* out, float* workspace, int64_t workspace_floats, int64_t M,
                                    int64_t N, int64_t K, int64_t x_stride_m, int prepared, int dtype, void* stream) {
  SGLM_CHECK_ARG(dtype == SGL_MI355_BF16 || dtype == SGL_MI355_FP16, "nvfp4_gemm: activations must be Half or BFloat16");
  SGLM_CHECK_ARG(M >= 0 && N > 0 && K > 0 && M < (1ll << 31) && N < (1ll << 31) && K < (1ll << 31), "nvfp4_gemm: bad shape");
  SGLM_CHECK_ARG(K % 16 == 0, "Unsupported model when in features size is not multiple of 16");
  SGLM_CHECK_ARG(!prepared || has_prepared_form(N, K),
                 "nvfp4_gemm: the prepared layout needs N %% 16 == 0 and K %% 128 == 0 (N=%ld K=%ld)", (long)N, (long)K);
  SGLM_CHECK_ARG(x_stride_m >= K && x_stride_m % 8 == 0, "nvfp4_gemm: x rows must be >= K apart and 16-byte aligned");
  if (M == 0) return 0;
  SGLM_CHECK_ARG(x && weight && weight_scale && weight_scale_2 && out, "nvfp4_gemm: null tensor pointer");
  SGLM_CHECK_ARG(reinterpret_cast<uintptr_t>(x) % 16 == 0 && reinterpret_cast<uintptr_t>(weight) % 16 == 0 &&
                     reinterpret_cast<uintptr_t>(weight_scale) % 2 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0 &&
                     reinterpret_cast<uintptr_t>(workspace) % 16 == 0 && reinterpret_cast<uintptr_t>(bias) % 2 == 0,
                 "nvfp4_gemm: operands must be 16-byte aligned");
  Nvfp4Args p{x, x_stride_m, (const uint8_t*)weight, (const uint8_t*)weight_scale, weight_scale_2, bias, out, nullptr,
              (int)M, (int)N, (int)K, 0};
  hipStream_t s = as_stream(stream);
  return dtype == SGL_MI355_BF16 ? launch_nvfp4<SGL_MI355_BF16>(p, prepared, workspace, workspace_floats, s)
                                 : launch_nvfp4<SGL_MI355_FP16>(p, prepared, workspace, workspace_floats, s);
}

extern "C" const char* sgl_mi355_nvfp4_last_kernel(void) { return g_nvfp4_last_kernel; }
