// W8A8 INT8 GEMM for MI355X / gfx950: per-token activation scales, per-channel weight scales, int32 accumulation.
//
// Replaces:
//   * int8_scaled_mm(mat_a, mat_b, scales_a, scales_b, out_dtype, bias) -> Tensor
//       schema sgl-kernel/csrc/common_extension.cc:102-104, checks and dispatch sgl-kernel/csrc/gemm/int8_gemm_kernel.cu:663-745,
//       epilogue sgl-kernel/csrc/cutlass_extensions/epilogue/epilogue_per_row_per_col_scale.h:278,301
//   reached from W8A8Int8LinearMethod.apply (w8a8_int8.py:390-394) behind per_token_quant_int8 (csrc/quant_int8.hip).
//
//   acc = sum_k a[m,k] b[k,n]                       exact, int32
//   t   = fl32(scales_b[n] * scales_a[m])
//   r   = fl32(fl32(acc) * t)                       v_cvt_f32_i32 rounds to nearest even
//   r   = fl32(r + fl32(bias[n]))                   only with a bias; never contracted into an fma
//   out = round16(r)
// Integer sums do not depend on their order, so every form below -- any K slicing, any tile -- gives the same bits.
//
// Both forms run v_mfma_i32_16x16x64_i8 with the WEIGHT as the MFMA's A operand and the activation as its B operand: lane
// (r16 = lane % 16, g = lane / 16) feeds weight column r16 / token r16 at the 16 bytes k = 16 g .. 16 g + 15 of a 64-k
// half-step, and its four accumulator registers are token r16 x columns 4 g .. 4 g + 3: one scale product per register,
// one 8-byte store per fragment.  A 1-KiB piece of the fragment-major weight (include/sgl_mi355.h "Pre-shuffled FP8
// weights": a byte layout) is exactly that operand for one 16-column block and one half-step: piece (n / 16) (K / 64) + k / 64,
// lane l at byte 16 l.
//
//   * M <= 64: `int8_stream` / `int8_stream_rowmajor`, a weight streamer.  A workgroup stages its K slice of the activations
//     (row-major in LDS, rows padded by 16 bytes) once; each of its eight waves then owns 16-column blocks and pulls their
//     weight pieces from global memory straight into VGPRs with non-temporal 16-byte loads, eight pieces in flight, nothing
//     of the weight in LDS and no barrier in the loop.  K is cut into ceil(K / 2048) slices: one slice runs the epilogue,
//     more leave int32 slabs workspace[slice][M][N] that a finalize kernel sums AS INTEGERS before the one conversion.
//   * M > 64: `int8_tiled`, 128 x 128 tiles, four waves of 64 x 64, k-step 128.  On a fragment-major weight a wave loads its
//     eight weight fragments of the NEXT k-step from global memory into VGPRs while the MFMAs of this one run (no LDS, no
//     barrier for them; two register sets, the loop unrolled by two so that they never move); the activation tile goes
//     through double-buffered LDS in the fragment-major image (register staged, one barrier per k-step).  The 64 int32
//     accumulators stay where they are for the whole K loop.  A row-major weight goes through LDS beside the activations,
//     zero-filled past K.
#include "common.h"

namespace sglm {
namespace {

struct Int8Args {
  const int8_t* a;
  int64_t a_sm;  // bytes between rows of A
  const int8_t* b;
  int64_t b_sn;  // bytes between rows of W (row-major form)
  const float* sa;
  const float* sb;
  const void* bias;
  void* out;
  int32_t* slabs;  // streamer, split-K: [slices][M][N] int32
  int M, N, K;
  int blocks_per_wg;  // streamer: 16-column blocks per workgroup (blockIdx.x)
};

thread_local const char* g_int8_last_kernel = "";

__device__ __forceinline__ i32x4 mfma_i8(i32x4 w, i32x4 a, i32x4 c) {
  return __builtin_amdgcn_mfma_i32_16x16x64_i8(w, a, c, 0, 0, 0);
}

// the epilogue of the header comment for token m (scale sa_m) and columns n .. n + 3; every operation rounds on its own
template <int OUT_DTYPE>
__device__ __forceinline__ typename Half16<OUT_DTYPE>::x4 finish4(i32x4 acc, float sa_m, const float* sb, const void* bias, int n) {
  using H = Half16<OUT_DTYPE>;
  typename H::x4 o;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    float v = __fmul_rn((float)acc[r], __fmul_rn(sb[n + r], sa_m));
    if (bias) v = __fadd_rn(v, H::to_f32(reinterpret_cast<const typename H::T*>(bias)[n + r]));
    o[r] = H::from_f32(v);
  }
  return o;
}

// ------------------------------------------------------------------------------------------
// weight streamer: M <= 16 MB rows.  grid (column-block groups, K slices), 8 waves.
// Neither number below is a tuned crossover: 64 rows x (2048 + 16) bytes = 129 KiB is what one workgroup can stage of the
// CU's 160 KiB of LDS, so the streamer ends at 64 rows and a K slice at 2048.
constexpr int kStreamWaves = 8;
constexpr int kStreamMaxRows = 64;
constexpr int kSliceK = 2048;
// LDS row stride = slice bytes + 16: (16 h + 4) dwords with h half-steps, i.e. an odd number of 4-dword groups, so the 16
// tokens x 16 bytes that one lane group reads with ds_read_b128 fall on 16 different groups of four banks
constexpr int kRowPad = 16;
constexpr int kInFlight = 8;  // weight pieces (1 KiB per wave each) in flight

template <int OUT_DTYPE, int MB, bool SHUF, bool DIRECT>
__global__ __launch_bounds__(64 * kStreamWaves) void int8_stream_kernel(Int8Args p) {
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
  const int nh = (klen + 63) >> 6;  // 64-k half-steps of this slice (the last may be partial on a row-major weight)
  const int row_stride = nh * 64 + kRowPad;

  // rows beyond M and bytes beyond K are staged as zeros: they reach accumulators that are never stored / add nothing
  const int chunks = nh * 4;
  for (int i = tid; i < R * chunks; i += NT) {
    const int m = i / chunks, c = i - m * chunks;
    i32x4 v = i32x4{0, 0, 0, 0};
    if (m < p.M && c * 16 < klen) v = *reinterpret_cast<const i32x4*>(p.a + (int64_t)m * p.a_sm + k0 + c * 16);
    *reinterpret_cast<i32x4*>(smem + m * row_stride + c * 16) = v;
  }
  __syncthreads();

  const int nblocks = (p.N + 15) >> 4;
  const int nb_begin = blockIdx.x * p.blocks_per_wg;
  const int nb_end = nb_begin + p.blocks_per_wg < nblocks ? nb_begin + p.blocks_per_wg : nblocks;
  const char* abase = smem + r16 * row_stride + g * 16;
  for (int nb = nb_begin + wave; nb < nb_end; nb += kStreamWaves) {
    // this lane's 16 weight bytes of half-step 0 of the slice (64-bit offsets: a weight may be larger than 2 GiB)
    const int8_t* wp;
    if constexpr (SHUF) {
      wp = p.b + ((int64_t)nb * (p.K >> 6) + (k0 >> 6)) * 1024 + lane * 16;
    } else {
      const int n = nb * 16 + r16 < p.N ? nb * 16 + r16 : p.N - 1;  // N % 16 == 8: the upper lanes shadow the last column
      wp = p.b + (int64_t)n * p.b_sn + k0 + g * 16;
    }
    // a half-step beyond the slice re-reads its last one (never consumed); on a row-major weight the lanes past K read
    // the row's first bytes instead and are zeroed
    auto piece = [&](int h) __attribute__((always_inline)) -> i32x4 {
      const int hh = h < nh ? h : nh - 1;
      if constexpr (SHUF) {
        return __builtin_nontemporal_load(reinterpret_cast<const i32x4*>(wp + (int64_t)hh * 1024));
      } else {
        const bool valid = hh * 64 + g * 16 < klen;
        const i32x4 v = __builtin_nontemporal_load(reinterpret_cast<const i32x4*>(wp + (valid ? hh * 64 : -g * 16)));
        return valid ? v : i32x4{0, 0, 0, 0};
      }
    };
    i32x4 q[kInFlight];
#pragma unroll
    for (int i = 0; i < kInFlight; ++i) q[i] = piece(i);
    i32x4 acc[MB];
#pragma unroll
    for (int mi = 0; mi < MB; ++mi) acc[mi] = i32x4{0, 0, 0, 0};
    for (int h0 = 0; h0 < nh; h0 += kInFlight) {
#pragma unroll
      for (int i = 0; i < kInFlight; ++i) {
        const i32x4 w = q[i];
        q[i] = piece(h0 + i + kInFlight);
        const int h = h0 + i;
        if (h < nh) {
#pragma unroll
          for (int mi = 0; mi < MB; ++mi)
            acc[mi] = mfma_i8(w, *reinterpret_cast<const i32x4*>(abase + 16 * mi * row_stride + h * 64), acc[mi]);
        }
      }
    }
    // acc[mi][r] = C[token 16 mi + r16][column 16 nb + 4 g + r]; N % 8 == 0: a lane's four columns are all in or all out
    const int n = nb * 16 + 4 * g;
    if (n < p.N) {
#pragma unroll
      for (int mi = 0; mi < MB; ++mi) {
        const int m = 16 * mi + r16;
        if (m < p.M) {
          if constexpr (DIRECT) {
            using H = Half16<OUT_DTYPE>;
            *reinterpret_cast<typename H::x4*>(reinterpret_cast<typename H::T*>(p.out) + (int64_t)m * p.N + n) =
                finish4<OUT_DTYPE>(acc[mi], p.sa[m], p.sb, p.bias, n);
          } else {
            *reinterpret_cast<i32x4*>(p.slabs + ((int64_t)slice * p.M + m) * p.N + n) = acc[mi];
          }
        }
      }
    }
  }
}

// completion of the split-K streamer: the slices are summed as integers, then the one conversion
template <int OUT_DTYPE>
__global__ __launch_bounds__(256) void int8_finalize_kernel(const int32_t* __restrict__ slabs, int SK, int64_t MN, int N,
                                                            const float* __restrict__ sa, const float* __restrict__ sb,
                                                            const void* bias, void* out) {
  using H = Half16<OUT_DTYPE>;
  const int64_t total = MN >> 2;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    i32x4 v = *reinterpret_cast<const i32x4*>(slabs + i * 4);
    for (int s = 1; s < SK; ++s) v += *reinterpret_cast<const i32x4*>(slabs + s * MN + i * 4);
    const int64_t m = (i * 4) / N;  // N % 8 == 0: the four columns share a row
    const int n = (int)(i * 4 - m * N);
    *reinterpret_cast<typename H::x4*>(reinterpret_cast<typename H::T*>(out) + i * 4) = finish4<OUT_DTYPE>(v, sa[m], sb, bias, n);
  }
}

// ------------------------------------------------------------------------------------------
// tiles: 128 x 128 outputs, k-step 128, four waves as 2 x 2, each 64 x 64 = 4 x 4 fragments.
// LDS image of an operand tile: [16-row block cb][half-step h][g][r16][16 B] = 8 x 2 KiB, so that a fragment is one
// conflict-free 1-KiB read at cb * 2048 + h * 1024 + lane * 16 -- the order the fragment-major weight has in memory.
constexpr int kTileOperand = 8 * 2048;

template <int OUT_DTYPE, bool SHUF>
__global__ __launch_bounds__(256) void int8_tiled_kernel(Int8Args p) {
  using H = Half16<OUT_DTYPE>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int STAGE = SHUF ? kTileOperand : 2 * kTileOperand;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int r16 = lane & 15, g = lane >> 4;
  const int tiles_m = (p.M + 127) >> 7;
  // M fastest: the workgroups of a column panel of W run together and share it in L2
  const int m0 = ((int)blockIdx.x % tiles_m) << 7, n0 = ((int)blockIdx.x / tiles_m) << 7;
  const int ksteps = (p.K + 127) >> 7;

  // staging map: thread t moves the 16-byte pieces t + 256 i of a 16-KiB image: rows 32 i + 16 (t / 128) + t % 16 at the
  // k offset koff (the same for all four).  Rows past the edge re-read the last valid one, their results are never stored.
  const int koff = ((tid >> 6) & 1) * 64 + ((tid >> 4) & 3) * 16;
  const int8_t* a_ptr[4];
  const int8_t* b_ptr[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = 32 * i + 16 * (tid >> 7) + (tid & 15);
    a_ptr[i] = p.a + (int64_t)(m0 + row < p.M ? m0 + row : p.M - 1) * p.a_sm + koff;
    if constexpr (!SHUF) b_ptr[i] = p.b + (int64_t)(n0 + row < p.N ? n0 + row : p.N - 1) * p.b_sn + koff;
  }
  // fragment-major weight: the wave's four column blocks (a block past N shadows the last one)
  const int8_t* w_ptr[4];
  if constexpr (SHUF) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int nb = (n0 >> 4) + wn * 4 + i < (p.N >> 4) ? (n0 >> 4) + wn * 4 + i : (p.N >> 4) - 1;
      w_ptr[i] = p.b + (int64_t)nb * (p.K >> 6) * 1024 + lane * 16;
    }
  }

  i32x4 ra[4], rb[4];
  auto gload = [&](int ks) __attribute__((always_inline)) {
    // K % 128 != 0 (row-major weights only): the 16-byte pieces past K are zeros in both operands
    const bool valid = SHUF || ks * 128 + koff < p.K;
    const int64_t off = valid ? (int64_t)ks * 128 : -(int64_t)koff;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      ra[i] = *reinterpret_cast<const i32x4*>(a_ptr[i] + off);
      if (!valid) ra[i] = i32x4{0, 0, 0, 0};
      if constexpr (!SHUF) {
        rb[i] = *reinterpret_cast<const i32x4*>(b_ptr[i] + off);
        if (!valid) rb[i] = i32x4{0, 0, 0, 0};
      }
    }
  };
  auto lstore = [&](int stage) __attribute__((always_inline)) {
    char* s = smem + stage * STAGE + tid * 16;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      *reinterpret_cast<i32x4*>(s + i * 4096) = ra[i];
      if constexpr (!SHUF) *reinterpret_cast<i32x4*>(s + kTileOperand + i * 4096) = rb[i];
    }
  };
  auto wload = [&](int ks, i32x4 (&w)[4][2]) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int h = 0; h < 2; ++h) w[i][h] = *reinterpret_cast<const i32x4*>(w_ptr[i] + ((int64_t)ks * 2 + h) * 1024);
  };

  i32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = i32x4{0, 0, 0, 0};

  // one k-step: the next step's global loads are issued first and land under this step's 32 MFMAs (the last step re-reads
  // itself into the idle stage: branch-free, so that the staging registers stay registers)
  auto step = [&](int kt, i32x4 (&wc)[4][2], i32x4 (&wnext)[4][2]) __attribute__((always_inline)) {
    const int st = kt & 1;
    const int nxt = kt + 1 < ksteps ? kt + 1 : kt;
    gload(nxt);
    if constexpr (SHUF) wload(nxt, wnext);
    const char* sA = smem + st * STAGE + lane * 16;
    i32x4 af[4][2];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int h = 0; h < 2; ++h) af[j][h] = *reinterpret_cast<const i32x4*>(sA + (wm * 4 + j) * 2048 + h * 1024);
    if constexpr (!SHUF) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int h = 0; h < 2; ++h) wc[i][h] = *reinterpret_cast<const i32x4*>(sA + kTileOperand + (wn * 4 + i) * 2048 + h * 1024);
    }
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = mfma_i8(wc[i][h], af[j][h], acc[i][j]);
    lstore(st ^ 1);
    __syncthreads();
  };

  i32x4 w0[4][2], w1[4][2];
  gload(0);
  lstore(0);
  if constexpr (SHUF) wload(0, w0);
  __syncthreads();
  for (int kt = 0; kt < ksteps; kt += 2) {
    step(kt, w0, w1);
    if (kt + 1 < ksteps) step(kt + 1, w1, w0);
  }

  // acc[i][j][r] = C[m0 + 64 wm + 16 j + r16][n0 + 64 wn + 16 i + 4 g + r]; N % 8 == 0: a lane's four columns are all in or out
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int n = n0 + wn * 64 + 16 * i + 4 * g;
    if (n < p.N) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int m = m0 + wm * 64 + 16 * j + r16;
        if (m < p.M)
          *reinterpret_cast<typename H::x4*>(reinterpret_cast<typename H::T*>(p.out) + (int64_t)m * p.N + n) =
              finish4<OUT_DTYPE>(acc[i][j], p.sa[m], p.sb, p.bias, n);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------
inline int stream_slices(int64_t K) { return (int)((K + kSliceK - 1) / kSliceK); }

template <int OUT_DTYPE, int MB, bool SHUF>
int launch_stream(Int8Args p, int32_t* ws, int64_t ws_ints, hipStream_t s) {
  const int SK = stream_slices(p.K);
  SGLM_CHECK_ARG(SK == 1 || (ws != nullptr && ws_ints >= (int64_t)SK * p.M * p.N),
                 "int8_scaled_mm: workspace of %ld int32 required for %d K slices (got %ld)", (long)((int64_t)SK * p.M * p.N), SK,
                 (long)(ws ? ws_ints : 0));
  p.slabs = ws;
  // one 16-column block per wave, more where that would be more workgroups than 1024 (four rounds of the chip)
  const int nblocks = (p.N + 15) >> 4;
  p.blocks_per_wg = kStreamWaves;
  while ((int64_t)((nblocks + p.blocks_per_wg - 1) / p.blocks_per_wg) * SK > 1024) p.blocks_per_wg *= 2;
  constexpr int kMaxLds = 16 * MB * (kSliceK + kRowPad);
  const int klen = p.K < kSliceK ? p.K : kSliceK;
  const int lds = 16 * MB * (((klen + 63) >> 6) * 64 + kRowPad);
  static int attr_rc = [] {
    int rc = check_hip(hipFuncSetAttribute(reinterpret_cast<const void*>(int8_stream_kernel<OUT_DTYPE, MB, SHUF, true>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLds),
                       "hipFuncSetAttribute");
    return rc ? rc
              : check_hip(hipFuncSetAttribute(reinterpret_cast<const void*>(int8_stream_kernel<OUT_DTYPE, MB, SHUF, false>),
                                              hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLds),
                          "hipFuncSetAttribute");
  }();
  if (attr_rc) return attr_rc;
  g_int8_last_kernel = SHUF ? "int8_stream" : "int8_stream_rowmajor";
  const dim3 grid((unsigned)((nblocks + p.blocks_per_wg - 1) / p.blocks_per_wg), (unsigned)SK);
  if (SK == 1) {
    hipLaunchKernelGGL((int8_stream_kernel<OUT_DTYPE, MB, SHUF, true>), grid, dim3(64 * kStreamWaves), lds, s, p);
    return check_hip(hipGetLastError(), "int8_stream launch");
  }
  hipLaunchKernelGGL((int8_stream_kernel<OUT_DTYPE, MB, SHUF, false>), grid, dim3(64 * kStreamWaves), lds, s, p);
  int rc = check_hip(hipGetLastError(), "int8_stream launch");
  if (rc) return rc;
  const int64_t MN = (int64_t)p.M * p.N;
  hipLaunchKernelGGL((int8_finalize_kernel<OUT_DTYPE>), dim3((unsigned)((MN / 4 + 255) / 256)), dim3(256), 0, s,
                     (const int32_t*)ws, SK, MN, p.N, p.sa, p.sb, p.bias, p.out);
  return check_hip(hipGetLastError(), "int8_finalize launch");
}

template <int OUT_DTYPE, bool SHUF>
int launch_int8(const Int8Args& p, int32_t* ws, int64_t ws_ints, hipStream_t s) {
  if (p.M <= 16) return launch_stream<OUT_DTYPE, 1, SHUF>(p, ws, ws_ints, s);
  if (p.M <= 32) return launch_stream<OUT_DTYPE, 2, SHUF>(p, ws, ws_ints, s);
  if (p.M <= kStreamMaxRows) return launch_stream<OUT_DTYPE, 4, SHUF>(p, ws, ws_ints, s);
  const int64_t tiles = (int64_t)((p.M + 127) >> 7) * ((p.N + 127) >> 7);
  SGLM_CHECK_ARG(tiles < (1ll << 31), "int8_scaled_mm: M x N of %d x %d has too many tiles", p.M, p.N);
  constexpr int lds = 2 * (SHUF ? kTileOperand : 2 * kTileOperand);
  static int attr_rc = check_hip(hipFuncSetAttribute(reinterpret_cast<const void*>(int8_tiled_kernel<OUT_DTYPE, SHUF>),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, lds),
                                 "hipFuncSetAttribute");
  if (attr_rc) return attr_rc;
  g_int8_last_kernel = "int8_tiled";
  hipLaunchKernelGGL((int8_tiled_kernel<OUT_DTYPE, SHUF>), dim3((unsigned)tiles), dim3(256), lds, s, p);
  return check_hip(hipGetLastError(), "int8_tiled launch");
}

int int8_impl(int b_shuf, const void* mat_a, const void* mat_b, const float* scales_a, const float* scales_b, const void* bias,
              void* out, int32_t* workspace, int64_t workspace_ints, int64_t M, int64_t N, int64_t K, int64_t a_stride_m,
              int64_t b_stride_n, int out_dtype, void* stream) {
  SGLM_CHECK_ARG(out_dtype == SGL_MI355_BF16 || out_dtype == SGL_MI355_FP16, "out_dtype must be Half or BFloat16");
  SGLM_CHECK_ARG(M >= 0 && N > 0 && K > 0 && M < (1ll << 31) && N < (1ll << 31) && K < (1ll << 31), "int8_scaled_mm: bad shape");
  SGLM_CHECK_ARG(K % 16 == 0, "mat_a.size(1) must be multiple of 16 for memory alignment");
  SGLM_CHECK_ARG(N % 8 == 0, "mat_b.size(1) must be multiple of 8 for memory alignment");
  SGLM_CHECK_ARG(!b_shuf || (N % 16 == 0 && K % 512 == 0),
                 "int8_scaled_mm_wshuffled: N %% 16 == 0 and K %% 512 == 0 required (N=%ld K=%ld)", (long)N, (long)K);
  SGLM_CHECK_ARG(a_stride_m % 16 == 0 && a_stride_m >= K && (b_shuf || (b_stride_n % 16 == 0 && b_stride_n >= K)),
                 "int8_scaled_mm: row strides must be >= K and multiples of 16 bytes");
  if (M == 0) return 0;
  SGLM_CHECK_ARG(mat_a && mat_b && scales_a && scales_b && out, "int8_scaled_mm: null tensor pointer");
  SGLM_CHECK_ARG(reinterpret_cast<uintptr_t>(mat_a) % 16 == 0 && reinterpret_cast<uintptr_t>(mat_b) % 16 == 0 &&
                     reinterpret_cast<uintptr_t>(out) % 16 == 0 && reinterpret_cast<uintptr_t>(workspace) % 16 == 0,
                 "int8_scaled_mm: operands must be 16-byte aligned");
  Int8Args p{(const int8_t*)mat_a, a_stride_m, (const int8_t*)mat_b, b_stride_n, scales_a, scales_b, bias, out, nullptr,
             (int)M, (int)N, (int)K, 0};
  hipStream_t s = as_stream(stream);
  if (b_shuf)
    return out_dtype == SGL_MI355_BF16 ? launch_int8<SGL_MI355_BF16, true>(p, workspace, workspace_ints, s)
                                       : launch_int8<SGL_MI355_FP16, true>(p, workspace, workspace_ints, s);
  return out_dtype == SGL_MI355_BF16 ? launch_int8<SGL_MI355_BF16, false>(p, workspace, workspace_ints, s)
                                     : launch_int8<SGL_MI355_FP16, false>(p, workspace, workspace_ints, s);
}

}  // namespace
}  // namespace sglm

using namespace sglm;

extern "C" int sgl_mi355_int8_scaled_mm(const void* mat_a, const void* mat_b, const float* scales_a, const float* scales_b,
                                        const void* bias, void* out, int32_t* workspace, int64_t workspace_ints, int64_t M,
                                        int64_t N, int64_t K, int64_t a_stride_m, int64_t b_stride_n, int out_dtype,
                                        void* stream) {
  return int8_impl(0, mat_a, mat_b, scales_a, scales_b, bias, out, workspace, workspace_ints, M, N, K, a_stride_m, b_stride_n,
                   out_dtype, stream);
}

extern "C" int sgl_mi355_int8_scaled_mm_wshuffled(const void* mat_a, const void* mat_b, const float* scales_a,
                                                  const float* scales_b, const void* bias, void* out, int32_t* workspace,
                                                  int64_t workspace_ints, int64_t M, int64_t N, int64_t K, int64_t a_stride_m,
                                                  int out_dtype, void* stream) {
  return int8_impl(1, mat_a, mat_b, scales_a, scales_b, bias, out, workspace, workspace_ints, M, N, K, a_stride_m, K, out_dtype,
                   stream);
}

extern "C" const char* sgl_mi355_int8_last_kernel(void) { return g_int8_last_kernel; }
