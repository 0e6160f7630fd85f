// Block-scaled FP8 (OCP e4m3fn) GEMM for MI355X / gfx950: 128 x 128 weight blocks, 1 x 128 activation groups.
//
// Replaces:
//   * fp8_blockwise_scaled_mm(mat_a, mat_b, scales_a, scales_b, out_dtype)
//       schema sgl-kernel/csrc/common_extension.cc:112-114, checks csrc/gemm/fp8_blockwise_gemm_kernel.cu:345-423,
//       semantics sgl-kernel/tests/test_fp8_blockwise_gemm.py:19-59
//   reached from Fp8LinearMethod.apply through per_token_group_quant_fp8 (fp8_utils.py:180-210, 287-307).
//
//   out[m, n] = round16( sum over kb of ( sum_{k in block kb} a[m,k] b[k,n] )_f32 * sa[m, kb] * sb[kb, n / 128] )
//   with a bias: round16(f32(round16(acc)) + f32(bias[n])) -- the reference adds the bias to the rounded output
//   (fp8_utils.py:305-306), so there are two roundings.
//
// The scales change along K, so the per-channel kernels of gemm_fp8.hip (one fp32 accumulator over the whole K range,
// scaled once in the epilogue) cannot express this.  Here one v_mfma_scale_f32_16x16x128_f8f6f4 (E8M0 operands fixed at
// 2^0) consumes exactly one 128-k block of a 16 x 16 fragment into a FRESH zero-C accumulator, and the result is folded
// into the running sum with run = fma(blk, sa * sb, run).  The fragment is oriented with the WEIGHT as the MFMA's A
// operand and the activation as its B operand: a lane's four accumulator registers are then four consecutive output
// columns (one 128-wide n-block) of ONE token, so the lane needs one sa * sb product and four FMAs per MFMA, and it
// stores its four results as one 8-byte piece of an output row.
//
// Both operands hand lane group g the bytes [16 g, 16 g + 16) and [64 + 16 g, 64 + 16 g + 16) of each 128-byte k-step
// (the fragment-major order of sgl_mi355_fp8_shuffle_weight); the MFMA's k index is contracted, so the permutation only
// has to be the same on both sides.
//
// Two forms (launch_block below picks; every M >= 1 goes to one of them):
//   * M <= 64: `block_stream` / `block_stream_rowmajor` -- weight streaming.  A workgroup stages its K slice of the
//     activation tile (fragment-major, conflict-free 16-byte reads) and of the [M, K/128] scales in LDS once, every wave
//     owns 16-column blocks and walks the slice in 128-k steps with four weight fragments in flight.  Split-K over
//     workgroups at multiples of 128 k, at most 8 steps (1024 k) per slice: the slices hold already-scaled partial
//     sums, the finalize kernel adds them in slice order, rounds and adds the bias.  K <= 1024 is one slice and stores
//     the output directly.
//   * M > 64: `block_tiled` -- 128 x 128 tiles, 128-deep k-step, four waves as 2 x 2 with 4 x 4 fragments each.  The
//     tile's N extent equals block_n, so sb is one scalar per (tile, k-step); sa is loaded beside the A tile.  Both
//     operands are staged global -> registers -> LDS (double-buffered) in the fragment-major image, which for a
//     pre-shuffled weight is a straight copy of eight 2-KiB pieces.
#include "common.h"

namespace sglm {
namespace {

typedef int v8i32_t __attribute__((ext_vector_type(8)));

struct BlockArgs {
  const uint8_t* a;
  int64_t a_sm;  // bytes between rows of A
  const uint8_t* b;
  int64_t b_sn;  // bytes between rows of W (row-major form)
  int b_shuf;    // 1: W is fragment-major (GemmArgs::b_shuf of gemm_fp8.hip, include/sgl_mi355.h)
  const float* sa;
  int64_t sa_sm, sa_sk;  // element strides of scales_a [M, K/128]
  const float* sb;
  int64_t sb_sk, sb_sn;  // element strides of scales_b [K/128, ceil(N/128)]
  const void* bias;
  void* out;
  float* slabs;  // streamer, split-K: [slices][M][N] fp32
  int M, N, K;
  int steps_per_slice;  // streamer: 128-k steps per K slice (blockIdx.y)
  int blocks_per_wg;    // streamer: 16-column blocks per workgroup (blockIdx.x)
};

struct Frag {  // one lane's 32 k-bytes of a 16-row fragment = one operand of the 16x16x128 MFMA
  i32x4 v[2];
};
__device__ __forceinline__ v8i32_t operand(const Frag& f) { return __builtin_shufflevector(f.v[0], f.v[1], 0, 1, 2, 3, 4, 5, 6, 7); }

// one 128-k block of a 16 x 16 fragment into a fresh accumulator: r[j] = C[token r16][column 4 g + j]
__device__ __forceinline__ f32x4 mfma_block(const Frag& w, const Frag& a) {
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(operand(w), operand(a), f32x4{0.f, 0.f, 0.f, 0.f}, 0 /* e4m3 */, 0 /* e4m3 */,
                                                          0, 0x7F7F7F7F /* 2^0 */, 0, 0x7F7F7F7F);
}

// the two roundings of the reference: the accumulator to the 16-bit dtype, then (rounded + bias) again
template <int OUT_DTYPE>
__device__ __forceinline__ typename Half16<OUT_DTYPE>::x4 finish4(f32x4 acc, const void* bias, int n) {
  using H = Half16<OUT_DTYPE>;
  typename H::x4 o;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    o[r] = H::from_f32(acc[r]);
    if (bias) o[r] = H::from_f32(H::to_f32(o[r]) + H::to_f32(reinterpret_cast<const typename H::T*>(bias)[n + r]));
  }
  return o;
}

// ------------------------------------------------------------------------------------------
// decode streamer: M <= 16 MB.  grid (column-block groups, K slices), 8 waves.
// LDS: activation image [step][half][g][R rows][16 B] (R = 16 MB), then the scales [step][R] fp32.
constexpr int kStreamWaves = 8;
constexpr int kStreamMaxSteps = 8;  // 128-k steps per K slice: 64 rows x 1 KiB = 64 KiB of LDS at most

template <int OUT_DTYPE, int MB, bool DIRECT>
__global__ __launch_bounds__(64 * kStreamWaves) void fp8_block_stream_kernel(BlockArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int R = 16 * MB;
  constexpr int NT = 64 * kStreamWaves;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r16 = lane & 15, g = lane >> 4;
  const int ksteps = p.K >> 7;
  const int slice = blockIdx.y;
  const int s0 = slice * p.steps_per_slice;
  const int ns = ksteps - s0 < p.steps_per_slice ? ksteps - s0 : p.steps_per_slice;
  float* lsc = reinterpret_cast<float*>(smem + p.steps_per_slice * 128 * R);

  // rows beyond M are staged as zeros (their scales too): they only reach accumulators that are never stored
  for (int i = tid; i < ns * R * 8; i += NT) {
    const int c = i & 7, m = (i >> 3) % R, s = i / (8 * R);  // c = 4 half + g: 16-byte chunk of the row's k-step
    i32x4 v = i32x4{0, 0, 0, 0};
    if (m < p.M) v = *reinterpret_cast<const i32x4*>(p.a + (int64_t)m * p.a_sm + (int64_t)(s0 + s) * 128 + c * 16);
    *reinterpret_cast<i32x4*>(smem + s * 128 * R + c * R * 16 + m * 16) = v;
  }
  for (int i = tid; i < ns * R; i += NT) {
    const int m = i % R, s = i / R;
    lsc[i] = m < p.M ? p.sa[(int64_t)m * p.sa_sm + (int64_t)(s0 + s) * p.sa_sk] : 0.f;
  }
  __syncthreads();

  const int nblocks = p.N >> 4;
  const int nb_begin = blockIdx.x * p.blocks_per_wg;
  const int nb_end = nb_begin + p.blocks_per_wg < nblocks ? nb_begin + p.blocks_per_wg : nblocks;
  for (int nb = nb_begin + wave; nb < nb_end; nb += kStreamWaves) {
    // this lane's weight bytes of k-step 0, the second 16 bytes and the distance between k-steps
    const uint8_t* wp;
    int wsecond, wstep;
    if (p.b_shuf) {
      wp = p.b + ((int64_t)nb * ksteps + s0) * 2048 + lane * 16;
      wsecond = 1024;
      wstep = 2048;
    } else {
      wp = p.b + (int64_t)(nb * 16 + r16) * p.b_sn + (int64_t)s0 * 128 + g * 16;
      wsecond = 64;
      wstep = 128;
    }
    // the slice's weight-block scales of this n-block: lane s holds step s
    const float sbl = p.sb[(int64_t)(nb >> 3) * p.sb_sn + (int64_t)(s0 + (lane < ns ? lane : ns - 1)) * p.sb_sk];

    constexpr int PB = 4;  // weight fragments in flight
    Frag q[PB];
#pragma unroll
    for (int i = 0; i < PB; ++i) {
      const uint8_t* src = wp + (i < ns ? i : ns - 1) * wstep;
      q[i].v[0] = *reinterpret_cast<const i32x4*>(src);
      q[i].v[1] = *reinterpret_cast<const i32x4*>(src + wsecond);
    }
    f32x4 run[MB];
#pragma unroll
    for (int mi = 0; mi < MB; ++mi) run[mi] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < ns; s += PB) {
#pragma unroll
      for (int i = 0; i < PB; ++i) {
        const Frag w = q[i];
        {  // refill (a step beyond the slice re-reads its last step; never consumed)
          const int nxt = s + i + PB;
          const uint8_t* src = wp + (nxt < ns ? nxt : ns - 1) * wstep;
          q[i].v[0] = *reinterpret_cast<const i32x4*>(src);
          q[i].v[1] = *reinterpret_cast<const i32x4*>(src + wsecond);
        }
        const int st = s + i;
        if (st < ns) {
          const float sbv = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(sbl), st));
          const char* abase = smem + st * 128 * R + g * R * 16 + r16 * 16;
#pragma unroll
          for (int mi = 0; mi < MB; ++mi) {
            Frag a;
            a.v[0] = *reinterpret_cast<const i32x4*>(abase + mi * 256);
            a.v[1] = *reinterpret_cast<const i32x4*>(abase + mi * 256 + 4 * R * 16);
            const float sc = lsc[st * R + 16 * mi + r16] * sbv;
            const f32x4 blk = mfma_block(w, a);
#pragma unroll
            for (int r = 0; r < 4; ++r) run[mi][r] = fmaf(blk[r], sc, run[mi][r]);
          }
        }
      }
    }
    // run[mi][r] = C[token 16 mi + r16][column 16 nb + 4 g + r]
    const int n = nb * 16 + 4 * g;
#pragma unroll
    for (int mi = 0; mi < MB; ++mi) {
      const int m = 16 * mi + r16;
      if (m < p.M) {
        if constexpr (DIRECT) {
          using H = Half16<OUT_DTYPE>;
          *reinterpret_cast<typename H::x4*>(reinterpret_cast<typename H::T*>(p.out) + (int64_t)m * p.N + n) =
              finish4<OUT_DTYPE>(run[mi], p.bias, n);
        } else {
          *reinterpret_cast<f32x4*>(p.slabs + ((int64_t)slice * p.M + m) * p.N + n) = run[mi];
        }
      }
    }
  }
}

// completion of the split-K streamer: slices summed in slice order, then the two roundings
template <int OUT_DTYPE>
__global__ __launch_bounds__(256) void fp8_block_finalize_kernel(const float* __restrict__ slabs, int SK, int64_t MN, int N,
                                                                 const void* bias, void* out) {
  using H = Half16<OUT_DTYPE>;
  const int64_t total = MN >> 2;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    f32x4 v = *reinterpret_cast<const f32x4*>(slabs + i * 4);
    for (int s = 1; s < SK; ++s) {
      const f32x4 t = *reinterpret_cast<const f32x4*>(slabs + s * MN + i * 4);
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] += t[r];
    }
    const int n = (int)((i * 4) % N);  // N % 16 == 0: the four columns share a row
    *reinterpret_cast<typename H::x4*>(reinterpret_cast<typename H::T*>(out) + i * 4) = finish4<OUT_DTYPE>(v, bias, n);
  }
}

// ------------------------------------------------------------------------------------------
// prefill tiles: 128 x 128 x 128, four waves as 2 x 2, each 64 x 64 = 4 x 4 fragments.
// LDS per stage: A image then W image, each [16-row block cb][half][g][r16][16 B] = 8 x 2 KiB.
constexpr int kTileOperand = 8 * 2048;
constexpr int kTileStage = 2 * kTileOperand;

template <int OUT_DTYPE>
__global__ __launch_bounds__(256) void fp8_block_tiled_kernel(BlockArgs p) {
  using H = Half16<OUT_DTYPE>;
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

  // staging map: thread t moves the 16-byte pieces t + 256 i of each operand's 16-KiB image; rows past the edge re-read
  // a valid row (column block), their results are never stored
  const uint8_t* a_ptr[4];
  const uint8_t* w_ptr[4];
  const int wstep = p.b_shuf ? 2048 : 128;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int idx = tid + 256 * i;
    const int cb = idx >> 7, koff = ((idx >> 6) & 1) * 64 + ((idx >> 4) & 3) * 16, row = cb * 16 + (idx & 15);
    const int m = m0 + row < p.M ? m0 + row : p.M - 1;
    a_ptr[i] = p.a + (int64_t)m * p.a_sm + koff;
    if (p.b_shuf) {
      const int nbk = (n0 >> 4) + cb < (p.N >> 4) ? (n0 >> 4) + cb : (p.N >> 4) - 1;
      w_ptr[i] = p.b + (int64_t)nbk * ksteps * 2048 + (idx & 127) * 16;
    } else {
      const int n = n0 + row < p.N ? n0 + row : p.N - 1;
      w_ptr[i] = p.b + (int64_t)n * p.b_sn + koff;
    }
  }
  // sa of this lane's four tokens (one per activation fragment) and the tile's sb: one scalar per k-step
  const float* sa_ptr[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int m = m0 + wm * 64 + 16 * j + r16;
    sa_ptr[j] = p.sa + (int64_t)(m < p.M ? m : p.M - 1) * p.sa_sm;
  }
  const float* sb_ptr = p.sb + (int64_t)(n0 >> 7) * p.sb_sn;

  i32x4 ra[4], rw[4];
  float rsa[4], rsb;
  auto gload = [&](int ks) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      ra[i] = *reinterpret_cast<const i32x4*>(a_ptr[i] + (int64_t)ks * 128);
      rw[i] = *reinterpret_cast<const i32x4*>(w_ptr[i] + (int64_t)ks * wstep);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) rsa[j] = sa_ptr[j][(int64_t)ks * p.sa_sk];
    rsb = sb_ptr[(int64_t)ks * p.sb_sk];
  };
  auto lstore = [&](int stage) __attribute__((always_inline)) {
    char* sA = smem + stage * kTileStage;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      *reinterpret_cast<i32x4*>(sA + (tid + 256 * i) * 16) = ra[i];
      *reinterpret_cast<i32x4*>(sA + kTileOperand + (tid + 256 * i) * 16) = rw[i];
    }
  };

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  float sc[4];

  gload(0);
  lstore(0);
#pragma unroll
  for (int j = 0; j < 4; ++j) sc[j] = rsa[j] * rsb;
  __syncthreads();
  for (int kt = 0; kt < ksteps; ++kt) {
    const int st = kt & 1;
    // in flight under this step's MFMAs (the last step re-reads itself into the idle stage: branch-free, so that the
    // staging registers stay registers)
    gload(kt + 1 < ksteps ? kt + 1 : kt);
    const char* sA = smem + st * kTileStage + lane * 16;
    const char* sW = sA + kTileOperand;
    Frag af[4], wf[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      af[i].v[0] = *reinterpret_cast<const i32x4*>(sA + (wm * 4 + i) * 2048);
      af[i].v[1] = *reinterpret_cast<const i32x4*>(sA + (wm * 4 + i) * 2048 + 1024);
      wf[i].v[0] = *reinterpret_cast<const i32x4*>(sW + (wn * 4 + i) * 2048);
      wf[i].v[1] = *reinterpret_cast<const i32x4*>(sW + (wn * 4 + i) * 2048 + 1024);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const f32x4 blk = mfma_block(wf[i], af[j]);
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[i][j][r] = fmaf(blk[r], sc[j], acc[i][j][r]);
      }
    lstore(st ^ 1);
#pragma unroll
    for (int j = 0; j < 4; ++j) sc[j] = rsa[j] * rsb;
    __syncthreads();
  }

  // acc[i][j][r] = C[m0 + 64 wm + 16 j + r16][n0 + 64 wn + 16 i + 4 g + r]; N % 16 == 0: a fragment is all-in or all-out
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int n = n0 + wn * 64 + 16 * i + 4 * g;
    if (n0 + wn * 64 + 16 * i < p.N) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int m = m0 + wm * 64 + 16 * j + r16;
        if (m < p.M)
          *reinterpret_cast<typename H::x4*>(reinterpret_cast<typename H::T*>(p.out) + (int64_t)m * p.N + n) =
              finish4<OUT_DTYPE>(acc[i][j], p.bias, n);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------
constexpr int kStreamMaxRows = 64;

// K slices of the streamer: whole 128-k steps, at most kStreamMaxSteps per slice
inline int stream_slices(int64_t K) { return (int)(((K >> 7) + kStreamMaxSteps - 1) / kStreamMaxSteps); }

template <int OUT_DTYPE, int MB>
int launch_stream(BlockArgs p, float* ws, int64_t ws_floats, hipStream_t s) {
  const int ksteps = p.K >> 7;
  const int SK = stream_slices(p.K);
  p.steps_per_slice = ksteps < kStreamMaxSteps ? ksteps : kStreamMaxSteps;
  SGLM_CHECK_ARG(SK == 1 || (ws != nullptr && ws_floats >= (int64_t)SK * p.M * p.N),
                 "fp8_blockwise_scaled_mm: workspace of %ld floats required for %d K slices (got %ld)",
                 (long)((int64_t)SK * p.M * p.N), SK, (long)(ws ? ws_floats : 0));
  p.slabs = ws;
  // one 16-column block per wave, more where that would be far more workgroups than the chip holds at once
  const int nblocks = p.N >> 4;
  p.blocks_per_wg = kStreamWaves;
  while (p.blocks_per_wg < 4 * kStreamWaves && (int64_t)((nblocks + p.blocks_per_wg - 1) / p.blocks_per_wg) * SK > 1024)
    p.blocks_per_wg *= 2;
  const int lds = p.steps_per_slice * (128 + 4) * 16 * MB;
  static int attr_rc = [] {
    int rc = check_hip(hipFuncSetAttribute(reinterpret_cast<const void*>(fp8_block_stream_kernel<OUT_DTYPE, MB, true>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, kStreamMaxSteps * 132 * 16 * MB),
                       "hipFuncSetAttribute");
    return rc ? rc
              : check_hip(hipFuncSetAttribute(reinterpret_cast<const void*>(fp8_block_stream_kernel<OUT_DTYPE, MB, false>),
                                              hipFuncAttributeMaxDynamicSharedMemorySize, kStreamMaxSteps * 132 * 16 * MB),
                          "hipFuncSetAttribute");
  }();
  if (attr_rc) return attr_rc;
  set_fp8_last_kernel(p.b_shuf ? "block_stream" : "block_stream_rowmajor");
  const dim3 grid((unsigned)((nblocks + p.blocks_per_wg - 1) / p.blocks_per_wg), (unsigned)SK);
  if (SK == 1) {
    hipLaunchKernelGGL((fp8_block_stream_kernel<OUT_DTYPE, MB, true>), grid, dim3(64 * kStreamWaves), lds, s, p);
    return check_hip(hipGetLastError(), "fp8_block_stream launch");
  }
  hipLaunchKernelGGL((fp8_block_stream_kernel<OUT_DTYPE, MB, false>), grid, dim3(64 * kStreamWaves), lds, s, p);
  int rc = check_hip(hipGetLastError(), "fp8_block_stream launch");
  if (rc) return rc;
  const int64_t MN = (int64_t)p.M * p.N;
  hipLaunchKernelGGL((fp8_block_finalize_kernel<OUT_DTYPE>), dim3((unsigned)((MN / 4 + 255) / 256)), dim3(256), 0, s,
                     (const float*)ws, SK, MN, p.N, p.bias, p.out);
  return check_hip(hipGetLastError(), "fp8_block_finalize launch");
}

template <int OUT_DTYPE>
int launch_block(const BlockArgs& p, float* ws, int64_t ws_floats, hipStream_t s) {
  if (p.M <= 16) return launch_stream<OUT_DTYPE, 1>(p, ws, ws_floats, s);
  if (p.M <= 32) return launch_stream<OUT_DTYPE, 2>(p, ws, ws_floats, s);
  if (p.M <= kStreamMaxRows) return launch_stream<OUT_DTYPE, 4>(p, ws, ws_floats, s);
  const int64_t tiles = (int64_t)((p.M + 127) >> 7) * ((p.N + 127) >> 7);
  SGLM_CHECK_ARG(tiles < (1ll << 31), "fp8_blockwise_scaled_mm: M x N of %d x %d has too many tiles", p.M, p.N);
  static int attr_rc = check_hip(hipFuncSetAttribute(reinterpret_cast<const void*>(fp8_block_tiled_kernel<OUT_DTYPE>),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, 2 * kTileStage),
                                 "hipFuncSetAttribute");
  if (attr_rc) return attr_rc;
  set_fp8_last_kernel("block_tiled");
  hipLaunchKernelGGL((fp8_block_tiled_kernel<OUT_DTYPE>), dim3((unsigned)tiles), dim3(256), 2 * kTileStage, s, p);
  return check_hip(hipGetLastError(), "fp8_block_tiled launch");
}

int blockwise_impl(int b_shuf, const void* mat_a, const void* mat_b, const float* scales_a, const float* scales_b,
                   const void* bias, void* out, float* workspace, int64_t workspace_floats, int64_t M, int64_t N, int64_t K,
                   int64_t a_stride_m, int64_t b_stride_n, int64_t sa_stride_m, int64_t sa_stride_k, int64_t sb_stride_k,
                   int64_t sb_stride_n, int out_dtype, void* stream) {
  SGLM_CHECK_ARG(out_dtype == SGL_MI355_BF16 || out_dtype == SGL_MI355_FP16,
                 "fp8_blockwise_scaled_mm: out_dtype must be Half or BFloat16");
  SGLM_CHECK_ARG(M >= 0 && N > 0 && K > 0 && M < (1ll << 31) && N < (1ll << 31) && K < (1ll << 31),
                 "fp8_blockwise_scaled_mm: bad shape");
  SGLM_CHECK_ARG(K % 128 == 0, "fp8_blockwise_scaled_mm: K %% 128 == 0 required (K=%ld)", (long)K);
  SGLM_CHECK_ARG(N % 16 == 0, "fp8_blockwise_scaled_mm: N %% 16 == 0 required (N=%ld)", (long)N);
  SGLM_CHECK_ARG(a_stride_m % 16 == 0 && a_stride_m >= K && (b_shuf || (b_stride_n % 16 == 0 && b_stride_n >= K)),
                 "fp8_blockwise_scaled_mm: row strides must be >= K and multiples of 16 bytes");
  SGLM_CHECK_ARG(!b_shuf || K % 512 == 0, "fp8_blockwise_scaled_mm_wshuffled: K %% 512 == 0 required (K=%ld)", (long)K);
  SGLM_CHECK_ARG(sa_stride_m >= 0 && sa_stride_k >= 0 && sb_stride_k >= 0 && sb_stride_n >= 0,
                 "fp8_blockwise_scaled_mm: scale strides must not be negative");
  if (M == 0) return 0;
  SGLM_CHECK_ARG(mat_a && mat_b && scales_a && scales_b && out, "fp8_blockwise_scaled_mm: null tensor pointer");
  SGLM_CHECK_ARG(reinterpret_cast<uintptr_t>(mat_a) % 16 == 0 && reinterpret_cast<uintptr_t>(mat_b) % 16 == 0 &&
                     reinterpret_cast<uintptr_t>(out) % 16 == 0 && reinterpret_cast<uintptr_t>(workspace) % 16 == 0,
                 "fp8_blockwise_scaled_mm: operands must be 16-byte aligned");
  BlockArgs p{(const uint8_t*)mat_a, a_stride_m, (const uint8_t*)mat_b, b_stride_n, b_shuf, scales_a, sa_stride_m,
              sa_stride_k, scales_b, sb_stride_k, sb_stride_n, bias, out, nullptr, (int)M, (int)N, (int)K, 0, 0};
  hipStream_t s = as_stream(stream);
  return out_dtype == SGL_MI355_BF16 ? launch_block<SGL_MI355_BF16>(p, workspace, workspace_floats, s)
                                     : launch_block<SGL_MI355_FP16>(p, workspace, workspace_floats, s);
}

}  // namespace
}  // namespace sglm

using namespace sglm;

extern "C" int sgl_mi355_fp8_blockwise_scaled_mm(
    const void* mat_a, const void* mat_b, const float* scales_a, const float* scales_b, const void* bias, void* out,
    float* workspace, int64_t workspace_floats, int64_t M, int64_t N, int64_t K, int64_t a_stride_m, int64_t b_stride_n,
    int64_t sa_stride_m, int64_t sa_stride_k, int64_t sb_stride_k, int64_t sb_stride_n, int out_dtype, void* stream) {
  return blockwise_impl(0, mat_a, mat_b, scales_a, scales_b, bias, out, workspace, workspace_floats, M, N, K, a_stride_m,
                        b_stride_n, sa_stride_m, sa_stride_k, sb_stride_k, sb_stride_n, out_dtype, stream);
}

extern "C" int sgl_mi355_fp8_blockwise_scaled_mm_wshuffled(
    const void* mat_a, const void* mat_b, const float* scales_a, const float* scales_b, const void* bias, void* out,
    float* workspace, int64_t workspace_floats, int64_t M, int64_t N, int64_t K, int64_t a_stride_m, int64_t sa_stride_m,
    int64_t sa_stride_k, int64_t sb_stride_k, int64_t sb_stride_n, int out_dtype, void* stream) {
  return blockwise_impl(1, mat_a, mat_b, scales_a, scales_b, bias, out, workspace, workspace_floats, M, N, K, a_stride_m, K,
                        sa_stride_m, sa_stride_k, sb_stride_k, sb_stride_n, out_dtype, stream);
}

extern "C" int64_t sgl_mi355_fp8_blockwise_split_k(int64_t M, int64_t K) {
  return (M >= 1 && M <= kStreamMaxRows && K >= 128) ? stream_slices(K) : 1;
}
