// Which FP8 GEMM kernel a shape gets, and with what launch: the whole dispatch rule of gemm_fp8.hip as ONE pure host
// function.  fp8_plan(shape, knobs) launches nothing, keeps no state and touches no pointer; gemm_fp8.hip's launch()
// turns the plan it returns into the template instantiation and the launch, and sgl_mi355_fp8_gemm_plan hands the same
// plan to tests and tools on a machine without a GPU.  Plain C++17, no HIP headers.
#pragma once
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/sgl_mi355.h"

namespace sglm {

// Every tuning / A-B environment variable of the FP8 GEMM host code: name, default and parsing in one line each.  A
// default-constructed Fp8Knobs reads the environment; fp8_knobs() does that once per process.
struct Fp8Knobs {
  static int num(const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; }
  static bool set(const char* name) { return getenv(name) != nullptr; }
  // "a,b[,c]" lists: how many numbers were there (0 when unset), as sscanf counts them
  static int list(const char* name, const char* fmt, int* a, int* b, int* c = nullptr) { const char* e = getenv(name); return e ? sscanf(e, fmt, a, b, c) : 0; }
  unsigned oneshot_max_grid = (unsigned)num("SGL_MI355_ONESHOT_MAX_GRID", 256);  // tuning aid
  int wstream_ph = num("SGL_MI355_WSTREAM_PH", 32);                              // tuning aid (longest phase the streamer's search may take)
  int wstream_force_ph = 0, wstream_force_nc = 0;                                // tuning aid: "PH,nc" for the unsplit (no-slab) form
  int wstream_force_n = list("SGL_MI355_WSTREAM_FORCE", "%d,%d", &wstream_force_ph, &wstream_force_nc);
  int slab_force_ph = 0, slab_force_nc = 0, slab_force_sk = 0;                   // tuning aid: "PH,nc,SK" for the split-K (slab) form
  int slab_force_n = list("SGL_MI355_WSTREAM_SLAB_FORCE", "%d,%d,%d", &slab_force_ph, &slab_force_nc, &slab_force_sk);
  int skinny_nb = 0, skinny_wk = 0;                                              // tuning override: "NB,WK" (NB in {1,2,4}, WK in {2,4,8})
  int skinny_n = list("SGL_MI355_SKINNY", "%d,%d", &skinny_nb, &skinny_wk);
  bool no_astat = set("SGL_MI355_NO_ASTAT");                                     // tuning / A-B aid
  bool no_wstream = set("SGL_MI355_NO_WSTREAM");                                 // tuning / A-B aid
  bool no_wstream_m128 = set("SGL_MI355_NO_WSTREAM_M128");                       // A/B aid (65..128 rows stay on the tiled kernels)
  bool no_wstream_m256 = set("SGL_MI355_NO_WSTREAM_M256");                       // A/B aid (129..256 rows stay on the tiled kernels)
  bool wstream_m256_all = set("SGL_MI355_WSTREAM_M256_ALL");                     // =1 takes the 256-row streamer for every shape (A/B aid)
  bool no_oneshot = set("SGL_MI355_NO_ONESHOT");                                 // tuning / A-B aid
  bool no_prefill_splitk = set("SGL_MI355_NO_PREFILL_SPLITK");                   // A/B aid (no raw split-K tiled3 partials)
  int wstream_min_n = num("SGL_MI355_WSTREAM_MIN_N", 16 * 8 * 100);              // tuning aid (narrowest N of the direct streamer)
  int slab_min_mi = num("SGL_MI355_SLAB_MIN_MI", 0);                             // tuning aid (Mi weights from which slabs pay; 0 = the rule's own)
  int astat_min_mi = num("SGL_MI355_ASTAT_MIN_MI", 40);                          // tuning aid
  int tiled_v2 = num("SGL_MI355_TILED_V2", -1);                                  // 0 off; 2, 3, 8, 48, 84 force a variant
  int tiled_v3 = num("SGL_MI355_TILED_V3", -1);                                  // 0 off; 1 / 2 force 256x256x8 waves / 128x256x4 waves (A/B aid)
  int t3_gn = num("SGL_MI355_T3_GN", 0);                                         // tuning aid (column tiles per rasterisation group)
  int t3_cb = num("SGL_MI355_T3_CB", 0);                                         // =3|4 forces the 128 x 192 / 128 x 256 tile (A/B aid)
  int t3_ks = num("SGL_MI355_T3_KS", 0);                                         // =1|2 forces one / two k groups (A/B aid)
  bool tiled_scaled = num("SGL_MI355_TILED_SCALED", 1) != 0;                     // A-B aid (0: four plain MFMAs per k-step in the `tiled` kernel)
  int silu_gemm_min_tiles = num("SGL_MI355_SILU_GEMM_MIN_TILES", 192);           // tuning aid
};

inline const Fp8Knobs& fp8_knobs() {
  static const Fp8Knobs k;
  return k;
}

enum class Fp8Kind { MM = SGL_MI355_FP8_PLAN_MM, PARTIALS = SGL_MI355_FP8_PLAN_PARTIALS, PARTIALS_A16 = SGL_MI355_FP8_PLAN_PARTIALS_A16,
                     SILU_MUL = SGL_MI355_FP8_PLAN_SILU_MUL };

// What the decision depends on, and nothing else.
struct Fp8Shape {
  int64_t M, N, K;
  int64_t a_sm, b_sn;   // bytes between rows of A / of W (GemmArgs)
  int b_shuf;           // W in the pre-shuffled layout
  bool has_ws;          // a split-K workspace was passed ...
  int64_t ws_floats;    // ... of this many floats
  Fp8Kind kind;
};

// As the entry points fill GemmArgs: a pre-shuffled weight has no row stride (K stands in), and the a16 form stages its
// activations itself (`a` unused, a_sm = K).
inline Fp8Shape fp8_shape(Fp8Kind kind, int64_t M, int64_t N, int64_t K, int64_t a_sm, int64_t b_sn, int b_shuf, bool has_ws,
                          int64_t ws_floats) {
  return Fp8Shape{M, N, K, kind == Fp8Kind::PARTIALS_A16 ? K : a_sm, b_shuf ? K : b_sn, b_shuf ? 1 : 0, has_ws, ws_floats, kind};
}

enum class Fp8Family { NONE, SKINNY, ONESHOT, ASTAT, ASTAT_DIRECT, WSTREAM, WSTREAM_SLAB, TILED, TILED2, TILED3, TILED3_KS2, TILED3_SILU,
                       TILED3_RAWK };

// the exact strings sgl_mi355_fp8_last_kernel() reports
inline const char* fp8_family_name(Fp8Family f) {
  static const char* const names[] = {"", "skinny", "oneshot", "astat", "astat_direct", "wstream", "wstream_slab", "tiled", "tiled2",
                                      "tiled3", "tiled3_ks2", "tiled3_silu", "tiled3_rawk"};
  return names[(int)f];
}

// The public record (family name, template selectors, launch geometry, runtime kernel arguments: include/sgl_mi355.h) plus
// the outcome: rc != 0 is "no kernel for this shape", with the text set_error() gets.
struct Fp8Plan : sgl_mi355_fp8_plan {
  Fp8Family fam = Fp8Family::NONE;
  int rc = 0;
  char error[256] = "";
  Fp8Plan() : sgl_mi355_fp8_plan{} {}
  void family_is(Fp8Family f) {
    fam = f;
    snprintf(family, sizeof(family), "%s", fp8_family_name(f));
    grid_y = 1;
  }
};

// rows of the decode kernels' A image / 16 (M <= 64)
inline int mb_of(int64_t M) { return M <= 16 ? 1 : M <= 32 ? 2 : 4; }

// ---- dynamic LDS of each kernel form: the plan's `lds` and the launcher's per-instantiation attribute are the same number
constexpr int imax(int a, int b) { return a > b ? a : b; }
constexpr int skinny_lds(int mb, int nb, int wk) { return wk * mb * 16 * 16 * nb * 4; }
constexpr int wstream_lds(int mb, int ph, bool slab) {
  return imax(2 * ph * 16 * mb * 128,                      // the two A buffers
              8 * 16 * mb * (slab ? 20 * 4 : 24 * 2));     // epilogue patches of up to 8 consumer waves
}
// gemm_fp8.hip AStat<MB>
constexpr int astat_step_bytes(int mb) { return 4 * (16 * mb * 32 + 16); }
constexpr int astat_max_steps(int mb) { return (150 * 1024) / astat_step_bytes(mb); }
constexpr int kAstatWaves = 16;
constexpr int kTiledLds = 2 * 2 * (4 * (128 * 32 + 16) + 48);  // gemm_fp8.hip 2 * kStageBytes
constexpr int tiled2_lds(int nstage, int ri, int wm, int wn) {
  return imax(nstage * (16 * ri * wm + 64 * wn) * 128, wm * wn * 64 * 72 * 2);
}
constexpr int tiled3_lds(int wm, int cb, int ks) {
  return ks == 2 ? imax(3 * 2 * 128 * 128, 4 * 8 * cb * 4 * 64 * 4)   // stages | the k groups' hand-over area
                 : imax(3 * 128 * wm * 128, wm * 4 * 64 * 72 * 2);    // stages | epilogue patches
}

// picks (S, WK) with WK * S == K / 128, S <= 4, WK <= 8; false when the shape does not qualify
inline bool plan_oneshot(const Fp8Shape& p, const Fp8Knobs& k, Fp8Plan& pl) {
  const int MB = mb_of(p.M);
  if ((p.K & 127) != 0 || (p.N & 7) != 0) return false;
  if ((!p.b_shuf && p.N * p.b_sn >= ((int64_t)1 << 32)) || p.M * p.a_sm >= ((int64_t)1 << 32)) return false;
  const int steps = (int)(p.K >> 7);
  int S = 0;
  for (int c = 1; c <= 4; ++c)
    if (steps % c == 0 && steps / c <= 8) { S = c; break; }
  if (S == 0) return false;
  const int WK = steps / S;
  const unsigned grid = (unsigned)((p.N + 15) / 16);
  // M > 32: 167 VGPRs -> one workgroup per CU; a second round of workgroups (N = 6144: 384) costs more than the
  // pipelined kernel's 32-column tiles (measured 23.0 vs 20.6 us), so only take shapes that fit one round.
  // (one k-step per wave is cheap enough for several rounds: K = 1024, N = 8192 -- 512 workgroups -- 8.2 us vs 14.4)
  if (MB == 4 && grid > k.oneshot_max_grid && !(S == 1 && grid <= 1024)) return false;
  pl.family_is(Fp8Family::ONESHOT);
  pl.mb = MB; pl.s = S; pl.wk = WK;
  pl.grid_x = (int32_t)grid; pl.block = 64 * WK; pl.lds = WK * MB * 16 * 16 * 4;
  return true;
}

// The weight streamer.  Shapes: K % 128 == 0 and K / 128 a multiple of a phase length PH in {32, 16, 8} (PH * MB <= 32).
// !slabs: one workgroup per 8 column blocks over all of K (wide N).  Otherwise K is split into SK slices of whole phases so
// that ~256 workgroups exist, partials go to fp32 slabs and a finalize kernel applies the reference epilogue (narrow N,
// long K: down_proj).  partials: leave the raw fp32 partial sums in the slabs (any slice count >= 1); the epilogue runs
// inside the consumer kernel (sgl_mi355_*_from_partials).
inline bool plan_wstream(const Fp8Shape& p, const Fp8Knobs& k, int MB, bool slabs, Fp8Plan& pl) {
  const bool partials = p.kind != Fp8Kind::MM;
  if ((p.K & 127) != 0 || (p.N & 7) != 0 || (p.a_sm & 15) != 0) return false;
  if (!p.b_shuf && p.N * p.b_sn >= ((int64_t)1 << 32)) return false;  // per-lane weight offsets are 32-bit
  const int steps = (int)(p.K >> 7);
  const int nblocks = (int)((p.N + 15) / 16);
  // Pick (PH, consumer waves, K slices): one workgroup per CU (the A buffers fill most of the LDS) and a CU draws
  // only ~10 B/clk from HBM, so minimise the k-steps on the busiest CU (+ ~4 steps' worth of barrier per phase).
  // Without slabs: all of K per workgroup, longest phase (N = 28672: 7 consumers -> exactly 256 workgroups).
  int PH = 0, nc = 8, SK = 1, pps = 0;
  int64_t best = 1 << 30;
  // K / 128 not a multiple of 8 (e.g. 3584 = 28 steps): phases of 4 steps, four weight steps in flight
  // (phases of 2 steps for the split-K form -- 192 workgroups instead of 48 on the TP = 8 qkv shape 4096 x 768 -- were
  //  tried: one rank's TP = 4 / 8 step 3.07 -> 3.04 / 2.42 -> 2.45 ms, i.e. nothing; those shapes are launch-bound)
  const int ph_min = MB >= 16 ? 2 : (steps % 8 == 0 && MB <= 4) ? 8 : 4;  // (MB = 8 / 16: 4 / 2 steps are the 64-KiB buffer)
  for (int ph = 32 / MB; ph >= ph_min; ph >>= 1) {
    if (ph > k.wstream_ph && ph > 8) continue;
    if (steps % ph != 0) continue;
    const int P = steps / ph;
    for (int c = 8; c >= 4; --c) {
      const int groups_c = (nblocks + c - 1) / c;
      int sk = 1, pp = P;
      if (slabs) {
        int sk_max = 256 / groups_c;
        if (sk_max < 1) sk_max = 1;
        if (sk_max > P) sk_max = P;
        pp = (P + sk_max - 1) / sk_max;
        sk = (P + pp - 1) / pp;
      }
      const int rounds = (groups_c * sk + 255) / 256;
      const int64_t cost = (int64_t)rounds * c * pp * (ph + (MB >= 16 ? 1 : 4));  // (a barrier per two steps is the only form at 256 rows)
      if (cost < best) { best = cost; PH = ph; nc = c; SK = sk; pps = pp; }
    }
    if (!slabs) break;  // the longest phase that divides K
  }
  const auto force_ok = [&](int fph, int fnc) {
    return (fph == 4 || fph == 8 || fph == 16 || fph == 32) && fph * MB <= 32 && steps % fph == 0 && fnc >= 1 && fnc <= 8;
  };
  if (k.wstream_force_n == 2 && !slabs && force_ok(k.wstream_force_ph, k.wstream_force_nc)) {
    PH = k.wstream_force_ph;
    nc = k.wstream_force_nc;
    SK = 1;
    pps = steps / PH;
  }
  if (k.slab_force_n == 3 && slabs && force_ok(k.slab_force_ph, k.slab_force_nc) && k.slab_force_sk >= 1) {
    const int P = steps / k.slab_force_ph;
    PH = k.slab_force_ph;
    nc = k.slab_force_nc;
    pps = (P + k.slab_force_sk - 1) / k.slab_force_sk;
    SK = (P + pps - 1) / pps;
  }
  if (PH == 0) return false;
  if (p.kind == Fp8Kind::PARTIALS_A16 && (!slabs || pps != 1)) return false;  // the a16 fill covers single-phase slices only
  const int groups = (nblocks + nc - 1) / nc;
  if (slabs && ((SK < 2 && !partials) || p.ws_floats < (int64_t)SK * p.M * p.N)) return false;
  // the phase lengths the kernel is built with: 32 at MB = 1, 16 up to MB = 2, 8 up to MB = 4, 4 up to MB = 8, 2 at MB = 16
  // (MB = 8 / 16 have phases of four / two k-steps only)
  if (MB == 1 && PH == 32) pl.ph = 32;
  else if (MB <= 2 && PH == 16) pl.ph = 16;
  else if (MB <= 8 && PH == 4) pl.ph = 4;
  else if (MB <= 4) pl.ph = 8;
  else if (MB == 16 && PH == 2) pl.ph = 2;
  else return false;
  pl.family_is(slabs ? Fp8Family::WSTREAM_SLAB : Fp8Family::WSTREAM);
  pl.mb = MB;
  pl.grid_x = groups; pl.grid_y = SK; pl.block = 64 * (nc + 1); pl.lds = wstream_lds(MB, pl.ph, slabs);
  pl.sk = SK; pl.per_slice = pps; pl.waves = nc; pl.groups = groups;
  pl.finalize = slabs && !partials;
  return true;
}

// wide N with a K tail or an odd step count: the A-stationary kernel without slabs (phase-filled A image)
inline bool plan_astat_direct(const Fp8Shape& p, Fp8Plan& pl) {
  const int MB = mb_of(p.M);
  const int steps_total = (int)((p.K + 127) >> 7);
  const int nblocks = (int)((p.N + 15) / 16);
  int max_steps = astat_max_steps(MB) & ~7;  // multiple of the prefetch depth
  int SK = (steps_total + max_steps - 1) / max_steps;
  int steps_per_slice = (((steps_total + SK - 1) / SK) + 7) & ~7;
  if (steps_per_slice > max_steps) return false;
  SK = (steps_total + steps_per_slice - 1) / steps_per_slice;
  if (p.N * p.b_sn >= ((int64_t)1 << 32)) return false;  // per-lane weight offsets are 32-bit
  const int ns_last = steps_total - (SK - 1) * steps_per_slice;
  const bool exact = (p.K & 127) == 0 && (ns_last & 7) == 0;
  // waves per workgroup: one workgroup per CU (the A image fills the LDS), so pick the count that leaves
  // the fewest column blocks on the busiest CU (N = 28672: 7 waves -> 256 workgroups, 8 -> only 224).
  // (measured at N = 28672: M = 16 28.0 us with 7 waves vs 29.0 with 8; M = 64 prefers 8 waves: 39.9 vs 42.3)
  int nw = 8, best = 1 << 30;
  for (int c = 8; c >= (MB == 4 ? 8 : 4); --c) {
    const int blocks = (nblocks + c - 1) / c;
    const int cost = ((blocks + 255) / 256) * c;
    if (cost < best) { best = cost; nw = c; }
  }
  pl.family_is(Fp8Family::ASTAT_DIRECT);
  pl.mb = MB; pl.exact = exact;
  pl.grid_x = (nblocks + nw - 1) / nw; pl.block = 64 * nw;
  pl.lds = imax(steps_per_slice * astat_step_bytes(MB), 8 * 16 * MB * 24 * 2);  // the A image | the epilogue patches
  pl.sk = SK; pl.per_slice = steps_per_slice; pl.waves = nw;
  return true;
}

// narrow N, very long K on a row-major weight: the A-stationary kernel with split-K slabs + finalize
inline bool plan_astat(const Fp8Shape& p, Fp8Plan& pl) {
  const int MB = mb_of(p.M);
  const int max_steps = astat_max_steps(MB);
  const int steps_total = (int)((p.K + 127) >> 7);
  const int nblocks = (int)((p.N + 15) / 16);
  // K-slices: at least enough for the slice of A to fit LDS; more when N is narrow, so that there are
  // >= ~2048 (column block, slice) items for 256 CUs x 8+ waves -- but never below 4 k-steps per item.
  int SK = (steps_total + max_steps - 1) / max_steps;
  const int want = (2048 + nblocks - 1) / nblocks;
  if (SK < want) SK = want;
  if (SK > steps_total / 4) SK = steps_total / 4;
  if (SK < 1) SK = 1;
  const int steps_per_slice = (steps_total + SK - 1) / SK;
  SK = (steps_total + steps_per_slice - 1) / steps_per_slice;
  if (steps_per_slice > max_steps) return false;
  if (!p.has_ws || p.ws_floats < (int64_t)SK * p.M * p.N) return false;
  int ngroups = 256 / SK;
  if (ngroups > nblocks) ngroups = nblocks;
  if (ngroups < 1) ngroups = 1;
  int nwaves = (nblocks + ngroups - 1) / ngroups;
  if (nwaves > kAstatWaves) nwaves = kAstatWaves;
  pl.family_is(Fp8Family::ASTAT);
  pl.mb = MB;
  pl.grid_x = ngroups * SK; pl.block = 64 * nwaves; pl.lds = steps_per_slice * astat_step_bytes(MB);
  pl.sk = SK; pl.per_slice = steps_per_slice; pl.waves = nwaves; pl.groups = ngroups;
  pl.finalize = 1;
  return true;
}

inline void plan_skinny(const Fp8Shape& p, const Fp8Knobs& k, Fp8Plan& pl) {
  // Wide N: 64-column wave tiles (activation L2 traffic = 1x the weight stream), K split 4 ways.
  // Narrow N: 32-column tiles and a deeper K split so that enough waves are in flight.
  int nb = (p.N >= 12288) ? 4 : 2;
  int wk = (p.N >= 12288) ? 4 : 8;
  if (k.skinny_n >= 1) nb = k.skinny_nb;
  if (k.skinny_n >= 2) wk = k.skinny_wk;
  // the built forms: NB in {1, 2, 4} x WK in {2, 4, 8}; anything else lands on the form's default WK / on NB = 2
  if (nb == 4) wk = (wk == 2 || wk == 8) ? wk : 4;
  else if (nb == 1) wk = (wk == 2 || wk == 4) ? wk : 8;
  else { nb = 2; wk = (wk == 2 || wk == 4) ? wk : 8; }
  pl.family_is(Fp8Family::SKINNY);
  pl.mb = mb_of(p.M); pl.nb = nb; pl.wk = wk;
  pl.grid_x = (int32_t)((p.N + 16 * nb - 1) / (16 * nb)); pl.block = 64 * wk; pl.lds = skinny_lds(pl.mb, nb, wk);
}

inline void plan_tiled3(const Fp8Shape& p, Fp8Family f, int wm, int cb, int ks, int raster_gn, Fp8Plan& pl) {
  pl.family_is(f);
  pl.wm = wm; pl.cb = cb; pl.ks = ks; pl.silu = f == Fp8Family::TILED3_SILU; pl.rawk = f == Fp8Family::TILED3_RAWK;
  const int tmb = 128 * wm, tnb = pl.silu ? 128 : 64 * cb;  // silu * mul: a tile's 128 gate + 128 up columns make 128 of the N / 2 outputs
  pl.grid_x = (int32_t)(unsigned)(((p.M + tmb - 1) / tmb) * (((pl.silu ? p.N >> 1 : p.N) + tnb - 1) / tnb));
  pl.block = 256 * wm * ks; pl.lds = tiled3_lds(wm, cb, ks);
  pl.raster_gn = raster_gn;
}

__attribute__((format(printf, 2, 3))) inline void unsupported(Fp8Plan& pl, const char* fmt, ...) {
  pl = Fp8Plan();
  pl.rc = SGL_MI355_ERR_UNSUPPORTED;
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(pl.error, sizeof(pl.error), fmt, ap);
  va_end(ap);
}

// fp8_scaled_mm(_wshuffled): the order of attempts.  A rung that declines (shape, 32-bit weight offsets, workspace too
// small, no phase length, ...) hands the shape to the next one.
inline void plan_mm(const Fp8Shape& p, const Fp8Knobs& k, Fp8Plan& pl) {
  if (p.M <= 64) {
    // >= ~100 workgroups of 8 column blocks (M = 64, K = 4096: N = 14336 21.6 us here vs 24.1 one-shot; at N = 7168 and
    // below the two tie or the one-shot kernel wins -- those shapes are latency-, not bandwidth-bound)
    if (!k.no_wstream && p.N >= k.wstream_min_n && plan_wstream(p, k, mb_of(p.M), false, pl)) return;
    // same shapes, K tails / odd step counts: phase-filled A image
    if (!k.no_astat && !p.b_shuf && p.N >= 16 * 8 * 160 && plan_astat_direct(p, pl)) return;
    // split-K slabs pay a finalize launch (~4 us): worth it from 40 Mi weights, and from 20 Mi at M > 32 where
    // the alternative re-reads the activations from L2 per wave (qkv 4096x6144: 12.6 + 4.2 us vs 21.2)
    const int steps128 = (int)(p.K >> 7);  // the one-shot kernel takes K/128 = WK * S with S <= 4, WK <= 8
    const bool oneshot_ok = (p.K & 127) == 0 && (steps128 <= 8 || (steps128 <= 32 && (steps128 % 4 == 0 || steps128 % 3 == 0 ||
                                                                                        (steps128 % 2 == 0 && steps128 <= 16))));
    const int64_t slab_min = (int64_t)(k.slab_min_mi ? k.slab_min_mi : (p.M > 32 ? (oneshot_ok ? 20 : 8) : 40)) << 20;
    // narrow N, long K: K split over workgroups, fp32 slabs
    if (!k.no_wstream && p.has_ws && p.N * p.K >= slab_min && plan_wstream(p, k, mb_of(p.M), true, pl)) return;
    if (!k.no_astat && !p.b_shuf && p.has_ws && p.N * p.K >= ((int64_t)k.astat_min_mi << 20) && plan_astat(p, pl)) return;
    if (!k.no_oneshot && plan_oneshot(p, k, pl)) return;
    if (p.b_shuf) {  // a pre-shuffled weight is only read by the weight-streaming, one-shot and tiled-v2 kernels
      if (plan_wstream(p, k, mb_of(p.M), false, pl)) return;
      unsupported(pl, "fp8_scaled_mm (pre-shuffled weight): no kernel for M=%d N=%d K=%d", (int)p.M, (int)p.N, (int)p.K);
      return;
    }
    plan_skinny(p, k, pl);
    return;
  }
  if (p.M <= 128) {
    // 65..128 rows (a decode batch of up to 128): still weight-bound, and the tiled kernels below would put these shapes on
    // N / 128 CUs (down_proj 4096 x 14336 at M = 128: 32 tiles, 64.8 us).  The weight streamer with 128-row A phases (MB = 8,
    // phases of four k-steps) keeps every CU streaming: direct form for wide N, split-K slabs + finalize otherwise.
    if (!k.no_wstream && !k.no_wstream_m128 && (p.K & 511) == 0) {
      if (p.N >= k.wstream_min_n && plan_wstream(p, k, 8, false, pl)) return;
      // split-K form from 8 Mi weights.  Eager launch loops, M = 128, us, tiled -> streamer: down_proj (4096 x 14336) 64.8 -> 25.8,
      // gate_up direct 31.5 -> 30.1, but o_proj (4096 x 4096) 21.3 -> 30.9 and qkv 22.0 -> 23.3; in the graph-replayed model step
      // (where the finalize launch costs a boundary, not a launch gap) taking all of them is still ahead: Llama-3-8B bs = 128
      // 11.18 ms tiled -> 10.03 with down / gate_up only -> 9.86 with all four; bs = 96 8.86 -> 8.63 (same box)
      if (p.has_ws && p.N * p.K >= ((int64_t)8 << 20) && plan_wstream(p, k, 8, true, pl)) return;
    }
  }
  if (p.M <= 256) {
    // 129..256 rows: the same again with a 256-row A image and phases of two k-steps (MB = 16).  Measured: see DESIGN 4.8.9.
    // At 256 rows the streamer is MFMA- / LDS-bound itself (64 MFMAs and 32 KB of fragment reads per wave and k-step), so only
    // the long-K, narrow-N layers gain, where the tiled kernels run on N / 128 CUs (eager loops, M = 256, us, tiled -> streamer:
    // down_proj 4096 x 14336 64.4 -> 37.7; gate_up 44.9 -> 54.7, qkv 22.4 -> 27.7, o 20.8 -> 25.7 stay tiled).
    const bool all256 = k.wstream_m256_all;
    if (!k.no_wstream && !k.no_wstream_m256 && (p.K & 511) == 0) {
      if (all256 && p.N >= k.wstream_min_n && plan_wstream(p, k, 16, false, pl)) return;
      if (p.has_ws && p.N * p.K >= ((int64_t)(all256 ? 8 : 40) << 20) && (all256 || p.K >= 2 * p.N) && plan_wstream(p, k, 16, true, pl))
        return;
    }
  }
  if (p.b_shuf && (p.K & 127) != 0) {
    unsupported(pl, "fp8_scaled_mm (pre-shuffled weight): K must be a multiple of 128");
    return;
  }
  // v2 (LDS-DMA + block-scaled MFMA) whenever K has no tail; variant by tile count (see the kernel's comment).
  const unsigned grid_s = (unsigned)(((p.M + 127) / 128) * ((p.N + 127) / 128));
  // Selection (measured, M = 4096 / 512, PFLOP/s): 256x256 x 8 waves 1.62-2.26 wherever there are enough of the big
  // tiles (>= 192: three quarters of the CUs) -- e.g. 2.05 vs 1.57 at 4096x4096x4096; 128x128: with at most one tile per
  // CU three stages and EIGHT waves (32x64 per wave: two waves per SIMD hide each other's latency; M = 1024 o/down
  // 26.7 / 74.4 us vs 29.0 / 81.9 with four waves), else two stages x two workgroups per CU.
  // (A 4-wave 256x256 with 128x128 wave tiles -- MFMA-bound on paper -- reached only 1.47-2.12: with one wave per SIMD
  //  every barrier and first-fragment latency is exposed.)
  const unsigned grid_b = (unsigned)(((p.M + 255) / 256) * ((p.N + 255) / 256));
  int v2 = k.tiled_v2 >= 0 ? k.tiled_v2 : (grid_b >= 192 ? 84 : (grid_s <= 256 ? 22 : 2));
  if (p.b_shuf && v2 == 0) v2 = 2;  // the register-staged predecessor below does not read the pre-shuffled layout
  // v3 (weights global -> VGPR, pre-shuffled weights only) from 192 tiles of 128 x 256 (same box, us, v2 -> v3: M = 1024 qkv
  // 38.4 -> 36.5, gate_up 116.4 -> 111.6; M = 2048 o 40.6 -> 37.6, down 122.0 -> 100.4; M = 4096 qkv 123.9 -> 93.5, gate_up
  // 436 -> 396; M = 8192 gate_up 920 -> 774, down 397 -> 358; below that the 128 x 128 v2 tiles fill the chip better).
  // Column tiles per rasterisation group: 4 (1 / 2 / 4 / 8 / 16 at M = 4096 gate_up: 437 / 418 / 408 / 403 / 435 us).
  const int v3 = k.tiled_v3;
  const int raster_gn = k.t3_gn > 0 ? k.t3_gn : 4;
  // 128 x 256 tiles, or 128 x 192 where that leaves less work on the busiest CU: tiles per CU (rounded up) x tile width.  Only
  // the qkv-like widths gain (4096 -> 6144, same box, 256- vs 192-wide: M = 1024 36.5 -> 33.9 us, 192 -> 256 tiles; M = 2048
  // 53.0 -> 49.6, 384 -> 512 tiles); wherever the products tie the wider tile wins (M = 4096 93.2 vs 102.4) and forcing the
  // narrow one elsewhere costs 10-20 % (profiles/r03_prefill_gemm_cb3.txt).
  const unsigned tiles_m3 = (unsigned)((p.M + 127) / 128);
  const unsigned grid_4 = tiles_m3 * (unsigned)((p.N + 255) / 256), grid_c3 = tiles_m3 * (unsigned)((p.N + 191) / 192);
  const unsigned cost4 = ((grid_4 + 255) / 256) * 4, cost3 = ((grid_c3 + 255) / 256) * 3;
  const int cb = (k.t3_cb == 3 || k.t3_cb == 4) ? k.t3_cb : (cost3 < cost4 ? 3 : 4);
  const unsigned grid_3 = cb == 3 ? grid_c3 : grid_4;
  if (p.b_shuf && (p.K & 511) == 0 && (v3 > 0 || (v3 != 0 && grid_3 >= 192))) {
    // one tile per CU or fewer (M = 1024 qkv: 256 tiles of 128 x 192): the eight-wave form with two k groups (see the kernel)
    if (v3 <= 0 && (k.t3_ks == 2 || (k.t3_ks != 1 && grid_3 <= 256))) return plan_tiled3(p, Fp8Family::TILED3_KS2, 1, cb, 2, raster_gn, pl);
    if (v3 == 1) return plan_tiled3(p, Fp8Family::TILED3, 2, 4, 1, raster_gn, pl);
    // Round 5: few row tiles x a very wide output (M = 1024 gate_up of Llama-3-8B: 4 x 112 tiles of 256 x 256 = 1.75 rounds of one
    // eight-wave workgroup per CU) take the 256 x 256 form: 112.0 vs 124.4-126.8 us for the 128 x 256 form's 896 tiles (the same
    // 1.75 rounds at two per CU, half the operand reuse per byte entering the CU), and ahead of the vendor library's 116.4
    // (profiles/r05_prefill_gemm_forms.txt).  Everywhere else measured the 256 x 256 form loses (M = 1024 qkv / o / down: 53 / 50 /
    // 147 us against 33 / 25 / 72; M = 4096 qkv / gate_up / down 108 / 418 / 186 against 92 / 393 / 180), so the rule is narrow.
    if (v3 < 0 && (p.M + 255) / 256 <= 4 && grid_b >= 384 && grid_b <= 512) return plan_tiled3(p, Fp8Family::TILED3, 2, 4, 1, raster_gn, pl);
    return plan_tiled3(p, Fp8Family::TILED3, 1, cb, 1, raster_gn, pl);
  }
  if (v2 && (p.K & 127) == 0) {
    struct V2 { int v, nstage, ri, wm, wn; };
    static const V2 forms[] = {{22, 3, 2, 4, 2},  // 128x128 with 8 waves (32x64 per wave)
                               {84, 2, 8, 2, 4}, {48, 3, 4, 4, 2}, {8, 3, 8, 2, 2}, {2, 2, 4, 2, 2}, {-1, 3, 4, 2, 2}};
    const V2* f = forms;
    while (f->v != v2 && f->v != -1) ++f;  // (any other number: three stages of 128x128 on four waves)
    pl.family_is(Fp8Family::TILED2);
    pl.nstage = f->nstage; pl.ri = f->ri; pl.wm = f->wm; pl.wn = f->wn;
    const int tmb = 16 * f->ri * f->wm, tnb = 64 * f->wn;
    pl.grid_x = (int32_t)(unsigned)(((p.M + tmb - 1) / tmb) * ((p.N + tnb - 1) / tnb));
    pl.block = 64 * f->wm * f->wn; pl.lds = tiled2_lds(f->nstage, f->ri, f->wm, f->wn);
    return;
  }
  pl.family_is(Fp8Family::TILED);
  pl.scaled = k.tiled_scaled;
  pl.grid_x = (int32_t)grid_s; pl.block = 256; pl.lds = kTiledLds;
}

// fp8_scaled_mm_partials(_wshuffled / _a16): raw split-K partial sums for a consumer that runs the epilogue
inline void plan_partials(const Fp8Shape& p, const Fp8Knobs& k, Fp8Plan& pl) {
  if (p.kind == Fp8Kind::PARTIALS_A16) {
    if (p.M > 64) {
      unsupported(pl, "fp8_scaled_mm_partials_a16: only the decode kernels (M <= 64) have this form");
    } else if (!plan_wstream(p, k, mb_of(p.M), true, pl)) {
      unsupported(pl, "fp8_scaled_mm_partials_a16: shape (M=%ld N=%ld K=%ld) has no single-phase split-K form", (long)p.M, (long)p.N, (long)p.K);
    }
    return;
  }
  if (p.M > 128) {
    // prefill sizes (round 5): the tiled kernel's raw split-K form where 128 x 256 tiles alone would leave the chip half empty
    // and K is long enough to cut -- down_proj 14336 -> 4096 at 512 / 1024 rows (tools/exp/splitk_prefill_probe.py: the GEMM body
    // 85 -> 57 us at 1024 rows).  Everything else has no such form: the caller runs the GEMM that finishes itself.
    const int64_t tiles = ((p.M + 127) / 128) * ((p.N + 255) / 256);
    const int64_t steps = p.K >> 7;
    int S = tiles > 0 ? (int)(256 / tiles) : 0;
    if (S > 4) S = 4;
    while (S >= 2 && (steps % S != 0 || (steps / S) % 4 != 0 || steps / S < 16)) --S;
    if (k.no_prefill_splitk || !p.b_shuf || !(p.N > 0 && p.K > 0 && p.N % 16 == 0 && p.K % 512 == 0) || p.K < 8192 || S < 2 ||
        (p.N & 7) != 0 || p.ws_floats < (int64_t)S * p.M * p.N) {
      unsupported(pl, "fp8_scaled_mm_partials: no split-K form for M=%ld N=%ld K=%ld (prefill sizes: pre-shuffled weight, K >= 8192, "
                  "at most 128 tiles of 128 x 256)", (long)p.M, (long)p.N, (long)p.K);
      return;
    }
    plan_tiled3(p, Fp8Family::TILED3_RAWK, 1, 4, 1, 4, pl);
    pl.grid_x = (int32_t)tiles; pl.grid_y = S;
    pl.sk = S; pl.k_steps_per_slice = (int)(steps / S);
    return;
  }
  if (!plan_wstream(p, k, p.M <= 64 ? mb_of(p.M) : 8, true, pl))  // (65..128 rows: 128-row phases)
    unsupported(pl, "fp8_scaled_mm_partials: shape (M=%ld N=%ld K=%ld) is not on the split-K weight-streaming path", (long)p.M,
                (long)p.N, (long)p.K);
}

// Which kernel does (M, N, K) get, and why: read this function and the plan_* rungs it names, in order.
inline Fp8Plan fp8_plan(const Fp8Shape& p, const Fp8Knobs& k) {
  Fp8Plan pl;
  switch (p.kind) {
    case Fp8Kind::MM: plan_mm(p, k, pl); break;
    case Fp8Kind::PARTIALS:
    case Fp8Kind::PARTIALS_A16: plan_partials(p, k, pl); break;
    case Fp8Kind::SILU_MUL: {
      // gate_up with silu * mul in the epilogue: prefill sizes only, at least 192 tiles of 128 rows x 128 output columns
      const int64_t tiles = ((p.M + 127) / 128) * ((p.N / 2 + 127) / 128);
      if (p.M <= 64 || tiles < k.silu_gemm_min_tiles)
        unsupported(pl, "fp8_scaled_mm_silu_mul: only prefill sizes (M > 64, at least %d tiles of 128 x 128 outputs) have the fused form",
                    k.silu_gemm_min_tiles);
      else plan_tiled3(p, Fp8Family::TILED3_SILU, 1, 4, 1, k.t3_gn > 0 ? k.t3_gn : 4, pl);
      break;
    }
  }
  return pl;
}

}  // namespace sglm
