// laser_amd/csrc/asm_plan.h -- the launch model of the hand-scheduled assembly kernels: which kernel (asm_kernels.h) and which launch
// plan (plain, K-cut, strided, hybrid) a GEMM or a convolution gets, and the scheduler block of the kernel arguments that says so to
// the kernel.  Host arithmetic only: no HIP header, no device, and no global -- the options a decision depends on arrive as one
// AsmOptions value, taken once per call by the launcher (gemm_f32_asm.cpp), so a launch is planned under one setting even while
// another thread changes an option.  tests/cpp/asm_plan_host.cpp builds this header with g++ alone.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cmath>

#include "asm_kernels.h"
#include "gemm_args.h"

namespace laser_hip {

// The options the model reads (include/laser_hip.h documents each under its name), as the launcher found them at the start of a call
struct AsmOptions {
  int asm_plan = 0;          // 0 = the launch model decides; 1 = one tile per workgroup only; 2 = K-slice cuts, 3 = strided whole tiles, 4 = hybrid, whenever legal
  int asm_kernel = -1;       // force an index of kKernels (tuning sweeps); -1 = the model decides
  int asm_tile = -1;         // the tile class pinned for this thread's launches (the thread's own pin, else option "asm_tile"); -1 = none
  int asm_wgs = 0, asm_slice = 0;   // workgroups of a persistent launch (0 = every slot of the chip); K-tiles per slice of a cut one-chain launch (0 = the model decides)
  int asm_group_m = 0;       // tile rows per raster group of the f32 GEMM launches (0 = 4 for 256-row tiles, else 8); f64 launches: always 8
  int split_tail = 1;        // 0 = never cut a tile along K
  int f32_asm = 1, f64_asm = 1;   // 0 = never the assembly kernels; 1 = where the model expects them ahead; 2 = whenever eligible
  int conv_walk = 1;         // the convolution's unit walkers: 1 = where they apply, 0 = never, 2 = whenever there are two units, >= 3: that many workgroups
  int asm_noseed = 0, asm_test_giveup = 0;   // tests: 1 = a piece never takes its received sum early (the two-run receive path); 1 = every receiver of a cut launch gives up at once (the error report)
};

// the scheduler block of the kernel arguments (f32_kernel.py KA_SCHED): the workgroup -> tile map is arithmetic in the kernel
// (XCD-aware chunking of the workgroup ids + grouped raster: the ic / jr partition of gemm.nim:160-176), no table
struct SchedArgs {
  uint32_t tiles_m, tiles_n, group_m, gsz_last, mg_width, mg_gm, mg_last, xcd_q;
  uint32_t xcd_r, P, mg_P, units_q, units_r, slice_len, flags_bits, mg_G;
  uint64_t ws, flags;
};
static_assert(sizeof(SchedArgs) == 80, "f32_kernel.py KA_SCHED");

// x / d in the kernels = mulhi(x, magic(d)) with magic(d) = floor(2^32 / d) + 1 (0 for d == 1): exact while x * d < 2^32
inline uint32_t magic_u32(uint64_t d) { return d <= 1 ? 0u : (uint32_t)(((uint64_t)1 << 32) / d + 1); }

// G workgroups walk equal shares of the T * P units of T tiles: some tile straddles two workgroups (an XCD's share of the tiles may be
// one more or less than T / 8: then its units do not divide evenly even where U / G does)
inline bool plan_cuts_a_tile(int64_t T, int64_t P, int64_t G) {
  const int64_t U = T * P;
  return U % G != 0 || (U / G) % P != 0 || (G >= 8 && T % 8 != 0);
}
// launches that cut tiles run two-level (fill_sched): 8 XCDs x G / 8 workgroups; with eight or more workgroups nothing else is legal
inline bool plan_two_level(bool cuts, int64_t T, int64_t G) { return cuts && G >= 8 && G % 8 == 0 && T >= 8; }

// Tile map + unit arithmetic of a launch of G workgroups over tiles_m x tiles_n tiles, each cut into P slices of slice_len
// elements of K (P == 1: no cut).  two_level (launches that cut tiles, G a multiple of 8): XCD x = workgroup id % 8 owns the whole
// tiles [T x / 8, T (x + 1) / 8) and its G / 8 workgroups share them -- a cut tile's sender is always started before its receiver
// (asmgen/f32_kernel.py KA_SCHED).  ws / flags: the device addresses of the stream's workspace and of its first hand-over flag (0: a
// launch that cuts nothing).  false: a quotient of the in-kernel arithmetic would leave the range of its magic number.
inline bool fill_sched(SchedArgs &sc, int64_t tiles_m, int64_t tiles_n, int group_m, int64_t G, int64_t P, int64_t slice_len, uint64_t ws, uint64_t flags,
                       bool xcd, bool two_level, const AsmOptions &o, int64_t T_cover = 0) {
  // (T_cover: the launch covers that many tiles of the raster only -- the unit arithmetic runs over them, the raster constants stay
  // those of the whole grid; the kernel adds the launch's first tile, KA_TAB)
  const int64_t Tgrid = tiles_m * tiles_n, T = T_cover > 0 ? T_cover : Tgrid, U = T * P;
  if (group_m <= 0 || group_m > tiles_m) group_m = (int)tiles_m;   // one group: tile rows fastest (the convolution's order)
  const int64_t width = (int64_t)group_m * tiles_n, gsz_last = tiles_m % group_m ? tiles_m % group_m : group_m;
  if ((double)Tgrid * (double)width >= 4.0e9 || (double)U * (double)P >= 4.0e9 || G < 1 || G > U) return false;
  const int64_t q = U / G, r = U % G;
  if ((double)G * (double)r * (double)G >= 4.0e9 || tiles_m > 0x7fffffff || tiles_n > 0x7fffffff || U > 0x7fffffff || Tgrid >= ((int64_t)1 << 28)) return false;
  if (two_level && (G % 8 != 0 || T < 8 || (T / 8) * P < G / 8 || (double)(U / 8 + P) * (double)(G / 8) >= 4.0e9)) return false;
  sc.tiles_m = (uint32_t)tiles_m; sc.tiles_n = (uint32_t)tiles_n; sc.group_m = (uint32_t)group_m; sc.gsz_last = (uint32_t)gsz_last;
  sc.mg_width = magic_u32((uint64_t)width); sc.mg_gm = magic_u32((uint64_t)group_m); sc.mg_last = magic_u32((uint64_t)gsz_last);
  sc.xcd_q = (xcd || two_level) && G >= 8 ? (uint32_t)(G / 8) : 0; sc.xcd_r = (xcd || two_level) && G >= 8 ? (uint32_t)(G % 8) : 0;
  sc.P = (uint32_t)P; sc.mg_P = magic_u32((uint64_t)P); sc.units_q = (uint32_t)(two_level ? T : q); sc.units_r = (uint32_t)(two_level ? 0 : r);
  sc.slice_len = (uint32_t)slice_len; sc.flags_bits = (o.asm_noseed ? 1u : 0u) | (two_level ? 2u : 0u) | (o.asm_test_giveup ? 8u : 0u);
  sc.mg_G = magic_u32((uint64_t)(two_level ? G / 8 : G));
  sc.ws = ws; sc.flags = flags;
  return true;
}

// One launch of the tiled problem described by (tiles, K): which plan.
//   plain:      one tile per workgroup, the hardware hands tiles to CUs as they free up: ceil(T / slots) rounds.
//   persistent: G = every slot of the chip (or fewer), each workgroup walks an equal share of the T * P units (unit = one K slice of
//               one tile; laser-order: slice = kc, the unit Laser's own pc loop restarts its chain at, gemm.nim:150-158; one chain: a
//               slice length chosen here).  A tile that straddles two workgroups is started by the owner of its slice 0, which sends
//               the running sum on through the workspace (one tile-sized hand-over per cut, whatever P); the next workgroup
//               continues it, in order: laser-order results are the SAME bits as the sequential loop's (asmgen/f32_kernel.py sched_next).
struct Plan {
  bool persistent = false;
  bool strided = false;      // persistent, whole tiles only: workgroup v takes tiles v, v + G, v + 2G ... (pipelined transitions)
  int64_t G = 0, P = 1, slice_len = 0;
  double time_us = 1e300;
  // hybrid (round 6; strided only): the strided launch covers the whole rounds of the raster, tiles [0, T - rem_tiles); the remaining
  // rem_tiles tiles -- a fraction of a round that would cost every workgroup's wait for the few that got one more tile -- follow as a
  // second launch of rem_G workgroups that cuts them along K into rem_P slices (the kernels' tile base, KA_TAB; f32_kernel.py prologue)
  int64_t rem_tiles = 0, rem_G = 0, rem_P = 1, rem_slice_len = 0;
};

// (pipe_us < 0: this problem may not pipeline its tile transitions; cus: compute units of the device -- the efficiency table was measured on the unpartitioned MI355X, 256 CUs)
inline Plan plan_launch(const KernelInfo &ki, int64_t tiles, int64_t K, int64_t batch, bool exact, int kc, double cu_flops_per_us, bool may_cut,
                        double pipe_us, int cus, bool allow_hybrid, const AsmOptions &o) {
  const int64_t kCUs = cus;
  Plan best;
  const double tile_us = 2.0 * ki.bm * ki.bn * (double)K / cu_flops_per_us;
  const int64_t slots = o.asm_wgs > 0 ? std::min<int64_t>(o.asm_wgs, 4096) : (int64_t)kCUs * ki.occ;
  {
    const int64_t t = tiles * batch, rounds = (t + kCUs - 1) / kCUs;
    best.G = tiles;
    best.slice_len = (K + ki.bk - 1) / ki.bk * ki.bk;
    best.time_us = (double)rounds * tile_us / (rounds == 1 ? ki.eff_alone : ki.eff) + ki.fixed_us;
    // More tiles than workgroup slots and a kernel that pipelines its tile transitions (pipe_us > 0: the caller has checked that this
    // problem may -- beta == 0, plain epilogue, whole K-tiles): every slot of the chip gets one persistent workgroup that walks the
    // tiles v, v + G, v + 2G ...: the same tiles at the same time as the rounds of the plain launch (an XCD's workgroups on one
    // contiguous chunk of the raster), minus what a fresh workgroup per tile costs -- drain, C store burst, prologue, first loads.
    // (pipe_us < 0: this problem may not pipeline; asm_plan = 3 forces the plan wherever it is legal -- sweeps, tests)
    if (pipe_us >= 0.0 && batch == 1 && o.asm_plan != 1 && o.asm_plan != 2 && ((pipe_us > 0.0 && tiles > slots) || (o.asm_plan >= 3 && tiles >= 2))) {
      const int64_t G = std::min(slots, tiles), per_wg = (tiles + G - 1) / G;
      if (per_wg >= 2) {
        best.persistent = true;
        best.strided = true;
        best.G = G;
        best.P = 1;
        best.time_us -= (double)(per_wg - 1) * pipe_us;
        best.time_us *= 1.01;      // (a static share of a ragged number of rounds: 5632^3 .. 7936^3 ran 0.5 .. 2 % over this estimate, x16_ab_big2_n.jsonl)
      }
    }
    if (o.asm_plan == 3) return best;
  }
  if (o.asm_plan == 1 || !may_cut || batch != 1 || !o.split_tail) return best;
  const int64_t kt = (K + ki.bk - 1) / ki.bk;
  // the best plan that cuts `tiles` tiles along K (remainder: the tiles are what a strided launch leaves over -- ranges shorter than a
  // tile are what it is for)
  const auto best_cut = [&](int64_t tiles, bool remainder) {
  Plan pers;
  // candidate cuts: laser-order: the kc slices; one chain: 1..16 slices of equal numbers of K-tiles (or the forced length)
  int64_t cuts[18];
  int ncuts = 0;
  if (exact) {
    cuts[ncuts++] = kc;
  } else if (o.asm_slice > 0) {
    cuts[ncuts++] = (int64_t)o.asm_slice * ki.bk;
  } else {
    for (int64_t p = 1; p <= 16 && p <= kt; p++) {
      // (two or three long slices per tile: every workgroup's range is a send piece + a receive piece and the launch runs about one
      // slice longer than the model says -- 3328^3 one chain on 256x128 in 3 slices: 117.9 TFLOP/s where the plain 160x96 launch runs
      // 137.7; 2048^3 / 1920^3 in 2: 0.77 / 0.69 of peak, profiles/r06/size_sweep_vendor_j.jsonl, x16_ab_mid_g.jsonl)
      if ((p == 2 || p == 3) && o.asm_plan != 2 && !remainder) continue;
      const int64_t len = (kt + p - 1) / p * ki.bk;
      if (len >= 4 * ki.bk || p == 1) cuts[ncuts++] = len;
    }
  }
  for (int i = 0; i < ncuts; i++) {
    const int64_t len = cuts[i], P = (K + len - 1) / len, U = tiles * P;
    int64_t G = std::min(slots, U);
    if (G >= 8) {                                         // launches that cut tiles: 8 XCDs x G / 8 workgroups (fill_sched), and no
      if (tiles < 8) continue;                            // more workgroups on an XCD than the XCD with the fewest tiles has units
      G = 8 * std::min(G / 8, (tiles / 8) * P);
    }
    const bool cut = plan_cuts_a_tile(tiles, P, G);
    if (!cut && G >= tiles && o.asm_plan != 2 && !remainder) continue;  // one whole tile per workgroup: that is the plain launch
    // many tiles per workgroup: the workgroups of an XCD drift apart in the tile order and lose their shared panels -- the plain
    // launch keeps them on neighbouring tiles
    if ((double)U / (double)G / (double)P > 4.0 && o.asm_plan != 2) continue;
    const int64_t q = U / G, r = U % G;
    // ranges much shorter than a tile: a workgroup waits for the sum of a predecessor that is still computing it (hand-over
    // chains); such problems are few-tile x long-K: the slice-parallel form / the plain launch serve them
    if (q < P - 2 && o.asm_plan != 2 && !remainder) continue;
    // the busiest CU: its workgroups' units back to back (the r longer ranges are spread evenly over the workgroup ids), at the
    // average unit length (the last slice of a tile is shorter)
    const int64_t wg_per_cu = (G + kCUs - 1) / kCUs;
    const double extras = r ? std::min((double)wg_per_cu, std::ceil((double)r * (double)wg_per_cu / (double)G)) : 0.0;
    const double units_cu = (double)(q * wg_per_cu) + extras;
    const double unit_us = tile_us / (double)P;
    // fitted to the round-4 sweeps (profiles/r04/plan_sweep_*).  The 64x64 kernels' rate differs by up to 10 % between boxes
    // (3072^3 plain: 130 TFLOP/s on one MI355X, 145.6 on another in the same hour; the large tiles repeat within 1 %), so their table
    // entries sit at the low end and ties go to the larger tile.  Three-per-CU tiles: a workgroup that walks about one tile keeps
    // its XCD's workgroups on neighbouring tiles and runs a little better than the plain launch's rounds; walking several tiles
    // they drift apart in the tile order and lose shared panels.  A launch that cuts tiles pays ~8 us (the two extra runs of a cut
    // tile, its hand-over through the workspace) whatever its length -- all workgroups pay it at the same time, so the CU's other
    // workgroups do not hide it -- and ranges shorter than a tile minus one slice wait on their predecessors
    const double tiles_per_wg = (double)U / (double)G / (double)P;
    double eff = G >= (int64_t)kCUs * ki.occ ? (ki.occ >= 3 ? (tiles_per_wg <= 1.3 ? std::min(ki.eff + 0.025, 0.97) : ki.eff - 0.045) : ki.eff)
                                             : ki.eff_alone + (ki.eff - ki.eff_alone) * std::min(1.0, (double)(wg_per_cu - 1) / std::max(1, ki.occ - 1));
    double t_us = units_cu * unit_us / eff + ki.fixed_us + (cut ? 8.0 : 0.0);
    if (cut && q < P - 1) t_us *= 1.0 + 0.25 * (double)(P - 1 - q) / (double)P;
    // (round 6: against the plain launches of the 16x16-block tiles -- whose estimates land within 1 % -- the persistent plans ran
    // 3 .. 7 % over this estimate at 2560^3 .. 5120^3 (profiles/r06/x16_ab_*.jsonl: 5120^3 1915-1966 us for 1829, 3584^3 669 for 640,
    // 3072^3 427 for 414, 2560^3 251 for 238): the workgroups of a CU do not stay in step for the whole launch)
    t_us *= exact ? 1.045 : 1.10;      // (one chain: 4 .. 7 % more again -- 3328^3 566 us for 529, 6912^3 4760 for 4513, 7936^3 7120 for 6824: x16_ab_big2_n.jsonl)
    if (t_us < pers.time_us) {       // the best cut; it replaces the plain launch only with a margin (below)
      pers.persistent = true;
      pers.G = G; pers.P = P; pers.slice_len = len;
      pers.time_us = t_us;
    }
  }
  return pers;
  };
  // hybrid: the whole rounds strided, the rest of the raster cut along K over every slot (a strided launch of 5.3 rounds takes 6).
  // Measured (profiles/r06/plan_ab_frac_hybrid_ab.jsonl, 256x128 and 256x256 tiles at 4608^3 .. 7424^3): the second launch takes
  // 0.35 + 0.95 x its share of a round, in tile times -- its workgroups sit on K ranges of their own, so nothing of an operand panel is
  // shared through L2 the way a round of whole tiles shares it -- in ONE-CHAIN mode: 0.46 / 0.62 / 0.71 tile times for 0.13 / 0.28 /
  // 0.53 of a round (6656^3 131 -> 143 TFLOP/s, 5888^3 135 -> 141, 4608^3 137 -> 142).  Laser-order: a workgroup folds its slices onto
  // the received sum IN ORDER, so all but the first slice of its piece wait for the predecessor's whole piece (f32_kernel.py
  // sched_next): with ranges much shorter than a tile the pieces of a tile run one after the other -- 0.76 .. 1.08 tile times whatever
  // the share -- and the extra strided round is no worse: not offered (asm_plan = 4 forces it: same bits).
  if (allow_hybrid && best.strided && o.asm_plan != 3 && tiles % best.G >= 8 && tiles / best.G >= 1 && (!exact || o.asm_plan == 4)) {
    const int64_t R = tiles % best.G, full = tiles / best.G;
    const Plan rem = best_cut(R, true);
    if (rem.persistent) {
      const double t = ((double)full + 0.35 + 0.95 * (double)R / (double)best.G) * tile_us / ki.eff + ki.fixed_us + 8.0 - (double)(full - 1) * std::max(0.0, pipe_us);
      if (t < 0.985 * best.time_us || o.asm_plan == 4) {
        best.rem_tiles = R; best.rem_G = rem.G; best.rem_P = rem.P; best.rem_slice_len = rem.slice_len;
        best.time_us = t;
      }
    }
  }
  if (o.asm_plan == 4) return best;
  const Plan pers = best_cut(tiles, false);
  if (pers.persistent && (pers.time_us < 1.0 * best.time_us || o.asm_plan == 2)) return pers;      // (0.96 before the 1.045 above: the same margin)
  return best;
}

// What the float32 and the float64 kernels differ in, in the eyes of the model and of the launcher
template <typename T>
struct AsmFloat;
template <>
struct AsmFloat<float> {
  static constexpr int kc = 512;                                 // the laser-order slice (gemm_tiling.nim)
  static constexpr double cu_flops_per_us = 157.3e6 / 256.0;     // 157.3 TFLOP/s of f32 matrix peak over the full chip's CUs
  static constexpr int max_bm = 256;                             // rows of the tallest tile: what A's 32-bit byte offsets must span
  static constexpr bool hybrid = true;
  static int enabled(const AsmOptions &o) { return o.f32_asm; }
  static int group_m(const AsmOptions &o, const KernelInfo &ki) { return o.asm_group_m > 0 ? o.asm_group_m : (ki.bm >= 2 * ki.bn) ? 4 : 8; }
};
template <>
struct AsmFloat<double> {
  static constexpr int kc = 256;                                 // kc = 256 doubles (gemm_tiling.nim:310)
  static constexpr double cu_flops_per_us = 78.6e6 / 256.0;      // 78.6 TFLOP/s of f64 matrix peak
  static constexpr int max_bm = 128;
  static constexpr bool hybrid = false;                          // (the hybrid plan is fitted and tested on the f32 kernels only: not offered)
  static int enabled(const AsmOptions &o) { return o.f64_asm; }
  static int group_m(const AsmOptions &, const KernelInfo &) { return 8; }
};

// What a chooser makes of a GEMM: the kernel (kKernels index), its launch plan, and what the launcher needs of the problem's reading
// (start from a fresh one)
struct AsmChoice {
  int pick = -1;
  Plan plan;
  bool exact = false;   // laser-order slices: the mode asks for them and K is longer than one
  bool nt = false;      // B passed transposed (unit row stride: every column is k-contiguous)
  int64_t ldb = 0;
  int tiles_m = 0, tiles_n = 0;
};

// What both float types ask of the operands: batches as grid y, A with unit column stride, B row-major-like or passed transposed, C's
// rows its slow direction, and 32-bit byte offsets inside the descriptors.  Sets c.nt and c.ldb.
template <typename T>
bool gemm_operands_fit(const GemmArgs<T> &a, AsmChoice &c) {
  if (a.batch < 1 || a.batch > 65535 || a.col0 != 0 || a.done_flags != nullptr) return false;
  if (a.batch > 1 && (a.bsA < 0 || a.bsB < 0 || a.bsC < 0)) return false;
  // C: rows are the slow direction of the view -- a tile's rows beyond M are dropped by the descriptor's size alone (they lie past
  // the last row), which needs every row to end before the next one starts
  if (a.csA != 1 || a.csC < 1 || a.rsC < (a.N - 1) * a.csC + 1) return false;
  // (tile-padded pre-pack images -- Mext / Next / Kext beyond M / N / K, gemm_prepacked.nim:63-292 -- are plain padded row-major
  // copies: the kernels bound every access by M, N, K themselves and never need the padding)
  if (a.Mext < a.M || a.Next < a.N || a.Kext < a.K) return false;
  // B: row-major-like (unit column stride), or passed transposed (unit row stride: every column is k-contiguous)
  c.nt = a.csB != 1 && a.rsB == 1;
  if (!c.nt && a.csB != 1) return false;
  c.ldb = c.nt ? a.csB : a.rsB;
  if (a.rsA < a.K || c.ldb < (c.nt ? a.K : a.N)) return false;
  // 32-bit byte offsets inside the descriptors
  const double el = sizeof(T), rows = AsmFloat<T>::max_bm;
  if ((double)a.rsA * el * rows >= 4.0e9) return false;
  if ((c.nt ? (double)c.ldb * el * rows : (double)a.K * (double)c.ldb * el) >= 4.0e9) return false;
  if (((double)(a.M - 1) * (double)a.rsC + (double)(a.N - 1) * (double)a.csC + 1.0) * el > 2147483648.0) return false;
  return true;
}

// One candidate row for a problem whose operands fit (c.exact set): price its best launch plan and keep it if it beats the choice so
// far.  fused: a bias / activation epilogue; pre: a fused prologue; pinned: the caller asked for this tile class.
// Which tile and which plan.  Workgroups that share a CU share its matrix pipes, so whatever the number of workgroup slots a
// plain launch of T tiles takes ceil(T / 256) times one tile's matrix time: the smaller the tile the finer the quantisation, the
// larger the tile the closer a CU gets to the peak (the eff columns of kKernels); the persistent plan (plan_launch) cuts the
// quantisation to one K slice.  3072^3: 288 tiles of 256x128 = 2 rounds for 1.125 rounds of work, or 6.75 slices per CU.
template <typename T>
void consider_kernel(int k, const GemmArgs<T> &a, bool laser_order, bool fused, bool pre, bool pinned, int cus, const AsmOptions &o, AsmChoice &c) {
  const KernelInfo &ki = kKernels[k];
  // (batched problems -- gemm_strided_batched, the kc slices of the slice-parallel form -- are grid y: every tile count is per launch)
  const int64_t tm = (a.M + ki.bm - 1) / ki.bm, tn = (a.N + ki.bn - 1) / ki.bn, t = tm * tn;
  if ((double)t * 8.0 * (double)tn >= 4.0e9) return;    // the in-kernel tile arithmetic's range (fill_sched)
  // below ~5/8 of a round of the larger tiles (3/8 of the 64x64 ones) the compiler-scheduled kernels' slice-parallel and
  // small-problem forms do better; no lower bound under a pin (the caller asked for THIS kernel family)
  if (AsmFloat<T>::enabled(o) < 2 && !pinned && t * a.batch < (ki.bm == 64 ? 3 : 5) * (int64_t)cus / 8) return;
  // pipelined tile transitions (round 6): beta == 0, plain epilogue, whole K-tiles, three or more of them (f32_kernel.py /
  // f64_kernel.py once()); a pinned tile runs one tile per workgroup -- a persistent plan counts on every workgroup slot of the
  // chip -- and so do the `_pre` variants
  const bool may_pipe = !fused && a.beta == T(0) && a.K % ki.bk == 0 && a.K >= 3 * ki.bk && !pinned && !pre;
  // (laser-order with K <= kc is ONE chain that must stay one chain: cuts only at kc boundaries, or anywhere in one-chain mode)
  const Plan p = plan_launch(ki, t, a.K, a.batch, c.exact, AsmFloat<T>::kc, AsmFloat<T>::cu_flops_per_us, (c.exact || !laser_order) && !pre && !pinned,
                             may_pipe ? ki.pipe_us : -1.0, cus, AsmFloat<T>::hybrid, o);
  if (p.time_us < 0.99 * c.plan.time_us) c.plan = p, c.pick = k, c.tiles_m = (int)tm, c.tiles_n = (int)tn;   // (near ties go to the larger tile: less L2 traffic)
}

// float32: which kernel and which launch plan for this problem on a device of `cus` compute units.  false: not this kernel family's
// class of problem.  A with unit column stride, B row-major-like or passed transposed, C with any positive strides (the epilogue's
// address arithmetic takes the column stride; rows are the tile's fast direction).
inline bool choose_gemm_f32_asm(const GemmArgs<float> &a, bool laser_order, int cus, const AsmOptions &o, AsmChoice &c) {
  if (!o.f32_asm) return false;
  // fused epilogue (laser_hip_gemm_strided_ex_*): bias views with non-negative element strides, no activation or relu; tanh /
  // sigmoid stay on the compiler-scheduled kernels (their library bodies are what the bit-exact tests pin)
  const bool fused = a.bias != nullptr || a.act != 0;
  if (a.act != 0 && a.act != 1) return false;
  if (a.bias != nullptr && (a.rsBias < 0 || a.csBias < 0 || a.rsBias > 0x3fffffff || a.csBias > 0x3fffffff || (a.batch > 1 && a.bsBias != 0) ||
                            ((double)(a.M - 1) * a.rsBias + (double)(a.N - 1) * a.csBias + 1.0) * 4.0 >= 2147483648.0))
    return false;
  if (a.csC > 0x3fffffff || !gemm_operands_fit(a, c)) return false;
  // (a ragged last K-tile is zero-filled piece-wise -- 16 bytes = 4 k -- and, when K % 4 != 0, element-wise in the staging registers)
  if (a.K < 1 || a.M < 1 || a.N < 1) return false;
  // laser-order results need the kc = 512 slices only when K > 512; one chain otherwise (the laser-order kernels are
  // plain single-chain kernels then: their fold tile is never reached)
  c.exact = laser_order && a.K > AsmFloat<float>::kc;
  const bool lo_row = c.exact || a.K <= AsmFloat<float>::kc;   // the rows taken: laser-order ones (with K <= 512 in either mode), else one-chain ones
  const bool pre = a.preA != 0 || a.preB != 0;
  // A pinned tile class (option "asm_tile" / the sharded entry point's LASER_HIP_SHARD_PIN_TILE on its worker threads): the local
  // products of a multi-GPU run that shares the CUs with RCCL's kernels.  Class 1 has no laser-order row: where the row is
  // laser-order it is class 0's 256x128 tile.
  int tile_pin = o.asm_tile;
  if (tile_pin == 1 && kF32Rows.k[1][lo_row][c.nt][0] < 0) tile_pin = 0;
  // near ties go to the class asked first: within a block family, the larger tile (less L2 traffic, fewer workgroups)
  const int order[10] = {0, 1, 2, 3, 4, 9, 8, 6, 7, 5};
  for (int oi = 0; oi < 10; oi++) {
    const int ci = order[oi];
    const int k0 = kF32Rows.k[ci][lo_row][c.nt][0];
    if (tile_pin >= 0 && ci != tile_pin) continue;
    if (k0 < 0 || (o.asm_kernel >= 0 && k0 != o.asm_kernel)) continue;
    // 16x16-block tiles (f32x16_kernel.py): 16-byte pieces are all-or-nothing (K % 4 == 0); they have no `_pre` variants (the fused
    // epilogue -- bias view + relu -- and a column stride on C are theirs too)
    if (kKernels[k0].fam == kF32x16 && a.K % 4 != 0) continue;
    // the one-chain kernels' fused epilogue has no C read: beta != 0 with a bias / activation only on the laser-order kernels
    if (fused && !kKernels[k0].exact && a.beta != 0.0f) continue;
    const int k = kF32Rows.k[ci][lo_row][c.nt][pre];       // fused prologue: the variants that apply it in the staging registers
    if (k >= 0) consider_kernel(k, a, laser_order, fused, pre, tile_pin >= 0, cus, o, c);
  }
  return c.pick >= 0;
}

// float64 (kernels of laser_amd/asmgen/f64_kernel.py): row-major A and C, B row-major or passed transposed, any alpha / beta, K even,
// batches as grid y; no fused epilogue or prologue, no tile pin.
inline bool choose_gemm_f64_asm(const GemmArgs<double> &a, bool laser_order, int cus, const AsmOptions &o, AsmChoice &c) {
  if (!o.f64_asm) return false;
  if (a.bias != nullptr || a.act != 0 || a.csC != 1 || !gemm_operands_fit(a, c)) return false;
  if (a.K < 2 || a.K % 2 != 0) return false;   // 16-byte pieces = 2 k
  // laser-order: the laser-order rows only where kc cuts the chain
  c.exact = laser_order && a.K > AsmFloat<double>::kc;
  for (const auto &tile_rows : kF64Rows.k) {     // 128x128x16, then 64x64x16
    const int k = tile_rows[c.exact][c.nt];
    if (o.asm_kernel >= 0 && k != o.asm_kernel) continue;
    consider_kernel(k, a, laser_order, false, false, false, cus, o, c);
  }
  return c.pick >= 0;
}

// what the assembly convolution launcher makes of a call: the kernel (kKernels index) and its unit walker, the padded K, the geometry
// and the tile grid
struct ConvClass {
  int pick = -1, walker = -1, tiles_m = 0, tiles_n = 0;
  int64_t kH = 0, kW = 0, sH = 0, sW = 0, taps = 0, oW = 0, oH = 0, npix = 0, Cin = 0, Kp = 0, tiles = 0;
  bool exact = false;
};
// false: not the convolution launcher's class (launch_conv_f32_asm's comment) on a device of `cus` compute units
inline bool conv_asm_classify(const GemmArgs<float> &a, bool laser_order, int cus, const AsmOptions &o, ConvClass &cc) {
  if (!o.f32_asm) return false;
  if (a.col0 != 0 || a.cs_imgs != 0) return false;
  if (a.alpha != 1.0f || a.beta != 0.0f) return false;
  // fused epilogue (laser_hip_conv2d_im2col_ex_f32: per-channel bias, relu) as in the GEMM kernels; tanh / sigmoid: the compiler kernels
  if (a.act != 0 && a.act != 1) return false;
  if (a.bias != nullptr && (a.rsBias < 0 || a.csBias < 0 || a.bsBias != 0 || a.rsBias > 0x3fffffff || a.csBias > 0x3fffffff ||
                            ((double)(a.M - 1) * a.rsBias + (double)(a.N - 1) * a.csBias + 1.0) * 4.0 >= 2147483648.0))
    return false;
  const int64_t kH = a.ckH, kW = a.ckW, sH = a.csH, sW = a.csW, taps = kH * kW;
  if (kH < 1 || kW < 1 || kH > 255 || kW > 255 || taps > 49 || sH < 1 || sW < 1 || sH > 255 || sW > 255) return false;
  if (a.cpH < 0 || a.cpW < 0 || a.cpH > 255 || a.cpW > 255) return false;
  if (a.cH + 2 * a.cpH < kH || a.cW + 2 * a.cpW < kW) return false;
  const int64_t oW = (a.cW + 2 * a.cpW - kW) / sW + 1, oH = (a.cH + 2 * a.cpH - kH) / sH + 1, npix = oH * oW;
  if (oW != a.coW || oW <= 0 || oH <= 0) return false;
  if (a.K % taps != 0 || a.K < taps || a.csC != 1 || a.rsC != npix) return false;
  if (a.N > npix || (a.N != npix && a.N % 128 != 0)) return false;
  if (a.batch < 1 || a.batch > 65535 || a.M > 0xffff * 64ll) return false;
  const int64_t Cin = a.K / taps;
  const int64_t Kp = (a.K + 3) / 4 * 4;          // filter rows as whole 16-byte pieces
  if ((double)Cin * a.cH * a.cW * 4.0 >= 2.0e9 || (double)a.M * npix * 4.0 >= 2.0e9 || (double)Kp * 4.0 * 256 >= 4.0e9 ||
      (double)Kp * (double)taps >= 4.0e9)      // (the in-kernel k / taps: x * d < 2^32)
    return false;
  const bool exact = laser_order && a.K > 512;
  const bool lo_row = exact || a.K <= 512;   // (as in choose_gemm_f32_asm)
  // rows of the tile by the number of output channels: the smallest padded row count, weighted by what each tile reaches (the
  // 256-row tile's tap table ends at 31 taps)
  int pick = -1, walker = -1;
  double best_cost = 1e300;
  for (int i = 0; i < 3; i++) {     // 256, 128, 64 rows
    const KernelInfo &kc = kKernels[kConvRows.k[i][lo_row]];
    if (kc.bm == 256 && taps > 31) continue;
    const double cost = (double)((a.M + kc.bm - 1) / kc.bm * kc.bm) / kc.eff;
    if (cost < 0.99 * best_cost) best_cost = cost, pick = kConvRows.k[i][lo_row], walker = kConvRows.walker[i][lo_row];
  }
  const KernelInfo &ki = kKernels[pick];
  const int tiles_m = (int)((a.M + ki.bm - 1) / ki.bm), tiles_n = (int)((a.N + ki.bn - 1) / ki.bn);
  const int64_t tiles = (int64_t)tiles_m * tiles_n;
  if ((double)tiles * (double)tiles >= 4.0e9) return false;   // the in-kernel tile arithmetic's range (fill_sched)
  if (o.f32_asm < 2 && tiles * a.batch < 5 * (int64_t)cus / 8) return false;
  // a 256-row tile that is mostly padding (few output channels) loses to the compiler-scheduled 128 / 64-row tiles
  if (o.f32_asm < 2 && (double)a.M * (double)a.N < 0.75 * (double)tiles * ki.bm * ki.bn) return false;
  if ((double)npix * (double)oW >= 4.0e9) return false;
  // the 64-row tile (two workgroups per CU, each at half the CU's rate): a CU works through ceil(units / CUs) units' worth of time
  // whatever the count; where that leaves a fifth of the chip idle the compiler-scheduled kernels' smaller tiles are ahead by 6 - 10 %
  // (profiles/r06/conv_m64_ab_w.jsonl: 800 units = 3.125 per CU, 320 units = 1.25 per CU), elsewhere behind by 4 - 25 %
  if (o.f32_asm < 2 && ki.bm == 64) {
    const int64_t units_ = tiles * a.batch, per_cu = (units_ + cus - 1) / cus;
    if ((double)units_ < 0.8 * (double)(per_cu * cus)) return false;
  }
  cc.pick = pick; cc.walker = walker; cc.tiles_m = tiles_m; cc.tiles_n = tiles_n; cc.tiles = tiles;
  cc.kH = kH; cc.kW = kW; cc.sH = sH; cc.sW = sW; cc.taps = taps; cc.oW = oW; cc.oH = oH; cc.npix = npix; cc.Cin = Cin; cc.Kp = Kp;
  cc.exact = exact;
  return true;
}

// Where to cut the pixel axis of a convolution whose main part the assembly kernels would take (round 6: the launch plan of
// gemm_mfma.hip plan_split is written for the compiler-scheduled configurations' tiles; in laser-order mode it cut 3136 pixels at
// 2048 where the 128-pixel assembly tile wants 3072: 109 against 127 TFLOP/s on 5x5 64 -> 128 channels, conv_geometry_ab_w.jsonl).
// Candidates: the whole image, or the first k whole 128-pixel tiles of every image with the rest as a tail launch.  A CU works
// through ceil(units / CUs) units one after the other (two workgroups of the 64-row tile share a CU at half its rate each: the same
// time); the tail is priced as a launch of its own at a fraction of the chip's rate (C4's 64-pixel tail: 14.4 us).
// Returns -1: not the assembly launcher's class (the caller keeps its own plan), 0: one launch, > 0: the cut.
inline int64_t conv_plan_cut(GemmArgs<float> a, bool laser_order, int cus, const AsmOptions &o) {
  const double cu_rate = 157.3e12 / 256.0;
  const auto main_us = [&](const ConvClass &cc) {
    const KernelInfo &ki = kKernels[cc.pick];
    const int64_t units = cc.tiles * a.batch;
    const double unit_us = 2.0 * ki.bm * ki.bn * (double)cc.Kp / (cu_rate * (ki.eff + 0.02)) * 1e6;
    return 8.0 + (double)((units + cus - 1) / cus) * unit_us;
  };
  double best = 1e300;
  int64_t best_cut = -1;
  ConvClass cc;
  if (conv_asm_classify(a, laser_order, cus, o, cc)) best = main_us(cc), best_cut = 0;
  const int64_t npix = a.N, kfull = npix / 128;
  for (int64_t k = kfull; k >= 1 && k >= kfull - 12; k--) {
    if (k * 128 == npix) continue;
    a.N = k * 128;
    if (!conv_asm_classify(a, laser_order, cus, o, cc)) continue;
    // (the 64-row tile with a short reduction: a cut launch loses 5 - 10 % to one launch of the compiler-scheduled kernels, K = 288 / 864;
    // from K = 1152 on it is 5 - 9 % ahead: profiles/r06/conv_m64_ab_x.jsonl)
    if (kKernels[cc.pick].bm == 64 && cc.Kp < 1024) continue;
    const double tail_flops = 2.0 * (double)a.M * (double)(npix - k * 128) * (double)a.K * (double)a.batch;
    const double t = main_us(cc) + 12.0 + tail_flops / 50.0e6;       // (us: 12 + flops / 50 TFLOP/s)
    if (t < 0.98 * best) best = t, best_cut = k * 128;
  }
  return best_cut;
}

}  // namespace laser_hip
