// laser_amd/csrc/gemm_route.cpp -- which kernel family runs a GemmArgs<T> on a stream: run_gemm<T> for the six element types, and
// run_small_mapped<T> for the zero-copy host path.  Policy only: every launcher lives beside its kernels (common.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "capi_internal.h"

namespace laser_hip {
namespace {

// One rung of a ladder: a launcher that answers hipErrorNotSupported leaves the problem to the next rung.
#define LH_RUNG(call)                                  \
  do {                                                 \
    const hipError_t e_ = (call);                      \
    if (e_ != hipErrorNotSupported) return e_;         \
  } while (0)

// the tiled kernels of a float type: hand-scheduled where they apply, else compiler-scheduled
hipError_t launch_tiled(const GemmArgs<float> &a, hipStream_t s) {
  if (f32_cfg_now() < 0) LH_RUNG(launch_gemm_f32_asm(a, laser_order_now(), s));  // (batched: the hand-scheduled kernels take the batch index as grid y)
  return launch_gemm_f32(a, f32_cfg_now(), laser_order_now(), s);
}
hipError_t launch_tiled(const GemmArgs<double> &a, hipStream_t s) {
  if (g_ctx.f64_mfma) LH_RUNG(launch_gemm_f64_asm(a, laser_order_now(), s));
  return launch_gemm_f64(a, laser_order_now(), s);
}

// Slice-parallel GEMM for problems with few output tiles and a long K (tall-skinny products, small M x N with a huge
// K): Laser's kc slices are independent chains from +0 -- only their sums are added in order (gemm.nim:150-158) -- so
// the slices are computed as ONE batched launch (batch = slice, K = kc, each a single-chain product into a workspace
// W[p][M][N]) and folded by an ordered combine pass.  Same fused multiply-adds in the same order, same unfused
// alpha / beta arithmetic => bit-identical to the sequential kernel, with ceil(K / kc) times the workgroups.
// Returns hipErrorNotSupported when the shape does not call for it.
template <typename T>
hipError_t gemm_slice_parallel(const GemmArgs<T> &a, int kc, hipStream_t s) {
  if (!g_ctx.slice_parallel || a.batch != 1 || a.bias != nullptr || a.act != 0) return hipErrorNotSupported;
  if (a.M <= 0 || a.N <= 0 || a.K <= kc) return hipErrorNotSupported;
  const int64_t tiles64 = ((a.M + 63) / 64) * ((a.N + 63) / 64);
  const int64_t nfull = a.K / kc, nsl = (a.K + kc - 1) / kc;
  const double ws_bytes = (double)nsl * (double)a.M * (double)a.N * sizeof(T);
  // measured boundary (scripts/slice_parallel_threshold_probe.py, slice_parallel_min_probe.py): the fewer the tiles the
  // fewer slices it takes to pay -- up to ~150 tiles of 64x64 from two slices on (768^2 x 1536: +20 %), up to ~400 from
  // five (1280^2 x 2560: +17 %; 1024^2 x 2048 with four: -3 %), up to ~600 from six (1536^2 x 6144: +24 %); from ~1000
  // tiles on the sequential loop wins (2048^3: -14 %)
  int64_t need = tiles64 <= 150 ? 2 : tiles64 <= 400 ? 5 : tiles64 <= 600 ? 6 : (int64_t)1 << 40;
  if (a.K % kc != 0 && need < 3) need = 3;  // a ragged last slice is a launch of its own: 768^3 (512 + 256) loses
  if (g_ctx.slice_parallel_tiles > 0) need = tiles64 <= g_ctx.slice_parallel_tiles.load() ? (int64_t)g_ctx.slice_parallel_min.load() : (int64_t)1 << 40;  // tuning override
  if (nsl < need || nsl > 65535 || ws_bytes > 1.5e9) return hipErrorNotSupported;
  T *W = nullptr;
  hipError_t e = scratch_alloc_async((void **)&W, (size_t)ws_bytes, s);
  if (e != hipSuccess) return e;
  const int64_t mn = a.M * a.N;
  GemmArgs<T> b = a;
  b.alpha = (T)1; b.beta = (T)0;
  b.C = W; b.rsC = a.N; b.csC = 1; b.bsC = mn;
  b.K = kc; b.Kext = kc;
  b.batch = (int32_t)nfull;
  b.bsA = (int64_t)kc * a.csA;  // slice p starts kc columns of A / rows of B further on
  b.bsB = (int64_t)kc * a.rsB;
  e = launch_tiled(b, s);
  if (e == hipSuccess && nsl > nfull) {  // the ragged last slice
    GemmArgs<T> c = b;
    c.batch = 1;
    c.K = a.K - nfull * kc; c.Kext = c.K;
    c.A = a.A + nfull * b.bsA;
    c.B = a.B + nfull * b.bsB;
    c.C = W + nfull * mn;
    e = launch_tiled(c, s);
  }
  if (e == hipSuccess) e = launch_combine_slices<T>(a.C, a.rsC, a.csC, W, a.M, a.N, (int)nsl, a.alpha, a.beta, s);
  const hipError_t e2 = scratch_free_async(W, s);
  return e != hipSuccess ? e : e2;
}

hipError_t run_gemm_core(const GemmArgs<float> &a, hipStream_t s);
hipError_t run_gemm_core(const GemmArgs<double> &a, hipStream_t s);

// Ragged-by-a-few problems (4100^3, 4095 x 4097 x 4099): 1..8 rows / columns past a multiple of 64 cost a whole extra row /
// column of tiles (4100 = 16 x 256 + 4: 17 tile rows for 16.02 tile rows of work).  Elements of C are independent and the
// streaming kernel for M <= 8 or N <= 8 (gemm_skinny.hip) runs the same k-ascending, kc-sliced chain per element as the tiled
// kernels, so those few rows / columns are peeled off and streamed (HBM-bound, ~20 us each at 4100^3), and the tiled
// launch sees whole tiles: bit-identical to the single launch.  Laser-order arithmetic only (the streaming kernel always
// restarts its chain every kc), i.e. laser-order mode or K <= kc; plain (unfused, unbatched, not pre-packed) problems.
template <typename T>
hipError_t run_gemm_peeled(const GemmArgs<T> &a, int kc, bool *taken, hipStream_t s) {
  *taken = false;
  if (!g_ctx.skinny || !g_split_tail || a.batch != 1 || a.bias != nullptr || a.act != 0) return hipSuccess;
  if (!(laser_order_now() || a.K <= kc) || a.Mext != a.M || a.Next != a.N || a.K < 256) return hipSuccess;
  const int64_t rM = a.M % 64, rN = a.N % 64;
  const bool peel_m = rM >= 1 && rM <= 8 && a.M >= 1024 && a.N >= 512;
  const bool peel_n = rN >= 1 && rN <= 8 && a.N >= 1024 && a.M - (peel_m ? rM : 0) >= 512;
  if (!peel_m && !peel_n) return hipSuccess;
  *taken = true;
  const int64_t M1 = peel_m ? a.M - rM : a.M, N1 = peel_n ? a.N - rN : a.N;
  GemmArgs<T> m = a;  // whole tiles
  m.M = M1; m.Mext = M1; m.N = N1; m.Next = N1;
  hipError_t e = run_gemm_core(m, s);
  if (e == hipSuccess && peel_n) {  // columns [N1, N) of rows [0, M1)
    GemmArgs<T> r = a;
    r.M = M1; r.Mext = M1; r.N = rN; r.Next = rN;
    r.B = a.B + N1 * a.csB;
    r.C = a.C + N1 * a.csC;
    e = launch_gemm_skinny<T>(r, true, kc, s);
  }
  if (e == hipSuccess && peel_m) {  // rows [M1, M), every column
    GemmArgs<T> b = a;
    b.M = rM; b.Mext = rM;
    b.A = a.A + M1 * a.rsA;
    b.C = a.C + M1 * a.rsC;
    e = launch_gemm_skinny<T>(b, true, kc, s);
  }
  return e == hipErrorNotSupported ? hipErrorInvalidValue : e;
}

// Fused prologue on a path that has no kernel for it: the operand is materialised once (relu applied while it is copied into a
// dense row-major scratch matrix -- "during the prepacking", README.md:243-244) and the plain problem runs on it.
template <typename T>
hipError_t run_gemm_prologue_materialised(const GemmArgs<T> &a, hipStream_t s) {
  if (a.batch != 1 || a.Mext != a.M || a.Next != a.N || a.Kext != a.K) return hipErrorInvalidValue;
  const size_t nA = a.preA ? (size_t)a.M * a.K : 0, nB = a.preB ? (size_t)a.K * a.N : 0;
  if (nA + nB == 0) return hipErrorInvalidValue;
  T *scratch = nullptr;
  hipError_t e = scratch_alloc_async((void **)&scratch, (nA + nB) * sizeof(T), s);
  if (e != hipSuccess) return e;
  GemmArgs<T> b = a;
  b.preA = b.preB = 0;
  if (a.preA) {
    e = launch_pack_pad<T>(scratch, a.M, a.K, a.A, a.M, a.K, a.rsA, a.csA, s, 1);
    b.A = scratch; b.rsA = a.K; b.csA = 1;
  }
  if (e == hipSuccess && a.preB) {
    e = launch_pack_pad<T>(scratch + nA, a.K, a.N, a.B, a.K, a.N, a.rsB, a.csB, s, 1);
    b.B = scratch + nA; b.rsB = a.N; b.csB = 1;
  }
  if (e == hipSuccess) e = run_gemm<T>(b, s);
  const hipError_t e2 = scratch_free_async(scratch, s);
  return e != hipSuccess ? e : e2;
}

// float32: a pinned compiler-kernel configuration (f32_cfg_now() >= 0) switches every rung off but the last
hipError_t run_gemm_core(const GemmArgs<float> &a, hipStream_t s) {
  const bool any = f32_cfg_now() < 0, laser = laser_order_now();
  if (any && g_ctx.skinny) LH_RUNG(launch_gemm_skinny<float>(a, laser, 512, s));  // matrix-vector-like shapes: an HBM stream, not a tile problem
  if (any) LH_RUNG(launch_gemm_small<float>(a, laser, 512, s));  // few 32x32 blocks / batches of tiny matrices: one wave per block, no LDS round trips
  // Up to ~150 tiles of 64x64 the slice-parallel form (kc slices as one batched launch + ordered combine) fills the chip
  // better than any single launch; above that the hand-scheduled assembly kernels come first (their 64x64 tile covers the
  // few-tile x long-K problems the slice-parallel form was built for: 1024^2 x 8192 = 256 tiles).
  // (a pinned assembly tile class -- option "asm_tile", the sharded entry points' LASER_HIP_SHARD_PIN_TILE -- asks for THAT kernel
  // family: the slice-parallel form does not come first then)
  const bool few_tiles = ((a.M + 63) / 64) * ((a.N + 63) / 64) <= 150 && asm_tile_pin_now() < 0;
  g_last_f32_asm = 0;
  if (any && few_tiles) LH_RUNG(gemm_slice_parallel<float>(a, 512, s));
  // (a badly filled last round of tiles is the assembly launcher's business: its persistent plan hands the chip's workgroup slots
  // equal numbers of kc slices and finishes a cut tile with an in-kernel ordered fix-up -- asm_plan.h plan_launch)
  if (any) LH_RUNG(launch_gemm_f32_asm(a, laser, s));
  if (any && !few_tiles) LH_RUNG(gemm_slice_parallel<float>(a, 512, s));
  return launch_gemm_f32(a, f32_cfg_now(), laser, s);
}
// float64: option "f64_mfma" gates the matrix-core rungs; the streaming kernel and the VALU kernel do not need it
hipError_t run_gemm_core(const GemmArgs<double> &a, hipStream_t s) {
  const bool laser = laser_order_now();
  if (g_ctx.skinny) LH_RUNG(launch_gemm_skinny<double>(a, laser, 256, s));
  if (!g_ctx.f64_mfma) return launch_gemm_valu<double>(a, laser, s);
  LH_RUNG(launch_gemm_small<double>(a, laser, 256, s));
  const bool few_tiles = ((a.M + 63) / 64) * ((a.N + 63) / 64) <= 150;   // (same rule as float32)
  g_last_f64_asm = 0;
  g_last_split = 0;
  if (few_tiles) LH_RUNG(gemm_slice_parallel<double>(a, 256, s));
  LH_RUNG(launch_gemm_f64_asm(a, laser, s));   // the hand-scheduled assembly kernels (laser_amd/asmgen/f64_kernel.py)
  if (!few_tiles) LH_RUNG(gemm_slice_parallel<double>(a, 256, s));
  return launch_gemm_f64(a, laser, s);  // v_mfma_f64_16x16x4_f64: a k-ordered fma chain
}

// Integer K beyond one launch of the limb kernels (their accumulator groups are never folded): arithmetic mod 2^n is
// associative, so C = alpha * sum_chunks(A_c B_c) + beta * C0 is computed chunk by chunk -- the first with (alpha, beta), the
// rest with (alpha, 1) -- bit for bit the single product.  hipErrorNotSupported (nothing launched): not the kernels' class.
template <typename T, typename FA, typename FC>
hipError_t int_gemm_k_chunks(const GemmArgs<T> &a, void *ws, hipStream_t s, FA first_launch, FC fallback_launch, int64_t kChunk) {
  hipError_t e = hipErrorNotSupported;
  for (int64_t k0 = 0; k0 < a.K; k0 += kChunk) {
    GemmArgs<T> c = a;
    c.K = std::min(kChunk, a.K - k0);
    c.Kext = c.K;
    c.A = a.A + k0 * a.csA;
    c.B = a.B + k0 * a.rsB;
    if (k0 > 0) c.beta = (T)1;
    e = first_launch(c, ws, s);
    if (e == hipErrorNotSupported) {
      if (k0 == 0) return e;
      e = fallback_launch(c, ws, s);
    }
    if (e != hipSuccess) return e;
  }
  return e;
}

// What the limb-decomposed integer GEMMs differ in.  int32 / int64 (mod 2^32 / 2^64; four / eight int8 limbs, gemm_i32_mfma.hip,
// gemm_i64_mfma.hip): the hand-scheduled kernel (laser_amd/asmgen/i8_kernel.py) first, the compiler-scheduled one where it does not
// apply; "last_i32_asm" is theirs to set.  int8 / int16 (mod 2^8 / 2^16, uint8 / uint16 on the same bits; one / two digit planes,
// gemm_narrow_mfma.hip): one launcher; "last_narrow_mfma" tells whether it ran.
template <typename T>
struct LimbGemm {
  using Launch = hipError_t (*)(const GemmArgs<T> &, void *, hipStream_t);
  const std::atomic<bool> &enabled;
  int skinny_kc;
  size_t (*workspace_bytes)(int64_t, int64_t, int64_t);
  Launch first, fallback;
  int64_t k_chunk;
  bool narrow;
};
template <typename T>
LimbGemm<T> limb_gemm() {
  if constexpr (std::is_same<T, int32_t>::value)
    return {g_ctx.i32_mfma, 512, gemm_i32_mfma_workspace_bytes, launch_gemm_i32_asm, launch_gemm_i32_mfma, 8192, false};
  else if constexpr (std::is_same<T, int64_t>::value)
    return {g_ctx.i64_mfma, 256, gemm_i64_mfma_workspace_bytes, launch_gemm_i64_asm, launch_gemm_i64_mfma, 8192, false};
  else
    return {g_ctx.narrow_mfma, 0, gemm_narrow_mfma_workspace_bytes<T>, launch_gemm_narrow_mfma<T>, launch_gemm_narrow_mfma<T>, NARROW_MAX_K, true};
}

// Integer GEMMs: the streaming kernel for M or N <= 8; single problems with enough work on the int8 matrix cores, the limb planes
// in stream-ordered scratch (concurrent streams never share a buffer) and K beyond one launch in chunks; the VALU kernel
// otherwise (batches included).
template <typename T>
hipError_t run_gemm_int(const GemmArgs<T> &a, hipStream_t s) {
  const LimbGemm<T> t = limb_gemm<T>();
  if (t.narrow) g_last_narrow_mfma = 0;
  if (g_ctx.skinny) LH_RUNG(launch_gemm_skinny<T>(a, false, t.skinny_kc, s));
  const double work = (double)a.M * (double)a.N * (double)a.K;
  if (!(t.enabled && a.batch == 1 && work >= 64.0 * 64.0 * 64.0 * 8.0)) return launch_gemm_valu<T>(a, false, s);
  void *ws = nullptr;
  hipError_t e = scratch_alloc_async(&ws, t.workspace_bytes(a.M, a.N, a.K), s);
  if (e != hipSuccess) return e;
  if (!t.narrow) g_last_i32_asm = 0;
  e = a.K > t.k_chunk ? int_gemm_k_chunks<T>(a, ws, s, t.first, t.fallback, t.k_chunk) : t.first(a, ws, s);
  if (e == hipErrorNotSupported) e = t.fallback(a, ws, s);
  if (t.narrow && e == hipSuccess) g_last_narrow_mfma = 1;
  const hipError_t e2 = scratch_free_async(ws, s);
  return e != hipSuccess ? e : e2;
}

}  // namespace

std::atomic<int> g_last_narrow_mfma{0};

template <>
hipError_t run_gemm<float>(const GemmArgs<float> &a, hipStream_t s) {
  if (a.preA || a.preB) {      // the `_pre` assembly kernels (relu in the staging registers), else one materialising pass
    if (f32_cfg_now() < 0) LH_RUNG(launch_gemm_f32_asm(a, laser_order_now(), s));
    g_last_f32_asm = 0;
    return run_gemm_prologue_materialised<float>(a, s);
  }
  if (f32_cfg_now() < 0) {
    bool taken;
    const hipError_t e = run_gemm_peeled<float>(a, 512, &taken, s);
    if (taken) return e;
  }
  return run_gemm_core(a, s);
}
template <>
hipError_t run_gemm<double>(const GemmArgs<double> &a, hipStream_t s) {
  if (a.preA || a.preB) return run_gemm_prologue_materialised<double>(a, s);
  if (g_ctx.f64_mfma) {
    bool taken;
    const hipError_t e = run_gemm_peeled<double>(a, 256, &taken, s);
    if (taken) return e;
  }
  return run_gemm_core(a, s);
}
template <>
hipError_t run_gemm<int32_t>(const GemmArgs<int32_t> &a, hipStream_t s) { return run_gemm_int(a, s); }
template <>
hipError_t run_gemm<int64_t>(const GemmArgs<int64_t> &a, hipStream_t s) { return run_gemm_int(a, s); }
template <>
hipError_t run_gemm<int8_t>(const GemmArgs<int8_t> &a, hipStream_t s) { return run_gemm_int(a, s); }
template <>
hipError_t run_gemm<int16_t>(const GemmArgs<int16_t> &a, hipStream_t s) { return run_gemm_int(a, s); }

template <typename T>
hipError_t run_small_mapped(const GemmArgs<T> &a, hipStream_t s) {
  if constexpr (std::is_same<T, float>::value)
    return launch_gemm_small<float>(a, laser_order_now(), 512, s, true);
  else if constexpr (std::is_same<T, double>::value)
    return launch_gemm_small<double>(a, laser_order_now(), 256, s, true);
  else
    return hipErrorNotSupported;
}
template hipError_t run_small_mapped<float>(const GemmArgs<float> &, hipStream_t);
template hipError_t run_small_mapped<double>(const GemmArgs<double> &, hipStream_t);
template hipError_t run_small_mapped<int32_t>(const GemmArgs<int32_t> &, hipStream_t);
template hipError_t run_small_mapped<int64_t>(const GemmArgs<int64_t> &, hipStream_t);
template hipError_t run_small_mapped<int8_t>(const GemmArgs<int8_t> &, hipStream_t);
template hipError_t run_small_mapped<int16_t>(const GemmArgs<int16_t> &, hipStream_t);
#undef LH_RUNG

}  // namespace laser_hip
