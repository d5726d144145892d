// laser_amd/csrc/gemm_narrow_mfma.hip -- int8 / int16 GEMM (also uint8 / uint16: the same bits), bit-exact mod 2^8 / 2^16,
// on the gfx950 int8 matrix cores.
//
// The int32 kernel's decomposition (gemm_i32_mfma.hip) over balanced base-256 digits, cut to the narrow widths:
//
//     int8 :  a == s0(a)                     (mod 2^8)       -> a*b == s0 t0                        (one product)
//     int16:  a == s0(a) + 256 s1(a)         (mod 2^16)      -> a*b == s0 t0 + 256 (s0 t1 + s1 t0)  (three products)
//
// so sum_k a_ik b_kj == G0 + 256 G1 with G0 = sum s0 t0, G1 = sum (s0 t1 + s1 t0): NP = sizeof(T) int8 planes per operand,
// NP accumulator groups, `v_mfma_i32_32x32x32_i8` on each product.  The int8 digit is the byte itself (read as int8, it is
// == a mod 256 for int8 and uint8 alike); the int16 split is (a + 0x80) ^ 0x80 -- the low byte stays a's (as int8: the
// balanced digit), the high byte takes the carry (any representative mod 256 will do, 256^2 == 0 mod 2^16).
//
// Structure:
//   1. narrow_planes_kernel: strided operand -> NP k-contiguous int8 planes P_p[x][k], zero-padded to the tile, through an
//      LDS tile read along the source's contiguous axis (16-byte loads where the layout allows) and written as 16-byte chunks;
//      B is transposed on the way.
//   2. gemm_narrow_kernel<NP>: 8 waves, LDS-DMA staging (`global_load_lds_dwordx4`, no staging registers) into a ring of
//      NSTAGE stages (2 for int8, 3 for int16), source-side chunk swizzle (conflict-free 32-row ds_read_b128 without padding), XCD-aware remap and
//      grouped raster.  One loaded plane pair feeds one MFMA for int8 (2.5 for the int32 kernel), so the int8 tile is
//      larger -- 256 x 256, 128 k per stage -- to keep the bytes per MFMA from HBM/L2 near the int32 kernel's;
//      int16 (two groups) runs 256 x 128, 64 k per stage.
//   Epilogue: x = G0 + (G1 << 8), C = alpha*x + beta*C0 in 32-bit unsigned arithmetic, narrowing 1- / 2-byte stores with
//   the caller's strides (beta == 0 never reads C).
// K per launch <= NARROW_MAX_K = 16384: |G_s| <= 2 * 2^14 * 2^14 = 2^29, so the int32 accumulators never rely on how the
// hardware treats overflow; the dispatcher runs longer K in chunks (int_gemm_k_chunks).
#include <type_traits>

#include "common.h"

namespace laser_hip {

namespace {

using i32x4 = __attribute__((ext_vector_type(4))) int;
using i32x16 = __attribute__((ext_vector_type(16))) int;
typedef __attribute__((address_space(3))) void lds_void_t;
typedef __attribute__((address_space(1))) const void glb_void_t;

// ---- 1. the packing pass ------------------------------------------------------------------------------------------
constexpr int NPK_THREADS = 256;

// planes[p][x][k] (int8), x < Xpad, k < Kpad; element (x, k) of the source at src[x*sx + k*sk] for x < X, k < K, zero
// elsewhere.  XF: the source is contiguous along x (a row-major B) -- the tile is 128 x by 32 k so that each source row
// segment is 128 / 256 bytes; otherwise 32 x by 128 k.  A tile is 4096 elements: 16 per thread.
// vec: unit stride along the contiguous axis, the other stride a multiple of 16 bytes, 16-byte aligned base (launcher).
template <typename T, bool XF>
__global__ void __launch_bounds__(NPK_THREADS) narrow_planes_kernel(int8_t *__restrict__ planes, const T *__restrict__ src, int64_t X,
                                                                     int64_t K, int64_t sx, int64_t sk, int64_t Xpad, int64_t Kpad,
                                                                     int tiles_k, int vec) {
  constexpr int NP = (int)sizeof(T);
  constexpr int TX = XF ? 128 : 32, TK = XF ? 32 : 128;
  constexpr int EV = 16 / NP;                // elements per 16 bytes
  constexpr int PAD = 16 / NP;               // one 16-byte chunk of padding per row: rows stay 16-byte aligned
  typedef __attribute__((ext_vector_type(4))) int v16;
  union VecT { v16 q; T e[EV]; };
  __shared__ __attribute__((aligned(16))) T tile[TX][TK + PAD];
  const int t = threadIdx.x;
  const int64_t x0 = (int64_t)(blockIdx.x / tiles_k) * TX, k0 = (int64_t)(blockIdx.x % tiles_k) * TK;
  if (vec && !XF) {          // k-contiguous rows: 16-byte loads along k, 16-byte LDS stores
    constexpr int VPR = TK / EV;
#pragma unroll
    for (int i = 0; i < TX * VPR / NPK_THREADS; i++) {
      const int v = t + i * NPK_THREADS, xl = v / VPR, kl = (v % VPR) * EV;
      const int64_t x = x0 + xl, k = k0 + kl;
      VecT u;
      if (x < X && k + EV <= K) {
        u.q = *reinterpret_cast<const v16 *>(src + x * sx + k);
      } else {
#pragma unroll
        for (int j = 0; j < EV; j++) u.e[j] = (x < X && k + j < K) ? src[x * sx + k + j] : (T)0;
      }
      *reinterpret_cast<v16 *>(&tile[xl][kl]) = u.q;
    }
  } else if (vec) {          // x-contiguous: 16-byte loads along x, element stores into the [x][k] tile
    constexpr int VPX = TX / EV;
#pragma unroll
    for (int i = 0; i < TK * VPX / NPK_THREADS; i++) {
      const int v = t + i * NPK_THREADS, kl = v / VPX, xl = (v % VPX) * EV;
      const int64_t x = x0 + xl, k = k0 + kl;
      VecT u;
      if (k < K && x + EV <= X) {
        u.q = *reinterpret_cast<const v16 *>(src + k * sk + x);
      } else {
#pragma unroll
        for (int j = 0; j < EV; j++) u.e[j] = (k < K && x + j < X) ? src[k * sk + x + j] : (T)0;
      }
#pragma unroll
      for (int j = 0; j < EV; j++) tile[xl + j][kl] = u.e[j];
    }
  } else {                   // any strides (negative included): predicated element loads, lanes along the smaller stride
#pragma unroll
    for (int i = 0; i < TX * TK / NPK_THREADS; i++) {
      const int e = t + i * NPK_THREADS;
      const int xl = XF ? e % TX : e / TK, kl = XF ? e / TX : e % TK;
      const int64_t x = x0 + xl, k = k0 + kl;
      tile[xl][kl] = (x < X && k < K) ? src[x * sx + k * sk] : (T)0;
    }
  }
  __syncthreads();
  // thread -> (x, 16-k chunk): NP 16-byte stores (one per plane)
  const int xl = XF ? t % TX : t / (TK / 16), kc = XF ? t / TX : t % (TK / 16);
  const int64_t x = x0 + xl, kq = (k0 >> 4) + kc;
  if (x >= Xpad || kq * 16 >= Kpad) return;
  const int64_t plane = Xpad * Kpad;
  int8_t *dst = planes + x * Kpad + kq * 16;
  if constexpr (NP == 1) {
    *reinterpret_cast<v16 *>(dst) = *reinterpret_cast<const v16 *>(&tile[xl][kc * 16]);
  } else {
    const v16 lo = *reinterpret_cast<const v16 *>(&tile[xl][kc * 16]), hi = *reinterpret_cast<const v16 *>(&tile[xl][kc * 16 + 8]);
    // per 16-bit element a = H:L, (a + 0x80) ^ 0x80 keeps L and turns H into H + L[7] (mod 256): both halves of a word at once
    uint32_t raw[8], hb[8];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      raw[j] = (uint32_t)lo[j];
      raw[4 + j] = (uint32_t)hi[j];
    }
#pragma unroll
    for (int j = 0; j < 8; j++) hb[j] = (((raw[j] >> 8) & 0x00ff00ffu) + ((raw[j] >> 7) & 0x00010001u)) & 0x00ff00ffu;
    // bytes 0 and 2 of two consecutive words = four consecutive k: digit 0 from the raw words, digit 1 from hb
    v16 p0, p1;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      p0[j] = (int)__builtin_amdgcn_perm(raw[2 * j + 1], raw[2 * j], 0x06040200u);
      p1[j] = (int)__builtin_amdgcn_perm(hb[2 * j + 1], hb[2 * j], 0x06040200u);
    }
    *reinterpret_cast<v16 *>(dst) = p0;
    *reinterpret_cast<v16 *>(dst + plane) = p1;
  }
}

template <typename T>
hipError_t launch_narrow_planes(int8_t *dst, const T *src, int64_t X, int64_t K, int64_t sx, int64_t sk, int64_t Xpad, int64_t Kpad,
                                hipStream_t s) {
  const bool xf = (sx < 0 ? -sx : sx) < (sk < 0 ? -sk : sk);
  const int64_t ev = 16 / (int64_t)sizeof(T);
  const int vec = ((uintptr_t)src % 16 == 0) && (xf ? (sx == 1 && sk > 0 && sk % ev == 0) : (sk == 1 && sx > 0 && sx % ev == 0));
  const int64_t TX = xf ? 128 : 32, TK = xf ? 32 : 128;
  const int64_t tiles_x = (Xpad + TX - 1) / TX, tiles_k = (Kpad + TK - 1) / TK;
  if (tiles_x * tiles_k > 0x7fffffffll) return hipErrorInvalidValue;
  auto kern = xf ? narrow_planes_kernel<T, true> : narrow_planes_kernel<T, false>;
  hipLaunchKernelGGL(kern, dim3((unsigned)(tiles_x * tiles_k)), dim3(NPK_THREADS), 0, s, dst, src, X, K, sx, sk, Xpad, Kpad, (int)tiles_k, vec);
  return hipGetLastError();
}

// ---- 2. GEMM on the planes ------------------------------------------------------------------------------------------
constexpr int NTHREADS = 512;

template <int NP>
struct NarrowCfg {
  static constexpr int BM = 256, BN = NP == 1 ? 256 : 128;      // workgroup tile
  static constexpr int WM = NP == 1 ? 128 : 64, WN = 64;        // wave tile
  static constexpr int WAVES_N = BN / WN;                       // 4 / 2 (x 2 / 4 along M = 8 waves)
  static constexpr int FM = WM / 32, FN = WN / 32;              // 32 x 32 blocks per wave
  static constexpr int BK = NP == 1 ? 128 : 64;                 // k bytes per plane row per stage
  static constexpr int CH = BK / 16;                            // 16-byte chunks per row
  static constexpr int ROWS = BM + BN;                          // rows of one plane (A then B) in a stage
  static constexpr int STAGE = NP * ROWS * BK;                  // 64 KiB / 48 KiB
  static constexpr int NSTAGE = NP == 1 ? 2 : 3;                // LDS ring: the DMA runs NSTAGE - 1 tiles ahead
  static constexpr int PIECES = STAGE / 1024 / 8;               // 1-KiB LDS-DMA pieces per wave per stage: 8 / 6
  static constexpr int RPP = 1024 / BK;                         // rows per piece
  static constexpr int KSTEPS = BK / 32;                        // 32-k MFMA steps per stage
  static_assert(STAGE % (8 * 1024) == 0 && PIECES % KSTEPS == 0, "stage = whole pieces, spread evenly over the k steps");
  static_assert(NSTAGE * STAGE <= 160 * 1024, "LDS budget");
};
// chunk swizzle of row r: slot = chunk ^ swz(r).  The 16 lanes of each ds_read_b128 lane group (rows {0-3,12-15,20-27} /
// {4-11,16-19,28-31} of a 32-row fragment, one chunk) then cover the 16 distinct 16-byte bank slots of a 256-byte line.
template <int CH>
__device__ __forceinline__ int swz(int r) { return (r / (16 / CH)) & (CH - 1); }

template <typename T>
struct NarrowArgs {
  const int8_t *Ap, *Bp;   // [NP][Mpad][Kpad], [NP][Npad][Kpad]
  int64_t planeA, planeB, Kpad;
  int64_t M, N;
  uint32_t alpha, beta;
  T *C;
  int64_t rsC, csC;
  int32_t tiles_m, tiles_n, group_m;
};

template <typename T>
__global__ void __launch_bounds__(NTHREADS, 1) gemm_narrow_kernel(const NarrowArgs<T> g) {
  constexpr int NP = (int)sizeof(T);
  using Cf = NarrowCfg<NP>;
  constexpr int BM = Cf::BM, BN = Cf::BN, BK = Cf::BK, CH = Cf::CH, FM = Cf::FM, FN = Cf::FN, STAGE = Cf::STAGE;
  extern __shared__ __attribute__((aligned(16))) int8_t nsmem[];

  // XCD-aware bijective remap + grouped raster (as gemm_i8limb_kernel)
  const int nwg = gridDim.x;
  int wgid;
  {
    const int bid = blockIdx.x, xcd = bid % 8, loc = bid / 8, q = nwg / 8, r = nwg % 8;
    wgid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + loc;
  }
  const int width = g.group_m * g.tiles_n;
  const int first_m = (wgid / width) * g.group_m;
  const int gsz = min(g.tiles_m - first_m, g.group_m);
  const int pid_m = first_m + (wgid % width) % gsz;
  const int pid_n = (wgid % width) / gsz;
  const int64_t m0 = (int64_t)pid_m * BM, n0 = (int64_t)pid_n * BN;

  const int t = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int lane = t & 63, lo = lane & 31, hi = lane >> 5;
  const int wm0 = (wave / Cf::WAVES_N) * Cf::WM, wn0 = (wave % Cf::WAVES_N) * Cf::WN;

  // LDS-DMA: the stage image is [plane][A rows BM | B rows BN][BK bytes], cut into 1-KiB pieces of RPP rows; piece q = i*8 + wave.
  // lane -> row lane / CH of the piece, slot lane % CH; it fetches source chunk slot ^ swz(row).  For CH = 8 a piece is 8 rows
  // and swz depends on the piece's parity, which is the wave's (q = i*8 + wave; ROWS is a multiple of 16).
  const int drow = lane / CH;
  const int dchunk = (lane % CH) ^ swz<CH>(drow + (CH == 8 ? 8 * (wave & 1) : 0));
  const int64_t dlane = (int64_t)drow * g.Kpad + dchunk * 16;
  const int8_t *dsrc[Cf::PIECES];
#pragma unroll
  for (int i = 0; i < Cf::PIECES; i++) {
    const int row = (i * 8 + wave) * Cf::RPP;     // in the stage image
    const int p = row / Cf::ROWS, r = row % Cf::ROWS;
    dsrc[i] = (r < BM ? g.Ap + p * g.planeA + (m0 + r) * g.Kpad : g.Bp + p * g.planeB + (n0 + r - BM) * g.Kpad) + dlane;
  }
  auto dma_piece = [&](int stage, int64_t k0, int i) __attribute__((always_inline)) {
    __builtin_amdgcn_global_load_lds((glb_void_t *)(dsrc[i] + k0), (lds_void_t *)(nsmem + stage * STAGE + (i * 8 + wave) * 1024), 16, 0, 0);
  };

  i32x16 acc[NP][FM][FN];   // [group][m block][n block]
#pragma unroll
  for (int s = 0; s < NP; s++)
#pragma unroll
    for (int i = 0; i < FM; i++)
#pragma unroll
      for (int j = 0; j < FN; j++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc[s][i][j][r] = 0;

  // fragments: lane (row lo, k half hi) reads 16 consecutive k bytes -- the same k pattern for A and B
  const int fsw = swz<CH>(lo);
  const int a_off = (wm0 + lo) * BK, b_off = (BM + wn0 + lo) * BK;
  i32x4 fa[2][NP][FM], fb[2][NP][FN];
  auto ld_frags = [&](const int8_t *st, int ks, int slot) __attribute__((always_inline)) {
    const int c = ((ks * 2 + hi) ^ fsw) * 16;
#pragma unroll
    for (int p = 0; p < NP; p++) {
#pragma unroll
      for (int i = 0; i < FM; i++) fa[slot][p][i] = *reinterpret_cast<const i32x4 *>(st + p * Cf::ROWS * BK + a_off + i * 32 * BK + c);
#pragma unroll
      for (int j = 0; j < FN; j++) fb[slot][p][j] = *reinterpret_cast<const i32x4 *>(st + p * Cf::ROWS * BK + b_off + j * 32 * BK + c);
    }
  };

  constexpr int NSTAGE = Cf::NSTAGE;
  const int nkt = (int)(g.Kpad / BK);
  // prologue: tiles 0 .. NSTAGE-2 in flight, wait for tile 0
#pragma unroll
  for (int i = 0; i < Cf::PIECES; i++) dma_piece(0, 0, i);
  if (NSTAGE == 3 && nkt > 1) {
#pragma unroll
    for (int i = 0; i < Cf::PIECES; i++) dma_piece(1, BK, i);
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(Cf::PIECES) : "memory");
  } else {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __syncthreads();

  constexpr int PPS = Cf::PIECES / Cf::KSTEPS;   // DMA pieces of the next stage per k step
  auto k_tile = [&](auto MORE_, int kt) __attribute__((always_inline)) {
    constexpr bool more = decltype(MORE_)::value;
    const int8_t *st = nsmem + (kt % NSTAGE) * STAGE;
    const int nst = (kt + NSTAGE - 1) % NSTAGE;             // the stage tile kt + NSTAGE - 1 goes to (read at kt - 1: free)
    const int64_t k1 = (int64_t)(kt + NSTAGE - 1) * BK;
    ld_frags(st, 0, 0);
#pragma unroll
    for (int ks = 0; ks < Cf::KSTEPS; ks++) {
      const int cur = ks & 1;
      if (ks + 1 < Cf::KSTEPS) ld_frags(st, ks + 1, cur ^ 1);   // next step's fragments ahead of this step's MFMAs
      __builtin_amdgcn_sched_barrier(0);
      // products (p, q) with p + q < NP, each over every block before the next: neighbouring MFMAs never share an accumulator
      constexpr int NPROD = NP == 1 ? 1 : 3;
#pragma unroll
      for (int pr = 0; pr < NPROD; pr++) {
        const int pa = pr == 2 ? 1 : 0, pb = pr == 1 ? 1 : 0;
#pragma unroll
        for (int i = 0; i < FM; i++) {
#pragma unroll
          for (int j = 0; j < FN; j++) {
            acc[pa + pb][i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[cur][pa][i], fb[cur][pb][j], acc[pa + pb][i][j], 0, 0, 0);
            // the next stage's DMA pieces ride between the MFMAs of the step
            if (more && pr == 0 && i * FN + j < PPS) dma_piece(nst, k1, ks * PPS + i * FN + j);
          }
        }
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    // tile kt + 1 must have landed (own DMA: vmcnt; the pieces just issued for a later tile may stay in flight) and every wave
    // must be done reading this stage
    if constexpr (NSTAGE == 3 && more)
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(Cf::PIECES) : "memory");
    else
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  };
  int kt = 0;
  for (; kt < nkt - (NSTAGE - 1); kt++) k_tile(std::true_type{}, kt);
  for (; kt < nkt; kt++) k_tile(std::false_type{}, kt);

  // epilogue: C = alpha*(G0 + 256*G1) + beta*C0 mod 2^n; beta == 0 never reads C
#pragma unroll
  for (int i = 0; i < FM; i++)
#pragma unroll
    for (int j = 0; j < FN; j++)
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int64_t row = m0 + wm0 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
        const int64_t col = n0 + wn0 + j * 32 + lo;
        if (row < g.M && col < g.N) {
          T *p = g.C + row * g.rsC + col * g.csC;
          uint32_t x = (uint32_t)acc[0][i][j][r];
          if constexpr (NP == 2) x += (uint32_t)acc[1][i][j][r] << 8;
          uint32_t v = g.alpha * x;
          if (g.beta != 0) v += g.beta * (uint32_t)*p;
          *p = (T)v;
        }
      }
}

inline int64_t rup64(int64_t v, int64_t m) { return (v + m - 1) / m * m; }

}  // namespace

template <typename T>
size_t gemm_narrow_mfma_workspace_bytes(int64_t M, int64_t N, int64_t K) {
  using Cf = NarrowCfg<(int)sizeof(T)>;
  const int64_t Kpad = rup64(K < NARROW_MAX_K ? K : NARROW_MAX_K, Cf::BK);
  return (size_t)(sizeof(T) * (rup64(M, Cf::BM) + rup64(N, Cf::BN)) * Kpad);
}

// ws: gemm_narrow_mfma_workspace_bytes(M, N, K) bytes of device memory usable on stream s; K <= NARROW_MAX_K
template <typename T>
hipError_t launch_gemm_narrow_mfma(const GemmArgs<T> &a, void *ws, hipStream_t s) {
  if (a.M <= 0 || a.N <= 0 || a.K <= 0) return hipSuccess;
  if (a.K > NARROW_MAX_K || a.batch != 1) return hipErrorInvalidValue;
  constexpr int NP = (int)sizeof(T);
  using Cf = NarrowCfg<NP>;
  const int64_t Mpad = rup64(a.M, Cf::BM), Npad = rup64(a.N, Cf::BN), Kpad = rup64(a.K, Cf::BK);
  if ((Mpad / Cf::BM) * (Npad / Cf::BN) > 0x7fffffffll) return hipErrorInvalidValue;
  int8_t *Ap = (int8_t *)ws, *Bp = Ap + NP * Mpad * Kpad;
  hipError_t e = launch_narrow_planes<T>(Ap, a.A, a.M, a.K, a.rsA, a.csA, Mpad, Kpad, s);
  if (e != hipSuccess) return e;
  e = launch_narrow_planes<T>(Bp, a.B, a.N, a.K, a.csB, a.rsB, Npad, Kpad, s);
  if (e != hipSuccess) return e;
  constexpr size_t lds = Cf::NSTAGE * Cf::STAGE;
  static PerDeviceOnce attr;
  e = attr.run([&] {
    return hipFuncSetAttribute(reinterpret_cast<const void *>(gemm_narrow_kernel<T>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  });
  if (e != hipSuccess) return e;
  NarrowArgs<T> g;
  g.Ap = Ap; g.Bp = Bp;
  g.planeA = Mpad * Kpad; g.planeB = Npad * Kpad; g.Kpad = Kpad;
  g.M = a.M; g.N = a.N;
  g.alpha = (uint32_t)(int32_t)a.alpha; g.beta = (uint32_t)(int32_t)a.beta;
  g.C = a.C; g.rsC = a.rsC; g.csC = a.csC;
  g.tiles_m = (int)(Mpad / Cf::BM); g.tiles_n = (int)(Npad / Cf::BN);
  g.group_m = 4;
  hipLaunchKernelGGL(gemm_narrow_kernel<T>, dim3((unsigned)(g.tiles_m * g.tiles_n)), dim3(NTHREADS), lds, s, g);
  return hipGetLastError();
}

template size_t gemm_narrow_mfma_workspace_bytes<int8_t>(int64_t, int64_t, int64_t);
template size_t gemm_narrow_mfma_workspace_bytes<int16_t>(int64_t, int64_t, int64_t);
template hipError_t launch_gemm_narrow_mfma<int8_t>(const GemmArgs<int8_t> &, void *, hipStream_t);
template hipError_t launch_gemm_narrow_mfma<int16_t>(const GemmArgs<int16_t> &, void *, hipStream_t);

}  // namespace laser_hip
