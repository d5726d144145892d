// laser_amd/csrc/asm_kernels.h -- the table of the hand-scheduled assembly kernels (laser_amd/asmgen/): one row per kernel, and the
// rows the choosers of asm_plan.h take, found by attribute at compile time.  No HIP dependency.
#pragma once
#include <stdint.h>

namespace laser_hip {

// What a kernel is: the choosers look rows up by these attributes (find_kernel), never by position
enum Family : uint8_t {
  kF32,        // float32 GEMM on 32x32 blocks (laser_amd/asmgen/f32_kernel.py)
  kF32x16,     // float32 GEMM on 16x16 blocks (v_mfma_f32_16x16x4_f32; asmgen/f32x16_kernel.py)
  kF64,        // float64 GEMM (v_mfma_f64_16x16x4_f64; asmgen/f64_kernel.py)
  kI32,        // int32 GEMM via four int8 limb planes (asmgen/i8_kernel.py)
  kI64,        // int64 GEMM via eight int8 limb planes (i8_kernel.py "i64_64x64x32")
  kConv,       // implicit-GEMM convolution, any kernel size / stride / zero padding (conv_kernel.py)
  kConvWalk,   // the same as unit walkers (f32_kernel.py Cfg.cpers): a workgroup runs units (image, tile) g, g + G, g + 2G ... and goes
               // from one to the next inside its K loop (the next unit's first gathers before the old tile's last K-tiles are
               // multiplied, the old tile's C stores from the gaps of the new tile's first K-tile body)
};
struct KernelInfo {
  const char *symbol;
  Family fam;
  bool exact;   // laser-order: the chain restarts every kc (gemm.nim:150-158); false: one chain over the whole K
  bool nt;      // B passed transposed (unit ROW stride: k-contiguous like A, BASELINE configs[2])
  bool pre;     // fused prologue: relu on A's and / or B's elements in the staging registers; one tile per workgroup
  int cls;      // tile class of option "asm_tile" (the f32 GEMM families; -1 for the others)
  int bm, bn, bk;
  // tile-choice model (round 4: refitted to profiles/r04/plan_sweep_f32_mid_v2.jsonl, every candidate x plan forced; round 6: the 128x128x16 tile's
  // alone-on-its-CU figure 0.935 -> 0.92 -- 2048^3, one round of 256 tiles: 128.4 us against the 32-deep variant's 126.6, x16_ab_mid_j.jsonl): fraction of the matrix peak a CU reaches on this tile when
  // its workgroup slots are full / when one workgroup has the CU to itself, and the launch's fixed cost (prologue, first
  // loads, epilogue of the last round) in microseconds
  double eff, eff_alone, fixed_us;
  int occ;   // workgroups of this kernel a CU holds (registers / LDS)
  // Kernels whose persistent workgroups go from one whole tile to the next without leaving the K loop (asmgen/f32_kernel.py Cfg.pipe:
  // the next tile's first K-tiles are fetched by the last bodies of this one, its first body stores this one's C): what one such
  // transition saves against a fresh workgroup per tile, in microseconds (0: the kernel has no pipelined transition).  Measured:
  // profiles/r06/pipe_*.jsonl.  256x128x32 (one workgroup per CU): pipe_ab_{big,mid}_b.jsonl (plain vs strided, interleaved, same
  // bits): +0.2 ... +0.5 % at 4096^3 ... 8192^3, +1.6 % at 5120^3, +1.3 ... +2.3 % on the convolution's GEMM twin (8192x3072x1152:
  // three tiles of 36 K-tiles per workgroup).  128x128x32: +0.3 ... +3 %, a tile the model rarely picks.  The 16x16-block tiles
  // (f32x16_kernel.py trans_after) and float64 128x128x16 (f64_kernel.py trans_after): one workgroup per CU too.  256x256x16: -1.8 ...
  // +1.1 % (sixteen blocks' stores in the first sixteen gaps of a 16-deep body): left alone.  Two or three workgroups per CU
  // (128x128x16, 64x64) cover each other's transitions already, and a static share of the tiles quantises in workgroup slots where
  // the plain launch quantises in CUs: -0.3 ... -14 %
  double pipe_us;
  // what tells a row from the others of its family with the same exact / nt / pre: the tile class, or the tile's rows
  constexpr int tile() const { return cls >= 0 ? cls : bm; }
};
// One row per kernel.  The position is visible outside this file -- last_f32_asm / last_f64_asm / last_i32_asm = 1 + index, option
// "asm_kernel", laser_hip_plan_f32, bench.py's ASM_KERNEL_SYMBOLS -- so rows are appended, never moved.
// Tile classes: 0 = the large tile (laser-order 256x128x32, one chain 256x256x16), 1 = 256x128x32 one chain (finer tile quantisation
// for the fast mode), 2 = 128x128x16, 3 = 128x128x32 (one workgroup per CU: one round of 129 .. 256 tiles, where a workgroup has its
// CU to itself), 4 = 64x64x32 (three workgroups per CU: problems of few tiles -- 1024^3 = 32 tiles of 256x128 for 256 CUs -- and the
// tile quantisation of mid-size ones -- 3072^3 = 1.125 rounds of 256x128); on 16x16 blocks, tiles whose sides are multiples of 32 for
// the problems the 32x32-block tiles quantise badly: 5 = 96x96, 6 = 160x96, 7 = 128x96, 8 = 192x96, 9 = 160x160 (the reference's own
// benchmark shape 1920^3, gemm_bench_float32.nim:383-410, is 240 tiles of 160x96 against 225 of 128x128 on 256 CUs; 1536^3 is 256
// tiles of 96x96 against 144 of 128x128).  The convolution tiles: 256x128 (up to 31 taps), 128x128 and 64x128 (fewer output channels).
constexpr int kNumKernels = 72;
constexpr KernelInfo kKernels[kNumKernels] = {
    // symbol                          family     exact nt pre  cls   bm   bn  bk eff    alone  fixed occ pipe_us
    {"lh_f32_exact_256x128x32",        kF32,      1,    0, 0,    0, 256, 128, 32, 0.965, 0.965, 10.0,  1, 2.5}, // 0
    {"lh_f32_fast_256x256x16",         kF32,      0,    0, 0,    0, 256, 256, 16, 0.98,  0.98,  12.0,  1, 0},   // 1
    {"lh_f32_exact_128x128x16",        kF32,      1,    0, 0,    2, 128, 128, 16, 0.95,  0.92,   6.0,  2, 0},   // 2
    {"lh_f32_fast_128x128x16",         kF32,      0,    0, 0,    2, 128, 128, 16, 0.96,  0.93,   6.0,  2, 0},   // 3
    {"lh_f32_exact_256x128x32_nt",     kF32,      1,    1, 0,    0, 256, 128, 32, 0.965, 0.965, 10.0,  1, 2.5}, // 4
    {"lh_f32_fast_256x256x16_nt",      kF32,      0,    1, 0,    0, 256, 256, 16, 0.98,  0.98,  12.0,  1, 0},   // 5
    {"lh_f32_exact_128x128x16_nt",     kF32,      1,    1, 0,    2, 128, 128, 16, 0.95,  0.92,   6.0,  2, 0},   // 6
    {"lh_f32_fast_128x128x16_nt",      kF32,      0,    1, 0,    2, 128, 128, 16, 0.96,  0.93,   6.0,  2, 0},   // 7
    {"lh_f32_fast_256x128x32",         kF32,      0,    0, 0,    1, 256, 128, 32, 0.97,  0.97,  10.0,  1, 2.5}, // 8
    {"lh_f32_fast_256x128x32_nt",      kF32,      0,    1, 0,    1, 256, 128, 32, 0.97,  0.97,  10.0,  1, 2.5}, // 9
    {"lh_f32_conv_exact_256x128x32",   kConv,     1,    0, 0,   -1, 256, 128, 32, 0.88,  0.88,  15.0,  1, 0},   // 10
    {"lh_f32_conv_fast_256x128x32",    kConv,     0,    0, 0,   -1, 256, 128, 32, 0.88,  0.88,  15.0,  1, 0},   // 11
    {"lh_f32_exact_64x64x32",          kF32,      1,    0, 0,    4,  64,  64, 32, 0.90,  0.84,   6.0,  3, 0},   // 12
    {"lh_f32_fast_64x64x32",           kF32,      0,    0, 0,    4,  64,  64, 32, 0.91,  0.85,   6.0,  3, 0},   // 13
    {"lh_f32_exact_64x64x32_nt",       kF32,      1,    1, 0,    4,  64,  64, 32, 0.90,  0.84,   6.0,  3, 0},   // 14
    {"lh_f32_fast_64x64x32_nt",        kF32,      0,    1, 0,    4,  64,  64, 32, 0.91,  0.85,   6.0,  3, 0},   // 15
    {"lh_f64_exact_128x128x16",        kF64,      1,    0, 0,   -1, 128, 128, 16, 0.937, 0.945,  8.0,  1, 3.0}, // 16
    {"lh_f64_fast_128x128x16",         kF64,      0,    0, 0,   -1, 128, 128, 16, 0.965, 0.97,   8.0,  1, 3.0}, // 17
    {"lh_f64_exact_64x64x16",          kF64,      1,    0, 0,   -1,  64,  64, 16, 0.915, 0.815,  3.0,  2, 0},   // 18
    {"lh_f64_fast_64x64x16",           kF64,      0,    0, 0,   -1,  64,  64, 16, 0.93,  0.83,   3.0,  2, 0},   // 19
    {"lh_i32_128x128x32",              kI32,      0,    0, 0,   -1, 128, 128, 32, 0.8,   0.8,   10.0,  1, 0},   // 20
    {"lh_f32_conv_exact_128x128x32",   kConv,     1,    0, 0,   -1, 128, 128, 32, 0.8,   0.8,   12.0,  1, 0},   // 21
    {"lh_f32_conv_fast_128x128x32",    kConv,     0,    0, 0,   -1, 128, 128, 32, 0.8,   0.8,   12.0,  1, 0},   // 22
    {"lh_f32_conv_exact_64x128x32",    kConv,     1,    0, 0,   -1,  64, 128, 32, 0.72,  0.72,   8.0,  2, 0},   // 23
    {"lh_f32_conv_fast_64x128x32",     kConv,     0,    0, 0,   -1,  64, 128, 32, 0.72,  0.72,   8.0,  2, 0},   // 24
    {"lh_f64_exact_128x128x16_nt",     kF64,      1,    1, 0,   -1, 128, 128, 16, 0.937, 0.945,  8.0,  1, 3.0}, // 25
    {"lh_f64_fast_128x128x16_nt",      kF64,      0,    1, 0,   -1, 128, 128, 16, 0.965, 0.97,   8.0,  1, 3.0}, // 26
    {"lh_f64_exact_64x64x16_nt",       kF64,      1,    1, 0,   -1,  64,  64, 16, 0.915, 0.815,  3.0,  2, 0},   // 27
    {"lh_f64_fast_64x64x16_nt",        kF64,      0,    1, 0,   -1,  64,  64, 16, 0.93,  0.83,   3.0,  2, 0},   // 28
    {"lh_i64_64x64x32",                kI64,      0,    0, 0,   -1,  64,  64, 32, 0.7,   0.7,   10.0,  1, 0},   // 29
    {"lh_f32_exact_128x128x32",        kF32,      1,    0, 0,    3, 128, 128, 32, 0.95,  0.95,   7.0,  1, 1.0}, // 30
    {"lh_f32_fast_128x128x32",         kF32,      0,    0, 0,    3, 128, 128, 32, 0.96,  0.96,   7.0,  1, 1.0}, // 31
    {"lh_f32_exact_128x128x32_nt",     kF32,      1,    1, 0,    3, 128, 128, 32, 0.95,  0.95,   7.0,  1, 1.0}, // 32
    {"lh_f32_fast_128x128x32_nt",      kF32,      0,    1, 0,    3, 128, 128, 32, 0.96,  0.96,   7.0,  1, 1.0}, // 33
    {"lh_f32_exact_256x128x32_pre",    kF32,      1,    0, 1,    0, 256, 128, 32, 0.92,  0.92,  10.0,  1, 0},   // 34
    {"lh_f32_exact_256x128x32_pre_nt", kF32,      1,    1, 1,    0, 256, 128, 32, 0.92,  0.92,  10.0,  1, 0},   // 35
    {"lh_f32_fast_256x256x16_pre",     kF32,      0,    0, 1,    0, 256, 256, 16, 0.93,  0.93,  12.0,  1, 0},   // 36
    {"lh_f32_fast_256x256x16_pre_nt",  kF32,      0,    1, 1,    0, 256, 256, 16, 0.93,  0.93,  12.0,  1, 0},   // 37
    {"lh_f32_exact_128x128x16_pre",    kF32,      1,    0, 1,    2, 128, 128, 16, 0.90,  0.86,   6.0,  2, 0},   // 38
    {"lh_f32_exact_128x128x16_pre_nt", kF32,      1,    1, 1,    2, 128, 128, 16, 0.90,  0.86,   6.0,  2, 0},   // 39
    {"lh_f32_fast_128x128x16_pre",     kF32,      0,    0, 1,    2, 128, 128, 16, 0.91,  0.87,   6.0,  2, 0},   // 40
    {"lh_f32_fast_128x128x16_pre_nt",  kF32,      0,    1, 1,    2, 128, 128, 16, 0.91,  0.87,   6.0,  2, 0},   // 41
    {"lh_f32_exact_64x64x32_pre",      kF32,      1,    0, 1,    4,  64,  64, 32, 0.84,  0.74,   3.0,  3, 0},   // 42
    {"lh_f32_exact_64x64x32_pre_nt",   kF32,      1,    1, 1,    4,  64,  64, 32, 0.84,  0.74,   3.0,  3, 0},   // 43
    {"lh_f32_fast_64x64x32_pre",       kF32,      0,    0, 1,    4,  64,  64, 32, 0.85,  0.76,   3.0,  3, 0},   // 44
    {"lh_f32_fast_64x64x32_pre_nt",    kF32,      0,    1, 1,    4,  64,  64, 32, 0.85,  0.76,   3.0,  3, 0},   // 45
    // (fitted to profiles/r06/x16_ab_{ref,mid}_g.jsonl, x16_ab_more_i.jsonl; the laser-order entries + 0.007 with the running sum in VGPRs, x16_ab_big2_n.jsonl; the many-round figures of pipe_ab_x16_p.jsonl at 7680^3 -- 0.963 / 0.972 on 160x160, 0.934 / 0.952 on 96x96 --: plain launches at 1536^3 .. 5120^3, 1000x3000x2000; the 64x64 tiles'
    // fixed cost 3 -> 6 us from the same runs: 1664^3 and 1000x3000x2000 took 84 / 98 us where the table said 80 / 92)
    {"lh_f32x16_exact_96x96x32",       kF32x16,   1,    0, 0,    5,  96,  96, 32, 0.925, 0.925,  5.0,  1, 1.5}, // 46
    {"lh_f32x16_fast_96x96x32",        kF32x16,   0,    0, 0,    5,  96,  96, 32, 0.943, 0.93,   5.0,  1, 1.5}, // 47
    {"lh_f32x16_exact_96x96x32_nt",    kF32x16,   1,    1, 0,    5,  96,  96, 32, 0.925, 0.925,  5.0,  1, 1.5}, // 48
    {"lh_f32x16_fast_96x96x32_nt",     kF32x16,   0,    1, 0,    5,  96,  96, 32, 0.943, 0.93,   5.0,  1, 1.5}, // 49
    {"lh_f32x16_exact_160x96x32",      kF32x16,   1,    0, 0,    6, 160,  96, 32, 0.952, 0.958,  6.0,  1, 1.5}, // 50
    {"lh_f32x16_fast_160x96x32",       kF32x16,   0,    0, 0,    6, 160,  96, 32, 0.96,  0.963,  6.0,  1, 1.5}, // 51
    {"lh_f32x16_exact_160x96x32_nt",   kF32x16,   1,    1, 0,    6, 160,  96, 32, 0.952, 0.958,  6.0,  1, 1.5}, // 52
    {"lh_f32x16_fast_160x96x32_nt",    kF32x16,   0,    1, 0,    6, 160,  96, 32, 0.96,  0.963,  6.0,  1, 1.5}, // 53
    {"lh_f32x16_exact_128x96x32",      kF32x16,   1,    0, 0,    7, 128,  96, 32, 0.938, 0.922,  5.5,  1, 1.5}, // 54
    {"lh_f32x16_fast_128x96x32",       kF32x16,   0,    0, 0,    7, 128,  96, 32, 0.935, 0.94,   5.5,  1, 1.5}, // 55
    {"lh_f32x16_exact_128x96x32_nt",   kF32x16,   1,    1, 0,    7, 128,  96, 32, 0.938, 0.922,  5.5,  1, 1.5}, // 56
    {"lh_f32x16_fast_128x96x32_nt",    kF32x16,   0,    1, 0,    7, 128,  96, 32, 0.935, 0.94,   5.5,  1, 1.5}, // 57
    {"lh_f32x16_exact_192x96x32",      kF32x16,   1,    0, 0,    8, 192,  96, 32, 0.95,  0.952,  6.5,  1, 1.5}, // 58
    {"lh_f32x16_fast_192x96x32",       kF32x16,   0,    0, 0,    8, 192,  96, 32, 0.962, 0.965,  6.5,  1, 1.5}, // 59
    {"lh_f32x16_exact_192x96x32_nt",   kF32x16,   1,    1, 0,    8, 192,  96, 32, 0.95,  0.952,  6.5,  1, 1.5}, // 60
    {"lh_f32x16_fast_192x96x32_nt",    kF32x16,   0,    1, 0,    8, 192,  96, 32, 0.962, 0.965,  6.5,  1, 1.5}, // 61
    {"lh_f32x16_exact_160x160x32",     kF32x16,   1,    0, 0,    9, 160, 160, 32, 0.959, 0.945,  8.0,  1, 1.5}, // 62
    {"lh_f32x16_fast_160x160x32",      kF32x16,   0,    0, 0,    9, 160, 160, 32, 0.968, 0.956,  8.0,  1, 1.5}, // 63
    {"lh_f32x16_exact_160x160x32_nt",  kF32x16,   1,    1, 0,    9, 160, 160, 32, 0.959, 0.945,  8.0,  1, 1.5}, // 64
    {"lh_f32x16_fast_160x160x32_nt",   kF32x16,   0,    1, 0,    9, 160, 160, 32, 0.968, 0.956,  8.0,  1, 1.5}, // 65
    {"lh_f32_conv_exact_256x128x32_p", kConvWalk, 1,    0, 0,   -1, 256, 128, 32, 0.90,  0.90,  15.0,  1, 0},   // 66
    {"lh_f32_conv_fast_256x128x32_p",  kConvWalk, 0,    0, 0,   -1, 256, 128, 32, 0.90,  0.90,  15.0,  1, 0},   // 67
    {"lh_f32_conv_exact_128x128x32_p", kConvWalk, 1,    0, 0,   -1, 128, 128, 32, 0.82,  0.82,  12.0,  1, 0},   // 68
    {"lh_f32_conv_fast_128x128x32_p",  kConvWalk, 0,    0, 0,   -1, 128, 128, 32, 0.82,  0.82,  12.0,  1, 0},   // 69
    {"lh_f32_conv_exact_64x128x32_p",  kConvWalk, 1,    0, 0,   -1,  64, 128, 32, 0.74,  0.74,   8.0,  2, 0},   // 70
    {"lh_f32_conv_fast_64x128x32_p",   kConvWalk, 0,    0, 0,   -1,  64, 128, 32, 0.74,  0.74,   8.0,  2, 0}    // 71
};
// The row of the kernel with these attributes, -1 if there is none.  tile: the tile class of the f32 GEMM families, the tile's rows
// (bm) for the others.
constexpr int find_kernel(Family fam, int tile, bool exact, bool nt = false, bool pre = false) {
  for (int k = 0; k < kNumKernels; k++) {
    const KernelInfo &r = kKernels[k];
    if (r.fam == fam && r.tile() == tile && r.exact == exact && r.nt == nt && r.pre == pre) return k;
  }
  return -1;
}
constexpr bool kernel_attributes_unique() {
  for (int k = 0; k < kNumKernels; k++)
    if (find_kernel(kKernels[k].fam, kKernels[k].tile(), kKernels[k].exact, kKernels[k].nt, kKernels[k].pre) != k) return false;
  return true;
}
static_assert(kernel_attributes_unique(), "two rows of kKernels with the same attributes: find_kernel sees the first only");

// The choosers' rows, resolved at compile time.  f32 GEMMs: [tile class][laser-order][B transposed][fused prologue]
struct F32Rows { int k[10][2][2][2]; };
constexpr F32Rows kF32Rows = [] {
  F32Rows t{};
  for (int c = 0; c < 10; c++)
    for (int e = 0; e < 2; e++)
      for (int n = 0; n < 2; n++)
        for (int p = 0; p < 2; p++) t.k[c][e][n][p] = find_kernel(c < 5 ? kF32 : kF32x16, c, e, n, p);   // (5..9: 16x16 blocks)
  return t;
}();
// f64 GEMMs: [128x128x16, 64x64x16][laser-order][B transposed]
struct F64Rows { int k[2][2][2]; };
constexpr F64Rows kF64Rows = [] {
  F64Rows t{};
  for (int i = 0; i < 2; i++)
    for (int e = 0; e < 2; e++)
      for (int n = 0; n < 2; n++) t.k[i][e][n] = find_kernel(kF64, i == 0 ? 128 : 64, e, n);
  return t;
}();
// convolutions by tile rows: [256, 128, 64][laser-order], and the unit walker of each
struct ConvRows { int k[3][2], walker[3][2]; };
constexpr ConvRows kConvRows = [] {
  ConvRows t{};
  for (int i = 0; i < 3; i++)
    for (int e = 0; e < 2; e++) {
      t.k[i][e] = find_kernel(kConv, 256 >> i, e);
      t.walker[i][e] = find_kernel(kConvWalk, 256 >> i, e);
    }
  return t;
}();
constexpr int kI32Row = find_kernel(kI32, 128, false), kI64Row = find_kernel(kI64, 64, false);
static_assert(kI32Row >= 0 && kI64Row >= 0, "the integer limb kernels");

}  // namespace laser_hip
