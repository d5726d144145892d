// laser_amd/csrc/softmax_axis_plan.h -- which kernel laser_hip_softmax_axis_f32_dev launches for a shape, with what strip
// width, grid and LDS (include/laser_hip.h "exp and row softmax"; the kernels are in softmax_axis.hip and log_softmax.hip).
// Plain C++ with no includes and no HIP: the library's launcher and a host program read the same function.
//
// The operand is (outer, n, inner) with the softmax along n.  inner == 1 is the row case (codes 0 .. 2 of the row kernels,
// one row per outer index).  Otherwise a workgroup of 256 lanes owns a strip: LH_SOFTMAX_AXIS_CW consecutive inner positions
// of one outer index over all n.  A lane takes 4 adjacent columns (one 16-byte vector where `vec` allows it), so CW / 4
// lanes span a strip row and 1024 / CW row lanes walk down it.
//   8  resident   n <= LH_SOFTMAX_AXIS_RESIDENT_N: the strip is read once into registers (the lanes of a workgroup hold at
//                 most 2048 x 16 elements between them), and written once
//   9  streaming  longer n: three passes over the strip, one chunk of 8192 rows at a time
//   + 4 when `vec` is 0 (single-element accesses)
#ifndef LASER_HIP_SOFTMAX_AXIS_PLAN_H
#define LASER_HIP_SOFTMAX_AXIS_PLAN_H

#ifndef LH_SOFTMAX_AXIS_CW
#define LH_SOFTMAX_AXIS_CW 16  // strip width in columns.  16 is what the library ships and the tests run; -DLH_SOFTMAX_AXIS_CW=32
                               // builds too, only to repeat the recorded comparison (profiles/softmax/README.md: slower everywhere)
#endif
// the strip stays in registers while a lane's share is at most 128 values: 2 elements per leaf of the order with 16 columns
// (4 per leaf, 256 values and their addresses, does not fit the 512 registers of a lane without spilling)
#define LH_SOFTMAX_AXIS_RESIDENT_N (LH_SOFTMAX_AXIS_CW == 16 ? 2048 : 1024)
#define LH_SOFTMAX_AXIS_MAX_N_PLAN (1ll << 20)    // 128 chunk partials per column (LASER_HIP_SOFTMAX_AXIS_MAX_N)
#define LH_SOFTMAX_ROWS_MAX_N_PLAN (1ll << 26)    // LASER_HIP_SOFTMAX_MAX_N
#define LH_SOFTMAX_MAX_WORKGROUPS 2048

// LDS of the kernels: the lexp table, the fold scratch, and what each kernel adds
#define LH_SOFTMAX_LDS_LUT 4096
#define LH_SOFTMAX_LDS_RED (260 * 4)

// The strip kernels' plan.  out4 = {kernel code, strip width CW, workgroups, LDS bytes}.  The grid is min(2048, strips) on
// every device, as the row kernels' is; `cus` (compute units of the device) is taken for symmetry with laser_hip_plan_f32
// and does not change the plan.  Returns 0, or -1 for a shape the entry point refuses (outer < 0, n < 1, inner < 1, n past
// the bound).
static inline int lh_softmax_axis_strip_plan(const long long outer, const long long n, const long long inner, const int vec,
                                             const int cus, long long *out4) {
  if (outer < 0 || n < 1 || inner < 1 || n > LH_SOFTMAX_AXIS_MAX_N_PLAN) return -1;
  (void)cus;
  const long long cap = LH_SOFTMAX_MAX_WORKGROUPS;
  const int cw = LH_SOFTMAX_AXIS_CW;
  const long long per_outer = inner / cw + (inner % cw != 0);  // strips of one outer index
  // min(outer * per_outer, cap) without forming a product that could overflow
  long long groups = cap;
  if (outer == 0) groups = 0;
  else if (per_outer < cap && outer < cap && outer * per_outer < cap) groups = outer * per_outer;
  const int k = n <= LH_SOFTMAX_AXIS_RESIDENT_N ? 8 : 9;
  out4[0] = k + (vec ? 0 : 4);
  out4[1] = cw;
  out4[2] = groups;
  // table + one 16-byte vector per lane for the folds + the column maxima of the four waves + the column sums
  // (+ 128 chunk partials per column when streaming)
  out4[3] = LH_SOFTMAX_LDS_LUT + 256 * 16 + 4 * cw * 4 + cw * 4 + (k == 9 ? 128 * cw * 4 : 0);
  return 0;
}

// The plan of laser_hip_softmax_axis_f32_dev for a shape.  inner == 1 is planned with a unit axis stride, the row kernels
// (CW = 0): softmax_wave_kernel (4 rows per workgroup), softmax_block_kernel, softmax_long_kernel; a lone column with another
// axis stride takes the strip kernels (lh_softmax_axis_strip_plan).
static inline int lh_softmax_axis_plan(const long long outer, const long long n, const long long inner, const int vec, const int cus,
                                       long long *out4) {
  if (inner != 1) return lh_softmax_axis_strip_plan(outer, n, inner, vec, cus, out4);
  if (outer < 0 || n < 1 || n > LH_SOFTMAX_ROWS_MAX_N_PLAN) return -1;
  (void)cus;
  const long long cap = LH_SOFTMAX_MAX_WORKGROUPS;
  const int k = n <= 1024 ? 0 : n <= 8192 ? 1 : 2;
  const long long want = k == 0 ? outer / 4 + (outer % 4 != 0) : outer;
  out4[0] = k + (vec ? 0 : 4);
  out4[1] = 0;
  out4[2] = want < cap ? want : cap;
  out4[3] = LH_SOFTMAX_LDS_LUT + (k >= 1 ? LH_SOFTMAX_LDS_RED : 0) + (k == 2 ? 8192 * 4 : 0);
  return 0;
}

#endif  // LASER_HIP_SOFTMAX_AXIS_PLAN_H
