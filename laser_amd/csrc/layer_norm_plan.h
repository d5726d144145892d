// laser_amd/csrc/layer_norm_plan.h -- what laser_hip_layer_norm_f32_dev and laser_hip_layer_norm_grad_f32_dev launch for a
// shape (include/laser_hip.h "Layer normalization"; the kernels are in layer_norm.hip).  Plain C++ with no includes and no
// HIP: the library's launchers and a host program read the same function.
//
// The operands are (rows, n) with unit column stride.
//   what 0 (forward) and 1 (dx): the row kernels, three lane mappings chosen by n alone, as softmax_rows_plan.h has them
//     0  n <= 1024: one wave per row, four rows per workgroup of 256 lanes
//     1  n <= 8192 (one chunk of the order): one workgroup per row, the row in registers
//     2  longer rows, n <= 2^26: one workgroup streams the row's chunks
//     + 4 when `vec` is 0 (single-element accesses: a base, a row stride or gamma / beta off the 16-byte alignment)
//     At most 2048 workgroups, which stride over the rows; one launch (none for rows = 0); no scratch.
//   what 2 (dgamma and dbeta, both asked for): the column kernel, a workgroup per unit of (chunk of 8192 rows) x (strip of
//     LH_LAYER_NORM_CW columns); code 0 = the vector instance, 1 = single elements; min(2048, units) workgroups.
//     rows <= 8192   one launch writes both sums
//     longer         three launches: the chunk partials of both sums go to two row-major (chunks, n) scratch matrices, and
//                    the bias gradient's launch (bias_grad_plan.h) folds each with rows = chunks.  rows <= 2^26 keeps
//                    chunks <= 8192, one chunk.  (One sum asked for alone: one fold launch and one matrix fewer.)
#ifndef LASER_HIP_LAYER_NORM_PLAN_H
#define LASER_HIP_LAYER_NORM_PLAN_H

#define LH_LAYER_NORM_MAX_N (1ll << 26)       // LASER_HIP_LAYER_NORM_MAX_N
#define LH_LAYER_NORM_MAX_ROWS (1ll << 26)    // LASER_HIP_LAYER_NORM_MAX_ROWS: parameter gradients only
#define LH_LAYER_NORM_WAVE_N 1024             // the longest row of one wave: 64 lanes x 4 leaves x 4 elements
#define LH_LAYER_NORM_CHUNK 8192              // one chunk of the order: LH_REDUCE_STEPS x LH_REDUCE_LANES x 4
#define LH_LAYER_NORM_CW 8                    // strip width of the column kernel (profiles/layer_norm/README.md has the reason)
#define LH_LAYER_NORM_MAX_WORKGROUPS 2048
#define LH_LAYER_NORM_FORWARD 0
#define LH_LAYER_NORM_DX 1
#define LH_LAYER_NORM_PARAMS 2

// out4 = {kernel code of the first launch, workgroups of the first launch, launches, scratch bytes}.  Returns 0, or -1 with
// nothing written for what the entry points refuse: rows < 0, n < 1, n > 2^26, an unknown `what`, rows > 2^26 for what = 2.
static inline int lh_layer_norm_plan(const long long rows, const long long n, const int vec, const int what, long long *out4) {
  if (rows < 0 || n < 1 || n > LH_LAYER_NORM_MAX_N) return -1;
  const long long cap = LH_LAYER_NORM_MAX_WORKGROUPS;
  if (what == LH_LAYER_NORM_FORWARD || what == LH_LAYER_NORM_DX) {
    const int k = n <= LH_LAYER_NORM_WAVE_N ? 0 : n <= LH_LAYER_NORM_CHUNK ? 1 : 2;
    const long long want = k == 0 ? rows / 4 + (rows % 4 != 0) : rows;
    out4[0] = k + (vec ? 0 : 4);
    out4[1] = want < cap ? want : cap;
    out4[2] = rows == 0 ? 0 : 1;
    out4[3] = 0;
    return 0;
  }
  if (what != LH_LAYER_NORM_PARAMS || rows > LH_LAYER_NORM_MAX_ROWS) return -1;
  // rows == 0 is one (empty) chunk: its partial is the order's init, +0
  const long long chunks = rows == 0 ? 1 : rows / LH_LAYER_NORM_CHUNK + (rows % LH_LAYER_NORM_CHUNK != 0);
  const long long strips = n / LH_LAYER_NORM_CW + (n % LH_LAYER_NORM_CW != 0);
  const long long units = chunks * strips;  // <= 2^13 * 2^23
  out4[0] = vec ? 0 : 1;
  out4[1] = units < cap ? units : cap;
  out4[2] = chunks > 1 ? 3 : 1;
  out4[3] = chunks > 1 ? 2 * chunks * n * 4 : 0;  // <= 2^43
  return 0;
}

#endif  // LASER_HIP_LAYER_NORM_PLAN_H
