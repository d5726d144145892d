// laser_amd/csrc/softmax_rows_plan.h -- which kernel the row launchers of log_softmax.hip (softmax, logsumexp, log-softmax,
// softmax cross-entropy) start for a shape, with what grid and LDS (include/laser_hip.h "log, logsumexp, log-softmax and
// cross-entropy").  Plain C++ with no includes and no HIP: the library's launchers and a host program read the same function.
//
// Three lane mappings, chosen by n alone:
//   0  n <= 1024: one wave per row, four rows per workgroup of 256 lanes
//   1  n <= 8192 (one chunk of the order): one workgroup per row, the row in registers
//   2  longer rows, n <= 2^26: one workgroup streams the row, chunk partials in LDS
//   + 4 when `vec` is 0 (single-element accesses: a base or a row stride off its 16-byte alignment)
// At most LH_SOFTMAX_ROWS_MAX_WORKGROUPS workgroups, which stride over the rows.
#ifndef LASER_HIP_SOFTMAX_ROWS_PLAN_H
#define LASER_HIP_SOFTMAX_ROWS_PLAN_H

#define LH_SOFTMAX_ROWS_MAX_N (1ll << 26)        // LASER_HIP_SOFTMAX_MAX_N
#define LH_SOFTMAX_ROWS_WAVE_N 1024              // the longest row of one wave: 64 lanes x 4 leaves x 4 elements
#define LH_SOFTMAX_ROWS_CHUNK_N 8192             // one chunk of the order: LH_REDUCE_STEPS x LH_REDUCE_LANES x 4
#define LH_SOFTMAX_ROWS_MAX_WORKGROUPS 2048      // = LH_SOFTMAX_MAX_WORKGROUPS (softmax_axis_plan.h): 8 on each of 256 CUs
#define LH_SOFTMAX_ROWS_LDS_LUT 4096             // the lexp table
#define LH_SOFTMAX_ROWS_LDS_RED (260 * 4)        // the fold scratch
#define LH_SOFTMAX_ROWS_LDS_PART (8192 * 4)      // the chunk partials of a long row

// out3 = {kernel code, workgroups, LDS bytes}.  Returns 0, or -1 for a shape the entry points refuse (rows < 0, n < 1,
// n > 2^26).  rows = 0 plans no workgroup.
static inline int lh_softmax_rows_plan(const long long rows, const long long n, const int vec, long long *out3) {
  if (rows < 0 || n < 1 || n > LH_SOFTMAX_ROWS_MAX_N) return -1;
  const long long cap = LH_SOFTMAX_ROWS_MAX_WORKGROUPS;
  const int k = n <= LH_SOFTMAX_ROWS_WAVE_N ? 0 : n <= LH_SOFTMAX_ROWS_CHUNK_N ? 1 : 2;
  const long long want = k == 0 ? rows / 4 + (rows % 4 != 0) : rows;
  out3[0] = k + (vec ? 0 : 4);
  out3[1] = want < cap ? want : cap;
  out3[2] = LH_SOFTMAX_ROWS_LDS_LUT + (k >= 1 ? LH_SOFTMAX_ROWS_LDS_RED : 0) + (k == 2 ? LH_SOFTMAX_ROWS_LDS_PART : 0);
  return 0;
}

// The softmax gradient's row kernels (softmax_grad.hip) take the same three lane mappings at the same thresholds, the same
// codes and the same grid; they gather from no table, so only the LDS differs.  out3 and the return value as above.
static inline int lh_softmax_grad_rows_plan(const long long rows, const long long n, const int vec, long long *out3) {
  long long p[3];
  if (lh_softmax_rows_plan(rows, n, vec, p) != 0) return -1;
  const int k = (int)p[0] & 3;
  out3[0] = p[0];
  out3[1] = p[1];
  out3[2] = (k >= 1 ? LH_SOFTMAX_ROWS_LDS_RED : 0) + (k == 2 ? LH_SOFTMAX_ROWS_LDS_PART : 0);
  return 0;
}

#endif  // LASER_HIP_SOFTMAX_ROWS_PLAN_H
