// laser_amd/csrc/select_plan.h -- what laser_hip_topk_rows_f32_dev and laser_hip_argmax_rows_f32_dev launch for a shape
// (include/laser_hip_select.h "Row top-k, argmax and top-k sampling"; the kernels are in select.hip).  Plain C++ with no
// includes and no HIP: the library's launchers and the CPU suite read the same function.
//
// The source is (rows, n) with unit column stride.  Three lane mappings chosen by n alone, as the other row kernels have them:
//   0  wave       n <= 256: one wave per row, four rows per workgroup of 256 lanes; the row's composites are sorted whole
//   1  resident   n <= 8192: one workgroup per row, 32 keys per lane loaded once; every pass runs from registers
//   2  streaming  n <= 2^24: one workgroup re-reads the row for each pass: four digit passes and one collection pass
//   + 4 when `vec` is 0 (single-element loads: the source's base or row stride off the 16-byte alignment)
// At most 2048 workgroups, which stride over the rows; one launch (none for rows = 0); no scratch.  argmax takes the mapping
// and the grid of k = 1 (its wave kernel needs no LDS, its workgroup kernel 32 bytes).
#ifndef LASER_HIP_SELECT_PLAN_H
#define LASER_HIP_SELECT_PLAN_H

#define LH_SELECT_MAX_N (1ll << 24)      // LASER_HIP_SELECT_MAX_N
#define LH_SELECT_MAX_ROWS (1ll << 26)   // LASER_HIP_SELECT_MAX_ROWS
#define LH_SELECT_MAX_K 1024             // LASER_HIP_SELECT_MAX_K
#define LH_SELECT_WAVE_N 256             // the longest row of one wave: 64 lanes x 4 elements
#define LH_SELECT_RESIDENT_N 8192        // the longest row a workgroup holds in registers: 256 lanes x 8 steps x 4 elements
#define LH_SELECT_MAX_WORKGROUPS 2048
#define LH_SELECT_COLLECT_CHUNK 4096     // elements of one chunk of the streaming collection pass: 256 lanes x 4 steps x 4
#define LH_SELECT_LDS_WAVE 8192          // 4 waves x 256 composites of 8 bytes
// 1024 composites + 256 histogram bins + the wave counts of a chunk (2 x 8 steps x 4 waves) + 4 words of pass state
#define LH_SELECT_LDS_BLOCK (1024 * 8 + 256 * 4 + 2 * 8 * 4 * 4 + 16)

// out3 = {kernel code, workgroups, LDS bytes of a workgroup}.  Returns 0, or -1 with nothing written for what the entry point
// refuses: rows outside 0 .. 2^26, n outside 1 .. 2^24, k outside 1 .. min(n, 1024).
static inline int lh_topk_plan(const long long rows, const long long n, const long long k, const int vec, long long *out3) {
  if (rows < 0 || rows > LH_SELECT_MAX_ROWS || n < 1 || n > LH_SELECT_MAX_N) return -1;
  if (k < 1 || k > n || k > LH_SELECT_MAX_K) return -1;
  const int code = n <= LH_SELECT_WAVE_N ? 0 : n <= LH_SELECT_RESIDENT_N ? 1 : 2;
  const long long want = code == 0 ? rows / 4 + (rows % 4 != 0) : rows;
  out3[0] = code + (vec ? 0 : 4);
  out3[1] = want < LH_SELECT_MAX_WORKGROUPS ? want : LH_SELECT_MAX_WORKGROUPS;
  out3[2] = code == 0 ? LH_SELECT_LDS_WAVE : LH_SELECT_LDS_BLOCK;
  return 0;
}

#endif  // LASER_HIP_SELECT_PLAN_H
