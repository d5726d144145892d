// laser_amd/csrc/scan_plan.h -- what laser_hip_cumsum_*_dev launches for a shape (include/laser_hip.h "Row cumsum, searchsorted
// and the inverse-CDF sampler"; the kernel is in scan.hip, the order in scan_core.h).  Plain C++ with no HIP: the library's
// launcher and a host program read the same function.
//
// A workgroup has LH_SCAN_LANES lanes, a lane owns one run of R = LH_SCAN_RUN elements per tile.
//   0  a wave per row        n <= LH_SCAN_WAVE * R: the row is one tile of a wave; a workgroup owns LH_SCAN_LANES / LH_SCAN_WAVE
//                            rows at a time
//   1  a workgroup per row   longer rows: a tile is LH_SCAN_LANES * R elements and the workgroup walks ceil(n / tile) of them
// Either way a workgroup takes its groups of rows with a grid-sized stride, and no workgroup waits on another.  Whether a
// launch uses 16-byte accesses depends on the operands' addresses and strides, not on the shape: it is not part of the plan.
#ifndef LASER_HIP_SCAN_PLAN_H
#define LASER_HIP_SCAN_PLAN_H

#include "scan_core.h"

#define LH_SCAN_MAX_N (1ll << 24)  // LASER_HIP_SCAN_MAX_N
#define LH_SCAN_LANES 256          // lanes of a workgroup
#define LH_SCAN_WAVE 64            // lanes that own a short row
#define LH_SCAN_WGS_PER_CU 8       // the grid is capped at this many workgroups per compute unit
#define LH_SCAN_DEFAULT_CUS 256    // cus <= 0

// out4 = {variant, rows a workgroup owns at a time, workgroups, tiles per row}.  elem_size: 4 or 8.  Returns 0, or -1 for a
// shape the entry points refuse (rows < 0, n outside 1 .. 2^24) or another element size.
static inline int lh_scan_plan(const long long rows, const long long n, const int elem_size, const int cus, long long *out4) {
  if (rows < 0 || n < 1 || n > LH_SCAN_MAX_N || (elem_size != 4 && elem_size != 8)) return -1;
  const int variant = n <= (long long)LH_SCAN_WAVE * LH_SCAN_RUN ? 0 : 1;
  const long long per = variant == 0 ? LH_SCAN_LANES / LH_SCAN_WAVE : 1;
  const long long tile = (LH_SCAN_LANES / per) * LH_SCAN_RUN;
  const long long cap = (long long)(cus > 0 ? cus : LH_SCAN_DEFAULT_CUS) * LH_SCAN_WGS_PER_CU;
  const long long want = rows / per + (rows % per != 0);
  out4[0] = variant;
  out4[1] = per;
  out4[2] = want < cap ? want : cap;
  out4[3] = (n + tile - 1) / tile;
  return 0;
}

#endif  // LASER_HIP_SCAN_PLAN_H
