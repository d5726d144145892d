// laser_amd/csrc/sampler_plan.h -- the size of an F+tree image and what laser_hip_sampler_build_f32_dev launches for a shape
// (include/laser_hip.h "F+tree weighted sampler"; the kernels are in sampler.hip).  Plain C++ with no includes and no HIP:
// the library's launcher and a host program read the same functions.
//
// A row of n weights has P = the next power of two >= n leaves and an image of 2 P elements.
//   0  rows in LDS   P <= LH_SAMPLER_SMALL_P: a workgroup of 256 lanes owns LH_SAMPLER_SMALL_LEAVES / P whole rows, forms every
//                    level in LDS and writes the images out as contiguous runs; one launch
//   1  segments      longer rows: a workgroup owns LH_SAMPLER_SEG consecutive leaves of one row (4 per lane) and writes the leaf
//                    level and the 10 levels above it, down to one node per segment; a second launch on the same stream, one
//                    workgroup per row, forms the P / LH_SAMPLER_SEG - 1 nodes above those and slot 0
#ifndef LASER_HIP_SAMPLER_PLAN_H
#define LASER_HIP_SAMPLER_PLAN_H

#define LH_SAMPLER_MAX_N (1ll << 24)      // LASER_HIP_SAMPLER_MAX_N
#define LH_SAMPLER_SEG 1024               // leaves of one segment: 256 lanes x 4
#define LH_SAMPLER_SMALL_P 512            // rows of at most this many leaves are built whole, in LDS
#define LH_SAMPLER_SMALL_LEAVES 1024      // leaves of the rows one workgroup of the LDS kernel owns (2048 floats of LDS)
#define LH_SAMPLER_MAX_WORKGROUPS 16384   // both launches walk their units with a grid-sized stride past this

// P and log2(P) for 1 <= n <= 2^24
static inline long long lh_sampler_leaves(const long long n, int *log2p) {
  long long p = 1;
  int l = 0;
  while (p < n) {
    p *= 2;
    l++;
  }
  if (log2p) *log2p = l;
  return p;
}

// 2 P, or -1 for n outside 1 .. 2^24
static inline int lh_sampler_tree_elems(const long long n, long long *elems) {
  if (n < 1 || n > LH_SAMPLER_MAX_N) return -1;
  *elems = 2 * lh_sampler_leaves(n, 0);
  return 0;
}

// out4 = {kernel code, leaves a workgroup owns in one step, workgroups of the first launch, workgroups of the second launch
// (0: there is none)}.  Returns 0, or -1 for a shape the entry point refuses (rows < 0, n outside 1 .. 2^24).
static inline int lh_sampler_plan(const long long rows, const long long n, long long *out4) {
  if (rows < 0 || n < 1 || n > LH_SAMPLER_MAX_N) return -1;
  const long long cap = LH_SAMPLER_MAX_WORKGROUPS;
  const long long p = lh_sampler_leaves(n, 0);
  if (p <= LH_SAMPLER_SMALL_P) {
    const long long per = LH_SAMPLER_SMALL_LEAVES / p;  // rows of one workgroup
    const long long want = rows / per + (rows % per != 0);
    out4[0] = 0;
    out4[1] = LH_SAMPLER_SMALL_LEAVES;
    out4[2] = want < cap ? want : cap;
    out4[3] = 0;
    return 0;
  }
  const long long segs = p / LH_SAMPLER_SEG;  // at most 2^14
  // min(rows * segs, cap) without forming a product that could overflow
  long long groups = cap;
  if (rows < cap && rows * segs < cap) groups = rows * segs;
  out4[0] = 1;
  out4[1] = LH_SAMPLER_SEG;
  out4[2] = groups;
  out4[3] = rows < cap ? rows : cap;
  return 0;
}

#endif  // LASER_HIP_SAMPLER_PLAN_H
