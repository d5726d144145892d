// laser_amd/csrc/bias_grad_plan.h -- what laser_hip_bias_grad_f32_dev launches for a shape (include/laser_hip.h "Dense-layer
// backward"; the kernel is in dense_grad.hip).  Plain C++ with no includes and no HIP: the library's launcher and a host
// program read the same function.
//
// The operand is (rows, n) with unit column stride; db[j] is the sum down column j in the order of "Reductions" applied to
// that column as a 1-D array of `rows` float32 (E = 4, init +0).  A workgroup of 256 lanes owns one unit: a chunk of
// LH_BIAS_GRAD_CHUNK = 8192 rows (one chunk of the order) by a strip of LH_BIAS_GRAD_CW = 16 columns (64 contiguous bytes
// per row: 4 lanes of 4 columns span a strip row, 64 row lanes walk down it).  Unit u is chunk u / strips, strip u % strips,
// so neighbouring workgroups read neighbouring 64-byte runs.  The grid is min(2048, units); workgroups stride over the units.
//   rows <= 8192   one launch: the one chunk's partial is the result, written to db
//   longer         two launches: the chunk partials P[c, j] go to a row-major (chunks, n) scratch matrix, and the same
//                  kernel (no activation, no dz) folds P with rows = chunks.  rows <= 2^26 keeps chunks <= 8192, one chunk.
// Kernel codes: 0 = the vector instance (16-byte accesses wherever 4 columns lie inside n), 1 = single elements.
#ifndef LASER_HIP_BIAS_GRAD_PLAN_H
#define LASER_HIP_BIAS_GRAD_PLAN_H

#define LH_BIAS_GRAD_CW 16                  // strip width in columns
#define LH_BIAS_GRAD_CHUNK 8192             // rows of one chunk of the order: LH_REDUCE_STEPS * LH_REDUCE_LANES * 4
#define LH_BIAS_GRAD_MAX_ROWS (1ll << 26)   // LASER_HIP_BIAS_GRAD_MAX_ROWS: 8192 chunks, whose partials are one chunk
#define LH_BIAS_GRAD_MAX_WORKGROUPS 2048

// out4 = {kernel code of the first launch, workgroups of the first launch, launches, scratch floats}.  `vec`: bases and row
// strides allow 16-byte vectors; `cus` (compute units of the device) is taken for symmetry with laser_hip_plan_f32 and does
// not change the plan.  n == 0: nothing is launched, {code, 0, 0, 0}.  Returns 0, or -1 for a shape the entry point refuses
// (rows < 0, rows > 2^26, n < 0, or a scratch matrix whose size in bytes does not fit 63 bits).
static inline int lh_bias_grad_plan(const long long rows, const long long n, const int vec, const int cus, long long *out4) {
  if (rows < 0 || rows > LH_BIAS_GRAD_MAX_ROWS || n < 0) return -1;
  (void)cus;
  const long long cap = LH_BIAS_GRAD_MAX_WORKGROUPS;
  // rows == 0 is one (empty) chunk: its partial is the order's init, +0
  const long long chunks = rows == 0 ? 1 : rows / LH_BIAS_GRAD_CHUNK + (rows % LH_BIAS_GRAD_CHUNK != 0);
  if (chunks > 1 && n > (1ll << 60) / chunks) return -1;
  const long long strips = n / LH_BIAS_GRAD_CW + (n % LH_BIAS_GRAD_CW != 0);
  // min(chunks * strips, cap) without forming a product that could overflow
  long long groups = cap;
  if (strips < cap && chunks * strips < cap) groups = chunks * strips;  // (chunks <= 8192)
  out4[0] = vec ? 0 : 1;
  out4[1] = groups;
  out4[2] = n == 0 ? 0 : chunks > 1 ? 2 : 1;
  out4[3] = chunks > 1 ? chunks * n : 0;
  return 0;
}

#endif  // LASER_HIP_BIAS_GRAD_PLAN_H
