// laser_amd/csrc/attention_plan.h -- what laser_hip_attention_f32_dev launches for a shape (include/laser_hip.h "Attention";
// the kernel is in attention.hip).  Plain C++ with no includes and no HIP: the library's launcher and a host program read the
// same function.
//
// One kernel form, the streaming one: a workgroup of 256 lanes owns LH_ATTENTION_BM query rows of one (batch, head) slice and
// sweeps the keys three times in tiles of LH_ATTENTION_BN (attention.hip says how).  No resident form is built.
//   kernel code 0   the vector instance: Q and K rows are fetched 16 bytes at a time (every base of Q and K 16-byte aligned,
//                   every stride of theirs a multiple of 4 elements)
//   kernel code 1   the single-element instance: any base, any stride.  Same values, same order, same bits.
// The units are the B*H*ceil(Tq / BM) query blocks; at most LH_ATTENTION_MAX_WORKGROUPS workgroups stride over them.
// LDS: the lexp table, the Q block, one K tile, one P tile and the fold scratch; rows of Q and K are padded to an odd
// number of words so that the 32 rows an MFMA operand reads lie in 32 banks.
#ifndef LASER_HIP_ATTENTION_PLAN_H
#define LASER_HIP_ATTENTION_PLAN_H

#define LH_ATTENTION_MAX_D 128          // LASER_HIP_ATTENTION_MAX_D: one 32-column block of O per wave
#define LH_ATTENTION_MAX_KEYS 65536     // LASER_HIP_ATTENTION_MAX_KEYS: 8 chunks of the reduction order
#define LH_ATTENTION_MAX_UNITS (1ll << 40)
#define LH_ATTENTION_BM 32              // query rows of a workgroup: one row block of the 32x32x2 MFMA
#define LH_ATTENTION_BN 128             // keys of a tile: 32 per wave
#define LH_ATTENTION_CHUNK 8192         // one chunk of the order: LH_REDUCE_STEPS x LH_REDUCE_LANES x 4
#define LH_ATTENTION_MAX_CHUNKS (LH_ATTENTION_MAX_KEYS / LH_ATTENTION_CHUNK)
#define LH_ATTENTION_MAX_WORKGROUPS 1024
#define LH_ATTENTION_LDS_LUT 4096       // the lexp table
#define LH_ATTENTION_P_LD (LH_ATTENTION_BN + 1)
// words of scratch: the waves' row maxima (4 x BM), the wave folds of a chunk (BM x 4 x 8), the chunk partials
// (BM x MAX_CHUNKS), the rows' maxima and sums (2 x BM)
#define LH_ATTENTION_LDS_RED_WORDS (4 * LH_ATTENTION_BM + LH_ATTENTION_BM * 32 + LH_ATTENTION_BM * LH_ATTENTION_MAX_CHUNKS + 2 * LH_ATTENTION_BM)

// words of a Q or K row in LDS: d rounded up to the MFMA's k step of 2, then to an odd number
static inline int lh_attention_ld(const long long d) { return (int)((d + (d & 1)) | 1); }

// out5 = {BM, kernel code, workgroups, LDS bytes, units}.  Returns 0, or -1 with nothing written for what the entry point
// refuses: bh < 0, tq < 0, tk outside 1..MAX_KEYS, d or dv outside 1..MAX_D, causal with tq > tk, more than 2^40 units.
// bh = 0 or tq = 0 plans no workgroup.
static inline int lh_attention_plan(const long long bh, const long long tq, const long long tk, const long long d, const long long dv,
                                    const int causal, const int vec, long long *out5) {
  if (bh < 0 || tq < 0 || tk < 1 || tk > LH_ATTENTION_MAX_KEYS || d < 1 || d > LH_ATTENTION_MAX_D || dv < 1 || dv > LH_ATTENTION_MAX_D)
    return -1;
  if (causal && tq > tk) return -1;
  const long long qblocks = tq / LH_ATTENTION_BM + (tq % LH_ATTENTION_BM != 0);
  if (bh != 0 && qblocks > LH_ATTENTION_MAX_UNITS / bh) return -1;
  const long long units = bh * qblocks;
  const long long cap = LH_ATTENTION_MAX_WORKGROUPS;
  const long long ld = lh_attention_ld(d);
  out5[0] = LH_ATTENTION_BM;
  out5[1] = vec ? 0 : 1;
  out5[2] = units < cap ? units : cap;
  out5[3] = LH_ATTENTION_LDS_LUT +
            4 * ((LH_ATTENTION_BM + LH_ATTENTION_BN) * ld + LH_ATTENTION_BM * LH_ATTENTION_P_LD + LH_ATTENTION_LDS_RED_WORDS);
  out5[4] = units;
  return 0;
}

#endif  // LASER_HIP_ATTENTION_PLAN_H
