// laser_amd/csrc/random_plan.h -- what a laser_hip_random_*_dev fill launches for a length, an element width and an offset
// (include/laser_hip.h "Random numbers"; the kernels are in random.hip, the generator in philox_core.h).  Plain C++ with no
// includes and no HIP: the library's launcher and a host program read the same functions.
//
// The n elements use the words offset .. offset + n * wpe - 1 of a stream (mod 2^64), wpe = 1 for the 32-bit element types and
// 2 for the 64-bit ones.  One lane computes one Philox block (4 words) per step and stores the elements that START in it:
// four 32-bit elements or two 64-bit ones.  With an odd offset a 64-bit element starts at word 1 or word 3 of a block, and the
// one at word 3 takes its high word from word 0 of the next block, which the same lane computes too (twice the arithmetic; an
// even offset never pays it).  A lane's elements are 16 contiguous bytes:
//   0  vector          every lane's run starts on a 16-byte boundary: one 16-byte store per block (a wave writes 1 KiB), the
//                      blocks only partly inside [0, n) -- the head when offset & 3 != 0, and the tail -- element by element
//   1  single-element  any other destination: the same bits, one store per element
// The grid is capped at LH_RANDOM_WG_PER_CU workgroups of 256 lanes per compute unit (full occupancy: 8 waves per SIMD); past
// that a lane walks several blocks with a grid-sized stride.
#ifndef LASER_HIP_RANDOM_PLAN_H
#define LASER_HIP_RANDOM_PLAN_H

#define LH_RANDOM_MAX_N (1ll << 60)   // LASER_HIP_RANDOM_MAX_N: n * wpe + 3 stays inside 63 bits
#define LH_RANDOM_WG_PER_CU 8
#define LH_RANDOM_DEFAULT_CUS 256     // cus <= 0: the MI355X's count

// the word of its block at which a lane's run of elements starts: 0, or 1 for a 64-bit element type at an odd offset
static inline int lh_random_unit_word(const int words_per_elem, const unsigned long long offset) {
  return words_per_elem == 2 ? (int)(offset & 1) : 0;
}

// 1 when the 16-byte runs of a destination at address `dst` do not start on 16-byte boundaries (the block of the first word
// starts (offset & 3) - unit_word words, of 4 bytes each, before the first element)
static inline int lh_random_dst_misaligned(const unsigned long long dst, const int words_per_elem, const unsigned long long offset) {
  const unsigned long long back = 4ull * ((offset & 3) - (unsigned long long)lh_random_unit_word(words_per_elem, offset));
  return ((dst - back) & 15) != 0;
}

// blocks in which at least one of the n elements starts (n >= 1)
static inline long long lh_random_blocks(const long long n, const int words_per_elem, const unsigned long long offset) {
  const long long last = (long long)(offset & 3) + (long long)words_per_elem * (n - 1);  // the last element's first word
  return (last >> 2) + 1;
}

// out4 = {variant (0 vector, 1 single-element), workgroups, most blocks one lane walks, index of the first block}.
// Returns 0, or -1 for what the entry points refuse (n outside 0 .. 2^60, words_per_elem not 1 or 2).  n = 0 launches nothing.
static inline int lh_random_plan(const long long n, const int words_per_elem, const unsigned long long offset, const int dst_misaligned,
                                 const int cus, long long *out4) {
  if (n < 0 || n > LH_RANDOM_MAX_N || (words_per_elem != 1 && words_per_elem != 2)) return -1;
  const long long cap = (long long)(cus > 0 ? cus : LH_RANDOM_DEFAULT_CUS) * LH_RANDOM_WG_PER_CU;
  out4[0] = dst_misaligned ? 1 : 0;
  out4[3] = (long long)(offset >> 2);
  if (n == 0) {
    out4[1] = 0;
    out4[2] = 0;
    return 0;
  }
  const long long blocks = lh_random_blocks(n, words_per_elem, offset);
  const long long want = (blocks + 255) / 256;
  const long long wgs = want < cap ? want : cap;
  out4[1] = wgs;
  out4[2] = (blocks + wgs * 256 - 1) / (wgs * 256);
  return 0;
}

#endif  // LASER_HIP_RANDOM_PLAN_H
