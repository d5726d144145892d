// laser_amd/csrc/embedding_plan.h -- what laser_hip_embedding_group_i32_dev and laser_hip_embedding_grad_f32_dev launch for a
// shape (include/laser_hip.h "Embedding"; the kernels are in embedding.hip).  Plain C++ with no includes and no HIP: the
// library's launchers and a host program read the same function.
//
// Grouping: a stable least-significant-digit radix sort of the token positions by key (the id, or `vocab` for every id
// outside [0, vocab)), LH_EMBEDDING_DIGIT_BITS = 8 bits per pass.  The largest key is `vocab`, so the sort takes
//   passes = max(1, ceil(bit_length(vocab) / 8))          vocab <= 255: 1, <= 65535: 2, <= 2^24 - 1: 3, <= 2^30: 4
// A wave of 64 lanes owns a tile of `tile` consecutive sort positions; tile is the smallest power of two >= 512 that keeps
// the (digit, tile) table at or below 2^22 counters (the row cumsum takes rows of up to 2^24), at most 4096 for 2^26 tokens.
// A workgroup is four waves.  A pass is three launches (per-tile digit histograms, one row cumsum of the table, the stable
// scatter); one more launch finds `starts` in the sorted keys by a lower-bound descent per id.  tokens = 0: that one alone.
//
// Gradient: two launches whenever dW has an element (vocab > 0 and dim > 0), whatever the ids are (the host never sees
// them): the short-segment kernel (a lane per id and four columns; ids of at most LH_EMBEDDING_SHORT occurrences, the
// empty ones included) and the long-segment kernel (a workgroup per long id and strip of LH_EMBEDDING_CW columns, chunks of
// LH_EMBEDDING_CHUNK gathered rows, the chunk partials folded in the same workgroup).  Kernel codes of the sums: 0 = the
// vector instances (16-byte accesses wherever 4 columns lie inside dim), 1 = single elements.
#ifndef LASER_HIP_EMBEDDING_PLAN_H
#define LASER_HIP_EMBEDDING_PLAN_H

#define LH_EMBEDDING_MAX_TOKENS (1ll << 26)  // LASER_HIP_EMBEDDING_MAX_TOKENS: positions fit int32, chunk partials one chunk
#define LH_EMBEDDING_MAX_VOCAB (1ll << 30)   // LASER_HIP_EMBEDDING_MAX_VOCAB: the key `vocab` fits int32 with room to spare
#define LH_EMBEDDING_DIGIT_BITS 8
#define LH_EMBEDDING_MIN_TILE 512            // sort positions of one wave, at least
#define LH_EMBEDDING_MAX_TILES (1ll << 14)   // tiles of one pass, at most: 256 counters each, a table of 2^22
#define LH_EMBEDDING_SHORT 32                // the longest segment of the short-segment kernel: 8 groups of 4 leaves
#define LH_EMBEDDING_CW 16                   // strip width of the long-segment kernel, as the bias gradient's
#define LH_EMBEDDING_CHUNK 8192              // one chunk of the order: LH_REDUCE_STEPS * LH_REDUCE_LANES * 4
#define LH_EMBEDDING_PTILE 4096              // sorted positions one long-segment workgroup searches for segment starts

// out8 = {sort passes, sort positions of one wave's tile, workgroups of a pass, kernel code of the sums, launches of the
// grouping, launches of the gradient with a group given, scratch bytes of the grouping, scratch bytes of the gradient that
// groups by itself (order and starts on top of the grouping's)}.  `vec`: bases and row strides of dW and dY allow 16-byte
// vectors; `cus` (compute units of the device) is taken for symmetry with laser_hip_plan_f32 and does not change the plan.
// Returns 0, or -1 with nothing written for a shape the entry points refuse.
static inline int lh_embedding_plan(const long long tokens, const long long vocab, const long long dim, const int vec, const int cus,
                                    long long *out8) {
  if (tokens < 0 || tokens > LH_EMBEDDING_MAX_TOKENS || vocab < 0 || vocab > LH_EMBEDDING_MAX_VOCAB || dim < 0) return -1;
  (void)cus;
  int bits = 0;
  while (bits < 31 && (vocab >> bits) != 0) bits++;
  long long passes = (bits + LH_EMBEDDING_DIGIT_BITS - 1) / LH_EMBEDDING_DIGIT_BITS;
  if (passes < 1) passes = 1;
  long long tile = LH_EMBEDDING_MIN_TILE;
  while (tokens / tile + (tokens % tile != 0) > LH_EMBEDDING_MAX_TILES) tile *= 2;
  const long long tiles = tokens / tile + (tokens % tile != 0);
  out8[0] = passes;
  out8[1] = tile;
  out8[2] = tiles / 4 + (tiles % 4 != 0);
  out8[3] = vec ? 0 : 1;
  out8[4] = tokens == 0 ? 1 : 3 * passes + 1;
  out8[5] = vocab > 0 && dim > 0 ? 2 : 0;
  // two tables of 256 counters per tile, and the second order buffer of a sort of two passes or more
  out8[6] = tokens == 0 ? 0 : 2 * 256 * tiles * 4 + (passes > 1 ? tokens * 4 : 0);
  out8[7] = out8[5] == 0 ? 0 : out8[6] + tokens * 4 + (vocab + 1) * 4;
  return 0;
}

#endif  // LASER_HIP_EMBEDDING_PLAN_H
