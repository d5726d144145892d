/* include/laser_hip_select.h -- row selection: a section of the C-ABI of liblaser_hip.so in a header of its own.
 *
 * The entry points below are exported by the same liblaser_hip.so and follow every convention of include/laser_hip.h (return
 * codes, laser_hip_last_error, element strides, `_dev` = device pointers, asynchronous on `stream`).  They are declared here,
 * and not in laser_hip.h, because the stream-order case table (tests/stream_order.py) pins the set of `_dev` declarations of
 * that header; their stream-order rows are in tests/test_gpu_select_stream_order.py.  Folding this header into laser_hip.h
 * and its rows into that table is left to a change that may edit the table.  laser_hip.h does not include this header;
 * laser.hpp does.
 *
 * ---- Row top-k, argmax and top-k sampling (f32): selection with a fully defined order ------------------------------------------
 * For every row of a float32 matrix: the k largest (or smallest) elements with their column indices.  Only integer
 * comparisons of bit patterns are involved, so every bit and every index of the result is defined.
 * The order.  For a float32 x with the bits b,
 *     key(x) = b ^ 0xFFFFFFFF   when the sign bit of b is set
 *              b ^ 0x80000000   otherwise
 *   Read as unsigned integers the keys ascend through: NaNs with the sign bit set, -Inf, the negative numbers, -0, +0, the
 *   positive numbers, +Inf, and last the NaNs with the sign bit clear.
 *   largest = 1 ranks the elements of a row by descending key; elements with the same key (identical bits) rank by ascending
 *   column index.  largest = 0 ranks by ascending key, with the same tie rule.  Output position 0 holds rank 0.
 * Consequences: a positive NaN is the largest element of its row and a negative NaN the smallest; -0 ranks below +0; the
 *   result is a function of the row's bits, k and `largest` alone: never of the grid, the stream, the base alignment, the
 *   strides or the lane mapping; what is asked for (values, indices or both) has the same bits whatever else is asked for.
 * laser_hip_topk_rows_f32_dev: row r of the source is the n contiguous floats at d_src + r * src_row_stride; for rank
 *   i < k, d_vals[r * vals_row_stride + i] receives the element (a bit copy: NaN payloads and -0 survive) and
 *   d_idx[r * idx_row_stride + i] its column.  Either output may be NULL (not wanted), but not both.
 *   Valid: 0 <= rows <= LASER_HIP_SELECT_MAX_ROWS (2^26), 1 <= n <= LASER_HIP_SELECT_MAX_N (2^24),
 *   1 <= k <= min(n, LASER_HIP_SELECT_MAX_K) (1024), largest 0 or 1, any base alignment.  Row strides must be at least the
 *   row length (n for the source, k for an output), except that the stride of a lone row is never applied.  The outputs may
 *   not overlap the source.  rows = 0 does nothing and returns 0.  Anything else -- a size past its limit, a short stride, a
 *   NULL source, both outputs NULL, an overlap -- gives LASER_HIP_E_INVALID with a text that names the limit, decided before
 *   a device is looked for.
 * laser_hip_argmax_rows_f32_dev: d_idx[r * idx_stride] = the column of rank 0 of row r and, unless d_val is NULL,
 *   d_val[r * val_stride] = that element: the bits of top-k with k = 1, from a single pass over the row (one maximum over the
 *   composite below; no histogram, no sort).  largest = 0 is argmin.  The same limits; strides >= 1.
 * laser_hip_take_rows_i32_dev: out[r, c] = src[r, j[r, c]] for c < num, and -1 where j[r, c] is outside [0, m): row r of
 *   src has m int32, rows r of j and out have num.  The last link of top-k sampling: it maps a draw among the k candidates
 *   back to a vocabulary id.  Valid: 0 <= rows <= 2^26, 1 <= m <= 2^24, 0 <= num <= 2^24, row strides as above; out may not
 *   overlap src or j.
 * Top-k sampling is a composition (laser_amd.sample_top_k, laser::sample_top_k): top-k values and indices, "Softmax" of the k
 *   values, "Row cumsum" of the probabilities, the inverse-CDF draw, then laser_hip_take_rows_i32_dev on the indices.  Every
 *   step has defined bits, so the drawn ids are a function of the logits and the uniform numbers alone.
 * Kernels (laser_amd/csrc/select.hip).  composite = key << 32 | (0xFFFFFFFF - column), with the key complemented on load for
 *   largest = 0: unique within a row, and descending composites are the order above.  Three lane mappings chosen by n alone,
 *   as the other row kernels have them, each with a 16-byte-vector instance (source base 16-byte aligned, source row stride
 *   a multiple of 4) and a single-element one: same bits.  At most 2048 workgroups, which stride over the rows.
 *     n <= 256    one wave per row, four rows per workgroup: the row's composites are sorted whole (a bitonic network on
 *                 the next power of two >= n in LDS; at this length cheaper than a selection)
 *     n <= 8192   one workgroup per row; the row is loaded once, 32 keys per lane, and every pass runs from registers
 *     n <= 2^24   one workgroup re-reads the row from global memory for each pass.  A row is read at most FIVE times:
 *                 four digit passes and one collection pass.
 *   The selection of the two workgroup mappings: four passes over 8-bit digits, most significant first.  A pass counts the
 *   keys that match the digits found so far in 256 integer bins in LDS and scans the bins from the top to the digit at which
 *   the running count reaches what is still needed.  Then the threshold key T and the number g of keys above it are known.
 *   The collection pass takes every key above T and, of the keys equal to T, the k - g with the LOWEST columns: the row is
 *   visited in column order with a prefix count, so the tie pick is positional.  The k composites are sorted by a bitonic
 *   network on the next power of two >= k in LDS.  No floating-point operation or atomic anywhere; the bin counts are
 *   integers, so the arrival order of the adds cannot show.
 * laser_hip_topk_plan: what laser_hip_topk_rows_f32_dev would launch, without a device.  out3 = {kernel code, workgroups,
 *   LDS bytes of a workgroup}.  Codes 0 / 1 / 2 = the three mappings above, + 4 for the single-element instance (vec = 0);
 *   workgroups = min(2048, ceil(rows / 4)) for code 0 and min(2048, rows) otherwise.  LASER_HIP_E_INVALID past the limits of
 *   rows, n and k.  The logic is laser_amd/csrc/select_plan.h, which has no HIP dependency.  argmax takes the mapping and the
 *   grid of k = 1.
 * laser_hip_topk_last_kernel(): the plan's kernel code of the last top-k launch in this process, that code + 8 after an
 *   argmax launch; -1 = none yet.  (A function of its own: the option table is a recorded set.)
 * Not built: float64 and integer keys; k > 1024; a full row sort; top-p (nucleus) filtering; selection along an axis other
 *   than the last; one very long row split over several workgroups (few rows x long n keeps few compute units busy).
 * No gfx950 device: LASER_HIP_E_NODEVICE. */
#ifndef LASER_HIP_SELECT_H
#define LASER_HIP_SELECT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LASER_HIP_SELECT_MAX_N (1ll << 24)
#define LASER_HIP_SELECT_MAX_ROWS (1ll << 26)
#define LASER_HIP_SELECT_MAX_K 1024
int laser_hip_topk_rows_f32_dev(float *d_vals, int64_t vals_row_stride, int32_t *d_idx, int64_t idx_row_stride, const float *d_src,
                                int64_t src_row_stride, int64_t rows, int64_t n, int64_t k, int largest, void *stream);
int laser_hip_argmax_rows_f32_dev(int32_t *d_idx, int64_t idx_stride, float *d_val, int64_t val_stride, const float *d_src,
                                  int64_t src_row_stride, int64_t rows, int64_t n, int largest, void *stream);
int laser_hip_take_rows_i32_dev(int32_t *d_out, int64_t out_row_stride, const int32_t *d_src, int64_t src_row_stride,
                                const int32_t *d_j, int64_t j_row_stride, int64_t rows, int64_t m, int64_t num, void *stream);
int laser_hip_topk_plan(int64_t rows, int64_t n, int64_t k, int vec, int64_t *out3);
int laser_hip_topk_last_kernel(void);

#ifdef __cplusplus
}
#endif
#endif /* LASER_HIP_SELECT_H */
