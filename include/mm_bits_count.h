/* mm_bits_count.h -- counting products on the bit-packed format of mm_gemm.h (mm_bits_*), and the packed transpose.
 *
 * Part of libmm_gemm_amd.so's C ABI and included by mm_gemm.h, so a client includes that header as before.  The family has a
 * header of its own, and the Python binding lists its symbols in BITS_COUNT_EXPORTS beside EXPORTS: mm_gemm.h's declarations
 * and EXPORTS are pinned symbol for symbol by the prototype table of tests/test_binding_calls.py.  Status codes, the storage
 * format, mm_last_error() and the tuning knobs are mm_gemm.h's. */
#ifndef MM_BITS_COUNT_H
#define MM_BITS_COUNT_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Counting products on the packed format, A x B^T: C[e,i,j] = sum_k (A[e,i,k] op Bt[e,j,k]) as int32, op AND (common
 * neighbours, set intersections, binarised dot products) or XOR (Hamming distances) on single bits.  A count over k needs
 * both operands packed along k: a is N x K with lda >= ceil(K / 32) words, bt is M x K with ldbt >= ceil(K / 32) words --
 * sets of row-stored codes as they lie (mm_bits_transpose_* below converts a K x M operand of mm_bits_gemm_*).  c is N x M
 * row-major int32: ldc >= M and stride_c count ELEMENTS; elements of a row beyond M, up to ldc, and the space between batch
 * elements are never written.  Padding bits of a and bt are ignored, whatever they hold -- under XOR too, where a padding
 * bit set in one operand alone must not count -- and words of a row beyond ceil(K / 32) are never read.  accumulate != 0:
 * C += counts, mod 2^32 like the library's integer Add.  stride_a or stride_bt 0 = one operand shared by the batch; with
 * batch > 1, stride_c >= (N - 1) ldc + M.  batch, N or M 0: MM_OK, nothing done (_launch reports 0 s); so is K = 0 when
 * accumulating; K = 0 in the plain form writes C = 0 (a and bt are then not read and may be null).  Refused with
 * MM_ERR_BAD_ARGUMENT before any device is touched: an op outside mm_bits_count_op_t, a null pointer, an ld below its row,
 * outputs of the batch that would overlap, and a span of C in bytes -- [base, base + 4 ((batch - 1) stride + (rows - 1) ld
 * + M)) -- that overlaps A's or Bt's.
 * Kernels (mm_kernel_name_bits_count; pure arithmetic, the launcher's own resolver):
 *   "bits_count_tile"   128 x 128 outputs per workgroup, 8 x 8 int32 accumulators per thread, K streamed through LDS in slabs
 *                       of 8 words (256 k) stored k-major, so a thread's 8 rows of A and 8 rows of Bt are two 16-byte LDS
 *                       reads each per word; per output and word one AND / XOR and one accumulating population count.
 *                       Serves lda % 4 == 0, ldbt % 4 == 0, ldc % 4 == 0 (16-byte loads of A and Bt, 16-byte loads and
 *                       stores of C) from ceil(N / 128) ceil(M / 128) >= 256 tiles, one per compute unit.
 *   "bits_count_plain"  the same loop on 64 x 64 outputs, 4 x 4 per thread, with one-word / one-element accesses: every
 *                       shape, every ld, any 4-byte aligned pointer.
 * Knob "bits_count_variant" (MM_BITS_COUNT_VARIANT): -1 the rule above, 0 bits_count_plain always, 1 bits_count_tile
 * wherever its ld rule holds, whatever the shape; any other value: MM_ERR_BAD_ARGUMENT ("invalid" as a name).  The name is
 * decided by shape and ld alone: a bits_count_tile launch whose a, bt or c is not 16-byte aligned -- base, or a batch stride
 * that is no multiple of 4 -- runs bits_count_plain instead, the same values, no error.  The time does not depend on the
 * data.  The batch is launched in chunks (knob "batch_chunk").  _enqueue / _launch as for mm_bits_gemm_*. */
typedef enum { MM_BITS_COUNT_AND = 0, MM_BITS_COUNT_XOR = 1 } mm_bits_count_op_t;
int mm_bits_count_enqueue(void *hip_stream, int op, const void *a_dev, const void *bt_dev, void *c_dev, unsigned size_n,
                          unsigned size_k, unsigned size_m, size_t lda, size_t ldbt, size_t ldc, unsigned batch,
                          size_t stride_a, size_t stride_bt, size_t stride_c, int accumulate);
int mm_bits_count_launch(int device, int op, const void *a_dev, const void *bt_dev, void *c_dev, unsigned size_n,
                         unsigned size_k, unsigned size_m, size_t lda, size_t ldbt, size_t ldc, unsigned batch,
                         size_t stride_a, size_t stride_bt, size_t stride_c, int accumulate, double *elapsed_seconds);
const char *mm_kernel_name_bits_count(unsigned size_n, unsigned size_k, unsigned size_m, size_t lda, size_t ldbt, size_t ldc,
                                      unsigned batch);

/* Packed transpose: src is rows x cols packed along cols (ld_src >= ceil(cols / 32) words), dst is cols x rows packed along
 * rows (ld_dst >= ceil(rows / 32) words), dst[j, i] = src[i, j]; batch strides in words.  Padding bits of src are ignored,
 * padding bits of dst are written 0, the words of a row beyond its word count are never touched on either side.  One
 * wavefront takes one word from each of 64 consecutive source rows and 32 ballots, one per bit position: two words of 32
 * destination rows.  Refused before any device is touched: a null pointer, an ld below its row, a destination whose rows or
 * batch elements would overlap, and a destination span overlapping the source's -- there is no in-place form
 * (MM_ERR_BAD_ARGUMENT).  rows, cols or batch 0: MM_OK, nothing done. */
int mm_bits_transpose_enqueue(void *hip_stream, const void *src_dev, void *dst_dev, unsigned rows, unsigned cols,
                              size_t ld_src, size_t ld_dst, unsigned batch, size_t stride_src, size_t stride_dst);
int mm_bits_transpose_launch(int device, const void *src_dev, void *dst_dev, unsigned rows, unsigned cols, size_t ld_src,
                             size_t ld_dst, unsigned batch, size_t stride_src, size_t stride_dst, double *elapsed_seconds);

#ifdef __cplusplus
}
#endif
#endif /* MM_BITS_COUNT_H */
