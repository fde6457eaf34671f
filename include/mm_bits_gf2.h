/* mm_bits_gf2.h -- the product over the field GF(2) on the bit-packed format of mm_gemm.h (mm_bits_*).
 *
 * Part of libmm_gemm_amd.so's C ABI and included by mm_gemm.h, so a client includes that header as before.  The call has a
 * header of its own, and the Python binding lists its symbols in BITS_GF2_EXPORTS beside EXPORTS: mm_gemm.h's declarations
 * and EXPORTS are pinned symbol for symbol by the prototype table of tests/test_binding_calls.py.  Status codes, the storage
 * format, mm_last_error() and the tuning knobs are mm_gemm.h's. */
#ifndef MM_BITS_GF2_H
#define MM_BITS_GF2_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Product over the field GF(2): C[e,i,j] = XOR_k (A[e,i,k] AND B[e,k,j]), packed in and packed out -- encoding and syndromes
 * of linear codes, parity checks, the inner product of GF(2) elimination.  Storage format, operand layout and argument rules
 * are exactly those of mm_bits_gemm_*: a is N x K packed along K, b is K x M packed along M, c is N x M packed along M; ld and
 * batch strides in words, a stride of 0 one operand shared by the batch; with batch > 1, stride_c >= (N - 1) ldc +
 * ceil(M / 32).  accumulate != 0: C <- C ^ A B (the valid bits of C's input take part, its padding bits are dropped), so
 * applying the same product twice restores C.  Padding bits of a and b are ignored WHATEVER THEY HOLD -- over XOR a stray
 * bit would flip results, so A's bits at k >= K in its last word and B's padding columns are dead, and rows of b at k >= K
 * are never read -- and the padding bits of c are written 0.  Words of a row beyond its word count, and the space between
 * batch elements, are never read or written.  batch, N or M 0: MM_OK, nothing done (_launch reports 0 s); so is K = 0 when
 * accumulating; K = 0 in the plain form writes C = 0, the empty sum (a and b are then not read and may be null).  Refused
 * with MM_ERR_BAD_ARGUMENT before any device is touched, with the statuses and texts of mm_bits_gemm_*: a null pointer, an ld
 * below its row's word count, outputs of the batch that would overlap, a span of C that overlaps A's or B's.
 * The result is exact arithmetic in a field: the same bits on every kernel, batch position and chunking.
 * Kernels (mm_kernel_name_bits_gf2; pure arithmetic, the launcher's own resolver):
 *   "bits_gf2_tile"   the Method of the Four Russians: 128 rows x 128 words of C per workgroup of 512 threads (8 wavefronts x
 *                     16 rows, 2 words per lane), K streamed in slabs of 32.  Per slab the workgroup builds, for each of the
 *                     8 groups of 4 consecutive k, the 16 XOR combinations of those 4 rows of B in LDS (64 KiB, Gray-code
 *                     order: one XOR per entry); a row of C then takes ONE 8-byte LDS read and two XORs per 4 k, the entry
 *                     chosen by a nibble of A's word.  The time does not depend on the data.  Serves N >= 128 and M >= 128
 *                     (the smallest shape of profiles/bits_gf2_sweep_mi355x.txt, swept at K = 4096: faster than
 *                     bits_gf2_plain there and at every larger shape) with ldb % 2 == 0 and ldc % 2 == 0 (8-byte loads of
 *                     B, 8-byte loads and stores of C).
 *   "bits_gf2_plain"  the mask loop of "bits_plain" with ^= for |=, 64 rows x 64 words, one-word accesses: every shape, every
 *                     ld, any 4-byte aligned pointer.  It skips the k no row of a wavefront has set (they contribute
 *                     nothing), so its time depends on the data, the result does not.
 * Knob "bits_gf2_variant" (MM_BITS_GF2_VARIANT): -1 the rule above, 0 bits_gf2_plain always, 1 bits_gf2_tile wherever its ld
 * rule holds, whatever the shape; any other value: MM_ERR_BAD_ARGUMENT ("invalid" as a name).  The name is decided by shape
 * and ld alone: a bits_gf2_tile launch whose b or c is not 8-byte aligned -- base, or an odd batch
 * stride -- runs bits_gf2_plain instead, the same bits, no error.  The batch is launched in chunks (knob "batch_chunk").
 * _enqueue / _launch as for mm_bits_gemm_*. */
int mm_bits_gf2_enqueue(void *hip_stream, const void *a_dev, const void *b_dev, void *c_dev, unsigned size_n, unsigned size_k,
                        unsigned size_m, size_t lda, size_t ldb, size_t ldc, unsigned batch, size_t stride_a,
                        size_t stride_b, size_t stride_c, int accumulate);
int mm_bits_gf2_launch(int device, const void *a_dev, const void *b_dev, void *c_dev, unsigned size_n, unsigned size_k,
                       unsigned size_m, size_t lda, size_t ldb, size_t ldc, unsigned batch, size_t stride_a,
                       size_t stride_b, size_t stride_c, int accumulate, double *elapsed_seconds);
const char *mm_kernel_name_bits_gf2(unsigned size_n, unsigned size_k, unsigned size_m, size_t lda, size_t ldb, size_t ldc,
                                    unsigned batch);


#ifdef __cplusplus
}
#endif
#endif /* MM_BITS_GF2_H */
