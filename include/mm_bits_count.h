/* mm_bits_count.h -- kept for clients that include it by name: the packed counting products (mm_bits_count_*) and the packed
 * transpose (mm_bits_transpose_*) are declared in mm_gemm.h, with the rest of the mm_bits_* family. */
#ifndef MM_BITS_COUNT_H
#define MM_BITS_COUNT_H
#include "mm_gemm.h"
#endif /* MM_BITS_COUNT_H */
