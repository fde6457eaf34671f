// Kernel sources compiled twice (mm_mfma_f64_kernels.inc, mm_mfma_f16_kernels.inc, mm_mfma_i8_kernels.inc,
// mm_mfma_f32_small.inc): with MM_BATCHED 0 they are the single-problem kernels, token for token the source they always
// were (so the same machine code); with MM_BATCHED 1 each kernel becomes its *_batched twin, which takes the batch and
// the element strides and derives (element, tile) from the workgroup id through batched_tile() (mm_common.h).
// MM_SEEDED 1 (with MM_BATCHED 1) compiles a third form, *_batched_seeded: the batched twin whose reduction starts at the
// value C holds (mm_gemm_*accumulate_*); the kernel sources test MM_SEEDED where the seed enters.
// No include guard: every kernel source includes this at its top and #undefs the three macros at its end.
#if MM_BATCHED && MM_SEEDED
#define MM_KNAME(name) name##_batched_seeded
#define MM_BATCH_PARAMS , unsigned batch, size_t stride_a, size_t stride_b, size_t stride_c
#define MM_TILE_LIN(bid, tiles) batched_tile(A, B, C, tiles, batch, stride_a, stride_b, stride_c)
#elif MM_BATCHED
#define MM_KNAME(name) name##_batched
#define MM_BATCH_PARAMS , unsigned batch, size_t stride_a, size_t stride_b, size_t stride_c
#define MM_TILE_LIN(bid, tiles) batched_tile(A, B, C, tiles, batch, stride_a, stride_b, stride_c)
#else
#define MM_KNAME(name) name
#define MM_BATCH_PARAMS
#define MM_TILE_LIN(bid, tiles) xcd_remap(bid, tiles)
#endif
