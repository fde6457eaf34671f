// Register-tiled VALU kernel for every semiring the matrix cores cannot serve: (Add, Min) distance
// products, integer types, max/min algebras.  This is the reference's generic
// OperatorMap/OperatorReduce ProcessingElement (kernel/Compute.cpp:120-139) on gfx950:
//   * 128 x 128 outputs per 256-thread workgroup, 8 x 8 per thread held in registers for the
//     whole K loop (the reference's "T^2 fast memory", kernel/Compute.cpp:25-27);
//   * A and B k-slabs (BK = 16) staged through LDS k-major, so one k-step is two 4-element
//     vector reads of A (rows are wave-broadcast) and two of B (16 lanes = 256 contiguous bytes);
//   * every output sees k ascending with a single accumulator: integer, min and max algebras are
//     therefore bit-identical to Naive (include/Utility.h:18-42), and so is float (Add, Min/Max)
//     (an IEEE add is the same value fused or not);
//   * the inner loop takes two k per trip so that float min/max reductions compile to
//     v_min3_f32 / v_max3_f32 (acc, s0, s1): 3 VALU instructions per 2 map-reduce steps.
// Included once per element-type group (mm_valu_tile_*.hip) to keep compile units parallel.
// Requirements of this fast path: K % 4 == 0, M % 4 == 0 (and N % 4 == 0 for a K x N A);
// anything else is served by the predicated ordered kernel.
#include "mm_common.h"

namespace mm {
namespace {

constexpr int VT_BM = 128, VT_BN = 128, VT_BK = 16, VT_PAD = 4;

template <typename T> struct alignas(4 * sizeof(T)) Vec4 { T v[4]; };

// MM_VT_EXACT (mm_valu_tile_fp_exact.hip, compiled with -ffp-contract=off): the SAME kernels as the k-ordered contract of
// MM_PATH_ORDERED wants them -- every operator exactly Op<> (std::min / std::max to the letter, NaN and signed-zero ties
// included), multiply and add two separately rounded instructions (v_pk_mul_f16 + v_pk_add_f16, binary16 accumulating in
// binary16; v_pk_mul_f32 + v_pk_add_f32; v_mul_f64 + v_add_f64), k ascending with one accumulator: bit-identical to Naive
// (include/Utility.h:18-42) and to mm_ordered.hip for every floating-point (map, reduce) pair, at register-tile speed.
#ifdef MM_VT_EXACT
template <int OP, typename T> struct FastOp : Op<OP, T> {};
#else
// Floating-point Min/Max in this fast path use the hardware minNum/maxNum (v_min_f32, v_min3_f32,
// v_min_f64, v_min_f16 ...) instead of std::min's compare-and-select: same value for every pair of
// numbers; they differ only when a NaN is involved (minNum drops it) or for (+0, -0) ties.  The
// ordered kernel keeps std::min/std::max semantics to the letter.
template <int OP, typename T> struct FastOp : Op<OP, T> {};
template <> struct FastOp<MM_OP_MIN, float> : Op<MM_OP_MIN, float> {
  __device__ static __forceinline__ float apply(float a, float b) { return __builtin_fminf(a, b); }
};
template <> struct FastOp<MM_OP_MAX, float> : Op<MM_OP_MAX, float> {
  __device__ static __forceinline__ float apply(float a, float b) { return __builtin_fmaxf(a, b); }
};
template <> struct FastOp<MM_OP_MIN, double> : Op<MM_OP_MIN, double> {
  __device__ static __forceinline__ double apply(double a, double b) { return __builtin_fmin(a, b); }
};
template <> struct FastOp<MM_OP_MAX, double> : Op<MM_OP_MAX, double> {
  __device__ static __forceinline__ double apply(double a, double b) { return __builtin_fmax(a, b); }
};
template <> struct FastOp<MM_OP_MIN, half_t> : Op<MM_OP_MIN, half_t> {
  __device__ static __forceinline__ half_t apply(half_t a, half_t b) { return __builtin_fminf16(a, b); }
};
template <> struct FastOp<MM_OP_MAX, half_t> : Op<MM_OP_MAX, half_t> {
  __device__ static __forceinline__ half_t apply(half_t a, half_t b) { return __builtin_fmaxf16(a, b); }
};
#endif


template <typename T, int MAP, int RED, bool AT>
__global__ __launch_bounds__(256) void valu_tile_kernel(const T *__restrict__ A, const T *__restrict__ B,
                                                        T *__restrict__ C, unsigned N, unsigned K, unsigned M,
                                                        unsigned tiles_n, unsigned tiles_m, unsigned kBand) {
#define MM_VT_BATCHED 0
#include "mm_valu_tile_body.inc"
#undef MM_VT_BATCHED
}

template <typename T, int MAP, int RED, bool AT>
__global__ __launch_bounds__(256) void valu_tile_batched_kernel(const T *__restrict__ A, const T *__restrict__ B,
                                                        T *__restrict__ C, unsigned N, unsigned K, unsigned M,
                                                        unsigned tiles_n, unsigned tiles_m, unsigned kBand,
    unsigned batch, size_t stride_a, size_t stride_b, size_t stride_c) {
#define MM_VT_BATCHED 1
#include "mm_valu_tile_body.inc"
#undef MM_VT_BATCHED
}

// accumulate (Problem::seed): valu_tile_batched_kernel with the acc tile loaded from C instead of set to identity()
template <typename T, int MAP, int RED, bool AT>
__global__ __launch_bounds__(256) void valu_tile_batched_seeded_kernel(const T *__restrict__ A, const T *__restrict__ B,
                                                        T *__restrict__ C, unsigned N, unsigned K, unsigned M,
                                                        unsigned tiles_n, unsigned tiles_m, unsigned kBand,
    unsigned batch, size_t stride_a, size_t stride_b, size_t stride_c) {
#define MM_VT_BATCHED 1
#define MM_VT_SEEDED 1
#include "mm_valu_tile_body.inc"
#undef MM_VT_SEEDED
#undef MM_VT_BATCHED
}

// -------------------------------------------------------------------------------------------------
// DMA-staged variant, row-major A (round 2 for the 4-byte types, round 3 for every element size).  The kernel above
// stages synchronously (global load -> LDS store -> barrier -> compute -> barrier: SQ_WAIT_ANY 32 % of the wave
// cycles); here both slabs are written by LDS-DMA (global_load_lds_dwordx4: no staging registers, no ds_write, no
// scatter), double-buffered, the next slab in flight under the current slab's VALU instructions, ONE barrier per slab.
// The slab depth follows the element size so that the BYTE geometry is the same for every type -- BK = 64 / sizeof(T)
// (16 for float / int, 8 for double / long, 32 for half / short, 64 for bytes):
//   A slab [128 rows][BK k] row-major = 64-byte rows (16-B chunk index ^ (row>>2)&3 on the DMA source so that the four
//     rows a wave reads at once fall into different slots); a thread reads its 8 rows' (k, k+1) pairs in one LDS read;
//   B slab [BK k][128 cols] exactly as in memory (8 KiB); a thread's 2 x 4 columns per k-step as vector reads.
// Per output the operation sequence is unchanged (k ascending, one accumulator): bit-identical to the kernel above and to
// Naive for the order-independent semirings it serves -- the reference's ProcessingElement runs ANY Data_t at full rate
// (kernel/Compute.cpp:120-139), and now so does this family.
// A partial last slab (K % BK != 0) is fetched as the LAST BK k of the matrix and consumed from the offset where the
// new k begin, so no address is ever clamped per lane.  Needs K >= BK, and K, M multiples of the 16-byte chunk.
constexpr int VTD_A_BYTES = VT_BM * 64, VTD_SLAB = 2 * VTD_A_BYTES;  // 8 KiB + 8 KiB

#define MM_DMA_PIECE(vo, sb, la) "s_mov_b32 m0, " la "\n\ts_nop 0\n\tglobal_load_lds_dwordx4 " vo ", " sb "\n\t"
// TI = output rows per thread.  8 (every type up to 4 bytes): 256 threads x (8 x 8) outputs.  4 (round 4, the 8-byte
// types): 512 threads x (4 x 8) outputs over the same 128 x 128 tile, slabs and DMA pieces -- 64 accumulator registers
// instead of 128, so two workgroups = 4 wavefronts per SIMD fit a CU where the 8 x 8 form fits 2 (fp64 VALU instructions
// issue every 4.26 cycles at 4 waves per SIMD against 4.51 at 2: profiles/r03s_probe_valu_issue_rates_incl_f64.txt).
// The per-output operation sequence does not depend on TI: same bits.
template <typename T, int MAP, int RED, int TI>
__global__ __launch_bounds__(TI == 8 ? 256 : 512, TI == 8 ? 1 : 4) void valu_tile_dma_kernel(const T *__restrict__ A, const T *__restrict__ B,
                                                            T *__restrict__ C, unsigned N, unsigned K, unsigned M,
                                                            unsigned tiles_n, unsigned tiles_m, unsigned kBand) {
#define MM_VT_BATCHED 0
#include "mm_valu_tile_dma_body.inc"
#undef MM_VT_BATCHED
}

template <typename T, int MAP, int RED, int TI>
__global__ __launch_bounds__(TI == 8 ? 256 : 512, TI == 8 ? 1 : 4) void valu_tile_dma_batched_kernel(const T *__restrict__ A, const T *__restrict__ B,
                                                            T *__restrict__ C, unsigned N, unsigned K, unsigned M,
                                                            unsigned tiles_n, unsigned tiles_m, unsigned kBand,
    unsigned batch, size_t stride_a, size_t stride_b, size_t stride_c) {
#define MM_VT_BATCHED 1
#include "mm_valu_tile_dma_body.inc"
#undef MM_VT_BATCHED
}

template <typename T, int MAP, int RED, int TI>
__global__ __launch_bounds__(TI == 8 ? 256 : 512, TI == 8 ? 1 : 4) void valu_tile_dma_batched_seeded_kernel(const T *__restrict__ A, const T *__restrict__ B,
                                                            T *__restrict__ C, unsigned N, unsigned K, unsigned M,
                                                            unsigned tiles_n, unsigned tiles_m, unsigned kBand,
    unsigned batch, size_t stride_a, size_t stride_b, size_t stride_c) {
#define MM_VT_BATCHED 1
#define MM_VT_SEEDED 1
#include "mm_valu_tile_dma_body.inc"
#undef MM_VT_SEEDED
#undef MM_VT_BATCHED
}
#undef MM_DMA_PIECE

// The DMA-staged kernel addresses a tile's rows with 32-bit byte offsets from a uniform base (128 rows x K, BK k-rows x
// M elements) and moves whole 16-byte chunks: K and M multiples of the chunk, K >= one slab, both spans below 4 GiB.
template <typename T>
bool vt_dma_serves(const Problem &p) {
  constexpr unsigned long long ES = sizeof(T), EPC = 16 / ES, BK = 64 / ES;
  return !p.a_transposed && p.k >= BK && p.k % EPC == 0 && p.m % EPC == 0 && p.m >= EPC && 128ull * p.k * ES < (1ull << 32) &&
         BK * (unsigned long long)p.m * ES < (1ull << 32);
}

// BATCHED: p.batch elements of p's shape in one launch (the *_batched_kernel forms), same tile and kernel choice per element
template <typename T, int MAP, int RED, bool BATCHED>
int vt_launch(hipStream_t s, const Problem &p) {
  const unsigned tiles_n = (p.n + VT_BM - 1) / VT_BM, tiles_m = (p.m + VT_BN - 1) / VT_BN;
  const unsigned grid = tiles_n * tiles_m * (BATCHED ? p.batch : 1u);
  // the kernels' argument lists: the single problem's, plus the batch and the element strides for the batched forms (whose
  // seeded twins, for p.seed, take the same arguments)
#define MM_VT_LAUNCH(KERNEL, BATCHED_KERNEL, SEEDED_KERNEL, THREADS, BAND)                                                    \
  do {                                                                                                                      \
    if constexpr (BATCHED) {                                                                                                \
      if (p.seed)                                                                                                           \
        hipLaunchKernelGGL(SEEDED_KERNEL, dim3(grid), dim3(THREADS), 0, s, (const T *)p.a, (const T *)p.b, (T *)p.c, p.n,  \
                           p.k, p.m, tiles_n, tiles_m, BAND, p.batch, p.stride_a, p.stride_b, p.stride_c);                \
      else                                                                                                                  \
        hipLaunchKernelGGL(BATCHED_KERNEL, dim3(grid), dim3(THREADS), 0, s, (const T *)p.a, (const T *)p.b, (T *)p.c, p.n, \
                           p.k, p.m, tiles_n, tiles_m, BAND, p.batch, p.stride_a, p.stride_b, p.stride_c);                \
    } else                                                                                                                  \
      hipLaunchKernelGGL(KERNEL, dim3(grid), dim3(THREADS), 0, s, (const T *)p.a, (const T *)p.b, (T *)p.c, p.n, p.k, p.m, \
                         tiles_n, tiles_m, BAND);                                                                           \
  } while (0)
  // valu_variant knob: 0 = the synchronous kernel; 2 = the DMA-staged kernel with 8 rows per thread for the 8-byte types too
  // (their default since round 4 is 4 rows per thread on 512 threads: 4 wavefronts per SIMD; for the narrower types the same
  // form measured flat, 0.97-1.015 x the 8-row form over float / half / int / uint8, k-ordered and fast alike:
  // profiles/r06f_valu_rows_per_thread_4_vs_8_flat.txt -- not instantiated)
  const int vv = tuning(TUNE_VALU_VARIANT);
  if (vt_dma_serves<T>(p) && vv != 0) {
    if constexpr (sizeof(T) == 8) {
      if (vv != 2) {
        MM_VT_LAUNCH((valu_tile_dma_kernel<T, MAP, RED, 4>), (valu_tile_dma_batched_kernel<T, MAP, RED, 4>),
                     (valu_tile_dma_batched_seeded_kernel<T, MAP, RED, 4>), 512,
                     band_rows(VT_BM, VT_BN, 2));
        return (int)hipGetLastError();
      }
    }
    MM_VT_LAUNCH((valu_tile_dma_kernel<T, MAP, RED, 8>), (valu_tile_dma_batched_kernel<T, MAP, RED, 8>),
                 (valu_tile_dma_batched_seeded_kernel<T, MAP, RED, 8>), 256,
                 band_rows(VT_BM, VT_BN, 2));
    return (int)hipGetLastError();
  }
  if (p.a_transposed)
    MM_VT_LAUNCH((valu_tile_kernel<T, MAP, RED, true>), (valu_tile_batched_kernel<T, MAP, RED, true>),
                 (valu_tile_batched_seeded_kernel<T, MAP, RED, true>), 256, band_rows());
  else
    MM_VT_LAUNCH((valu_tile_kernel<T, MAP, RED, false>), (valu_tile_batched_kernel<T, MAP, RED, false>),
                 (valu_tile_batched_seeded_kernel<T, MAP, RED, false>), 256, band_rows());
#undef MM_VT_LAUNCH
  return (int)hipGetLastError();
}

template <typename T, int MAP, bool BATCHED>
int vt_red(hipStream_t s, int red, const Problem &p) {
  switch (red) {
    case MM_OP_ADD: return vt_launch<T, MAP, MM_OP_ADD, BATCHED>(s, p);
    case MM_OP_MIN: return vt_launch<T, MAP, MM_OP_MIN, BATCHED>(s, p);
    case MM_OP_MAX: return vt_launch<T, MAP, MM_OP_MAX, BATCHED>(s, p);
  }
  return kErrNotSupported;  // Multiply / And reductions: ordered kernel
}

template <typename T, bool BATCHED = false>
int vt_type(hipStream_t s, const mm_config_t &cfg, const Problem &p) {
  if (p.k % 4 != 0 || p.m % 4 != 0 || (p.a_transposed && p.n % 4 != 0)) return kErrNotSupported;
  switch (cfg.map_op) {
    case MM_OP_MULTIPLY: return vt_red<T, MM_OP_MULTIPLY, BATCHED>(s, cfg.reduce_op, p);
    case MM_OP_ADD: return vt_red<T, MM_OP_ADD, BATCHED>(s, cfg.reduce_op, p);
    case MM_OP_MIN: return vt_red<T, MM_OP_MIN, BATCHED>(s, cfg.reduce_op, p);
    case MM_OP_MAX: return vt_red<T, MM_OP_MAX, BATCHED>(s, cfg.reduce_op, p);
    default: break;
  }
  return kErrNotSupported;  // And map: ordered kernel
}

}  // namespace
}  // namespace mm
