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


// F (mm_common.h): the single-problem kernel, its strided-batched form, or (Form::Seeded) the batched form with the acc tile
// loaded from C instead of set to identity()
template <Form F, typename T, int MAP, int RED, bool AT>
__global__ __launch_bounds__(256) void valu_tile_kernel(const T *__restrict__ A, const T *__restrict__ B,
                                                        T *__restrict__ C, unsigned N, unsigned K, unsigned M,
                                                        unsigned tiles_n, unsigned tiles_m, unsigned kBand,
                                                        unsigned batch, size_t stride_a, size_t stride_b, size_t stride_c) {
  __shared__ __attribute__((aligned(16))) T As[VT_BK][VT_BM + VT_PAD];
  __shared__ __attribute__((aligned(16))) T Bs[VT_BK][VT_BN + VT_PAD];
  const unsigned tid = threadIdx.x, tx = tid % 16, ty = tid / 16;
  const unsigned lin = form_tile<F>(A, B, C, tiles_n * tiles_m, batch, stride_a, stride_b, stride_c);
  const unsigned band = lin / (kBand * tiles_m), within = lin % (kBand * tiles_m);
  const unsigned rows_in_band = min(kBand, tiles_n - band * kBand);
  const unsigned row0 = (band * kBand + within % rows_in_band) * VT_BM, col0 = (within / rows_in_band) * VT_BN;

  T acc[8][8];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[i][j] = Op<RED, T>::identity();

  using V = Vec4<T>;
  if constexpr (F == Form::Seeded) {
    // accumulate: the acc tile starts from C, read with the Vec4 accesses the store below uses (a lane reads exactly what it
    // later writes); the loads are consumed at the first k-step, so they are in flight while the first slab is staged
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const unsigned r = row0 + (i < 4 ? ty * 4 + i : 64 + ty * 4 + (i - 4));
      if (r >= N) continue;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const unsigned c = col0 + h * 64 + tx * 4;
        if (c < M) {
          const V v = *(const V *)(C + (size_t)r * M + c);
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[i][h * 4 + e] = v.v[e];
        }
      }
    }
  }
  for (unsigned k0 = 0; k0 < K; k0 += VT_BK) {
    // ---- stage (K % 4 == 0, so a 4-wide k chunk is entirely inside or entirely outside) ----
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const unsigned idx = tid + 256 * u;
      if (AT) {  // A is K x N: rows of the tile are contiguous
        const unsigned kr = idx / 32, r4 = (idx % 32) * 4;
        V v = {};
        if (k0 + kr < K && row0 + r4 < N) v = *(const V *)(A + (size_t)(k0 + kr) * N + row0 + r4);
        *(V *)&As[kr][r4] = v;
      } else {   // A is N x K: 4 lanes cover one row's 16 k; scatter into the k-major image
        const unsigned r = idx / 4, kc = (idx % 4) * 4;
        V v = {};
        if (row0 + r < N && k0 + kc < K) v = *(const V *)(A + (size_t)(row0 + r) * K + k0 + kc);
#pragma unroll
        for (int e = 0; e < 4; ++e) As[kc + e][r] = v.v[e];
      }
      {
        const unsigned kr = idx / 32, c4 = (idx % 32) * 4;
        V v = {};
        if (k0 + kr < K && col0 + c4 < M) v = *(const V *)(B + (size_t)(k0 + kr) * M + col0 + c4);
        *(V *)&Bs[kr][c4] = v;
      }
    }
    __syncthreads();
    const unsigned kmax = min((unsigned)VT_BK, K - k0);  // multiple of 4
    for (unsigned kk = 0; kk < kmax; kk += 2) {
      T a0[8], b0[8], a1[8], b1[8];
      *(V *)&a0[0] = *(const V *)&As[kk][ty * 4];
      *(V *)&a0[4] = *(const V *)&As[kk][64 + ty * 4];
      *(V *)&b0[0] = *(const V *)&Bs[kk][tx * 4];
      *(V *)&b0[4] = *(const V *)&Bs[kk][64 + tx * 4];
      *(V *)&a1[0] = *(const V *)&As[kk + 1][ty * 4];
      *(V *)&a1[4] = *(const V *)&As[kk + 1][64 + ty * 4];
      *(V *)&b1[0] = *(const V *)&Bs[kk + 1][tx * 4];
      *(V *)&b1[4] = *(const V *)&Bs[kk + 1][64 + tx * 4];
#pragma unroll
      for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const T s0 = FastOp<MAP, T>::apply(a0[i], b0[j]);
          const T s1 = FastOp<MAP, T>::apply(a1[i], b1[j]);
          acc[i][j] = FastOp<RED, T>::apply(FastOp<RED, T>::apply(acc[i][j], s0), s1);  // k, then k+1
        }
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const unsigned r = row0 + (i < 4 ? ty * 4 + i : 64 + ty * 4 + (i - 4));
    if (r >= N) continue;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const unsigned c = col0 + h * 64 + tx * 4;
      if (c < M) {
        V v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v.v[e] = acc[i][h * 4 + e];
        *(V *)(C + (size_t)r * M + c) = v;
      }
    }
  }
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
template <Form F, typename T, int MAP, int RED, int TI>
__global__ __launch_bounds__(TI == 8 ? 256 : 512, TI == 8 ? 1 : 4) void valu_tile_dma_kernel(const T *__restrict__ A, const T *__restrict__ B,
                                                            T *__restrict__ C, unsigned N, unsigned K, unsigned M,
                                                            unsigned tiles_n, unsigned tiles_m, unsigned kBand,
                                                            unsigned batch, size_t stride_a, size_t stride_b, size_t stride_c) {
  static_assert(TI == 8 || TI == 4, "rows per thread");
  constexpr unsigned ES = sizeof(T), EPC = 16 / ES, BK = 64 / ES;   // bytes, elements per 16-B chunk, slab depth
  constexpr unsigned LPR = 8 * ES, KRP = 64 / LPR;                  // lanes per B k-row (128 cols), k-rows per 1-KiB piece
  constexpr unsigned NW = TI == 8 ? 4 : 8, PW = 8 / NW;             // wavefronts; DMA pieces of A (and of B) per wavefront and slab
  static_assert(VT_BN * ES * BK == VTD_A_BYTES && VT_BM == 128 && VT_BN == 128, "byte geometry");
  __shared__ __attribute__((aligned(16))) char smem[2 * VTD_SLAB];
  const unsigned tid = threadIdx.x, tx = tid % 16, ty = tid / 16;
  const unsigned lane = tid & 63u, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const unsigned lin = form_tile<F>(A, B, C, tiles_n * tiles_m, batch, stride_a, stride_b, stride_c);
  const unsigned band = lin / (kBand * tiles_m), within = lin % (kBand * tiles_m);
  const unsigned rows_in_band = min(kBand, tiles_n - band * kBand);
  const unsigned row0 = (band * kBand + within % rows_in_band) * VT_BM, col0 = (within / rows_in_band) * VT_BN;

  // DMA: 8 A pieces (16 rows x 64 B) and 8 B pieces (KRP k-rows x 128 cols) per slab, PW + PW per wave
  unsigned voff_a[PW], voff_b[PW];
#pragma unroll
  for (unsigned i = 0; i < PW; ++i) {
    const unsigned piece = wave + NW * i;
    const unsigned row = piece * 16 + lane / 4, pc = lane % 4;
    voff_a[i] = (min(row0 + row, N - 1) - row0) * K * ES + (pc ^ ((row >> 2) & 3u)) * 16;
    const unsigned kr = piece * KRP + lane / LPR, c = (lane % LPR) * EPC;
    voff_b[i] = kr * M * ES + (min(col0 + c, M - EPC) - col0) * ES;
  }
  const char *a_base = (const char *)A + (size_t)row0 * K * ES;
  const char *b_base = (const char *)B + (size_t)col0 * ES;
  const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char *)smem;
  const unsigned slabs = (K + BK - 1) / BK;
  auto issue = [&](unsigned t) {  // slab t -> buffer t & 1; the last slab starts at K - BK
    const unsigned k0 = min(t * BK, K - BK);
    const char *ap = a_base + (size_t)k0 * ES;
    const char *bp = b_base + (size_t)k0 * M * ES;
    const unsigned la0 = lds0 + (t & 1u) * VTD_SLAB + wave * 1024, la1 = la0 + 4 * 1024;
    const unsigned lb0 = la0 + VTD_A_BYTES, lb1 = lb0 + 4 * 1024;
    unsigned keep;
    if constexpr (PW == 2) {
      asm volatile("s_mov_b32 %0, m0\n\t" MM_DMA_PIECE("%1", "%5", "%7") MM_DMA_PIECE("%2", "%5", "%8")
                       MM_DMA_PIECE("%3", "%6", "%9") MM_DMA_PIECE("%4", "%6", "%10") "s_mov_b32 m0, %0"
                   : "=&s"(keep)
                   : "v"(voff_a[0]), "v"(voff_a[1]), "v"(voff_b[0]), "v"(voff_b[1]), "s"(ap), "s"(bp), "s"(la0), "s"(la1),
                     "s"(lb0), "s"(lb1)
                   : "memory");
    } else {
      asm volatile("s_mov_b32 %0, m0\n\t" MM_DMA_PIECE("%1", "%3", "%5") MM_DMA_PIECE("%2", "%4", "%6") "s_mov_b32 m0, %0"
                   : "=&s"(keep)
                   : "v"(voff_a[0]), "v"(voff_b[0]), "s"(ap), "s"(bp), "s"(la0), "s"(lb0)
                   : "memory");
    }
  };

  T acc[TI][8];
#pragma unroll
  for (int i = 0; i < TI; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[i][j] = Op<RED, T>::identity();

  using V = Vec4<T>;
  constexpr unsigned KSTEP = ES >= 4 ? 2 : 8 / ES;   // k per A read: 16 B (8-byte types) or 8 B
  struct alignas(KSTEP * sizeof(T)) PK { T v[KSTEP]; };
  // row i of this thread: TI == 8: ty*4 + i, then 64 + ty*4 + (i-4) (ty < 16); TI == 4: ty*4 + i (ty < 32).
  // Either way all of a thread's rows have (row >> 2) & 3 == ty & 3
  auto thread_row = [&](int i) -> unsigned { return TI == 8 ? (i < 4 ? ty * 4 + i : 64 + ty * 4 + (i - 4)) : ty * 4 + i; };
  const unsigned a_swz = ty & 3u;
  issue(0);
  if constexpr (F == Form::Seeded) {
    // accumulate: the acc tile starts from C, read with the Vec4 accesses the store below uses (a lane reads exactly what it
    // later writes), issued behind the first slab's DMA pieces; the loop's first vmcnt(0) waits for both
#pragma unroll
    for (int i = 0; i < TI; ++i) {
      const unsigned r = row0 + thread_row(i);
      if (r >= N) continue;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const unsigned c = col0 + h * 64 + tx * 4;
        if (c < M) {
          const V v = *(const V *)(C + (size_t)r * M + c);
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[i][h * 4 + e] = v.v[e];
        }
      }
    }
  }
  for (unsigned t = 0; t < slabs; ++t) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // own pieces of slab t have landed
    __syncthreads();                                  // everybody's have; buffer (t+1)&1 is no longer being read
    if (t + 1 < slabs) issue(t + 1);
    const char *as = smem + (t & 1u) * VTD_SLAB;
    const char *bs = as + VTD_A_BYTES;
    // a full slab uses k 0..BK-1 of the buffer; the (shifted) last slab only its new k
    const unsigned kbeg = t * BK - min(t * BK, K - BK);  // 0 except for a partial last slab
    // one LDS read per row fetches KSTEP consecutive k (8 or 16 bytes: a pair for 4- and 8-byte types, 4 / 8 k for
    // 2- / 1-byte types); the map-reduce steps then go pair by pair, k ascending
    for (unsigned kk = kbeg; kk < BK; kk += KSTEP) {
      PK av[TI];
      const unsigned kb = kk * ES, aoff = (((kb >> 4) ^ a_swz) * 16) + (kb & 15u);
#pragma unroll
      for (int i = 0; i < TI; ++i) av[i] = *(const PK *)(as + thread_row(i) * 64 + aoff);
#pragma unroll
      for (unsigned q = 0; q < KSTEP; q += 2) {
        T b0[8], b1[8];
        *(V *)&b0[0] = *(const V *)(bs + ((kk + q) * VT_BN + tx * 4) * ES);
        *(V *)&b0[4] = *(const V *)(bs + ((kk + q) * VT_BN + 64 + tx * 4) * ES);
        *(V *)&b1[0] = *(const V *)(bs + ((kk + q + 1) * VT_BN + tx * 4) * ES);
        *(V *)&b1[4] = *(const V *)(bs + ((kk + q + 1) * VT_BN + 64 + tx * 4) * ES);
#pragma unroll
        for (int i = 0; i < TI; ++i)
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const T s0 = FastOp<MAP, T>::apply(av[i].v[q], b0[j]);
            const T s1 = FastOp<MAP, T>::apply(av[i].v[q + 1], b1[j]);
            acc[i][j] = FastOp<RED, T>::apply(FastOp<RED, T>::apply(acc[i][j], s0), s1);  // k, then k+1
          }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < TI; ++i) {
    const unsigned r = row0 + thread_row(i);
    if (r >= N) continue;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const unsigned c = col0 + h * 64 + tx * 4;
      if (c < M) {
        V v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v.v[e] = acc[i][h * 4 + e];
        *(V *)(C + (size_t)r * M + c) = v;
      }
    }
  }
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

// One launch in form F: the problem at (a, b, c), or (F != Form::Single) p.batch elements of p's shape, same tile and kernel
// choice per element
template <Form F, typename T, int MAP, int RED>
int vt_launch_form(hipStream_t s, const Problem &p) {
  const unsigned tiles_n = (p.n + VT_BM - 1) / VT_BM, tiles_m = (p.m + VT_BN - 1) / VT_BN;
  const unsigned grid = tiles_n * tiles_m * (F == Form::Single ? 1u : p.batch);
  auto launch = [&](auto kernel, unsigned threads, unsigned band) {
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(threads), 0, s, (const T *)p.a, (const T *)p.b, (T *)p.c, p.n, p.k, p.m,
                       tiles_n, tiles_m, band, F == Form::Single ? 1u : p.batch, p.stride_a, p.stride_b, p.stride_c);
    return (int)hipGetLastError();
  };
  // valu_variant knob: 0 = the synchronous kernel; 2 = the DMA-staged kernel with 8 rows per thread for the 8-byte types too
  // (their default since round 4 is 4 rows per thread on 512 threads: 4 wavefronts per SIMD; for the narrower types the same
  // form measured flat, 0.97-1.015 x the 8-row form over float / half / int / uint8, k-ordered and fast alike:
  // profiles/r06f_valu_rows_per_thread_4_vs_8_flat.txt -- not instantiated)
  const int vv = tuning(TUNE_VALU_VARIANT);
  if (vt_dma_serves<T>(p) && vv != 0) {
    if constexpr (sizeof(T) == 8) {
      if (vv != 2) return launch(valu_tile_dma_kernel<F, T, MAP, RED, 4>, 512, band_rows(VT_BM, VT_BN, 2));
    }
    return launch(valu_tile_dma_kernel<F, T, MAP, RED, 8>, 256, band_rows(VT_BM, VT_BN, 2));
  }
  return p.a_transposed ? launch(valu_tile_kernel<F, T, MAP, RED, true>, 256, band_rows())
                        : launch(valu_tile_kernel<F, T, MAP, RED, false>, 256, band_rows());
}

// BATCHED: the p.batch elements of p in one launch, accumulating into C for p.seed
template <typename T, int MAP, int RED, bool BATCHED>
int vt_launch(hipStream_t s, const Problem &p) {
  if constexpr (!BATCHED) return vt_launch_form<Form::Single, T, MAP, RED>(s, p);
  else return p.seed ? vt_launch_form<Form::Seeded, T, MAP, RED>(s, p) : vt_launch_form<Form::Batched, T, MAP, RED>(s, p);
}

// TYPES: the element types the including unit instantiates.  An And map, a Multiply or And reduction: the ordered kernel
template <typename TYPES, bool BATCHED>
int vt_dispatch(hipStream_t s, const mm_config_t &cfg, const Problem &p) {
  if (p.k % 4 != 0 || p.m % 4 != 0 || (p.a_transposed && p.n % 4 != 0)) return kErrNotSupported;
  using Maps = Ops<MM_OP_MULTIPLY, MM_OP_ADD, MM_OP_MIN, MM_OP_MAX>;
  using Reds = Ops<MM_OP_ADD, MM_OP_MIN, MM_OP_MAX>;
  return switch_config<TYPES, Maps, Reds>(cfg, [&](auto t, auto map, auto red) {
    return vt_launch<type_of<decltype(t)>, decltype(map)::value, decltype(red)::value, BATCHED>(s, p);
  });
}

}  // namespace
}  // namespace mm
