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
// What this family's kernels share with each other, with valu_tile_nt and with argreduce_tile: mm_tile128.h.
// Included once per element-type group (mm_valu_tile_*.hip) to keep compile units parallel.
// Requirements of this fast path: K % 4 == 0, M % 4 == 0 (and N % 4 == 0 for a K x N A);
// anything else is served by the predicated ordered kernel.
#include "mm_tile128.h"

namespace mm {
namespace {

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
  __shared__ __attribute__((aligned(16))) T As[kBK128][kTile128 + kPad128];
  __shared__ __attribute__((aligned(16))) T Bs[kBK128][kTile128 + kPad128];
  const unsigned tid = threadIdx.x, tx = tid % 16, ty = tid / 16;
  const unsigned lin = form_tile<F>(A, B, C, tiles_n * tiles_m, batch, stride_a, stride_b, stride_c);
  unsigned row0, col0;
  band_origin(lin, tiles_n, tiles_m, kBand, kTile128, kTile128, row0, col0);

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
  for (unsigned k0 = 0; k0 < K; k0 += kBK128) {
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
    const unsigned kmax = min((unsigned)kBK128, K - k0);  // multiple of 4
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
//   A slab [128 rows][BK k] row-major = 64-byte rows, chunks swizzled on the DMA source; a thread reads its 8 rows' (k, k+1) pairs
//     in one LDS read -- A's side, the slab issue and the slab loop's head are Tile128Dma's (mm_tile128.h), valu_tile_nt_kernel's too;
//   B slab [BK k][128 cols] exactly as in memory (8 KiB); a thread's 2 x 4 columns per k-step as vector reads.
// Per output the operation sequence is unchanged (k ascending, one accumulator): bit-identical to the kernel above and to
// Naive for the order-independent semirings it serves -- the reference's ProcessingElement runs ANY Data_t at full rate
// (kernel/Compute.cpp:120-139), and now so does this family.
// A partial last slab (K % BK != 0) is fetched as the LAST BK k of the matrix and consumed from the offset where the
// new k begin, so no address is ever clamped per lane.  Needs K >= BK, and K, M multiples of the 16-byte chunk.
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
  using D = Tile128Dma<T, TI>;
  constexpr unsigned ES = D::ES, EPC = D::EPC, BK = D::BK, NW = D::NW, PW = D::PW, KSTEP = D::KSTEP;
  constexpr unsigned LPR = 8 * ES, KRP = 64 / LPR;                  // lanes per B k-row (128 cols), k-rows per 1-KiB piece
  __shared__ __attribute__((aligned(16))) char smem[2 * kDmaSlab128];
  const unsigned tid = threadIdx.x, tx = tid % 16, ty = tid / 16;
  const unsigned lane = tid & 63u, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const unsigned lin = form_tile<F>(A, B, C, tiles_n * tiles_m, batch, stride_a, stride_b, stride_c);
  unsigned row0, col0;
  band_origin(lin, tiles_n, tiles_m, kBand, kTile128, kTile128, row0, col0);

  // DMA: 8 A pieces (16 rows x 64 B) and 8 B pieces (KRP k-rows x 128 cols) per slab, PW + PW per wave
  unsigned voff_a[PW], voff_b[PW];
#pragma unroll
  for (unsigned i = 0; i < PW; ++i) {
    const unsigned piece = wave + NW * i;
    const unsigned row = piece * 16 + lane / 4;
    voff_a[i] = D::line_in_tile(row0, N, row) * K * ES + D::chunk(row, lane % 4);
    const unsigned kr = piece * KRP + lane / LPR, c = (lane % LPR) * EPC;
    voff_b[i] = kr * M * ES + (min(col0 + c, M - EPC) - col0) * ES;
  }
  const char *a_base = (const char *)A + (size_t)row0 * K * ES;
  const char *b_base = (const char *)B + (size_t)col0 * ES;
  const unsigned slabs = (K + BK - 1) / BK;
  auto issue = [&](unsigned t) {
    const unsigned k0 = D::slab_k0(t, K);
    D::issue(smem, t, wave, a_base + (size_t)k0 * ES, b_base + (size_t)k0 * M * ES, voff_a, voff_b);
  };

  T acc[TI][8];
#pragma unroll
  for (int i = 0; i < TI; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[i][j] = Op<RED, T>::identity();

  using V = Vec4<T>;
  const unsigned a_swz = ty & 3u;   // (row >> 2) & 3 of every row of this thread
  issue(0);
  if constexpr (F == Form::Seeded) {
    // accumulate: the acc tile starts from C, read with the Vec4 accesses the store below uses (a lane reads exactly what it
    // later writes), issued behind the first slab's DMA pieces; the loop's first vmcnt(0) waits for both
#pragma unroll
    for (int i = 0; i < TI; ++i) {
      const unsigned r = row0 + tile128_row<TI>(ty, i);
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
    unsigned kbeg;
    const char *as = D::next_slab(smem, t, slabs, K, issue, kbeg);
    const char *bs = as + kDmaSide128;
    // the map-reduce steps of one A read go pair by pair, k ascending
    for (unsigned kk = kbeg; kk < BK; kk += KSTEP) {
      typename D::PK av[TI];
      const unsigned kb = kk * ES, aoff = (((kb >> 4) ^ a_swz) * 16) + (kb & 15u);
#pragma unroll
      for (int i = 0; i < TI; ++i) av[i] = *(const typename D::PK *)(as + tile128_row<TI>(ty, i) * 64 + aoff);
#pragma unroll
      for (unsigned q = 0; q < KSTEP; q += 2) {
        T b0[8], b1[8];
        *(V *)&b0[0] = *(const V *)(bs + ((kk + q) * kTile128 + tx * 4) * ES);
        *(V *)&b0[4] = *(const V *)(bs + ((kk + q) * kTile128 + 64 + tx * 4) * ES);
        *(V *)&b1[0] = *(const V *)(bs + ((kk + q + 1) * kTile128 + tx * 4) * ES);
        *(V *)&b1[4] = *(const V *)(bs + ((kk + q + 1) * kTile128 + 64 + tx * 4) * ES);
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
    const unsigned r = row0 + tile128_row<TI>(ty, i);
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

// The DMA-staged kernels address a tile's lines with 32-bit byte offsets from a uniform base and move whole 16-byte chunks.
// The K rule of both (valu_tile_nt's whole shape rule): a row-major A, 128 lines x K below 4 GiB, K a multiple of the chunk and
// at least one slab.  vt_dma_serves: B's BK k-rows x M elements likewise, M a multiple of the chunk.
template <typename T>
bool vt_dma_k_serves(const Problem &p) {
  constexpr unsigned long long ES = sizeof(T), EPC = 16 / ES, BK = 64 / ES;
  return !p.a_transposed && p.k >= BK && p.k % EPC == 0 && 128ull * p.k * ES < (1ull << 32);
}
template <typename T>
bool vt_dma_serves(const Problem &p) {
  constexpr unsigned long long ES = sizeof(T), EPC = 16 / ES, BK = 64 / ES;
  return vt_dma_k_serves<T>(p) && p.m % EPC == 0 && p.m >= EPC && BK * (unsigned long long)p.m * ES < (1ull << 32);
}

// One launch of `kernel`, a form-F kernel of this family or of valu_tile_nt, over p's 128 x 128 tiles: the problem at (a, b, c),
// or (F != Form::Single) p.batch elements of p's shape
template <Form F, typename T, typename Kernel>
int vt_launch_kernel(hipStream_t s, const Problem &p, Kernel kernel, unsigned threads, unsigned band) {
  const unsigned tiles_n = (p.n + kTile128 - 1) / kTile128, tiles_m = (p.m + kTile128 - 1) / kTile128;
  const unsigned batch = F == Form::Single ? 1u : p.batch;
  hipLaunchKernelGGL(kernel, dim3(tiles_n * tiles_m * batch), dim3(threads), 0, s, (const T *)p.a, (const T *)p.b, (T *)p.c, p.n,
                     p.k, p.m, tiles_n, tiles_m, band, batch, p.stride_a, p.stride_b, p.stride_c);
  return (int)hipGetLastError();
}

// The same tile and kernel choice for every element of a batched form
template <Form F, typename T, int MAP, int RED>
int vt_launch_form(hipStream_t s, const Problem &p) {
  auto launch = [&](auto kernel, unsigned threads, unsigned band) { return vt_launch_kernel<F, T>(s, p, kernel, threads, band); };
  // valu_variant knob: 0 = the synchronous kernel; 2 = the DMA-staged kernel with 8 rows per thread for the 8-byte types too
  // (their default since round 4 is 4 rows per thread on 512 threads: 4 wavefronts per SIMD; for the narrower types the same
  // form measured flat, 0.97-1.015 x the 8-row form over float / half / int / uint8, k-ordered and fast alike:
  // profiles/r06f_valu_rows_per_thread_4_vs_8_flat.txt -- not instantiated)
  const int vv = tuning(TUNE_VALU_VARIANT);
  if (vt_dma_serves<T>(p) && vv != 0) {
    if constexpr (sizeof(T) == 8) {
      if (vv != 2) return launch(valu_tile_dma_kernel<F, T, MAP, RED, 4>, 512, band_rows(kTile128, kTile128, 2));
    }
    return launch(valu_tile_dma_kernel<F, T, MAP, RED, 8>, 256, band_rows(kTile128, kTile128, 2));
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
