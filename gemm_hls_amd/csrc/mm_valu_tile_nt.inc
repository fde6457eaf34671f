// "valu_tile_nt": the register-tiled VALU kernel of the A x B^T calls (mm_gemm_nt_*): C[i][j] = reduce_k map(A[i][k], Bt[j][k]),
// both operands stored with k contiguous.  valu_tile_dma_kernel (mm_valu_tile.inc) with B's slab staged the way A's is:
// the same 128 x 128 tile, thread grid, LDS-DMA double buffer, issue / wait / barrier protocol and, per output, the same
// k-ascending chain on one accumulator -- integer and Min / Max results keep Naive's bits, floating Min / Max are
// minNum / maxNum and floating (x, Add) may fuse, exactly as in valu_tile.
//
// The one observation this rests on: in this layout B's slab has the byte geometry of A's.
//   Bt slab [128 cols][64 bytes of k], staged by the same eight 1-KiB LDS-DMA pieces (16 cols x 64 B each), the 16-byte chunk
//     index ^ (col >> 2) & 3 on the DMA SOURCE; columns beyond M are clamped to M - 1 as A's rows are to N - 1, and a partial
//     last slab is fetched as the LAST BK k of the matrix for both operands: no per-lane address is ever out of range, and M
//     needs no divisibility.
//   A thread owns columns tx + 16 j, j < 8 (not valu_tile's tx * 4 + e, which would put the 16 tx lanes of one read on rows
//     256 bytes apart: one bank group, 4- to 16-way), and reads PK = KSTEP consecutive k per column as it does per row of A.
//     (col >> 2) & 3 == (tx >> 2) & 3 for every j: one read-side swizzle per thread.  The 16 columns a service group holds
//     (a 32-lane half of ds_read_b64: 16 tx x 2 ty; a 16-lane group of ds_read_b128: all 16 tx) fall into 16 distinct 16-byte
//     slots of the 256-byte bank row: c % 4 picks the 64-byte quarter, chunk ^ (c >> 2) & 3 the slot in it
//     (tests/test_layouts_nt.py replays both, and the DMA round trip, for every element size).
//   C is stored -- and for Form::Seeded first loaded -- element by element: the 16 tx lanes of a row write consecutive
//     elements, so C needs no alignment.
// 8-byte types keep valu_tile's TI = 4 / 512-thread form (64 accumulator registers, 4 wavefronts per SIMD); their PK reads are
// 16 bytes (ds_read_b128).
// Needs K >= BK = 64 / sizeof(T), K a multiple of the 16-byte chunk, 128 * K * sizeof(T) < 4 GiB, and A, Bt (bases and
// element strides) 16-byte aligned; everything else is ordered_nt's.
#include "mm_valu_tile.inc"

namespace mm {
namespace {

#define MM_DMA_PIECE(vo, sb, la) "s_mov_b32 m0, " la "\n\ts_nop 0\n\tglobal_load_lds_dwordx4 " vo ", " sb "\n\t"
template <Form F, typename T, int MAP, int RED, int TI>
__global__ __launch_bounds__(TI == 8 ? 256 : 512, TI == 8 ? 1 : 4) void valu_tile_nt_kernel(const T *__restrict__ A, const T *__restrict__ Bt,
                                                            T *__restrict__ C, unsigned N, unsigned K, unsigned M,
                                                            unsigned tiles_n, unsigned tiles_m, unsigned kBand,
                                                            unsigned batch, size_t stride_a, size_t stride_b, size_t stride_c) {
  static_assert(TI == 8 || TI == 4, "rows per thread");
  static_assert(F != Form::Single, "the A x B^T calls run the batched forms");
  constexpr unsigned ES = sizeof(T), BK = 64 / ES;   // bytes, slab depth
  constexpr unsigned NW = TI == 8 ? 4 : 8, PW = 8 / NW;   // wavefronts; DMA pieces of A (and of Bt) per wavefront and slab
  static_assert(VT_BN * ES * BK == VTD_A_BYTES && VT_BM == 128 && VT_BN == 128, "byte geometry");
  __shared__ __attribute__((aligned(16))) char smem[2 * VTD_SLAB];
  const unsigned tid = threadIdx.x, tx = tid % 16, ty = tid / 16;
  const unsigned lane = tid & 63u, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const unsigned lin = form_tile<F>(A, Bt, C, tiles_n * tiles_m, batch, stride_a, stride_b, stride_c);
  const unsigned band = lin / (kBand * tiles_m), within = lin % (kBand * tiles_m);
  const unsigned rows_in_band = min(kBand, tiles_n - band * kBand);
  const unsigned row0 = (band * kBand + within % rows_in_band) * VT_BM, col0 = (within / rows_in_band) * VT_BN;

  // DMA: 8 A pieces (16 rows x 64 B) and 8 Bt pieces (16 cols x 64 B) per slab, PW + PW per wave; row0 < N and col0 < M,
  // so the clamped line is inside the tile's own span
  unsigned voff_a[PW], voff_b[PW];
#pragma unroll
  for (unsigned i = 0; i < PW; ++i) {
    const unsigned piece = wave + NW * i;
    const unsigned line = piece * 16 + lane / 4, pc = lane % 4, chunk = (pc ^ ((line >> 2) & 3u)) * 16;
    voff_a[i] = (min(row0 + line, N - 1) - row0) * K * ES + chunk;
    voff_b[i] = (min(col0 + line, M - 1) - col0) * K * ES + chunk;
  }
  const char *a_base = (const char *)A + (size_t)row0 * K * ES;
  const char *b_base = (const char *)Bt + (size_t)col0 * K * ES;
  const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char *)smem;
  const unsigned slabs = (K + BK - 1) / BK;
  auto issue = [&](unsigned t) {  // slab t -> buffer t & 1; the last slab starts at K - BK
    const unsigned k0 = min(t * BK, K - BK);
    const char *ap = a_base + (size_t)k0 * ES;
    const char *bp = b_base + (size_t)k0 * ES;
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

  constexpr unsigned KSTEP = ES >= 4 ? 2 : 8 / ES;   // k per read: 16 B (8-byte types) or 8 B
  struct alignas(KSTEP * sizeof(T)) PK { T v[KSTEP]; };
  constexpr int JB = ES == 8 ? 4 : 8;
  // row i of this thread as in valu_tile_dma_kernel: all of them have (row >> 2) & 3 == ty & 3; column j: tx + 16 j
  auto thread_row = [&](int i) -> unsigned { return TI == 8 ? (i < 4 ? ty * 4 + i : 64 + ty * 4 + (i - 4)) : ty * 4 + i; };
  const unsigned a_swz = ty & 3u, b_swz = (tx >> 2) & 3u;
  issue(0);
  if constexpr (F == Form::Seeded) {
    // accumulate: the acc tile starts from C, read with the accesses the store below uses, issued behind the first slab's DMA
    // pieces; the loop's first vmcnt(0) waits for both
#pragma unroll
    for (int i = 0; i < TI; ++i) {
      const unsigned r = row0 + thread_row(i);
      if (r >= N) continue;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const unsigned c = col0 + tx + 16 * j;
        if (c < M) acc[i][j] = C[(size_t)r * M + c];
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
    for (unsigned kk = kbeg; kk < BK; kk += KSTEP) {
      PK av[TI];
      const unsigned kb = kk * ES, chunk = kb >> 4, sub = kb & 15u;
      const unsigned aoff = ((chunk ^ a_swz) * 16) + sub, boff = ((chunk ^ b_swz) * 16) + sub;
#pragma unroll
      for (int i = 0; i < TI; ++i) av[i] = *(const PK *)(as + thread_row(i) * 64 + aoff);
      // columns in batches of JB reads: the 8-byte form has 128 registers for its 64 of accumulators, so it holds 4 columns'
      // PK at a time (an output's own sequence does not change)
#pragma unroll
      for (int j0 = 0; j0 < 8; j0 += JB) {
        PK bv[JB];
#pragma unroll
        for (int j = 0; j < JB; ++j) bv[j] = *(const PK *)(bs + (tx + 16 * (j0 + j)) * 64 + boff);
#pragma unroll
        for (unsigned q = 0; q < KSTEP; q += 2)
#pragma unroll
          for (int i = 0; i < TI; ++i)
#pragma unroll
            for (int j = 0; j < JB; ++j) {
              const T s0 = FastOp<MAP, T>::apply(av[i].v[q], bv[j].v[q]);
              const T s1 = FastOp<MAP, T>::apply(av[i].v[q + 1], bv[j].v[q + 1]);
              acc[i][j0 + j] = FastOp<RED, T>::apply(FastOp<RED, T>::apply(acc[i][j0 + j], s0), s1);  // k, then k+1
            }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < TI; ++i) {
    const unsigned r = row0 + thread_row(i);
    if (r >= N) continue;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const unsigned c = col0 + tx + 16 * j;
      if (c < M) C[(size_t)r * M + c] = acc[i][j];
    }
  }
}
#undef MM_DMA_PIECE

// The shape rule of vt_nt_serves() for one element type
template <typename T>
bool vt_nt_shape_serves(const Problem &p) {
  constexpr unsigned long long ES = sizeof(T), EPC = 16 / ES, BK = 64 / ES;
  return !p.a_transposed && p.k >= BK && p.k % EPC == 0 && 128ull * p.k * ES < (1ull << 32);
}

// The p.batch elements of p in one launch, accumulating into C for p.seed
template <typename T, int MAP, int RED>
int vt_nt_launch(hipStream_t s, const Problem &p) {
  if (!vt_nt_shape_serves<T>(p)) return kErrNotSupported;
  const unsigned tiles_n = (p.n + VT_BM - 1) / VT_BM, tiles_m = (p.m + VT_BN - 1) / VT_BN;
  const unsigned grid = tiles_n * tiles_m * p.batch;
  auto launch = [&](auto kernel, unsigned threads) {
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(threads), 0, s, (const T *)p.a, (const T *)p.b, (T *)p.c, p.n, p.k, p.m,
                       tiles_n, tiles_m, band_rows(VT_BM, VT_BN, 2), p.batch, p.stride_a, p.stride_b, p.stride_c);
    return (int)hipGetLastError();
  };
  constexpr int TI = sizeof(T) == 8 ? 4 : 8;
  return p.seed ? launch(valu_tile_nt_kernel<Form::Seeded, T, MAP, RED, TI>, TI == 8 ? 256 : 512)
                : launch(valu_tile_nt_kernel<Form::Batched, T, MAP, RED, TI>, TI == 8 ? 256 : 512);
}

// TYPES: the element types the including unit instantiates.  An And map, a Multiply or And reduction: ordered_nt
template <typename TYPES>
int vt_nt_dispatch(hipStream_t s, const mm_config_t &cfg, const Problem &p) {
  using Maps = Ops<MM_OP_MULTIPLY, MM_OP_ADD, MM_OP_MIN, MM_OP_MAX>;
  using Reds = Ops<MM_OP_ADD, MM_OP_MIN, MM_OP_MAX>;
  return switch_config<TYPES, Maps, Reds>(cfg, [&](auto t, auto map, auto red) {
    return vt_nt_launch<type_of<decltype(t)>, decltype(map)::value, decltype(red)::value>(s, p);
  });
}

}  // namespace
}  // namespace mm
