// "valu_tile_nt": the register-tiled VALU kernel of the A x B^T calls (mm_gemm_nt_*): C[i][j] = reduce_k map(A[i][k], Bt[j][k]),
// both operands stored with k contiguous.  valu_tile_dma_kernel (mm_valu_tile.inc) with B's slab staged the way A's is: the
// tile, the thread grid, A's side, the slab issue and the slab loop's head are Tile128Dma's (mm_tile128.h), and per output it
// is the same k-ascending chain on one accumulator, with valu_tile's bits.  What is this kernel's own:
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

template <Form F, typename T, int MAP, int RED, int TI>
__global__ __launch_bounds__(TI == 8 ? 256 : 512, TI == 8 ? 1 : 4) void valu_tile_nt_kernel(const T *__restrict__ A, const T *__restrict__ Bt,
                                                            T *__restrict__ C, unsigned N, unsigned K, unsigned M,
                                                            unsigned tiles_n, unsigned tiles_m, unsigned kBand,
                                                            unsigned batch, size_t stride_a, size_t stride_b, size_t stride_c) {
  static_assert(F != Form::Single, "the A x B^T calls run the batched forms");
  using D = Tile128Dma<T, TI>;
  constexpr unsigned ES = D::ES, BK = D::BK, NW = D::NW, PW = D::PW, KSTEP = D::KSTEP;
  using PK = typename D::PK;
  __shared__ __attribute__((aligned(16))) char smem[2 * kDmaSlab128];
  const unsigned tid = threadIdx.x, tx = tid % 16, ty = tid / 16;
  const unsigned lane = tid & 63u, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const unsigned lin = form_tile<F>(A, Bt, C, tiles_n * tiles_m, batch, stride_a, stride_b, stride_c);
  unsigned row0, col0;
  band_origin(lin, tiles_n, tiles_m, kBand, kTile128, kTile128, row0, col0);

  // DMA: 8 A pieces (16 rows x 64 B) and 8 Bt pieces (16 cols x 64 B) per slab, PW + PW per wave; row0 < N and col0 < M,
  // so the clamped line is inside the tile's own span
  unsigned voff_a[PW], voff_b[PW];
#pragma unroll
  for (unsigned i = 0; i < PW; ++i) {
    const unsigned piece = wave + NW * i;
    const unsigned line = piece * 16 + lane / 4, chunk = D::chunk(line, lane % 4);
    voff_a[i] = D::line_in_tile(row0, N, line) * K * ES + chunk;
    voff_b[i] = D::line_in_tile(col0, M, line) * K * ES + chunk;
  }
  const char *a_base = (const char *)A + (size_t)row0 * K * ES;
  const char *b_base = (const char *)Bt + (size_t)col0 * K * ES;
  const unsigned slabs = (K + BK - 1) / BK;
  auto issue = [&](unsigned t) {
    const unsigned k0 = D::slab_k0(t, K);
    D::issue(smem, t, wave, a_base + (size_t)k0 * ES, b_base + (size_t)k0 * ES, voff_a, voff_b);
  };

  T acc[TI][8];
#pragma unroll
  for (int i = 0; i < TI; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[i][j] = Op<RED, T>::identity();

  constexpr int JB = ES == 8 ? 4 : 8;
  // column j of this thread: tx + 16 j, all with (col >> 2) & 3 == (tx >> 2) & 3
  const unsigned a_swz = ty & 3u, b_swz = (tx >> 2) & 3u;
  issue(0);
  if constexpr (F == Form::Seeded) {
    // accumulate: the acc tile starts from C, read with the accesses the store below uses, issued behind the first slab's DMA
    // pieces; the loop's first vmcnt(0) waits for both
#pragma unroll
    for (int i = 0; i < TI; ++i) {
      const unsigned r = row0 + tile128_row<TI>(ty, i);
      if (r >= N) continue;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const unsigned c = col0 + tx + 16 * j;
        if (c < M) acc[i][j] = C[(size_t)r * M + c];
      }
    }
  }
  for (unsigned t = 0; t < slabs; ++t) {
    unsigned kbeg;
    const char *as = D::next_slab(smem, t, slabs, K, issue, kbeg);
    const char *bs = as + kDmaSide128;
    for (unsigned kk = kbeg; kk < BK; kk += KSTEP) {
      PK av[TI];
      const unsigned kb = kk * ES, chunk = kb >> 4, sub = kb & 15u;
      const unsigned aoff = ((chunk ^ a_swz) * 16) + sub, boff = ((chunk ^ b_swz) * 16) + sub;
#pragma unroll
      for (int i = 0; i < TI; ++i) av[i] = *(const PK *)(as + tile128_row<TI>(ty, i) * 64 + aoff);
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
    const unsigned r = row0 + tile128_row<TI>(ty, i);
    if (r >= N) continue;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const unsigned c = col0 + tx + 16 * j;
      if (c < M) C[(size_t)r * M + c] = acc[i][j];
    }
  }
}

// The p.batch elements of p in one launch, accumulating into C for p.seed
template <typename T, int MAP, int RED>
int vt_nt_launch(hipStream_t s, const Problem &p) {
  if (!vt_dma_k_serves<T>(p)) return kErrNotSupported;
  constexpr int TI = sizeof(T) == 8 ? 4 : 8;
  const unsigned threads = TI == 8 ? 256 : 512, band = band_rows(kTile128, kTile128, 2);
  return p.seed ? vt_launch_kernel<Form::Seeded, T>(s, p, valu_tile_nt_kernel<Form::Seeded, T, MAP, RED, TI>, threads, band)
                : vt_launch_kernel<Form::Batched, T>(s, p, valu_tile_nt_kernel<Form::Batched, T, MAP, RED, TI>, threads, band);
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
