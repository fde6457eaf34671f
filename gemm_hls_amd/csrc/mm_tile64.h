// What the five fully predicated 64 x 64 kernels (ordered, ordered_nt, widen_ordered, argreduce, lse_exact) share.  256 threads
// own 64 x 64 outputs, thread (tid % 16, tid / 16) = (tx, ty) rows ty * 4 + i and columns tx + 16 j; K goes in slabs of 16
// through k-major LDS images As[k][row], Bs[k][col].  DESIGN.md 3.13.
#pragma once
#include "mm_common.h"

namespace mm {

constexpr int kTile = 64, kBK = 16, kPerThread = 4;   // outputs per workgroup edge, k per slab, outputs per thread edge

// A batched launch's workgroup, uniform (SGPRs): a 1-D grid of batch x tiles workgroups, XCD-remapped ids `lin` = e * tiles ..
// (e + 1) * tiles - 1 for element e (one element's tiles stay on one XCD), t row-major over the element's tiles
struct Tile64 {
  unsigned tiles_m, lin, e, t;
  __device__ __forceinline__ unsigned row0() const { return (t / tiles_m) * kTile; }
  __device__ __forceinline__ unsigned col0() const { return (t % tiles_m) * kTile; }
};
__device__ __forceinline__ Tile64 tile64_split(unsigned N, unsigned M) {
  const unsigned tiles_m = (M + kTile - 1) / kTile, tiles = tiles_m * ((N + kTile - 1) / kTile);
  const unsigned lin = xcd_remap(blockIdx.x, gridDim.x), e = lin / tiles;
  return {tiles_m, lin, e, lin - e * tiles};
}

// The tile's first row and column in a kernel of form F.  Form::Single: a 2-D grid of tiles, no stride is read.  Batched forms:
// A, B and C move to the workgroup's element, which is returned (argreduce_kernel moves I by it too) -- before row0 and col0
// are formed: the other order compiled the Seeded kernels to other code.  lse_exact_kernel uses the split itself: it reads
// its tile's flag before it moves anything, and through this function it ran 0.1 - 0.8 % slower.
template <Form F, typename PA, typename PB, typename PC>
__device__ __forceinline__ unsigned tile64_origin(PA &A, PB &B, PC &C, unsigned N, unsigned M, size_t stride_a, size_t stride_b,
                                                  size_t stride_c, unsigned &row0, unsigned &col0) {
  if constexpr (F == Form::Single) {
    row0 = blockIdx.y * kTile, col0 = blockIdx.x * kTile;
    return 0;
  } else {
    const Tile64 w = tile64_split(N, M);
    A += w.e * stride_a;
    B += w.e * stride_b;
    C += w.e * stride_c;
    row0 = w.row0(), col0 = w.col0();
    return w.e;
  }
}

struct Tile64Load { template <typename S> __device__ __forceinline__ S operator()(const S *p) const { return *p; } };   // the element as stored

// One slab of one operand (argreduce_kernel, lse_exact_kernel; the other three keep their own loops): lines
// line0 .. line0 + 63 (rows of A, columns of B) x k0 .. k0 + 15 of a row-major source into dst[k][line].  Consecutive lanes
// run along the source's contiguous axis.  KCONTIG (src is L x K): kk = tid % 16, line = tid / 16 + 16 i, and the image's rows
// are padded, because a wavefront writes down its columns.  Else (src is K x L): line = tid % 64, kk = tid / 64 + 4 i.
// A lane stores load(&element) inside the matrix, 0 for a line >= L, and beyond_k for k >= K whatever the line.
template <bool KCONTIG, typename T, int LD, typename S, typename Load = Tile64Load>
__device__ __forceinline__ void tile64_stage(T (&dst)[kBK][LD], const S *src, unsigned line0, unsigned L, unsigned k0,
                                             unsigned K, Load load = {}, T beyond_k = (T)0) {
  static_assert(LD >= kTile, "the image holds 64 lines per k");
  const unsigned tid = threadIdx.x;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const unsigned kk = KCONTIG ? tid % 16 : tid / 64 + 4 * i, line = KCONTIG ? tid / 16 + 16 * i : tid % 64;
    const unsigned gl = line0 + line, gk = k0 + kk;
    T v = beyond_k;
    if (gk < K) v = gl < L ? (T)load(src + (KCONTIG ? (size_t)gl * K + gk : (size_t)gk * L + gl)) : (T)0;
    dst[kk][line] = v;
  }
}

}  // namespace mm
