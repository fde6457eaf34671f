// What the four 128 x 128 register-tile kernels (valu_tile, valu_tile_dma, valu_tile_nt, argreduce_tile) share.  A workgroup
// owns 128 x 128 outputs; thread (tid % 16, tid / 16) = (tx, ty) holds TI x 8 of them in registers for the whole K loop: TI
// rows (tile128_row) and, except in valu_tile_nt, the two 4-wide column groups h * 64 + tx * 4, which move to and from C as
// Vec4 accesses.  Tiles are rasterised in bands (band_origin, mm_common.h).  DESIGN.md 3.17.
// Only what left every kernel's machine code as it was is here: values in, a value out, or a DMA kernel's former lambda body.
// A helper that took the accumulators or an LDS image by reference, or carried a loop, compiled the kernels to other code, so
// each kernel writes out its accumulator initialisation, its loops over the Vec4s of C it owns and over its rows of A, and
// (valu_tile_kernel, argreduce_tile_kernel) its synchronous staging and its rows.  profiles/tile128_isa_identity.txt.
#pragma once
#include "mm_common.h"

namespace mm {

// outputs per workgroup edge; the synchronously staged kernels' k per slab and the padding of their k-major images' rows
constexpr int kTile128 = 128, kBK128 = 16, kPad128 = 4;

template <typename T> struct alignas(4 * sizeof(T)) Vec4 { T v[4]; };

// Row i < TI of thread row ty in the DMA-staged kernels.  TI == 8 (256 threads, ty < 16): ty*4 + i, then 64 + ty*4 + (i-4);
// TI == 4 (512 threads, ty < 32): ty*4 + i.  Either way all of a thread's rows have (row >> 2) & 3 == ty & 3.
template <int TI> __device__ __forceinline__ unsigned tile128_row(unsigned ty, int i) {
  static_assert(TI == 8 || TI == 4, "rows per thread");
  return TI == 8 ? (i < 4 ? ty * 4 + i : 64 + ty * 4 + (i - 4)) : ty * 4 + i;
}

// ---- LDS-DMA staging (valu_tile_dma_kernel, valu_tile_nt_kernel) -------------------------------------------------------------
// Two slab buffers, each kDmaSide128 bytes of A and then as many of B, written by LDS-DMA (global_load_lds_dwordx4), eight
// 1-KiB pieces per operand and slab.  A k-contiguous operand's side is [128 lines][64 bytes of k], a piece 16 lines x 64 B.
constexpr int kDmaSide128 = kTile128 * 64, kDmaSlab128 = 2 * kDmaSide128;  // 8 KiB + 8 KiB

template <typename T, int TI>
struct Tile128Dma {
  static constexpr unsigned ES = sizeof(T), EPC = 16 / ES, BK = 64 / ES;   // bytes, elements per 16-B chunk, slab depth
  static constexpr unsigned NW = TI == 8 ? 4 : 8, PW = 8 / NW;   // wavefronts; DMA pieces of each operand per wavefront and slab
  static constexpr unsigned KSTEP = ES >= 4 ? 2 : 8 / ES;        // k per LDS read of a line: 16 B (8-byte types) or 8 B
  struct alignas(KSTEP * sizeof(T)) PK { T v[KSTEP]; };
  static_assert(kTile128 * ES * BK == kDmaSide128, "byte geometry");

  // A lane's byte offset into a k-contiguous operand is line_in_tile(..) * K * ES + chunk(..), for line = piece * 16 + lane / 4
  // and 16-byte slot pc = lane % 4 of its piece.  A line beyond the operand's L lines is clamped to L - 1, which line0 < L keeps
  // inside the tile's own span; the source chunk is the slot ^ (line >> 2) & 3, so that the four lines a wave reads at once
  // fall into different slots.
  static __device__ __forceinline__ unsigned line_in_tile(unsigned line0, unsigned L, unsigned line) { return min(line0 + line, L - 1) - line0; }
  static __device__ __forceinline__ unsigned chunk(unsigned line, unsigned pc) { return (pc ^ ((line >> 2) & 3u)) * 16; }
  // Slab t's first k: the last slab starts at K - BK, so a partial one is fetched as the LAST BK k of the matrix
  static __device__ __forceinline__ unsigned slab_k0(unsigned t, unsigned K) { return min(t * BK, K - BK); }

  // This wavefront's pieces of slab t -> buffer t & 1, from the uniform bases ap and bp plus the lanes' offsets
  static __device__ __forceinline__ void issue(const char *smem, unsigned t, unsigned wave, const char *ap, const char *bp,
                                               const unsigned (&voff_a)[PW], const unsigned (&voff_b)[PW]) {
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char *)smem;
    const unsigned la0 = lds0 + (t & 1u) * kDmaSlab128 + wave * 1024, la1 = la0 + 4 * 1024;
    const unsigned lb0 = la0 + kDmaSide128, lb1 = lb0 + 4 * 1024;
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
  }

  // The head of slab t's trip: ONE barrier per slab, the next slab in flight under this one's VALU instructions.  Returns the slab's
  // buffer (A's side; B's is kDmaSide128 further) and kbeg: a full slab uses k 0 .. BK-1 of it, the shifted last slab only its new k.
  template <typename Issue>
  static __device__ __forceinline__ const char *next_slab(const char *smem, unsigned t, unsigned slabs, unsigned K, Issue issue,
                                                          unsigned &kbeg) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // own pieces of slab t have landed
    __syncthreads();                                  // everybody's have; buffer (t+1)&1 is no longer being read
    if (t + 1 < slabs) issue(t + 1);
    kbeg = t * BK - slab_k0(t, K);  // 0 except for a partial last slab
    return smem + (t & 1u) * kDmaSlab128;
  }
};

}  // namespace mm
