// Bit-packed product over the field GF(2) (mm_bits_gf2_*; the format: include/mm_gemm.h): C = XOR_k (A AND B) on one bit per
// element, 32 columns per word.  Two kernels with the same bits: the mask loop of the Boolean product with ^= for |=
// ("bits_gf2_plain", mm_bits_product.inc) and the Method of the Four Russians on LDS tables ("bits_gf2_tile").
#include "mm_common.h"

namespace mm {
namespace {

#include "mm_bits_product.inc"

constexpr unsigned kGf2Threads = 512;    // 8 wavefronts, two per SIMD: one's scalar and LDS instructions issue beside the other's vector ones
constexpr unsigned kGf2Rows = 128;       // rows of C per workgroup: 8 wavefronts x kGf2WaveRows
constexpr unsigned kGf2WaveRows = 16;    // rows per wavefront = accumulator rows per thread
constexpr unsigned kGf2Words = 128;      // words of C per workgroup row: 2 consecutive words per lane
constexpr unsigned kGroups = kSlab / 4;  // groups of 4 consecutive k per slab: one table of 16 entries each

// One workgroup of 512 threads: 128 rows x 128 words of C, 16 rows per wavefront.  Per slab of 32 k it builds T[g][v] = XOR
// over the bits b of v of row 32 s + 4 g + b of B, for the 8 groups g of 4 consecutive k and the 16 values v of a nibble:
// wavefront g builds table g, its lane l loads words 2 l and 2 l + 1 of the group's 4 rows (8-byte loads) and walks the 16
// entries in Gray-code order, one uint2 XOR and one 8-byte LDS store per entry.  A row of C then takes one table entry per nibble of its word of A: the lanes of a wavefront span the words (2
// per lane), A's word is wave-uniform, so the nibble is one scalar bit-field extract, the entry one 8-byte LDS read of 512
// contiguous bytes (no bank conflict) and the update two vector XORs -- for 4 k.  Every slab costs the same whatever A and B
// hold: the time does not depend on the data.
// B and C in 8-byte accesses wherever a whole access lies inside the row's words (ldb % 2 == 0, ldc % 2 == 0,
// aligned bases and batch strides: the launcher's rule); an access that straddles ceil(M / 32) takes the one word.  Rows >= N,
// words >= ceil(M / 32), k >= K are predicated: no address outside an operand is formed, no word beyond a row's word count is
// touched.  Rows of B at k >= K enter the tables as 0 and A's last word is masked: no padding bit of either contributes.
__global__ __launch_bounds__(kGf2Threads) void bits_gf2_tile_kernel(const uint32_t *__restrict__ A, const uint32_t *__restrict__ B,
                                                                 uint32_t *__restrict__ C, unsigned N, unsigned K, unsigned M,
                                                                 size_t lda, size_t ldb, size_t ldc, unsigned tiles_w,
                                                                 unsigned tiles, size_t stride_a, size_t stride_b,
                                                                 size_t stride_c, int seed) {
  __shared__ __attribute__((aligned(16))) uint32_t sT[kGroups][16][kGf2Words];   // 64 KiB
  __shared__ uint32_t sA[kGf2Rows];

  const unsigned tid = threadIdx.x, lane = tid & 63;
  const unsigned wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const unsigned e = blockIdx.x / tiles, t = blockIdx.x - e * tiles;
  A += e * stride_a;
  B += e * stride_b;
  C += e * stride_c;
  const unsigned row0 = (t / tiles_w) * kGf2Rows, w0 = (t % tiles_w) * kGf2Words;
  const unsigned mw = (M + 31) / 32, kw = (K + 31) / 32;
  const uint32_t k_tail = (K & 31) ? (1u << (K & 31)) - 1 : ~0u;   // A's padding never contributes

  uint32_t acc[kGf2WaveRows][2];
#pragma unroll
  for (unsigned r = 0; r < kGf2WaveRows; ++r) acc[r][0] = acc[r][1] = 0;

  const unsigned grp = tid >> 6, pair = lane * 2;   // the table this thread builds, and its 2 words of it
  uint2 rb[4];                                      // the next slab's 4 rows of B, and word of A, on their way to LDS
  uint32_t ra = 0;
  auto load = [&](unsigned s) {
    const unsigned w = w0 + pair;
#pragma unroll
    for (unsigned b = 0; b < 4; ++b) {
      const unsigned k = s * kSlab + grp * 4 + b;
      rb[b] = make_uint2(0, 0);
      if (k >= K || w >= mw) continue;
      const uint32_t *src = B + (size_t)k * ldb + w;
      if (w + 2 <= mw) rb[b] = *reinterpret_cast<const uint2 *>(src);
      else rb[b].x = src[0];   // the row's last word alone
    }
    if (tid < kGf2Rows) {
      const unsigned row = row0 + tid;
      ra = row < N ? A[(size_t)row * lda + s] : 0u;
      if (s == kw - 1) ra &= k_tail;
    }
  };

  if (kw) load(0);
  for (unsigned s = 0; s < kw; ++s) {
    __syncthreads();   // the previous slab's tables have been read
    uint2 cur = make_uint2(0, 0);
    *reinterpret_cast<uint2 *>(&sT[grp][0][pair]) = cur;
#pragma unroll
    for (unsigned i = 1; i < 16; ++i) {   // Gray code: entry i ^ (i >> 1) differs from the one before in bit ctz(i)
      const uint2 x = rb[__builtin_ctz(i)];
      cur.x ^= x.x; cur.y ^= x.y;
      *reinterpret_cast<uint2 *>(&sT[grp][i ^ (i >> 1)][pair]) = cur;
    }
    if (tid < kGf2Rows) sA[tid] = ra;
    __syncthreads();
    if (s + 1 < kw) load(s + 1);   // in flight under the lookups

    const uint32_t mine = sA[wave * kGf2WaveRows + (lane & 15)];   // the wavefront's 16 words of A, one per lane
    const uint32_t *tl = &sT[0][0][lane * 2];
    // (unrolled over rows and nibbles: a constant nibble position is what makes the index one scalar bit-field extract and
    // the table's base an immediate offset of the read.  A row's 8 reads are issued before the row before it is combined: 16
    // reads in flight, all the wait counter tracks, or every row would wait for a whole LDS round trip.)
    uint2 x[2][kGroups];
    auto lookup = [&](unsigned r) {
      const uint32_t a = __builtin_amdgcn_readlane(mine, r);
#pragma unroll
      for (unsigned g = 0; g < kGroups; ++g)
        x[r & 1][g] = *reinterpret_cast<const uint2 *>(tl + (g * 16 + ((a >> (4 * g)) & 15u)) * kGf2Words);
    };
    lookup(0);
#pragma unroll
    for (unsigned r = 0; r < kGf2WaveRows; ++r) {
      if (r + 1 < kGf2WaveRows) lookup(r + 1);
#pragma unroll
      for (unsigned g = 0; g < kGroups; ++g) {
        acc[r][0] ^= x[r & 1][g].x;
        acc[r][1] ^= x[r & 1][g].y;
      }
    }
  }

  const uint32_t m_tail = (M & 31) ? (1u << (M & 31)) - 1 : ~0u;   // C's padding is written 0
  const unsigned w = w0 + lane * 2;
  if (w >= mw) return;   // (no barrier follows)
#pragma unroll
  for (unsigned r = 0; r < kGf2WaveRows; ++r) {
    const unsigned row = row0 + wave * kGf2WaveRows + r;
    if (row >= N) break;
    uint32_t *cp = C + (size_t)row * ldc + w;
    if (w + 2 <= mw) {
      uint2 v = make_uint2(acc[r][0], acc[r][1]);
      if (seed) {
        const uint2 o = *reinterpret_cast<const uint2 *>(cp);
        v.x ^= o.x;
        v.y ^= o.y;
      }
      if (w + 2 == mw) v.y &= m_tail;
      *reinterpret_cast<uint2 *>(cp) = v;
    } else {   // the row's last word alone
      uint32_t v = acc[r][0];
      if (seed) v ^= cp[0];
      cp[0] = v & m_tail;
    }
  }
}

int launch_tile(hipStream_t s, const BitsProblem &p) {
  const unsigned tiles_w = ((p.m + 31) / 32 + kGf2Words - 1) / kGf2Words, tiles_r = (p.n + kGf2Rows - 1) / kGf2Rows;
  const unsigned long long grid = (unsigned long long)tiles_w * tiles_r * p.batch;
  if (grid > 0x7fffffffull) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(bits_gf2_tile_kernel, dim3((unsigned)grid), dim3(kGf2Threads), 0, s, p.a, p.b, p.c, p.n, p.k, p.m, p.lda,
                     p.ldb, p.ldc, tiles_w, tiles_w * tiles_r, p.stride_a, p.stride_b, p.stride_c, p.seed ? 1 : 0);
  return (int)hipGetLastError();
}

}  // namespace

bool bits_gf2_tile_serves(size_t ldb, size_t ldc) { return ldb % 2 == 0 && ldc % 2 == 0; }

int launch_bits_gf2(hipStream_t s, const BitsProblem &p, bool tile) {
  return tile ? launch_tile(s, p) : launch_gemm<1, false, true>(s, p);
}

}  // namespace mm
