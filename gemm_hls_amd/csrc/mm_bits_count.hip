// Bit-packed counting products (mm_bits_count_*) and the packed transpose (mm_bits_transpose_*); the format: include/mm_gemm.h.
// C[i][j] = sum_k (A[i][k] op Bt[j][k]) as int32, op AND or XOR on single bits, both operands packed along k: one v_and_b32 /
// v_xor_b32 and one accumulating v_bcnt_u32_b32 per output and 32 k.
#include "mm_common.h"

namespace mm {
namespace {

constexpr unsigned kThreads = 256;   // 16 x 16 threads, each R x R outputs of a T x T tile (R = T / 16)
constexpr unsigned kSlab = 8;        // words of k per slab: 256 k

// One workgroup: T x T outputs.  Thread (ty, tx) owns rows (r / 4) * 64 + ty * 4 + r % 4 and columns (c / 4) * 64 + tx * 4 +
// c % 4: runs of 4, so that its operands are 16-byte LDS reads (16 lanes x 16 bytes side by side) and its rows of C 16-byte
// accesses.  Both operands lie row-major along k in memory and k-major in LDS (s[word][row]); the next slab's global loads
// stay in registers while the current slab is consumed.
// VEC: A and Bt in 16-byte loads and C in 16-byte accesses wherever a whole access lies inside the row (lda, ldbt, ldc % 4 ==
// 0, aligned bases and batch strides: the launcher's rule); everything else word by word.  Rows >= N or >= M, words >=
// ceil(K / 32), elements >= M of a row of C are predicated: no address outside an operand is formed.  Words out of range are
// staged as 0 and the last word of both operands is masked at staging, so padding counts 0 under both ops.
template <int T, bool VEC, bool XOR>
__global__ __launch_bounds__(kThreads, 4) void bits_count_kernel(const uint32_t *__restrict__ A, const uint32_t *__restrict__ Bt,
                                                              uint32_t *__restrict__ C, unsigned N, unsigned K, unsigned M,
                                                              size_t lda, size_t ldbt, size_t ldc, unsigned tiles_m,
                                                              unsigned tiles, size_t stride_a, size_t stride_bt,
                                                              size_t stride_c, int seed) {
  constexpr unsigned R = T / 16;                           // outputs per thread and dimension
  constexpr unsigned PER = VEC ? 4 : 1;                    // words per staging access
  constexpr unsigned RUN = kSlab / PER;                    // staging accesses per row and slab
  constexpr unsigned NL = T * RUN / kThreads;              // staging accesses per thread, operand and slab
  static_assert(R % 4 == 0 && T * RUN % kThreads == 0, "tile geometry");
  __shared__ __attribute__((aligned(16))) uint32_t sA[kSlab][T];
  __shared__ __attribute__((aligned(16))) uint32_t sB[kSlab][T];

  const unsigned tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const unsigned e = blockIdx.x / tiles, t = blockIdx.x - e * tiles;
  A += e * stride_a;
  Bt += e * stride_bt;
  C += e * stride_c;
  const unsigned row0 = (t / tiles_m) * T, col0 = (t % tiles_m) * T;
  const unsigned kw = (K + 31) / 32, slabs = (kw + kSlab - 1) / kSlab;
  const uint32_t k_tail = (K & 31) ? (1u << (K & 31)) - 1 : ~0u;   // padding of either operand never counts

  uint32_t acc[R][R];
#pragma unroll
  for (unsigned r = 0; r < R; ++r)
#pragma unroll
    for (unsigned c = 0; c < R; ++c) acc[r][c] = 0;

  uint32_t ra[NL][PER], rb[NL][PER];   // the next slab of A and of Bt on their way to LDS
  auto load_rows = [&](uint32_t (&reg)[NL][PER], const uint32_t *__restrict__ X, size_t ld, unsigned first, unsigned rows, unsigned s) {
#pragma unroll
    for (unsigned i = 0; i < NL; ++i) {
      const unsigned idx = tid + kThreads * i, row = first + idx / RUN, w = s * kSlab + (idx % RUN) * PER;
#pragma unroll
      for (unsigned j = 0; j < PER; ++j) reg[i][j] = 0;
      if (row >= rows || w >= kw) continue;
      const uint32_t *src = X + (size_t)row * ld + w;
      if (VEC && w + PER <= kw) {
        const uint4 v = *reinterpret_cast<const uint4 *>(src);
        reg[i][0] = v.x;
        if constexpr (PER == 4) { reg[i][1] = v.y; reg[i][2] = v.z; reg[i][3] = v.w; }
      } else {
#pragma unroll
        for (unsigned j = 0; j < PER; ++j)
          if (w + j < kw) reg[i][j] = src[j];
      }
#pragma unroll
      for (unsigned j = 0; j < PER; ++j)
        if (w + j == kw - 1) reg[i][j] &= k_tail;
    }
  };
  auto stage = [&](uint32_t (&dst)[kSlab][T], const uint32_t (&reg)[NL][PER]) {
#pragma unroll
    for (unsigned i = 0; i < NL; ++i) {
      const unsigned idx = tid + kThreads * i;
#pragma unroll
      for (unsigned j = 0; j < PER; ++j) dst[(idx % RUN) * PER + j][idx / RUN] = reg[i][j];
    }
  };

  if (slabs) {
    load_rows(ra, A, lda, row0, N, 0);
    load_rows(rb, Bt, ldbt, col0, M, 0);
  }
  for (unsigned s = 0; s < slabs; ++s) {
    __syncthreads();   // the previous slab has been read
    stage(sA, ra);
    stage(sB, rb);
    __syncthreads();
    if (s + 1 < slabs) {
      load_rows(ra, A, lda, row0, N, s + 1);
      load_rows(rb, Bt, ldbt, col0, M, s + 1);
    }
    const unsigned nw = min(kSlab, kw - s * kSlab);   // a short K does not pay for a whole slab
#pragma unroll 1   // (two words per trip let the compiler add their counts first: a fifth instruction per pair, twice the registers)
    for (unsigned w = 0; w < nw; ++w) {
      uint32_t a[R], b[R];
#pragma unroll
      for (unsigned h = 0; h < R / 4; ++h) {
        const uint4 va = *reinterpret_cast<const uint4 *>(&sA[w][h * 64 + ty * 4]);
        const uint4 vb = *reinterpret_cast<const uint4 *>(&sB[w][h * 64 + tx * 4]);
        a[4 * h] = va.x; a[4 * h + 1] = va.y; a[4 * h + 2] = va.z; a[4 * h + 3] = va.w;
        b[4 * h] = vb.x; b[4 * h + 1] = vb.y; b[4 * h + 2] = vb.z; b[4 * h + 3] = vb.w;
      }
#pragma unroll
      for (unsigned r = 0; r < R; ++r)
#pragma unroll
        for (unsigned c = 0; c < R; ++c) acc[r][c] += __popc(XOR ? a[r] ^ b[c] : a[r] & b[c]);
    }
  }

#pragma unroll
  for (unsigned r = 0; r < R; ++r) {
    const unsigned row = row0 + (r / 4) * 64 + ty * 4 + r % 4;
    if (row >= N) continue;
#pragma unroll
    for (unsigned h = 0; h < R / 4; ++h) {
      const unsigned col = col0 + h * 64 + tx * 4;
      if (col >= M) continue;
      uint32_t *cp = C + (size_t)row * ldc + col;
      if (VEC && col + 4 <= M) {
        uint4 v = make_uint4(acc[r][4 * h], acc[r][4 * h + 1], acc[r][4 * h + 2], acc[r][4 * h + 3]);
        if (seed) {   // mod 2^32, like the library's integer Add
          const uint4 o = *reinterpret_cast<const uint4 *>(cp);
          v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w;
        }
        *reinterpret_cast<uint4 *>(cp) = v;
        continue;
      }
#pragma unroll
      for (unsigned j = 0; j < 4; ++j) {
        if (col + j >= M) break;
        cp[j] = seed ? cp[j] + acc[r][4 * h + j] : acc[r][4 * h + j];
      }
    }
    __builtin_amdgcn_sched_barrier(0);   // row by row: the loads of a seeded C are not all hoisted above the first store
  }
}

template <int T, bool VEC, bool XOR>
int launch_count(hipStream_t s, const BitsProblem &p) {
  const unsigned tiles_m = (p.m + T - 1) / T, tiles_n = (p.n + T - 1) / T;
  const unsigned long long grid = (unsigned long long)tiles_m * tiles_n * p.batch;
  if (grid > 0x7fffffffull) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL((bits_count_kernel<T, VEC, XOR>), dim3((unsigned)grid), dim3(kThreads), 0, s, p.a, p.b, p.c, p.n, p.k, p.m,
                     p.lda, p.ldb, p.ldc, tiles_m, tiles_m * tiles_n, p.stride_a, p.stride_b, p.stride_c, p.seed ? 1 : 0);
  return (int)hipGetLastError();
}

// One wavefront per 64 source rows x one source word (32 columns): a lane loads the word of its row, ballot b is bit b of all
// 64 rows, i.e. two words of destination row 32 * word + b; lane b keeps ballot b and stores them.  Source rows >= rows are
// not read and count as 0, so the destination's padding bits are written 0; the source's last word is masked, so its padding
// never becomes a destination row.  Every destination word is written by exactly one lane.
__global__ __launch_bounds__(kThreads) void bits_transpose_kernel(const uint32_t *__restrict__ src, uint32_t *__restrict__ dst,
                                                                  unsigned rows, unsigned cols, size_t ld_src, size_t ld_dst,
                                                                  unsigned blocks, unsigned long long total, size_t stride_src,
                                                                  size_t stride_dst) {
  const unsigned lane = threadIdx.x & 63, cw = (cols + 31) / 32, rw = (rows + 31) / 32;
  const uint32_t c_tail = (cols & 31) ? (1u << (cols & 31)) - 1 : ~0u;
  const unsigned long long step = (unsigned long long)gridDim.x * (kThreads / 64);
  for (unsigned long long g = (unsigned long long)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6); g < total; g += step) {
    const unsigned blk = (unsigned)(g % blocks);          // 64 source rows
    const unsigned long long ew = g / blocks;
    const unsigned word = (unsigned)(ew % cw);            // 32 source columns
    const size_t e = (size_t)(ew / cw);
    const unsigned row = blk * 64 + lane;
    uint32_t v = row < rows ? src[e * stride_src + (size_t)row * ld_src + word] : 0u;
    if (word == cw - 1) v &= c_tail;
    unsigned long long mine = 0;
#pragma unroll
    for (unsigned b = 0; b < 32; ++b) {
      const unsigned long long m = __ballot((v >> b) & 1u);
      if (lane == b) mine = m;
    }
    const unsigned drow = word * 32 + lane;
    if (lane < 32 && drow < cols) {
      uint32_t *d = dst + e * stride_dst + (size_t)drow * ld_dst + blk * 2;
      d[0] = (uint32_t)mine;
      if (blk * 2 + 1 < rw) d[1] = (uint32_t)(mine >> 32);
    }
  }
}

constexpr unsigned long long kMaxGrid = 1ull << 20;   // workgroups of a transpose launch; the kernel strides over the rest

}  // namespace

bool bits_count_tile_serves(size_t lda, size_t ldbt, size_t ldc) { return lda % 4 == 0 && ldbt % 4 == 0 && ldc % 4 == 0; }

int launch_bits_count(hipStream_t s, const BitsProblem &p, bool xor_op, bool tile) {
  if (tile) return xor_op ? launch_count<128, true, true>(s, p) : launch_count<128, true, false>(s, p);
  return xor_op ? launch_count<64, false, true>(s, p) : launch_count<64, false, false>(s, p);
}

int launch_bits_transpose(hipStream_t s, const BitsConvert &c) {
  const unsigned blocks = (c.rows + 63) / 64;
  const unsigned long long total = (unsigned long long)c.batch * blocks * ((c.cols + 31) / 32);   // wavefronts of work
  const unsigned long long grid = (total + kThreads / 64 - 1) / (kThreads / 64);
  hipLaunchKernelGGL(bits_transpose_kernel, dim3((unsigned)(grid < kMaxGrid ? grid : kMaxGrid)), dim3(kThreads), 0, s,
                     (const uint32_t *)c.src, (uint32_t *)c.dst, c.rows, c.cols, c.ld_src, c.ld_dst, blocks, total, c.stride_src,
                     c.stride_dst);
  return (int)hipGetLastError();
}

}  // namespace mm
