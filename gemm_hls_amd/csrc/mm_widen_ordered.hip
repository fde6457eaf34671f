// "widen_ordered": the fallback of mm_gemm_widen_* -- int8_t operands to int sums, half operands to float sums -- one fully
// predicated kernel for both type pairs: any N, K, M, any element-aligned pointer or stride, row-major or K x N A.
//     acc = accumulate ? C : 0;  for k = 0 .. K-1: acc = acc + (W)a * (W)b        (W: the wide type)
// k ascending, one accumulator.  int: the product of two int8 values is exact and the sum wraps mod 2^32.  float: the product
// of two binary16 values is exact in f32, so the only roundings are the additions', in this order -- reproducible on the
// host with a float32 loop.  Compiled with -ffp-contract=off like mm_ordered.hip (and the pragma below says so again).
// Serves MM_PATH_ORDERED, the shapes the matrix-core kernels do not take, and operands that are not 16-byte aligned.
// BLOCKED (half under MM_PATH_AUTO where a matrix-core kernel was named but an operand is misaligned): the same terms summed
// in blocks -- 16 k into a partial sum, 64 partial sums into a middle one, the middle ones into the accumulator -- so that the
// longest chain of additions is 16 + 64 + K / 1024 instead of K and the result keeps the matrix-core kernels' bound of
// 1e-6 (|C_in| + |A||B|), which one accumulator over K terms does not (1.02e-6 measured at K = 512, growing with K).
// Organisation of mm_ordered.hip's kernel: 64 x 64 outputs per 256-thread workgroup through LDS, 4 x 4 per thread; the
// geometry constants and the tile origin are mm_tile64.h's.
#include "mm_tile64.h"

#pragma clang fp contract(off)

namespace mm {
namespace {

__device__ __forceinline__ int widen_mac(int acc, signed char a, signed char b) { return (int)((unsigned)acc + (unsigned)((int)a * (int)b)); }
__device__ __forceinline__ float widen_mac(float acc, _Float16 a, _Float16 b) { return acc + (float)a * (float)b; }

// F (mm_common.h): Form::Single is one problem on a 2-D grid of tiles; the batched forms run `batch` elements on a 1-D grid
// of batch x tiles workgroups, element-major; Form::Seeded starts every chain at the value C holds.
template <Form F, typename T, typename W, bool AT, bool BLOCKED = false>
__global__ __launch_bounds__(256) void widen_ordered_kernel(const T *__restrict__ A, const T *__restrict__ B, W *__restrict__ C,
                                                            unsigned N, unsigned K, unsigned M, size_t stride_a, size_t stride_b,
                                                            size_t stride_c) {
  __shared__ T As[kBK][kTile + 1];  // [k][row], +1: column reads of a row-major source
  __shared__ T Bs[kBK][kTile];      // [k][col]
  const unsigned tid = threadIdx.x;
  const unsigned tx = tid % 16, ty = tid / 16;
  unsigned row0, col0;
  tile64_origin<F>(A, B, C, N, M, stride_a, stride_b, stride_c, row0, col0);

  W acc[kPerThread][kPerThread];
#pragma unroll
  for (int i = 0; i < kPerThread; ++i)
#pragma unroll
    for (int j = 0; j < kPerThread; ++j) {
      const unsigned gr = row0 + ty * kPerThread + i, gc = col0 + tx + 16 * j;
      acc[i][j] = (W)0;
      if constexpr (F == Form::Seeded) {
        if (gr < N && gc < M) acc[i][j] = C[(size_t)gr * M + gc];
      }
    }

  W part[kPerThread][kPerThread], mid[kPerThread][kPerThread];   // BLOCKED only: this slab's sum, the sum of up to 64 slabs
  if constexpr (BLOCKED) {
#pragma unroll
    for (int i = 0; i < kPerThread; ++i)
#pragma unroll
      for (int j = 0; j < kPerThread; ++j) mid[i][j] = (W)0;
  }
  for (unsigned k0 = 0; k0 < K; k0 += kBK) {
    // stage A: 64 rows x 16 k (this kernel's own loops, not tile64_stage: DESIGN.md 3.13)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      unsigned r, kk;
      if (AT) { r = tid % 64; kk = tid / 64 + 4 * i; }   // A is K x N: consecutive lanes along N
      else    { kk = tid % 16; r = tid / 16 + 16 * i; }  // A is N x K: consecutive lanes along K
      const unsigned gr = row0 + r, gk = k0 + kk;
      T v = (T)0;
      if (gr < N && gk < K) v = AT ? A[(size_t)gk * N + gr] : A[(size_t)gr * K + gk];
      As[kk][r] = v;
    }
    // stage B: 16 k x 64 cols
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const unsigned c = tid % 64, kk = tid / 64 + 4 * i;
      const unsigned gc = col0 + c, gk = k0 + kk;
      Bs[kk][c] = (gc < M && gk < K) ? B[(size_t)gk * M + gc] : (T)0;
    }
    __syncthreads();
    const unsigned kmax = (K - k0) < (unsigned)kBK ? (K - k0) : (unsigned)kBK;
    W(&sum)[kPerThread][kPerThread] = BLOCKED ? part : acc;
    if constexpr (BLOCKED) {
#pragma unroll
      for (int i = 0; i < kPerThread; ++i)
#pragma unroll
        for (int j = 0; j < kPerThread; ++j) part[i][j] = (W)0;
    }
    for (unsigned kk = 0; kk < kmax; ++kk) {  // strictly ascending k
      T av[kPerThread], bv[kPerThread];
#pragma unroll
      for (int i = 0; i < kPerThread; ++i) av[i] = As[kk][ty * kPerThread + i];
#pragma unroll
      for (int j = 0; j < kPerThread; ++j) bv[j] = Bs[kk][tx + 16 * j];
#pragma unroll
      for (int i = 0; i < kPerThread; ++i)
#pragma unroll
        for (int j = 0; j < kPerThread; ++j) sum[i][j] = widen_mac(sum[i][j], av[i], bv[j]);
    }
    if constexpr (BLOCKED) {
      const bool flush = (k0 / kBK) % 64 == 63 || k0 + kBK >= K;   // uniform
#pragma unroll
      for (int i = 0; i < kPerThread; ++i)
#pragma unroll
        for (int j = 0; j < kPerThread; ++j) {
          mid[i][j] = mid[i][j] + part[i][j];
          if (flush) { acc[i][j] = acc[i][j] + mid[i][j]; mid[i][j] = (W)0; }
        }
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < kPerThread; ++i) {
    const unsigned gr = row0 + ty * kPerThread + i;
    if (gr >= N) continue;
#pragma unroll
    for (int j = 0; j < kPerThread; ++j) {
      const unsigned gc = col0 + tx + 16 * j;
      if (gc < M) C[(size_t)gr * M + gc] = acc[i][j];
    }
  }
}

template <typename T, typename W, bool AT, bool BLOCKED = false>
int launch_typed(hipStream_t s, const Problem &p) {
  const unsigned tiles_m = (p.m + kTile - 1) / kTile, tiles_n = (p.n + kTile - 1) / kTile;
  const T *a = (const T *)p.a, *b = (const T *)p.b;
  W *c = (W *)p.c;
  if (p.seed)
    hipLaunchKernelGGL((widen_ordered_kernel<Form::Seeded, T, W, AT, BLOCKED>), dim3(tiles_m * tiles_n * p.batch), dim3(256), 0, s, a, b, c,
                       p.n, p.k, p.m, p.stride_a, p.stride_b, p.stride_c);
  else if (p.batch > 1)
    hipLaunchKernelGGL((widen_ordered_kernel<Form::Batched, T, W, AT, BLOCKED>), dim3(tiles_m * tiles_n * p.batch), dim3(256), 0, s, a, b, c,
                       p.n, p.k, p.m, p.stride_a, p.stride_b, p.stride_c);
  else
    hipLaunchKernelGGL((widen_ordered_kernel<Form::Single, T, W, AT, BLOCKED>), dim3(tiles_m, tiles_n), dim3(256), 0, s, a, b, c, p.n, p.k,
                       p.m, (size_t)0, (size_t)0, (size_t)0);
  return (int)hipGetLastError();
}

}  // namespace

int launch_widen_ordered(hipStream_t s, mm_dtype_t dtype, const Problem &p, bool blocked) {
  if (dtype == MM_DTYPE_F16 && blocked)   // (int sums are exact in any order)
    return p.a_transposed ? launch_typed<_Float16, float, true, true>(s, p) : launch_typed<_Float16, float, false, true>(s, p);
  if (dtype == MM_DTYPE_I8) return p.a_transposed ? launch_typed<signed char, int, true>(s, p) : launch_typed<signed char, int, false>(s, p);
  if (dtype == MM_DTYPE_F16) return p.a_transposed ? launch_typed<_Float16, float, true>(s, p) : launch_typed<_Float16, float, false>(s, p);
  return kErrNotSupported;
}

}  // namespace mm
