// "ordered_nt": the parity anchor of the A x B^T calls (mm_gemm_nt_*).  mm_ordered.hip's 64 x 64 fully predicated kernel
// with B stored M x K row-major (Bt[j][k], k contiguous, like A):
//     acc = Reduce::identity() (or C[n,m] when seeded); for k = 0..K-1: acc = Reduce(acc, Map(A[n,k], Bt[m,k]))
// one accumulator, k ascending, multiply and add two separately rounded operations (this file is compiled with
// -ffp-contract=off): Naive (include/Utility.h:18-42) on the transposed operand, bit for bit, for every dtype and every
// (map, reduce); any N, K, M, any element-aligned pointer or stride.
// A kernel of its own beside mm_ordered.hip's (a flag threaded through that body would change what mm_ordered.hip compiles
// to); the geometry constants and the tile origin are mm_tile64.h's, the staging -- the k-contiguous mapping for A and Bt -- is here.
#include "mm_tile64.h"

namespace mm {
namespace {

// ACC: T for the Naive contract; float for half (Multiply, Add) under MM_PATH_AUTO where no matrix-core kernel serves (exact
// products, f32 accumulation, ONE rounding to binary16 on store: mfma_f16's contract, as "ordered_wide_f16" keeps it in the
// row-major calls).  F: Form::Batched or Form::Seeded (a single problem is a batch of one).
template <Form F, typename T, int MAP, int RED, typename ACC = T>
__global__ __launch_bounds__(256) void ordered_nt_kernel(const T *__restrict__ A, const T *__restrict__ Bt,
                                                         T *__restrict__ C, unsigned N, unsigned K, unsigned M,
                                                         size_t stride_a, size_t stride_b, size_t stride_c) {
  static_assert(F != Form::Single, "the A x B^T calls run the batched forms");
  __shared__ T As[kBK][kTile + 1];  // [k][row], +1: column reads of a row-major source
  __shared__ T Bs[kBK][kTile + 1];  // [k][col], +1: Bt is row-major in (col, k), staged as A is
  const unsigned tid = threadIdx.x;
  const unsigned tx = tid % 16, ty = tid / 16;
  unsigned row0, col0;
  tile64_origin<F>(A, Bt, C, N, M, stride_a, stride_b, stride_c, row0, col0);

  ACC acc[kPerThread][kPerThread];
#pragma unroll
  for (int i = 0; i < kPerThread; ++i)
#pragma unroll
    for (int j = 0; j < kPerThread; ++j) acc[i][j] = Op<RED, ACC>::identity();
  if constexpr (F == Form::Seeded) {
    // accumulate: the value C holds replaces identity() as the start of the chain
#pragma unroll
    for (int i = 0; i < kPerThread; ++i) {
      const unsigned gr = row0 + ty * kPerThread + i;
#pragma unroll
      for (int j = 0; j < kPerThread; ++j) {
        const unsigned gc = col0 + tx + 16 * j;
        if (gr < N && gc < M) acc[i][j] = (ACC)C[(size_t)gr * M + gc];
      }
    }
  }

  for (unsigned k0 = 0; k0 < K; k0 += kBK) {
    // stage A (64 rows x 16 k) and Bt (64 cols x 16 k), lanes along k (this kernel's own loop, not tile64_stage: DESIGN.md 3.13)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const unsigned kk = tid % 16, r = tid / 16 + 16 * i;
      const unsigned gr = row0 + r, gc = col0 + r, gk = k0 + kk;
      As[kk][r] = (gr < N && gk < K) ? A[(size_t)gr * K + gk] : (T)0;
      Bs[kk][r] = (gc < M && gk < K) ? Bt[(size_t)gc * K + gk] : (T)0;
    }
    __syncthreads();
    const unsigned kmax = (K - k0) < (unsigned)kBK ? (K - k0) : (unsigned)kBK;
    for (unsigned kk = 0; kk < kmax; ++kk) {  // strictly ascending k
      T av[kPerThread], bv[kPerThread];
#pragma unroll
      for (int i = 0; i < kPerThread; ++i) av[i] = As[kk][ty * kPerThread + i];
#pragma unroll
      for (int j = 0; j < kPerThread; ++j) bv[j] = Bs[kk][tx + 16 * j];
#pragma unroll
      for (int i = 0; i < kPerThread; ++i)
#pragma unroll
        for (int j = 0; j < kPerThread; ++j)
          acc[i][j] = Op<RED, ACC>::apply(acc[i][j], Op<MAP, ACC>::apply((ACC)av[i], (ACC)bv[j]));
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
      if (gc < M) C[(size_t)gr * M + gc] = (T)acc[i][j];
    }
  }
}

// One launch over the p.batch elements of p; p.seed: the chains start from C
template <typename T, int MAP, int RED, typename ACC = T>
int launch_t(hipStream_t s, const Problem &p) {
  if (p.n == 0 || p.m == 0 || p.batch == 0) return 0;
  const unsigned tiles_m = (p.m + kTile - 1) / kTile, tiles_n = (p.n + kTile - 1) / kTile;
  const dim3 grid(tiles_m * tiles_n * p.batch);
  if (p.seed)
    hipLaunchKernelGGL((ordered_nt_kernel<Form::Seeded, T, MAP, RED, ACC>), grid, dim3(256), 0, s, (const T *)p.a,
                       (const T *)p.b, (T *)p.c, p.n, p.k, p.m, p.stride_a, p.stride_b, p.stride_c);
  else
    hipLaunchKernelGGL((ordered_nt_kernel<Form::Batched, T, MAP, RED, ACC>), grid, dim3(256), 0, s, (const T *)p.a,
                       (const T *)p.b, (T *)p.c, p.n, p.k, p.m, p.stride_a, p.stride_b, p.stride_c);
  return (int)hipGetLastError();
}

}  // namespace

int launch_ordered_nt(hipStream_t s, const mm_config_t &cfg, const Problem &p) {
  return switch_config<AllTypes, AllOps, AllOps>(cfg, [&](auto t, auto map, auto red) {
    return launch_t<type_of<decltype(t)>, decltype(map)::value, decltype(red)::value>(s, p);
  });
}

int launch_half_wide_nt(hipStream_t s, const Problem &p) {
  return launch_t<half_t, MM_OP_MULTIPLY, MM_OP_ADD, float>(s, p);
}

}  // namespace mm
