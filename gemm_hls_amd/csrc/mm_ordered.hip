// MM_PATH_ORDERED ("hw_emu"): the plain gfx950 kernel that evaluates each output element the way
// the reference's Naive does (include/Utility.h:18-42):
//     acc = Reduce::identity(); for k = 0..K-1: acc = Reduce(acc, Map(A[n,k], B[k,m]))
// one accumulator, k ascending, multiply and add as two separately rounded operations (this file
// is compiled with -ffp-contract=off), binary16 accumulating in binary16.  Bit-identical to the
// reference for every dtype and every (map, reduce); fully predicated, any N, K, M.
// LDS-tiled (64 x 64 outputs per 256-thread workgroup, 4 x 4 per thread) so that it is usable
// for verification at real sizes, but it is the parity anchor, not the fast path.  The geometry constants and where the
// tile lies are mm_tile64.h's, shared with the other four kernels of this organisation.
#include "mm_tile64.h"

namespace mm {
namespace {

// ACC is the accumulator type: T itself for the Naive contract; float for the one exception,
// half (Multiply, Add) under MM_PATH_AUTO on shapes the matrix-core kernel does not take
// ("ordered_wide_f16": exact products, f32 accumulation, ONE rounding to binary16 on store -- the
// same contract as mfma_f16, so the AUTO path's half semantics do not change with the shape).
// F (mm_common.h): Form::Single is one problem on a 2-D grid of tiles; the batched forms run `p.batch` elements of one shape
// on a 1-D grid of batch x tiles workgroups, element-major, Form::Seeded with chains that start at the value C holds
// instead of identity().  Form::Single never reads the strides.
template <Form F, typename T, int MAP, int RED, bool AT, typename ACC = T>
__global__ __launch_bounds__(256) void ordered_kernel(const T *__restrict__ A, const T *__restrict__ B,
                                                      T *__restrict__ C, unsigned N, unsigned K, unsigned M,
                                                      size_t stride_a, size_t stride_b, size_t stride_c) {
  __shared__ T As[kBK][kTile + 1];  // [k][row], +1: column reads of a row-major source
  __shared__ T Bs[kBK][kTile];      // [k][col]
  const unsigned tid = threadIdx.x;
  const unsigned tx = tid % 16, ty = tid / 16;
  unsigned row0, col0;
  tile64_origin<F>(A, B, C, N, M, stride_a, stride_b, stride_c, row0, col0);

  ACC acc[kPerThread][kPerThread];
#pragma unroll
  for (int i = 0; i < kPerThread; ++i)
#pragma unroll
    for (int j = 0; j < kPerThread; ++j) acc[i][j] = Op<RED, ACC>::identity();
  if constexpr (F == Form::Seeded) {
    // accumulate: the value C holds replaces identity() as the start of the chain (Naive with acc = C[i][j]); the loads are
    // only consumed at the first k-step, so they are in flight while the first slab is staged
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

// One launch of ordered_kernel<F, ...>: the problem at (a, b, c), or (F != Form::Single) the p.batch elements of p
template <Form F, typename T, int MAP, int RED, bool AT, typename ACC>
int launch_at(hipStream_t s, const Problem &p) {
  const unsigned tiles_m = (p.m + kTile - 1) / kTile, tiles_n = (p.n + kTile - 1) / kTile;
  const dim3 grid = F == Form::Single ? dim3(tiles_m, tiles_n) : dim3(tiles_m * tiles_n * p.batch);
  hipLaunchKernelGGL((ordered_kernel<F, T, MAP, RED, AT, ACC>), grid, dim3(256), 0, s, (const T *)p.a, (const T *)p.b,
                     (T *)p.c, p.n, p.k, p.m, p.stride_a, p.stride_b, p.stride_c);
  return (int)hipGetLastError();
}

template <Form F, typename T, int MAP, int RED, typename ACC = T>
int launch_t(hipStream_t s, const Problem &p) {
  if (p.n == 0 || p.m == 0) return 0;
  return p.a_transposed ? launch_at<F, T, MAP, RED, true, ACC>(s, p) : launch_at<F, T, MAP, RED, false, ACC>(s, p);
}

template <Form F>
int launch_type(hipStream_t s, const mm_config_t &cfg, const Problem &p) {
  return switch_config<AllTypes, AllOps, AllOps>(cfg, [&](auto t, auto map, auto red) {
    return launch_t<F, type_of<decltype(t)>, decltype(map)::value, decltype(red)::value>(s, p);
  });
}

}  // namespace

int launch_half_wide(hipStream_t s, const Problem &p) {
  return launch_t<Form::Single, half_t, MM_OP_MULTIPLY, MM_OP_ADD, float>(s, p);
}

int launch_ordered(hipStream_t s, const mm_config_t &cfg, const Problem &p) { return launch_type<Form::Single>(s, cfg, p); }
// batched: the p.batch elements of p (strides p.stride_*) in one launch; p.seed: the chains start from C
int launch_ordered_batched(hipStream_t s, const mm_config_t &cfg, const Problem &p) {
  return p.seed ? launch_type<Form::Seeded>(s, cfg, p) : launch_type<Form::Batched>(s, cfg, p);
}
int launch_half_wide_batched(hipStream_t s, const Problem &p) {
  return p.seed ? launch_t<Form::Seeded, half_t, MM_OP_MULTIPLY, MM_OP_ADD, float>(s, p)
                : launch_t<Form::Batched, half_t, MM_OP_MULTIPLY, MM_OP_ADD, float>(s, p);
}

}  // namespace mm
