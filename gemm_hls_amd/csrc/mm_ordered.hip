// MM_PATH_ORDERED ("hw_emu"): the plain gfx950 kernel that evaluates each output element the way
// the reference's Naive does (include/Utility.h:18-42):
//     acc = Reduce::identity(); for k = 0..K-1: acc = Reduce(acc, Map(A[n,k], B[k,m]))
// one accumulator, k ascending, multiply and add as two separately rounded operations (this file
// is compiled with -ffp-contract=off), binary16 accumulating in binary16.  Bit-identical to the
// reference for every dtype and every (map, reduce); fully predicated, any N, K, M.
// LDS-tiled (64 x 64 outputs per 256-thread workgroup, 4 x 4 per thread) so that it is usable
// for verification at real sizes, but it is the parity anchor, not the fast path.
#include "mm_common.h"

namespace mm {
namespace {

constexpr int kTile = 64;   // outputs per workgroup edge
constexpr int kBK = 16;     // k-slab staged through LDS
constexpr int kPerThread = 4;

// ACC is the accumulator type: T itself for the Naive contract; float for the one exception,
// half (Multiply, Add) under MM_PATH_AUTO on shapes the matrix-core kernel does not take
// ("ordered_wide_f16": exact products, f32 accumulation, ONE rounding to binary16 on store -- the
// same contract as mfma_f16, so the AUTO path's half semantics do not change with the shape).
template <typename T, int MAP, int RED, bool AT, typename ACC = T>
__global__ __launch_bounds__(256) void ordered_kernel(const T *__restrict__ A, const T *__restrict__ B,
                                                      T *__restrict__ C, unsigned N, unsigned K,
                                                      unsigned M) {
#define MM_ORDERED_BATCHED 0
#include "mm_ordered_body.inc"
#undef MM_ORDERED_BATCHED
}

// `p.batch` elements of one shape in one launch: a 1-D grid of batch x tiles workgroups, element-major
template <typename T, int MAP, int RED, bool AT, typename ACC = T>
__global__ __launch_bounds__(256) void ordered_batched_kernel(const T *__restrict__ A, const T *__restrict__ B,
                                                              T *__restrict__ C, unsigned N, unsigned K, unsigned M,
                                                              size_t stride_a, size_t stride_b, size_t stride_c) {
#define MM_ORDERED_BATCHED 1
#include "mm_ordered_body.inc"
#undef MM_ORDERED_BATCHED
}

// accumulate (p.seed): ordered_batched_kernel whose chains start at the value C holds instead of identity()
template <typename T, int MAP, int RED, bool AT, typename ACC = T>
__global__ __launch_bounds__(256) void ordered_batched_seeded_kernel(const T *__restrict__ A, const T *__restrict__ B,
                                                                     T *__restrict__ C, unsigned N, unsigned K, unsigned M,
                                                                     size_t stride_a, size_t stride_b, size_t stride_c) {
#define MM_ORDERED_BATCHED 1
#define MM_ORDERED_SEEDED 1
#include "mm_ordered_body.inc"
#undef MM_ORDERED_SEEDED
#undef MM_ORDERED_BATCHED
}

// BATCHED: the p.batch elements of p (strides p.stride_*) in one launch of ordered_batched_kernel (p.seed: its seeded form)
template <typename T, int MAP, int RED, bool BATCHED, typename ACC = T>
int launch_t(hipStream_t s, const Problem &p) {
  if (p.n == 0 || p.m == 0) return 0;
  if constexpr (BATCHED) {
    const unsigned tiles = ((p.m + kTile - 1) / kTile) * ((p.n + kTile - 1) / kTile);
    if (p.seed) {
      if (p.a_transposed)
        hipLaunchKernelGGL((ordered_batched_seeded_kernel<T, MAP, RED, true, ACC>), dim3(tiles * p.batch), dim3(256), 0, s,
                           (const T *)p.a, (const T *)p.b, (T *)p.c, p.n, p.k, p.m, p.stride_a, p.stride_b, p.stride_c);
      else
        hipLaunchKernelGGL((ordered_batched_seeded_kernel<T, MAP, RED, false, ACC>), dim3(tiles * p.batch), dim3(256), 0, s,
                           (const T *)p.a, (const T *)p.b, (T *)p.c, p.n, p.k, p.m, p.stride_a, p.stride_b, p.stride_c);
      return (int)hipGetLastError();
    }
    if (p.a_transposed)
      hipLaunchKernelGGL((ordered_batched_kernel<T, MAP, RED, true, ACC>), dim3(tiles * p.batch), dim3(256), 0, s,
                         (const T *)p.a, (const T *)p.b, (T *)p.c, p.n, p.k, p.m, p.stride_a, p.stride_b, p.stride_c);
    else
      hipLaunchKernelGGL((ordered_batched_kernel<T, MAP, RED, false, ACC>), dim3(tiles * p.batch), dim3(256), 0, s,
                         (const T *)p.a, (const T *)p.b, (T *)p.c, p.n, p.k, p.m, p.stride_a, p.stride_b, p.stride_c);
    return (int)hipGetLastError();
  }
  dim3 grid((p.m + kTile - 1) / kTile, (p.n + kTile - 1) / kTile);
  if (p.a_transposed)
    hipLaunchKernelGGL((ordered_kernel<T, MAP, RED, true>), grid, dim3(256), 0, s, (const T *)p.a,
                       (const T *)p.b, (T *)p.c, p.n, p.k, p.m);
  else
    hipLaunchKernelGGL((ordered_kernel<T, MAP, RED, false>), grid, dim3(256), 0, s, (const T *)p.a,
                       (const T *)p.b, (T *)p.c, p.n, p.k, p.m);
  return (int)hipGetLastError();
}

template <typename T, int MAP, bool BATCHED>
int launch_red(hipStream_t s, int red, const Problem &p) {
  switch (red) {
    case MM_OP_ADD: return launch_t<T, MAP, MM_OP_ADD, BATCHED>(s, p);
    case MM_OP_MULTIPLY: return launch_t<T, MAP, MM_OP_MULTIPLY, BATCHED>(s, p);
    case MM_OP_AND: return launch_t<T, MAP, MM_OP_AND, BATCHED>(s, p);
    case MM_OP_MIN: return launch_t<T, MAP, MM_OP_MIN, BATCHED>(s, p);
    case MM_OP_MAX: return launch_t<T, MAP, MM_OP_MAX, BATCHED>(s, p);
  }
  return kErrNotSupported;
}

template <typename T, bool BATCHED>
int launch_map(hipStream_t s, const mm_config_t &cfg, const Problem &p) {
  switch (cfg.map_op) {
    case MM_OP_ADD: return launch_red<T, MM_OP_ADD, BATCHED>(s, cfg.reduce_op, p);
    case MM_OP_MULTIPLY: return launch_red<T, MM_OP_MULTIPLY, BATCHED>(s, cfg.reduce_op, p);
    case MM_OP_AND: return launch_red<T, MM_OP_AND, BATCHED>(s, cfg.reduce_op, p);
    case MM_OP_MIN: return launch_red<T, MM_OP_MIN, BATCHED>(s, cfg.reduce_op, p);
    case MM_OP_MAX: return launch_red<T, MM_OP_MAX, BATCHED>(s, cfg.reduce_op, p);
  }
  return kErrNotSupported;
}

template <bool BATCHED>
int launch_type(hipStream_t s, const mm_config_t &cfg, const Problem &p) {
  switch (cfg.dtype) {
    case MM_DTYPE_F32: return launch_map<float, BATCHED>(s, cfg, p);
    case MM_DTYPE_F64: return launch_map<double, BATCHED>(s, cfg, p);
    case MM_DTYPE_F16: return launch_map<half_t, BATCHED>(s, cfg, p);
    case MM_DTYPE_I8: return launch_map<int8_t, BATCHED>(s, cfg, p);
    case MM_DTYPE_U8: return launch_map<uint8_t, BATCHED>(s, cfg, p);
    case MM_DTYPE_I16: return launch_map<int16_t, BATCHED>(s, cfg, p);
    case MM_DTYPE_U16: return launch_map<uint16_t, BATCHED>(s, cfg, p);
    case MM_DTYPE_I32: return launch_map<int32_t, BATCHED>(s, cfg, p);
    case MM_DTYPE_U32: return launch_map<uint32_t, BATCHED>(s, cfg, p);
    case MM_DTYPE_I64: return launch_map<int64_t, BATCHED>(s, cfg, p);
    case MM_DTYPE_U64: return launch_map<uint64_t, BATCHED>(s, cfg, p);
  }
  return kErrNotSupported;
}

}  // namespace

int launch_half_wide(hipStream_t s, const Problem &p) {
  if (p.n == 0 || p.m == 0) return 0;
  dim3 grid((p.m + kTile - 1) / kTile, (p.n + kTile - 1) / kTile);
  if (p.a_transposed)
    hipLaunchKernelGGL((ordered_kernel<half_t, MM_OP_MULTIPLY, MM_OP_ADD, true, float>), grid, dim3(256), 0, s,
                       (const half_t *)p.a, (const half_t *)p.b, (half_t *)p.c, p.n, p.k, p.m);
  else
    hipLaunchKernelGGL((ordered_kernel<half_t, MM_OP_MULTIPLY, MM_OP_ADD, false, float>), grid, dim3(256), 0, s,
                       (const half_t *)p.a, (const half_t *)p.b, (half_t *)p.c, p.n, p.k, p.m);
  return (int)hipGetLastError();
}

int launch_ordered(hipStream_t s, const mm_config_t &cfg, const Problem &p) { return launch_type<false>(s, cfg, p); }
int launch_ordered_batched(hipStream_t s, const mm_config_t &cfg, const Problem &p) { return launch_type<true>(s, cfg, p); }
int launch_half_wide_batched(hipStream_t s, const Problem &p) {
  return launch_t<half_t, MM_OP_MULTIPLY, MM_OP_ADD, true, float>(s, p);
}

}  // namespace mm
