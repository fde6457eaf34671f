// Min- and Max-reduced semiring GEMM with the witness (mm_gemm_argreduce_*): for every output (e, i, j)
//     acc = seeded ? C[e,i,j] : Reduce::identity();  idx = seeded ? I[e,i,j] : -1
//     for k ascending: s = Map(A[e,i,k], B[e,k,j]); if (Min: s < acc / Max: acc < s) { acc = s; idx = index_base + k; }
// which is Op<RED>::apply's select (std::min / std::max, mm_common.h) with the winning k recorded beside it: C is the
// k-ordered contract's value bit for bit, ties keep the smallest k, a NaN mapped value is never taken, a NaN seed is
// never replaced.  Two kernels, one per-output sequence, so the same bits:
//   * argreduce_tile_kernel: 128 x 128 outputs per 256-thread workgroup, 8 x 8 values plus 8 x 8 int32 indices per
//     thread in registers for the whole K loop; A and B k-slabs (BK = 16) staged through LDS k-major, the next slab's
//     global loads in flight (registers) while the current one is consumed.  Per (output, k): map, compare, select the
//     value, select the index (the wave-uniform k, which the compiler copies into a VGPR once per step: the VOP3 select
//     spends its one constant-bus read on the lane mask).  Needs K % 4 == 0, M % 4 == 0 (N % 4 for a K x N A), no And
//     map, 16-byte aligned operands -- what valu_tile_serves() serves -- and an element of at most 4 bytes: 8 x 8
//     8-byte values, their indices and the prefetch do not fit 256 VGPRs (the compiler spilled to AGPRs, and the kernel
//     ran slower than argreduce), so the 8-byte types are not instantiated here.
//     valu_tile_kernel's geometry: constants and Vec4 in mm_tile128.h, the staging written out here (why: that header).
//   * argreduce_kernel: 64 x 64 outputs per 256-thread workgroup, 4 x 4 per thread, fully predicated: any shape, any
//     element-aligned pointer, every map.  The parity anchor (MM_PATH_ORDERED always runs it).  Tile origin and staging:
//     mm_tile64.h.
// Both take the batch through the workgroup id (batched_tile()), and `seeded` at run time.
// BT (mm_gemm_argreduce_nt_*, "argreduce_tile_nt" / "argreduce_nt"): B is stored M x K row-major (Bt[j][k]), which is A's
// N x K geometry, so it is fetched and staged as that branch stages A (argreduce_kernel: tile64_stage's k-contiguous
// mapping) -- into the same k-major Bs.  The LDS read side and
// the per-(output, k) sequence are untouched: the bits are those of the row-major kernel on a materialised transpose.
// BT = false compiles to what it did before the flag existed (profiles/nt_products_isa_identity.txt).
// Included once per element-type group (mm_argreduce_*.hip) to keep compile units parallel; every unit says
// `#pragma clang fp contract(off)` before including this: the map is one rounded operation, like Naive's.
#include "mm_tile128.h"
#include "mm_tile64.h"

namespace mm {
namespace {

// true when the mapped value s replaces acc (the select of Op<RED, T>::apply(acc, s))
template <int RED, typename T> __device__ __forceinline__ bool ar_takes(T s, T acc) {
  if constexpr (RED == MM_OP_MIN) return s < acc;
  else return acc < s;
}

// where the tile kernel's chains start: the value no mapped value loses to except NaN
template <int RED, typename T> __device__ __forceinline__ T ar_start() {
  if constexpr (std::is_floating_point<T>::value || std::is_same<T, half_t>::value)
    return RED == MM_OP_MIN ? (T)__builtin_inff() : (T)-__builtin_inff();
  else return Op<RED, T>::identity();
}

template <typename T, int MAP, int RED, bool AT, bool BT>
__global__ __launch_bounds__(256) void argreduce_tile_kernel(const T *__restrict__ A, const T *__restrict__ B,
                                                             T *__restrict__ C, int *__restrict__ I, unsigned N, unsigned K,
                                                             unsigned M, unsigned tiles_n, unsigned tiles_m, unsigned kBand,
                                                             unsigned batch, size_t stride_a, size_t stride_b,
                                                             size_t stride_c, int index_base, int seeded) {
  __shared__ __attribute__((aligned(16))) T As[kBK128][kTile128 + kPad128];
  __shared__ __attribute__((aligned(16))) T Bs[kBK128][kTile128 + kPad128];
  using V = Vec4<T>;
  using VI = Vec4<int>;
  const unsigned tid = threadIdx.x, tx = tid % 16, ty = tid / 16;
  // batched_tile()'s (element, tile) decomposition, with I moved by the element like C (same element strides)
  const unsigned tiles = tiles_n * tiles_m;
  const unsigned g = xcd_remap(blockIdx.x, tiles * batch), e = g / tiles, lin = g - e * tiles;
  A += e * stride_a;
  B += e * stride_b;
  C += e * stride_c;
  I += e * stride_c;
  unsigned row0, col0;
  band_origin(lin, tiles_n, tiles_m, kBand, kTile128, kTile128, row0, col0);

  // The chain runs from `start` (Min: +inf, Max: -inf for floating types; identity() for integers) with no index, and
  // the seed (C and I, or identity() and -1) is merged in at the store: the chain from the seed S takes the first k of the
  // least mapped value v when v < S (a NaN S, or a NaN v, takes nothing) and otherwise keeps S -- exactly what the chain
  // from `start` found, merged by "v < S ? (v, k) : (S, I)" (Max: S < v).  Same values, same indices, and no C or I
  // address lives across the K loop.
  T acc[8][8];
  int idx[8][8];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      acc[i][j] = ar_start<RED, T>();
      idx[i][j] = -1;
    }

  // slab k0's global loads (K % 4 == 0: a 4-wide k chunk is entirely inside or entirely outside)
  auto fetch_a = [&](unsigned k0, unsigned id) {
    V v = {};
    if (AT) {   // A is K x N: rows of the tile are contiguous
      const unsigned kr = id / 32, r4 = (id % 32) * 4;
      if (k0 + kr < K && row0 + r4 < N) v = *(const V *)(A + (size_t)(k0 + kr) * N + row0 + r4);
    } else {    // A is N x K: 4 lanes cover one row's 16 k
      const unsigned r = id / 4, kc = (id % 4) * 4;
      if (row0 + r < N && k0 + kc < K) v = *(const V *)(A + (size_t)(row0 + r) * K + k0 + kc);
    }
    return v;
  };
  auto fetch_b = [&](unsigned k0, unsigned id) {
    V v = {};
    if (BT) {   // B is M x K: 4 lanes cover one column's 16 k, as for an N x K A
      const unsigned c = id / 4, kc = (id % 4) * 4;
      if (col0 + c < M && k0 + kc < K) v = *(const V *)(B + (size_t)(col0 + c) * K + k0 + kc);
    } else {
      const unsigned kr = id / 32, c4 = (id % 32) * 4;
      if (k0 + kr < K && col0 + c4 < M) v = *(const V *)(B + (size_t)(k0 + kr) * M + col0 + c4);
    }
    return v;
  };
  auto stage = [&](unsigned id, const V &a, const V &b) {
    if (AT) {
      *(V *)&As[id / 32][(id % 32) * 4] = a;
    } else {
      const unsigned r = id / 4, kc = (id % 4) * 4;
#pragma unroll
      for (int e = 0; e < 4; ++e) As[kc + e][r] = a.v[e];
    }
    if (BT) {
      const unsigned c = id / 4, kc = (id % 4) * 4;
#pragma unroll
      for (int e = 0; e < 4; ++e) Bs[kc + e][c] = b.v[e];
    } else {
      *(V *)&Bs[id / 32][(id % 32) * 4] = b;
    }
  };

  V ra0 = fetch_a(0, tid), ra1 = fetch_a(0, tid + 256), rb0 = fetch_b(0, tid), rb1 = fetch_b(0, tid + 256);
  stage(tid, ra0, rb0);
  stage(tid + 256, ra1, rb1);
  __syncthreads();
  for (unsigned k0 = 0; k0 < K; k0 += kBK128) {
    const bool more = k0 + kBK128 < K;
    if (more) {   // in flight under this slab's VALU work
      ra0 = fetch_a(k0 + kBK128, tid);
      ra1 = fetch_a(k0 + kBK128, tid + 256);
      rb0 = fetch_b(k0 + kBK128, tid);
      rb1 = fetch_b(k0 + kBK128, tid + 256);
    }
    const unsigned kmax = min((unsigned)kBK128, K - k0);
    const int kg0 = index_base + (int)k0;   // global k of the slab's first step; uniform
#pragma unroll 1
    for (unsigned kk = 0; kk < kmax; ++kk) {
      T a[8], b[8];
      *(V *)&a[0] = *(const V *)&As[kk][ty * 4];
      *(V *)&a[4] = *(const V *)&As[kk][64 + ty * 4];
      *(V *)&b[0] = *(const V *)&Bs[kk][tx * 4];
      *(V *)&b[4] = *(const V *)&Bs[kk][64 + tx * 4];
      const int kg = kg0 + (int)kk;
#pragma unroll
      for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const T s = Op<MAP, T>::apply(a[i], b[j]);
          const bool t = ar_takes<RED>(s, acc[i][j]);
          acc[i][j] = t ? s : acc[i][j];
          idx[i][j] = t ? kg : idx[i][j];
        }
    }
    __syncthreads();
    if (more) {
      stage(tid, ra0, rb0);
      stage(tid + 256, ra1, rb1);
      __syncthreads();
    }
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const unsigned r = row0 + (i < 4 ? ty * 4 + i : 64 + ty * 4 + (i - 4));
    if (r >= N) continue;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const unsigned c = col0 + h * 64 + tx * 4;
      if (c < M) {
        V v;
        VI w;
        if (seeded) {
          v = *(const V *)(C + (size_t)r * M + c);
          w = *(const VI *)(I + (size_t)r * M + c);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            v.v[e] = Op<RED, T>::identity();
            w.v[e] = -1;
          }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const bool t = ar_takes<RED>(acc[i][h * 4 + e], v.v[e]);
          v.v[e] = t ? acc[i][h * 4 + e] : v.v[e];
          w.v[e] = t ? idx[i][h * 4 + e] : w.v[e];
        }
        *(V *)(C + (size_t)r * M + c) = v;
        *(VI *)(I + (size_t)r * M + c) = w;
      }
    }
  }
}

template <typename T, int MAP, int RED, bool AT, bool BT>
__global__ __launch_bounds__(256) void argreduce_kernel(const T *__restrict__ A, const T *__restrict__ B, T *__restrict__ C,
                                                        int *__restrict__ I, unsigned N, unsigned K, unsigned M,
                                                        size_t stride_a, size_t stride_b, size_t stride_c, int index_base,
                                                        int seeded) {
  __shared__ T As[kBK][kTile + 1];  // [k][row], +1: column reads of a row-major source
  __shared__ T Bs[kBK][kTile + (BT ? 1 : 0)];   // [k][col]; BT: +1, staged as a row-major A is
  const unsigned tx = threadIdx.x % 16, ty = threadIdx.x / 16;
  unsigned row0, col0;
  I += tile64_origin<Form::Batched>(A, B, C, N, M, stride_a, stride_b, stride_c, row0, col0) * stride_c;   // I moves with C

  T acc[kPerThread][kPerThread];
  int idx[kPerThread][kPerThread];
#pragma unroll
  for (int i = 0; i < kPerThread; ++i) {
    const unsigned gr = row0 + ty * kPerThread + i;
#pragma unroll
    for (int j = 0; j < kPerThread; ++j) {
      const unsigned gc = col0 + tx + 16 * j;
      acc[i][j] = Op<RED, T>::identity();
      idx[i][j] = -1;
      if (seeded && gr < N && gc < M) {
        acc[i][j] = C[(size_t)gr * M + gc];
        idx[i][j] = I[(size_t)gr * M + gc];
      }
    }
  }

  for (unsigned k0 = 0; k0 < K; k0 += kBK) {
    tile64_stage<!AT>(As, A, row0, N, k0, K);   // A is N x K, or (AT) K x N
    tile64_stage<BT>(Bs, B, col0, M, k0, K);    // B is K x M, or (BT) M x K
    __syncthreads();
    const unsigned kmax = (K - k0) < (unsigned)kBK ? (K - k0) : (unsigned)kBK;
    for (unsigned kk = 0; kk < kmax; ++kk) {  // strictly ascending k
      T av[kPerThread], bv[kPerThread];
#pragma unroll
      for (int i = 0; i < kPerThread; ++i) av[i] = As[kk][ty * kPerThread + i];
#pragma unroll
      for (int j = 0; j < kPerThread; ++j) bv[j] = Bs[kk][tx + 16 * j];
      const int kg = index_base + (int)(k0 + kk);
#pragma unroll
      for (int i = 0; i < kPerThread; ++i)
#pragma unroll
        for (int j = 0; j < kPerThread; ++j) {
          const T s = Op<MAP, T>::apply(av[i], bv[j]);
          const bool tk = ar_takes<RED>(s, acc[i][j]);
          acc[i][j] = tk ? s : acc[i][j];
          idx[i][j] = tk ? kg : idx[i][j];
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
      if (gc < M) {
        C[(size_t)gr * M + gc] = acc[i][j];
        I[(size_t)gr * M + gc] = idx[i][j];
      }
    }
  }
}

// One launch of KERN for p's layouts.  BT (the unit's): the M x K B instantiation, else the N x K or the K x N A one -- a
// unit holds the kernels of one B layout (mm_argreduce_*.hip: K x M; mm_argreduce_nt_*.hip: M x K).
#define MM_AR_LAUNCH(KERN, GRID, ...)                                                                                  \
  do {                                                                                                                 \
    if constexpr (BT) hipLaunchKernelGGL((KERN<T, MAP, RED, false, true>), GRID, dim3(256), 0, s, __VA_ARGS__);        \
    else if (p.a_transposed) hipLaunchKernelGGL((KERN<T, MAP, RED, true, false>), GRID, dim3(256), 0, s, __VA_ARGS__); \
    else hipLaunchKernelGGL((KERN<T, MAP, RED, false, false>), GRID, dim3(256), 0, s, __VA_ARGS__);                    \
  } while (0)

template <typename T, int MAP, int RED, bool BT>
int ar_launch(hipStream_t s, const Problem &p, int *index, int index_base, bool tile) {
  const int seeded = p.seed ? 1 : 0;
  if (p.b_transposed != BT || (BT && p.a_transposed)) return kErrNotSupported;
  if (tile) {
    if constexpr (MAP == MM_OP_AND || sizeof(T) > 4) {
      return kErrNotSupported;
    } else {
      const unsigned tiles_n = (p.n + kTile128 - 1) / kTile128, tiles_m = (p.m + kTile128 - 1) / kTile128;
      MM_AR_LAUNCH(argreduce_tile_kernel, dim3(tiles_n * tiles_m * p.batch), (const T *)p.a, (const T *)p.b, (T *)p.c, index,
                   p.n, p.k, p.m, tiles_n, tiles_m, band_rows(), p.batch, p.stride_a, p.stride_b, p.stride_c, index_base,
                   seeded);
      return (int)hipGetLastError();
    }
  }
  const unsigned tiles = ((p.m + kTile - 1) / kTile) * ((p.n + kTile - 1) / kTile);
  MM_AR_LAUNCH(argreduce_kernel, dim3(tiles * p.batch), (const T *)p.a, (const T *)p.b, (T *)p.c, index, p.n, p.k, p.m,
               p.stride_a, p.stride_b, p.stride_c, index_base, seeded);
  return (int)hipGetLastError();
}
#undef MM_AR_LAUNCH

// TYPES: the element types the including unit instantiates; BT: for an M x K B (mm_argreduce_nt_*.hip)
template <typename TYPES, bool BT = false>
int ar_dispatch(hipStream_t s, const mm_config_t &cfg, const Problem &p, int *index, int index_base, bool tile) {
  return switch_config<TYPES, AllOps, MinMaxOps>(cfg, [&](auto t, auto map, auto red) {
    return ar_launch<type_of<decltype(t)>, decltype(map)::value, decltype(red)::value, BT>(s, p, index, index_base, tile);
  });
}

}  // namespace
}  // namespace mm
