// Transposition pre-passes: dst[n][k] = src[k][n], out of place, for every element size.
//
// K x N -> N x K for 1- and 2-byte element types (MM_TRANSPOSED_A: the reference's ReadATransposed layout,
// kernel/Memory.cpp:205-261).  The half / int8 matrix-core kernels gather a K x N A slab out of
// LDS with twice the transpose-read instructions of a row-major one (24 instead of 16 LDS reads per wavefront and slab:
// every operand of v_mfma_*_16x16x* wants consecutive k of one row) and run 6-10 % behind the row-major kernels at every
// size.  The pre-pass moves N x K elements once in and once out -- O(N K) against the product's O(N K M) -- so for wide
// enough M it costs less than that: measured 3.5 % of the product at M = 16384, 2.2 % at 32768, 5 % at 6144-8192 for
// half (uint8: 3.4 / 2.1 / 8-11 %), against the K x N kernels' 7-15 % (profiles/r04b_kxn_prepass.txt,
// r04c_kxn_prepass_forced_small_m.txt); at 4096 the pass costs more than it returns.
// The product then runs the row-major default and gives ITS bits: a K x N call equals the row-major call.
//
// M x K -> K x M for every element size, strided over a batch (mm_gemm_nt_*, "nt_prepass": the matrix-core kernels read B
// as K x M).
//
// 128-byte x 128-byte element tiles through LDS: 16-byte loads along n (one request per line),
// element gather from LDS, 16-byte stores along k (one request per line).  Edges are predicated per 16-byte chunk
// (N and K are multiples of the chunk: 16 bytes' worth of elements -- guaranteed by the callers' serves() rules).
#include <algorithm>

#include "mm_common.h"

namespace mm {
namespace {

using u32x4 = __attribute__((ext_vector_type(4))) unsigned;

// Matrix blockIdx.y of the launch: src + y * stride_src -> dst + y * stride_dst (elements).
template <typename T>
__global__ __launch_bounds__(256) void transpose_kxn_small_kernel(const T *__restrict__ src, T *__restrict__ dst, unsigned K, unsigned N,
                                                                  size_t stride_src, size_t stride_dst) {
  constexpr unsigned ES = sizeof(T), EPC = 16 / ES, TS = 128 / ES;   // elements per 16-byte chunk; tile side (128 bytes)
  // LDS row pitch 132 B: a gathering wavefront reads 8 output chunks (k blocks EPC rows apart) x 8 columns per instruction;
  // EPC rows of 33 words put the k blocks 8 banks apart for 2-byte elements (conflict-free) and 16 apart for bytes (2-way);
  // 4-byte elements: 4 banks apart, each 32-lane half of the read (8 k blocks x 4 columns) on 32 distinct banks.
  // 8-byte elements need 8-byte aligned rows: 144 B = 36 words, k blocks (2 rows) 8 banks apart of the 64 a ds_read_b64
  // half sees, its 4 columns 2 banks each: conflict-free
  constexpr unsigned PITCH = ES == 8 ? 128 + 16 : 128 + 4;
  __shared__ __attribute__((aligned(16))) char tile[TS * PITCH];
  src += blockIdx.y * stride_src;
  dst += blockIdx.y * stride_dst;
  const unsigned blocks_n = (N + TS - 1) / TS;   // 1-D grid per matrix: either dimension may exceed the 65535 of gridDim.y
  const unsigned k0 = (blockIdx.x / blocks_n) * TS, n0 = (blockIdx.x % blocks_n) * TS;
  constexpr unsigned CHUNKS = TS * 8;             // 16-byte chunks in the tile (8-byte elements: 128, half the threads)
#pragma unroll
  for (unsigned i = 0; i < (CHUNKS + 255) / 256; ++i) {
    const unsigned c = threadIdx.x + 256 * i, kr = c >> 3, ch = c & 7u;
    if (CHUNKS % 256 != 0 && c >= CHUNKS) break;
    u32x4 v = (u32x4)0u;
    if (k0 + kr < K && n0 + ch * EPC < N) v = *(const u32x4 *)(src + (size_t)(k0 + kr) * N + n0 + ch * EPC);
#pragma unroll
    for (int j = 0; j < 4; ++j) *(unsigned *)(tile + kr * PITCH + ch * 16 + 4 * j) = v[j];   // rows are only 4-byte aligned
  }
  __syncthreads();
#pragma unroll
  for (unsigned i = 0; i < (CHUNKS + 255) / 256; ++i) {
    const unsigned c = threadIdx.x + 256 * i, kc = c & 7u, n = c >> 3;   // 8 lanes = the 128 bytes of one output row
    if (CHUNKS % 256 != 0 && c >= CHUNKS) break;
    union { T e[EPC]; u32x4 v; } out;
#pragma unroll
    for (unsigned j = 0; j < EPC; ++j) out.e[j] = *(const T *)(tile + (kc * EPC + j) * PITCH + n * ES);
    if (n0 + n < N && k0 + kc * EPC < K) *(u32x4 *)(dst + (size_t)(n0 + n) * K + k0 + kc * EPC) = out.v;
  }
}

template <typename T>
int launch_transpose_t(hipStream_t s, const void *src, void *dst, unsigned K, unsigned N, unsigned count, size_t stride_src,
                       size_t stride_dst) {
  constexpr unsigned TS = 128 / sizeof(T);
  const unsigned blocks = ((N + TS - 1) / TS) * ((K + TS - 1) / TS);
  for (unsigned e0 = 0; e0 < count; e0 += 65535u) {   // gridDim.y
    hipLaunchKernelGGL(transpose_kxn_small_kernel<T>, dim3(blocks, std::min(65535u, count - e0)), dim3(256), 0, s,
                       (const T *)src + (size_t)e0 * stride_src, (T *)dst + (size_t)e0 * stride_dst, K, N, stride_src, stride_dst);
    if (const int e = (int)hipGetLastError()) return e;
  }
  return 0;
}
}  // namespace

int launch_transpose_batched(hipStream_t s, const void *src, void *dst, unsigned K, unsigned N, unsigned elem_size, unsigned count,
                             size_t stride_src, size_t stride_dst) {
  (void)hipGetLastError();
  if (K == 0 || N == 0 || count == 0) return 0;
  switch (elem_size) {
    case 1: return launch_transpose_t<unsigned char>(s, src, dst, K, N, count, stride_src, stride_dst);
    case 2: return launch_transpose_t<unsigned short>(s, src, dst, K, N, count, stride_src, stride_dst);
    case 4: return launch_transpose_t<unsigned>(s, src, dst, K, N, count, stride_src, stride_dst);
    case 8: return launch_transpose_t<unsigned long long>(s, src, dst, K, N, count, stride_src, stride_dst);
    default: return kErrNotSupported;
  }
}

int launch_transpose_kxn(hipStream_t s, const void *src, void *dst, unsigned K, unsigned N, unsigned elem_size) {
  if (elem_size != 1 && elem_size != 2) return kErrNotSupported;
  return launch_transpose_batched(s, src, dst, K, N, elem_size, 1, 0, 0);
}

// K x N A through the pre-pass: worth it where the row-major default kernel serves the transposed problem and M is wide
// enough for the O(N K) pass to cost less than the K x N kernel's deficit: from M = 6144 (kxn_prepass_min_m overrides).
bool transposes_first_small(const Problem &p, unsigned elem_size) {
  const int knob = tuning(TUNE_KXN_PREPASS_MIN_M);
  const unsigned min_m = knob >= 0 ? (unsigned)knob : 6144u;   // measured: profiles/r04c_kxn_prepass_forced_small_m.txt
  return p.a_transposed && p.m >= min_m && p.n >= 1024 && (unsigned long long)p.n * p.k * elem_size <= (4ull << 30);
}

int launch_transposed_first(hipStream_t s, const Problem &p, unsigned elem_size, ProblemLauncher row_major, ProblemLauncher in_place) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return (int)e;
  hipMemPool_t pool = nullptr;
  if (int rc = workspace_pool(dev, &pool)) return rc;
  void *an = nullptr;
  if ((e = hipMallocFromPoolAsync(&an, (size_t)p.n * p.k * elem_size, pool, s)) != hipSuccess) {
    // no room for the N x K copy (up to 4 GiB next to a nearly full device): not an error -- the K x N kernels serve the
    // call without extra memory, as they did before the pre-pass existed; same contract, ~2-3 % slower
    (void)hipGetLastError();
    return in_place(s, p);
  }
  int rc = launch_transpose_kxn(s, p.a, an, p.k, p.n, elem_size);
  if (rc == 0) {
    Problem q = p;
    q.a = an;
    q.a_transposed = false;
    rc = row_major(s, q);
  }
  const hipError_t f = hipFreeAsync(an, s);
  return rc ? rc : (int)f;
}

}  // namespace mm
