// Bit-packed Boolean semiring (mm_bits_gemm_*, mm_bits_pack_*, mm_bits_unpack_*; the format: include/mm_gemm.h):
// C = OR_k (A AND B) on one bit per element, 32 columns per word, and the conversions from and to one byte per element.
#include "mm_common.h"

namespace mm {
namespace {

#include "mm_bits_product.inc"   // bits_gemm_kernel<W, VEC, XOR>, launch_gemm<W, VEC, XOR>; kThreads

// One wavefront per 64 columns of a row: a lane tests one byte, the ballot is the two words.  Bytes at columns >= cols are
// not read and count as 0, so the padding bits are written 0.
__global__ __launch_bounds__(kThreads) void bits_pack_kernel(const uint8_t *__restrict__ src, uint32_t *__restrict__ dst,
                                                             unsigned rows, unsigned cols, size_t ld_src, size_t ld_dst,
                                                             unsigned chunks, unsigned long long total, size_t stride_src,
                                                             size_t stride_dst) {
  const unsigned lane = threadIdx.x & 63, words = (cols + 31) / 32;
  const unsigned long long step = (unsigned long long)gridDim.x * (kThreads / 64);
  for (unsigned long long g = (unsigned long long)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6); g < total; g += step) {
    const unsigned chunk = (unsigned)(g % chunks);
    const unsigned long long er = g / chunks;
    const unsigned row = (unsigned)(er % rows);
    const size_t e = (size_t)(er / rows);
    const unsigned col = chunk * 64 + lane;
    const bool on = col < cols && src[e * stride_src + (size_t)row * ld_src + col] != 0;
    const unsigned long long m = __ballot(on);
    const unsigned word = chunk * 2 + lane;
    if (lane < 2 && word < words) dst[e * stride_dst + (size_t)row * ld_dst + word] = (uint32_t)(m >> (32 * lane));
  }
}

__global__ __launch_bounds__(kThreads) void bits_unpack_kernel(const uint32_t *__restrict__ src, uint8_t *__restrict__ dst,
                                                               unsigned rows, unsigned cols, size_t ld_src, size_t ld_dst,
                                                               unsigned long long total, size_t stride_src, size_t stride_dst) {
  const unsigned long long step = (unsigned long long)gridDim.x * kThreads;
  for (unsigned long long g = (unsigned long long)blockIdx.x * kThreads + threadIdx.x; g < total; g += step) {
    const unsigned col = (unsigned)(g % cols);
    const unsigned long long er = g / cols;
    const unsigned row = (unsigned)(er % rows);
    const size_t e = (size_t)(er / rows);
    const uint32_t word = src[e * stride_src + (size_t)row * ld_src + (col >> 5)];
    dst[e * stride_dst + (size_t)row * ld_dst + col] = (uint8_t)((word >> (col & 31)) & 1u);
  }
}

constexpr unsigned long long kMaxGrid = 1ull << 20;   // workgroups of a conversion launch; the kernels stride over the rest

}  // namespace

bool bits_tile_serves(size_t ldb, size_t ldc) { return ldb % 4 == 0 && ldc % 2 == 0; }

int launch_bits_gemm(hipStream_t s, const BitsProblem &p, bool tile) {
  return tile ? launch_gemm<2, true, false>(s, p) : launch_gemm<1, false, false>(s, p);
}

int launch_bits_pack(hipStream_t s, const BitsConvert &c) {
  const unsigned chunks = (c.cols + 63) / 64;
  const unsigned long long total = (unsigned long long)c.batch * c.rows * chunks;   // wavefronts of work
  const unsigned long long blocks = (total + kThreads / 64 - 1) / (kThreads / 64);
  hipLaunchKernelGGL(bits_pack_kernel, dim3((unsigned)(blocks < kMaxGrid ? blocks : kMaxGrid)), dim3(kThreads), 0, s,
                     (const uint8_t *)c.src, (uint32_t *)c.dst, c.rows, c.cols, c.ld_src, c.ld_dst, chunks, total, c.stride_src,
                     c.stride_dst);
  return (int)hipGetLastError();
}

int launch_bits_unpack(hipStream_t s, const BitsConvert &c) {
  const unsigned long long total = (unsigned long long)c.batch * c.rows * c.cols;   // bytes to write
  const unsigned long long blocks = (total + kThreads - 1) / kThreads;
  hipLaunchKernelGGL(bits_unpack_kernel, dim3((unsigned)(blocks < kMaxGrid ? blocks : kMaxGrid)), dim3(kThreads), 0, s,
                     (const uint32_t *)c.src, (uint8_t *)c.dst, c.rows, c.cols, c.ld_src, c.ld_dst, total, c.stride_src,
                     c.stride_dst);
  return (int)hipGetLastError();
}

}  // namespace mm
