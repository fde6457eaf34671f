// The wavefront kernel of the bit-packed transitive closure (mm_bits_closure_*): Warshall on one block of at most 64
// vertices, one row of 64 bits per lane, the pivot row by broadcast.  The on-chip closure (n <= 64) is this kernel alone; the
// blocked closure (mm_capi.hip) takes P | I from it and runs its panels and its rank-64 update on the product kernels.
#include "mm_common.h"

namespace mm {
namespace {

constexpr unsigned kThreads = 256;   // four graphs per workgroup

__global__ __launch_bounds__(kThreads) void bits_closure_diag_kernel(uint32_t *__restrict__ D, unsigned n, size_t ldd,
                                                                     unsigned graphs, size_t stride_d, unsigned k0,
                                                                     uint32_t *__restrict__ P, size_t stride_p) {
  const unsigned lane = threadIdx.x & 63, g = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  if (g >= graphs) return;   // the whole wavefront
  uint32_t *d = D + (size_t)g * stride_d;
  const unsigned bt = n - k0 < 64 ? n - k0 : 64, nw = (n + 31) / 32, w0 = k0 >> 5;   // k0 is a multiple of 64
  const bool two = w0 + 1 < nw;                                                       // the block's second word exists
  uint32_t lo = 0, hi = 0;
  if (lane < bt) {
    const uint32_t *row = d + (size_t)(k0 + lane) * ldd + w0;
    lo = row[0];
    if (two) hi = row[1];
  }
  // columns >= n are padding: ignored, and written 0
  const unsigned long long valid = bt == 64 ? ~0ull : (1ull << bt) - 1;
  lo &= (uint32_t)valid;
  hi &= (uint32_t)(valid >> 32);
  for (unsigned v = 0; v < bt; ++v) {
    const uint32_t plo = __builtin_amdgcn_readlane(lo, v), phi = __builtin_amdgcn_readlane(hi, v);
    const bool through = ((v < 32 ? lo >> v : hi >> (v - 32)) & 1u) != 0;
    if (through) {
      lo |= plo;
      hi |= phi;
    }
  }
  if (P) {   // P | I, 64 rows x 2 words; the rows beyond the block are 0
    if (lane < bt) {
      if (lane < 32) lo |= 1u << lane;
      else hi |= 1u << (lane - 32);
    }
    uint32_t *out = P + (size_t)g * stride_p + lane * 2;
    out[0] = lo;
    out[1] = hi;
  } else if (lane < bt) {
    uint32_t *row = d + (size_t)(k0 + lane) * ldd + w0;
    row[0] = lo;
    if (two) row[1] = hi;
  }
}

}  // namespace

int launch_bits_closure_diag(hipStream_t s, uint32_t *d, unsigned n, size_t ldd, unsigned graphs, size_t stride_d, unsigned k0,
                             uint32_t *pstar, size_t stride_p) {
  hipLaunchKernelGGL(bits_closure_diag_kernel, dim3((graphs + kThreads / 64 - 1) / (kThreads / 64)), dim3(kThreads), 0, s, d, n,
                     ldd, graphs, stride_d, k0, pstar, stride_p);
  return (int)hipGetLastError();
}

}  // namespace mm
