// int8_t -> int widening (mm_gemm_widen_*): the int8 matrix-core kernels of mm_mfma_i8_kernels.inc instantiated with an int C.
// Same kernel, same schedule as the narrow launch -- the one mfma_i8_batched_name() names for the shape -- with the epilogue
// that stores the i32 accumulators instead of their low 8 bits (mm_common.h: wide_store_*).  The sums are exact mod 2^32 on
// every kernel.  A unit of its own: mm_mfma_i8.hip is replaced as a whole in the lab library, whose resolver names no kernel
// of this table, so widening calls there run widen_ordered.
#include <cstring>
#include <type_traits>   // std::integral_constant in the kernels

#include "mm_common.h"

namespace mm {
namespace {

#include "mm_mfma_i8_kernels.inc"
#undef MM_DMA_PIECE

// narrow name (what mfma_i8_batched_name returns) -> the wide instantiation's
const char *const kNarrow[] = {"mfma_i8_256x256_pingpong_16x16x64", "mfma_i8_256x256_pingpong_32x32x32", "mfma_i8_256x256_pingpong_k64",
                               "mfma_i8_256x256_pingpong_k64_KxN", "mfma_i8_256x256x128_slab128", "mfma_i8_256x256x128_slab128_KxN",
                               "mfma_i8_64x256x128_slab128"};
const char *const kWide[] = {"mfma_i8_256x256_pingpong_16x16x64_wide", "mfma_i8_256x256_pingpong_32x32x32_wide",
                             "mfma_i8_256x256_pingpong_k64_wide", "mfma_i8_256x256_pingpong_k64_KxN_wide",
                             "mfma_i8_256x256x128_slab128_wide", "mfma_i8_256x256x128_slab128_KxN_wide",
                             "mfma_i8_64x256x128_slab128_wide"};
constexpr int kCount = sizeof(kNarrow) / sizeof(kNarrow[0]);

template <Form F>
int launch_index(hipStream_t s, const Problem &p, int k) {
  switch (k) {
    case 0: return launch_tile<F, mfma_i8_pp2s_kernel<F, int>, int>(s, p, GeoI8PP2::THREADS, GeoI8PP2::LDS_BYTES);
    case 1: return launch_tile<F, mfma_i8_pp2_kernel<F, int>, int>(s, p, GeoI8PP2::THREADS, GeoI8PP2::LDS_BYTES);
    case 2: return launch_tile<F, mfma_i8_pp_kernel<F, false, int>, int>(s, p, GeoI8PP::THREADS, GeoI8PP::LDS_BYTES);
    case 3: return launch_tile<F, mfma_i8_pp_kernel<F, true, int>, int>(s, p, GeoI8PP::THREADS, GeoI8PP::LDS_BYTES);
    case 4: return launch_tile<F, mfma_i8_kernel<F, GeoI8, false, int>, int>(s, p, GeoI8::THREADS, GeoI8::LDS_BYTES);
    case 5: return launch_tile<F, mfma_i8_kernel<F, GeoI8, true, int>, int>(s, p, GeoI8::THREADS, GeoI8::LDS_BYTES);
    case 6: return launch_tile<F, mfma_i8_kernel<F, GeoI8S, false, int>, int>(s, p, GeoI8S::THREADS, GeoI8S::LDS_BYTES, GeoI8S::BM);
    default: return kErrNotSupported;
  }
}

}  // namespace

int mfma_i8_wide_resolve(const Problem &p) {
  const char *narrow = mfma_i8_batched_name(p);
  for (int k = 0; k < kCount; ++k)
    if (strcmp(narrow, kNarrow[k]) == 0) return k;
  return -1;
}
const char *mfma_i8_wide_name(const Problem &p) { const int k = mfma_i8_wide_resolve(p); return k < 0 ? nullptr : kWide[k]; }
int launch_mfma_i8_wide(hipStream_t s, const Problem &p, int k) {
  return p.seed ? launch_index<Form::Seeded>(s, p, k) : launch_index<Form::Batched>(s, p, k);
}

}  // namespace mm
