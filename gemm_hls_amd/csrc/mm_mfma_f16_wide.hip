// half -> float widening (mm_gemm_widen_*): the f16 matrix-core kernels of mm_mfma_f16_kernels.inc instantiated with a float C.
// Same kernel, same schedule as the narrow launch -- the one mfma_f16_batched_name() names for the shape -- with the epilogue
// that stores the f32 accumulators instead of rounding them to binary16 (mm_common.h: wide_store_*): rounding the plain
// form's C once gives the narrow launch's bits.  A unit of its own: mm_mfma_f16.hip is replaced as a whole in the lab
// library, whose resolver names no kernel of this table, so widening calls there run widen_ordered.
#include <cstring>
#include <type_traits>   // std::integral_constant in the kernels

#include "mm_common.h"

namespace mm {
namespace {

#include "mm_mfma_f16_kernels.inc"
#undef MM_DMA_PIECE

// narrow name (what mfma_f16_batched_name returns) -> the wide instantiation's
const char *const kNarrow[] = {"mfma_f16_256x256_pingpong_16x16x32", "mfma_f16_256x256_pingpong_32x32x16",
                               "mfma_f16_256x256_pingpong_k32", "mfma_f16_256x256_pingpong_k32_KxN",
                               "mfma_f16_256x256x64_slab64", "mfma_f16_256x256x64_slab64_KxN", "mfma_f16_128x256x64_slab64",
                               "mfma_f16_64x256x64_slab64"};
const char *const kWide[] = {"mfma_f16_256x256_pingpong_16x16x32_wide", "mfma_f16_256x256_pingpong_32x32x16_wide",
                             "mfma_f16_256x256_pingpong_k32_wide", "mfma_f16_256x256_pingpong_k32_KxN_wide",
                             "mfma_f16_256x256x64_slab64_wide", "mfma_f16_256x256x64_slab64_KxN_wide",
                             "mfma_f16_128x256x64_slab64_wide", "mfma_f16_64x256x64_slab64_wide"};
constexpr int kCount = sizeof(kNarrow) / sizeof(kNarrow[0]);

template <Form F>
int launch_index(hipStream_t s, const Problem &p, int k) {
  switch (k) {
    case 0: return launch_tile<F, mfma_f16_pp2s_kernel<F, float>, float>(s, p, 256, 256, GeoPP2::THREADS, GeoPP2::LDS_BYTES);
    case 1: return launch_tile<F, mfma_f16_pp2_kernel<F, float>, float>(s, p, 256, 256, GeoPP2::THREADS, GeoPP2::LDS_BYTES);
    case 2: return launch_tile<F, mfma_f16_pp_kernel<F, false, float>, float>(s, p, 256, 256, GeoPP::THREADS, GeoPP::LDS_BYTES);
    case 3: return launch_tile<F, mfma_f16_pp_kernel<F, true, float>, float>(s, p, 256, 256, GeoPP::THREADS, GeoPP::LDS_BYTES);
    case 4: return launch_tile<F, mfma_f16_kernel<F, GeoH, false, float>, float>(s, p, GeoH::BM, GeoH::BN, GeoH::THREADS, GeoH::LDS_BYTES);
    case 5: return launch_tile<F, mfma_f16_kernel<F, GeoH, true, float>, float>(s, p, GeoH::BM, GeoH::BN, GeoH::THREADS, GeoH::LDS_BYTES);
    case 6: return launch_tile<F, mfma_f16_kernel<F, GeoHS, false, float>, float>(s, p, GeoHS::BM, GeoHS::BN, GeoHS::THREADS, GeoHS::LDS_BYTES);
    case 7: return launch_tile<F, mfma_f16_kernel<F, GeoHXS, false, float>, float>(s, p, GeoHXS::BM, GeoHXS::BN, GeoHXS::THREADS, GeoHXS::LDS_BYTES);
    default: return kErrNotSupported;
  }
}

}  // namespace

int mfma_f16_wide_resolve(const Problem &p) {
  const char *narrow = mfma_f16_batched_name(p);
  for (int k = 0; k < kCount; ++k)
    if (strcmp(narrow, kNarrow[k]) == 0) return k;
  return -1;
}
const char *mfma_f16_wide_name(const Problem &p) { const int k = mfma_f16_wide_resolve(p); return k < 0 ? nullptr : kWide[k]; }
int launch_mfma_f16_wide(hipStream_t s, const Problem &p, int k) {
  return p.seed ? launch_index<Form::Seeded>(s, p, k) : launch_index<Form::Batched>(s, p, k);
}

}  // namespace mm
