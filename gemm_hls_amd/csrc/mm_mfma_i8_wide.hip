// int8_t -> int widening (mm_gemm_widen_*): the int8 matrix-core kernels of mm_mfma_i8_kernels.inc instantiated with an int C.
// Same kernel, same schedule as the narrow launch: the row of the include's table that mfma_i8_batched_resolve() picks for the
// shape, launched by the include's launch_kind with C's type.  Its epilogue stores the i32 accumulators instead of their low
// 8 bits (mm_common.h: wide_store_*).  The sums are exact mod 2^32 on every kernel.
// A unit of its own: mm_mfma_i8.hip is replaced as a whole in the lab library, whose resolver's indices are not this table's.
// An index counts only where the narrow unit's name for it is the row's, so widening calls there run widen_ordered.
#include <cstring>
#include <type_traits>   // std::integral_constant in the kernels

#include "mm_common.h"
#include "mm_pingpong2.h"

namespace mm {
namespace {

#include "mm_mfma_i8_kernels.inc"

}  // namespace

int mfma_i8_wide_resolve(const Problem &p) {
  const int k = mfma_i8_batched_resolve(p);
  return k >= 0 && k < (int)K_NONE && strcmp(mfma_i8_batched_name(p), kTable[k].name) == 0 ? k : -1;
}
const char *mfma_i8_wide_name(const Problem &p) { const int k = mfma_i8_wide_resolve(p); return k < 0 ? nullptr : kTable[k].wide_name; }
int launch_mfma_i8_wide(hipStream_t s, const Problem &p, int k) {
  if (k < 0 || k >= (int)K_NONE) return kErrNotSupported;
  return p.seed ? launch_kind<Form::Seeded, int>(s, p, (Kind)k) : launch_kind<Form::Batched, int>(s, p, (Kind)k);
}

}  // namespace mm
