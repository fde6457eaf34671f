// argreduce over an M x K B (mm_gemm_argreduce_nt_*) instantiations: 8- and 16-bit integer element types.
#pragma clang fp contract(off)
#include "mm_argreduce.inc"
namespace mm {
int launch_argreduce_nt_int_narrow(hipStream_t s, const mm_config_t &cfg, const Problem &p, int *index, int index_base,
                                   bool tile) {
  return ar_dispatch<NarrowIntTypes, true>(s, cfg, p, index, index_base, tile);
}
}  // namespace mm
