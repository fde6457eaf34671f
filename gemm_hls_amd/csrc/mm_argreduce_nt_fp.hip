// argreduce over an M x K B (mm_gemm_argreduce_nt_*) instantiations: floating-point element types.
#pragma clang fp contract(off)   // the map is one rounded operation in Data_t, as in the k-ordered contract
#include "mm_argreduce.inc"
namespace mm {
int launch_argreduce_nt_fp(hipStream_t s, const mm_config_t &cfg, const Problem &p, int *index, int index_base, bool tile) {
  return ar_dispatch<FpTypes, true>(s, cfg, p, index, index_base, tile);
}
}  // namespace mm
