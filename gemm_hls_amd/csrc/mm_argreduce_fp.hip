// argreduce instantiations: floating-point element types.
#pragma clang fp contract(off)   // the map is one rounded operation in Data_t, as in the k-ordered contract
#include "mm_argreduce.inc"
namespace mm {
int launch_argreduce_fp(hipStream_t s, const mm_config_t &cfg, const Problem &p, int *index, int index_base, bool tile) {
  switch (cfg.dtype) {
    case MM_DTYPE_F32: return ar_type<float>(s, cfg, p, index, index_base, tile);
    case MM_DTYPE_F64: return ar_type<double>(s, cfg, p, index, index_base, tile);
    case MM_DTYPE_F16: return ar_type<half_t>(s, cfg, p, index, index_base, tile);
    default: return kErrNotSupported;
  }
}
}  // namespace mm
