// argreduce instantiations: 8- and 16-bit integers.
#pragma clang fp contract(off)
#include "mm_argreduce.inc"
namespace mm {
int launch_argreduce_int_narrow(hipStream_t s, const mm_config_t &cfg, const Problem &p, int *index, int index_base,
                                bool tile) {
  switch (cfg.dtype) {
    case MM_DTYPE_I8: return ar_type<int8_t>(s, cfg, p, index, index_base, tile);
    case MM_DTYPE_U8: return ar_type<uint8_t>(s, cfg, p, index, index_base, tile);
    case MM_DTYPE_I16: return ar_type<int16_t>(s, cfg, p, index, index_base, tile);
    case MM_DTYPE_U16: return ar_type<uint16_t>(s, cfg, p, index, index_base, tile);
    default: return kErrNotSupported;
  }
}
}  // namespace mm
