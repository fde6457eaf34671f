// argreduce instantiations: 8- and 16-bit integers.
#pragma clang fp contract(off)
#include "mm_argreduce.inc"
namespace mm {
int launch_argreduce_int_narrow(hipStream_t s, const mm_config_t &cfg, const Problem &p, int *index, int index_base,
                                bool tile) {
  return ar_dispatch<NarrowIntTypes>(s, cfg, p, index, index_base, tile);
}
}  // namespace mm
