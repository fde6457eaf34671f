// argreduce instantiations: 32- and 64-bit integers; and the family's dispatcher.
#pragma clang fp contract(off)
#include "mm_argreduce.inc"
namespace mm {
int launch_argreduce_fp(hipStream_t s, const mm_config_t &cfg, const Problem &p, int *index, int index_base, bool tile);
int launch_argreduce_int_narrow(hipStream_t s, const mm_config_t &cfg, const Problem &p, int *index, int index_base,
                                bool tile);

int launch_argreduce(hipStream_t s, const mm_config_t &cfg, const Problem &p, int *index, int index_base, bool tile) {
  if (p.b_transposed) return launch_argreduce_nt(s, cfg, p, index, index_base, tile);   // mm_argreduce_nt_*.hip
  switch (cfg.dtype) {
    case MM_DTYPE_F32: case MM_DTYPE_F64: case MM_DTYPE_F16: return launch_argreduce_fp(s, cfg, p, index, index_base, tile);
    case MM_DTYPE_I8: case MM_DTYPE_U8: case MM_DTYPE_I16: case MM_DTYPE_U16:
      return launch_argreduce_int_narrow(s, cfg, p, index, index_base, tile);
    default: return ar_dispatch<WideIntTypes>(s, cfg, p, index, index_base, tile);
  }
}
}  // namespace mm
