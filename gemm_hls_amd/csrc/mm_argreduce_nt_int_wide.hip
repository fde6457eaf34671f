// argreduce over an M x K B (mm_gemm_argreduce_nt_*) instantiations: 32- and 64-bit integers; and that form's dispatcher.
#pragma clang fp contract(off)
#include "mm_argreduce.inc"
namespace mm {
int launch_argreduce_nt_fp(hipStream_t s, const mm_config_t &cfg, const Problem &p, int *index, int index_base, bool tile);
int launch_argreduce_nt_int_narrow(hipStream_t s, const mm_config_t &cfg, const Problem &p, int *index, int index_base,
                                   bool tile);

int launch_argreduce_nt(hipStream_t s, const mm_config_t &cfg, const Problem &p, int *index, int index_base, bool tile) {
  switch (cfg.dtype) {
    case MM_DTYPE_F32: case MM_DTYPE_F64: case MM_DTYPE_F16: return launch_argreduce_nt_fp(s, cfg, p, index, index_base, tile);
    case MM_DTYPE_I8: case MM_DTYPE_U8: case MM_DTYPE_I16: case MM_DTYPE_U16:
      return launch_argreduce_nt_int_narrow(s, cfg, p, index, index_base, tile);
    default: return ar_dispatch<WideIntTypes, true>(s, cfg, p, index, index_base, tile);
  }
}
}  // namespace mm
