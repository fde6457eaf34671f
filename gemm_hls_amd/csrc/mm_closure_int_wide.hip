// closure instantiations: 32- and 64-bit integers; and the family's dispatcher.
#pragma clang fp contract(off)
#include "mm_closure.inc"
namespace mm {
int launch_closure_fp(hipStream_t s, const mm_config_t &cfg, const ClosureStep &st);
int launch_closure_int_narrow(hipStream_t s, const mm_config_t &cfg, const ClosureStep &st);

int launch_closure(hipStream_t s, const mm_config_t &cfg, const ClosureStep &st) {
  switch (cfg.dtype) {
    case MM_DTYPE_F32: case MM_DTYPE_F64: case MM_DTYPE_F16: return launch_closure_fp(s, cfg, st);
    case MM_DTYPE_I8: case MM_DTYPE_U8: case MM_DTYPE_I16: case MM_DTYPE_U16: return launch_closure_int_narrow(s, cfg, st);
    default: return cl_dispatch<WideIntTypes>(s, cfg, st);
  }
}
}  // namespace mm
