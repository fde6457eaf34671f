// closure instantiations: floating-point element types.
#pragma clang fp contract(off)   // the map is one rounded operation in Data_t, as in the k-ordered contract
#include "mm_closure.inc"
namespace mm {
int launch_closure_fp(hipStream_t s, const mm_config_t &cfg, const ClosureStep &st) {
  switch (cfg.dtype) {
    case MM_DTYPE_F32: return cl_type<float>(s, cfg, st);
    case MM_DTYPE_F64: return cl_type<double>(s, cfg, st);
    case MM_DTYPE_F16: return cl_type<half_t>(s, cfg, st);
    default: return kErrNotSupported;
  }
}
}  // namespace mm
