// closure instantiations: 8- and 16-bit integers.
#pragma clang fp contract(off)
#include "mm_closure.inc"
namespace mm {
int launch_closure_int_narrow(hipStream_t s, const mm_config_t &cfg, const ClosureStep &st) {
  switch (cfg.dtype) {
    case MM_DTYPE_I8: return cl_type<int8_t>(s, cfg, st);
    case MM_DTYPE_U8: return cl_type<uint8_t>(s, cfg, st);
    case MM_DTYPE_I16: return cl_type<int16_t>(s, cfg, st);
    case MM_DTYPE_U16: return cl_type<uint16_t>(s, cfg, st);
    default: return kErrNotSupported;
  }
}
}  // namespace mm
