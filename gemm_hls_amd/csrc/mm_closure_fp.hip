// closure instantiations: floating-point element types.
#pragma clang fp contract(off)   // the map is one rounded operation in Data_t, as in the k-ordered contract
#include "mm_closure.inc"
namespace mm {
int launch_closure_fp(hipStream_t s, const mm_config_t &cfg, const ClosureStep &st) {
  return cl_dispatch<FpTypes>(s, cfg, st);
}
}  // namespace mm
