// closure instantiations: 8- and 16-bit integers.
#pragma clang fp contract(off)
#include "mm_closure.inc"
namespace mm {
int launch_closure_int_narrow(hipStream_t s, const mm_config_t &cfg, const ClosureStep &st) {
  return cl_dispatch<NarrowIntTypes>(s, cfg, st);
}
}  // namespace mm
