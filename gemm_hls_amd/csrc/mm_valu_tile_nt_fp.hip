// valu_tile_nt instantiations: floating-point element types.
#include "mm_valu_tile_nt.inc"
namespace mm {
int launch_valu_tile_nt_fp(hipStream_t s, const mm_config_t &cfg, const Problem &p) { return vt_nt_dispatch<FpTypes>(s, cfg, p); }
}  // namespace mm
