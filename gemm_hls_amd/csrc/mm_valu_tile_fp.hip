// valu_tile instantiations: floating-point element types.
#include "mm_valu_tile.inc"
namespace mm {
int launch_valu_tile_fp(hipStream_t s, const mm_config_t &cfg, const Problem &p) { return vt_dispatch<FpTypes, false>(s, cfg, p); }
int launch_valu_tile_fp_batched(hipStream_t s, const mm_config_t &cfg, const Problem &p) { return vt_dispatch<FpTypes, true>(s, cfg, p); }
}  // namespace mm
