// valu_tile instantiations: 8- and 16-bit integers.
#include "mm_valu_tile.inc"
namespace mm {
int launch_valu_tile_int_narrow(hipStream_t s, const mm_config_t &cfg, const Problem &p) { return vt_dispatch<NarrowIntTypes, false>(s, cfg, p); }
int launch_valu_tile_int_narrow_batched(hipStream_t s, const mm_config_t &cfg, const Problem &p) { return vt_dispatch<NarrowIntTypes, true>(s, cfg, p); }
}  // namespace mm
