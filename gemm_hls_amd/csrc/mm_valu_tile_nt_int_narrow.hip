// valu_tile_nt instantiations: 8- and 16-bit integers.
#include "mm_valu_tile_nt.inc"
namespace mm {
int launch_valu_tile_nt_int_narrow(hipStream_t s, const mm_config_t &cfg, const Problem &p) { return vt_nt_dispatch<NarrowIntTypes>(s, cfg, p); }
}  // namespace mm
