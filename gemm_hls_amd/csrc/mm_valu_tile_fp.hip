// valu_tile instantiations: floating-point element types.
#include "mm_valu_tile.inc"
namespace mm {
namespace {
template <bool BATCHED>
int by_type(hipStream_t s, const mm_config_t &cfg, const Problem &p) {
  switch (cfg.dtype) {
    case MM_DTYPE_F32: return vt_type<float, BATCHED>(s, cfg, p);
    case MM_DTYPE_F64: return vt_type<double, BATCHED>(s, cfg, p);
    case MM_DTYPE_F16: return vt_type<half_t, BATCHED>(s, cfg, p);
    default: return kErrNotSupported;
  }
}
}  // namespace
int launch_valu_tile_fp(hipStream_t s, const mm_config_t &cfg, const Problem &p) { return by_type<false>(s, cfg, p); }
int launch_valu_tile_fp_batched(hipStream_t s, const mm_config_t &cfg, const Problem &p) { return by_type<true>(s, cfg, p); }
}  // namespace mm
