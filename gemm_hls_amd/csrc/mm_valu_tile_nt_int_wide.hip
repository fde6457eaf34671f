// valu_tile_nt instantiations: 32- and 64-bit integers; and the family's dispatcher.
#include "mm_valu_tile_nt.inc"
namespace mm {
int launch_valu_tile_nt_fp(hipStream_t s, const mm_config_t &cfg, const Problem &p);
int launch_valu_tile_nt_int_narrow(hipStream_t s, const mm_config_t &cfg, const Problem &p);

// By configuration and shape alone; the launch also needs A and Bt (bases and element strides) 16-byte aligned
bool valu_tile_nt_serves(const mm_config_t &cfg, const Problem &p) {
  const bool map_ok = cfg.map_op == MM_OP_MULTIPLY || cfg.map_op == MM_OP_ADD || cfg.map_op == MM_OP_MIN || cfg.map_op == MM_OP_MAX;
  const bool red_ok = cfg.reduce_op == MM_OP_ADD || cfg.reduce_op == MM_OP_MIN || cfg.reduce_op == MM_OP_MAX;
  if (!map_ok || !red_ok) return false;
  return switch_dtype<AllTypes>(cfg.dtype, [&](auto t) { return (int)vt_dma_k_serves<type_of<decltype(t)>>(p); }) == 1;
}

// the p.batch elements of p (strides p.stride_*), accumulating into C for p.seed
int launch_valu_tile_nt(hipStream_t s, const mm_config_t &cfg, const Problem &p) {
  switch (cfg.dtype) {
    case MM_DTYPE_F32: case MM_DTYPE_F64: case MM_DTYPE_F16: return launch_valu_tile_nt_fp(s, cfg, p);
    case MM_DTYPE_I8: case MM_DTYPE_U8: case MM_DTYPE_I16: case MM_DTYPE_U16:
      return launch_valu_tile_nt_int_narrow(s, cfg, p);
    default: return vt_nt_dispatch<WideIntTypes>(s, cfg, p);
  }
}
}  // namespace mm
