// Log-semiring product over an M x K B (mm_gemm_logsumexp_nt_*): "lse_exact_nt", and the expansion of the hybrid's EB from
// Bt as it lies.  Everything else of "lse_hybrid_nt" -- the maxima (lse_rowmax_kernel on Bt), the product, the epilogue --
// is mm_lse_fp.hip's.
#pragma clang fp contract(off)   // the terms are one rounded sum each, the error analysis to the letter
#include "mm_lse.inc"
namespace mm {

int launch_lse_exact_nt(hipStream_t s, const mm_config_t &cfg, const Problem &p, const int *flags) {
  if (p.a_transposed || !p.b_transposed) return kErrNotSupported;
  return lse_dispatch(cfg, [&](auto t, auto, auto red) {
    return lse_exact_launch<type_of<decltype(t)>, decltype(red)::value, false, true>(s, p, flags);
  });
}
int launch_lse_expand_nt(hipStream_t s, const mm_config_t &cfg, const LseOperand &op) {
  return lse_dispatch(cfg, [&](auto t, auto, auto red) {
    return lse_expand_launch<type_of<decltype(t)>, decltype(red)::value, false, true>(s, op);
  });
}

}  // namespace mm
