// Log-semiring product (mm_gemm_logsumexp_*): instantiations for half, float and double, and their launchers.
#pragma clang fp contract(off)   // the terms are one rounded sum each, the error analysis to the letter
#include "mm_lse.inc"
namespace mm {
namespace {

// r = the per-line maxima of op.x
template <typename T, int RED>
int lse_max_launch(hipStream_t s, const LseOperand &op) {
  using F = typename LseType<T>::F;
  const T *x = (const T *)op.x;
  F *r = (F *)op.r;
  if (op.x_kmajor)
    hipLaunchKernelGGL((lse_colmax_kernel<T, RED>), dim3(op.count * ((op.rows_p + 31) / 32)), dim3(256), 0, s, x, r,
                       op.rows, op.k, op.rows_p, op.stride_x, op.stride_r);
  else
    hipLaunchKernelGGL((lse_rowmax_kernel<T, RED>), dim3(op.count * op.rows_p), dim3(256), 0, s, x, r, op.rows, op.k,
                       op.rows_p, op.stride_x, op.stride_r);
  return (int)hipGetLastError();
}

template <typename T, int RED>
int lse_epilogue_launch(hipStream_t s, const LseEpilogue &ep) {
  using F = typename LseType<T>::F;
  // S below tau: the terms that underflowed in the prepass (each below 2^-126 resp. 2^-1022 absolute) may matter
  const F tau = sizeof(F) == 4 ? (F)0x1p-64 : (F)0x1p-512;
  const unsigned tiles = ((ep.m + kTile - 1) / kTile) * ((ep.n + kTile - 1) / kTile);
  hipLaunchKernelGGL((lse_epilogue_kernel<T, RED>), dim3(tiles * ep.batch), dim3(256), 0, s, (const F *)ep.s,
                     (const F *)ep.ra, (const F *)ep.rb, (T *)ep.c, ep.flags, ep.n, ep.m, ep.m_p, ep.stride_s, ep.stride_ra,
                     ep.stride_rb, ep.stride_c, tau, ep.seed ? 1 : 0, ep.force ? 1 : 0);
  return (int)hipGetLastError();
}

}  // namespace

int launch_lse_exact(hipStream_t s, const mm_config_t &cfg, const Problem &p, const int *flags) {
  if (p.b_transposed) return launch_lse_exact_nt(s, cfg, p, flags);   // mm_lse_nt_fp.hip
  return lse_dispatch(cfg, [&](auto t, auto, auto red) {
    using T = type_of<decltype(t)>;
    constexpr int RED = decltype(red)::value;
    return p.a_transposed ? lse_exact_launch<T, RED, true, false>(s, p, flags) : lse_exact_launch<T, RED, false, false>(s, p, flags);
  });
}
int launch_lse_prepass(hipStream_t s, const mm_config_t &cfg, const LseOperand &op) {
  if (int e = lse_dispatch(cfg, [&](auto t, auto, auto red) { return lse_max_launch<type_of<decltype(t)>, decltype(red)::value>(s, op); }))
    return e;
  if (!op.x_kmajor && op.out_kmajor) return launch_lse_expand_nt(s, cfg, op);   // an M x K B: mm_lse_nt_fp.hip
  return lse_dispatch(cfg, [&](auto t, auto, auto red) {
    using T = type_of<decltype(t)>;
    constexpr int RED = decltype(red)::value;
    return op.x_kmajor && op.out_kmajor ? lse_expand_launch<T, RED, true, true>(s, op)
           : op.x_kmajor ? lse_expand_launch<T, RED, true, false>(s, op) : lse_expand_launch<T, RED, false, false>(s, op);
  });
}
int launch_lse_epilogue(hipStream_t s, const mm_config_t &cfg, const LseEpilogue &ep) {
  return lse_dispatch(cfg, [&](auto t, auto, auto red) { return lse_epilogue_launch<type_of<decltype(t)>, decltype(red)::value>(s, ep); });
}

}  // namespace mm
