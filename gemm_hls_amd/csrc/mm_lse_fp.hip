// Log-semiring product (mm_gemm_logsumexp_*): instantiations for half, float and double, and their launchers.
#pragma clang fp contract(off)   // the terms are one rounded sum each, the error analysis to the letter
#include <algorithm>

#include "mm_lse.inc"
namespace mm {
namespace {

template <typename T, int RED>
int lse_exact_launch(hipStream_t s, const Problem &p, const int *flags) {
  const unsigned tiles = ((p.m + LSE_T - 1) / LSE_T) * ((p.n + LSE_T - 1) / LSE_T);
  const int seeded = p.seed ? 1 : 0;
  if (p.a_transposed)
    hipLaunchKernelGGL((lse_exact_kernel<T, RED, true>), dim3(tiles * p.batch), dim3(256), 0, s, (const T *)p.a,
                       (const T *)p.b, (T *)p.c, p.n, p.k, p.m, p.stride_a, p.stride_b, p.stride_c, seeded, flags);
  else
    hipLaunchKernelGGL((lse_exact_kernel<T, RED, false>), dim3(tiles * p.batch), dim3(256), 0, s, (const T *)p.a,
                       (const T *)p.b, (T *)p.c, p.n, p.k, p.m, p.stride_a, p.stride_b, p.stride_c, seeded, flags);
  return (int)hipGetLastError();
}

template <typename T, int RED>
int lse_prepass_launch(hipStream_t s, const LseOperand &op) {
  using F = typename LseType<T>::F;
  const T *x = (const T *)op.x;
  F *r = (F *)op.r, *e = (F *)op.e;
  if (op.x_kmajor)
    hipLaunchKernelGGL((lse_colmax_kernel<T, RED>), dim3(op.count * ((op.rows_p + 31) / 32)), dim3(256), 0, s, x, r,
                       op.rows, op.k, op.rows_p, op.stride_x, op.stride_r);
  else
    hipLaunchKernelGGL((lse_rowmax_kernel<T, RED>), dim3(op.count * op.rows_p), dim3(256), 0, s, x, r, op.rows, op.k,
                       op.rows_p, op.stride_x, op.stride_r);
  if (hipError_t err = hipGetLastError()) return (int)err;
  const unsigned long long total = (unsigned long long)op.count * op.rows_p * op.k_p;
  const unsigned grid = (unsigned)std::min<unsigned long long>((total + 255) / 256, 1ull << 20);
#define MM_LSE_EXPAND(XK, OK)                                                                                           \
  hipLaunchKernelGGL((lse_expand_kernel<T, RED, XK, OK>), dim3(grid), dim3(256), 0, s, x, (const F *)r, e, op.rows, op.k, \
                     op.rows_p, op.k_p, op.stride_x, op.stride_r, op.stride_e, total)
  if (op.x_kmajor && op.out_kmajor) MM_LSE_EXPAND(true, true);
  else if (op.x_kmajor) MM_LSE_EXPAND(true, false);
  else MM_LSE_EXPAND(false, false);
#undef MM_LSE_EXPAND
  return (int)hipGetLastError();
}

template <typename T, int RED>
int lse_epilogue_launch(hipStream_t s, const LseEpilogue &ep) {
  using F = typename LseType<T>::F;
  // S below tau: the terms that underflowed in the prepass (each below 2^-126 resp. 2^-1022 absolute) may matter
  const F tau = sizeof(F) == 4 ? (F)0x1p-64 : (F)0x1p-512;
  const unsigned tiles = ((ep.m + LSE_T - 1) / LSE_T) * ((ep.n + LSE_T - 1) / LSE_T);
  hipLaunchKernelGGL((lse_epilogue_kernel<T, RED>), dim3(tiles * ep.batch), dim3(256), 0, s, (const F *)ep.s,
                     (const F *)ep.ra, (const F *)ep.rb, (T *)ep.c, ep.flags, ep.n, ep.m, ep.m_p, ep.stride_s, ep.stride_ra,
                     ep.stride_rb, ep.stride_c, tau, ep.seed ? 1 : 0, ep.force ? 1 : 0);
  return (int)hipGetLastError();
}

// half / float / double x (Add, Min / Max) -> f(Tag<T>, Add, RED)
template <typename Fn>
int lse_dispatch(const mm_config_t &cfg, Fn f) {
  return switch_config<FpTypes, Ops<MM_OP_ADD>, MinMaxOps>(cfg, f);
}

}  // namespace

int launch_lse_exact(hipStream_t s, const mm_config_t &cfg, const Problem &p, const int *flags) {
  return lse_dispatch(cfg, [&](auto t, auto, auto red) { return lse_exact_launch<type_of<decltype(t)>, decltype(red)::value>(s, p, flags); });
}
int launch_lse_prepass(hipStream_t s, const mm_config_t &cfg, const LseOperand &op) {
  return lse_dispatch(cfg, [&](auto t, auto, auto red) { return lse_prepass_launch<type_of<decltype(t)>, decltype(red)::value>(s, op); });
}
int launch_lse_epilogue(hipStream_t s, const mm_config_t &cfg, const LseEpilogue &ep) {
  return lse_dispatch(cfg, [&](auto t, auto, auto red) { return lse_epilogue_launch<type_of<decltype(t)>, decltype(red)::value>(s, ep); });
}

}  // namespace mm
