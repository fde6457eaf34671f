// Log-semiring product (mm_gemm_logsumexp_*): for every output (e, i, j), with the terms s_k = A[e,i,k] + B[e,k,j] formed
// in the computation type F (f32 for half and float, f64 for double),
//     Max: C = log sum_k exp(s_k)          Min: C = -log sum_k exp(-s_k)
// (plus C's input value as one more term when seeded).  Min runs as Max on negated operands, negated on store.  Kernels:
//   * lse_exact_kernel: 64 x 64 outputs per 256-thread workgroup, 4 x 4 per thread, fully predicated (any shape, any
//     element-aligned pointer, both A layouts).  Each output keeps a running pair (m, s), s = sum exp(s_k - m), in
//     registers.  Per slab of LSE_SK k: t = a + b (v_add), the slab maximum (v_max3), a rescale only where the slab
//     maximum exceeds m by more than kLazy nats (so exp2 never sees an argument above 64 and s stays far from overflow),
//     then s += exp2(fma(t, log2 e, -m log2 e)) (v_fma, v_exp_f32, v_add).  The shift is clamped to a finite value, so
//     -inf - -inf never happens: an all -inf output keeps s = 0 and returns -inf.  It is the contract path, the hybrid's
//     fallback (flags != null: a workgroup whose tile flag is clear exits at once) and what MM_PATH_ORDERED runs.
//     BT ("lse_exact_nt", mm_gemm_logsumexp_nt_*): B is stored M x K row-major and staged as an N x K A is, into the same
//     k-major Bs; the slabs, their order and every output's sequence are the row-major kernel's, so are the bits.
//     The tile split and the staging are mm_tile64.h's, the staging with this kernel's load (sg * x in F) and A's -inf fill.
//   * lse_rowmax_kernel / lse_colmax_kernel / lse_expand_kernel: the hybrid's prepass -- per-row (per-column) maxima of an
//     operand, NaN-propagating, and E = exp(X - max) into a zero-padded row-major workspace matrix.
//   * lse_epilogue_kernel: C = ra_i + rb_j + log S (S = EA @ EB from the matrix cores), combined with C's input by a stable
//     log-add-exp when seeded; one flag per 64 x 64 tile, set when any output of the tile has S < tau (or NaN), a
//     non-finite result, or `force`: such a tile leaves C untouched for the fallback.
// No kernel here uses atomics, scratch or AGPRs; every store is a plain vector store.
#include "mm_tile64.h"

namespace mm {
namespace {

template <typename T> struct LseType { using F = float; };
template <> struct LseType<double> { using F = double; };

template <typename F> struct LseMath;
template <> struct LseMath<float> {
  static constexpr float kLog2e = 1.44269504088896340736f, kLn2 = 0.693147180559945309417f;
  static constexpr float kLazy = 44.0f;   // nats: 44 log2(e) = 63.48 < 64
  static constexpr float kBig = 3.40282346638528859812e+38f;
  __device__ static __forceinline__ float exp2(float x) { return __builtin_amdgcn_exp2f(x); }   // v_exp_f32
  __device__ static __forceinline__ float log2(float x) { return __builtin_amdgcn_logf(x); }    // v_log_f32
  __device__ static __forceinline__ float fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
  __device__ static __forceinline__ float exp(float x) { return expf(x); }
  __device__ static __forceinline__ float log(float x) { return logf(x); }
  __device__ static __forceinline__ float log1p(float x) { return log1pf(x); }
};
template <> struct LseMath<double> {
  static constexpr double kLog2e = 1.44269504088896340736, kLn2 = 0.693147180559945309417;
  static constexpr double kLazy = 44.0;
  static constexpr double kBig = 1.79769313486231570815e+308;
  // f64 has no exp instruction: one ocml exp2 per term (the slow path; it serves the fallback and MM_PATH_ORDERED)
  __device__ static __forceinline__ double exp2(double x) { return ::exp2(x); }
  __device__ static __forceinline__ double log2(double x) { return ::log2(x); }
  __device__ static __forceinline__ double fma(double a, double b, double c) { return __builtin_fma(a, b, c); }
  __device__ static __forceinline__ double exp(double x) { return ::exp(x); }
  __device__ static __forceinline__ double log(double x) { return ::log(x); }
  __device__ static __forceinline__ double log1p(double x) { return ::log1p(x); }
};

template <typename F> __device__ __forceinline__ F lse_ninf() { return -__builtin_huge_val(); }
template <> __device__ __forceinline__ float lse_ninf<float>() { return -__builtin_inff(); }

// the exponent shift -m log2(e), clamped to a finite value: m = -inf gives +big (every finite term then raises m first),
// m = +inf gives -big (a +inf term still gives exp2(+inf) = +inf, a finite one 0)
template <typename F> __device__ __forceinline__ F lse_shift(F m) {
  using X = LseMath<F>;
  const F v = -m * X::kLog2e;
  return v > X::kBig ? X::kBig : (v < -X::kBig ? -X::kBig : v);
}

// One output's running pair takes a slab whose largest term is mx: rescale where mx lies more than kLazy above m.
// A NaN mx (a slab of NaN terms) compares false and leaves the pair alone; the NaN terms themselves make s NaN.
template <typename F> __device__ __forceinline__ void lse_raise(F mx, F &m, F &nm, F &s) {
  using X = LseMath<F>;
  if (mx > m + X::kLazy) {
    const F nn = lse_shift(mx);
    s *= X::exp2(nn - nm);   // both finite; the difference may round to -inf: the old sum vanishes (0 stays 0, NaN NaN)
    m = mx;
    nm = nn;
  }
}

// log(s) + m in natural units (m = +inf: +inf or NaN; s = 0 only while m = -inf: -inf)
template <typename F> __device__ __forceinline__ F lse_finish(F m, F s) {
  using X = LseMath<F>;
  return m + X::log2(s) * X::kLn2;
}

template <typename T> __device__ __forceinline__ typename LseType<T>::F lse_load(const T *p) {
  return (typename LseType<T>::F)*p;
}

constexpr int LSE_SK = 4, LSE_APAD = 4;

template <typename T, int RED, bool AT, bool BT>
__global__ __launch_bounds__(256) void lse_exact_kernel(const T *__restrict__ A, const T *__restrict__ B, T *__restrict__ C,
                                                        unsigned N, unsigned K, unsigned M, size_t stride_a, size_t stride_b,
                                                        size_t stride_c, int seeded, const int *__restrict__ flags) {
  using F = typename LseType<T>::F;
  using X = LseMath<F>;
  constexpr F sg = RED == MM_OP_MIN ? (F)-1 : (F)1;
  // terms per slab: 4 for f32; f64 takes 1 (its ocml exp2 is long, and 4 x 4 outputs of f64 slabs spilled to AGPRs)
  constexpr int SK = sizeof(F) == 4 ? LSE_SK : 1;
  __shared__ __attribute__((aligned(16))) F As[kBK][kTile + LSE_APAD];   // [k][row]; the pad spreads the transposing writes
  __shared__ __attribute__((aligned(16))) F Bs[kBK][kTile + (BT ? LSE_APAD : 0)];   // [k][col]; BT: padded as As is
  const unsigned tx = threadIdx.x % 16, ty = threadIdx.x / 16;
  const Tile64 w = tile64_split(N, M);
  if (flags && flags[w.lin] == 0) return;   // the hybrid's fallback: this tile's outputs are already in C
  A += w.e * stride_a;   // what tile64_origin does, after the flag
  B += w.e * stride_b;
  C += w.e * stride_c;
  const unsigned row0 = w.row0(), col0 = w.col0();

  F m[kPerThread][kPerThread], nm[kPerThread][kPerThread], s[kPerThread][kPerThread];
#pragma unroll
  for (int i = 0; i < kPerThread; ++i)
#pragma unroll
    for (int j = 0; j < kPerThread; ++j) {
      m[i][j] = lse_ninf<F>();
      nm[i][j] = X::kBig;
      s[i][j] = (F)0;
      const unsigned gr = row0 + ty * kPerThread + i, gc = col0 + tx + 16 * j;
      if (seeded && gr < N && gc < M) {   // C's input value is one more term
        const F c = sg * lse_load(C + (size_t)gr * M + gc);
        lse_raise(c, m[i][j], nm[i][j], s[i][j]);
        s[i][j] += X::exp2(X::fma(c, X::kLog2e, nm[i][j]));
      }
    }

  for (unsigned k0 = 0; k0 < K; k0 += kBK) {
    // sg * x in F; k beyond K: A = -inf, B = 0, so the padded terms are -inf and add exactly nothing
    const auto load = [](const T *p) { return sg * lse_load(p); };
    tile64_stage<!AT>(As, A, row0, N, k0, K, load, lse_ninf<F>());   // A is N x K, or (AT) K x N
    tile64_stage<BT>(Bs, B, col0, M, k0, K, load);                   // B is K x M, or (BT) M x K
    __syncthreads();
#pragma unroll 1
    for (int kk = 0; kk < kBK; kk += SK) {
      F av[SK][kPerThread], bv[SK][kPerThread];
#pragma unroll
      for (int q = 0; q < SK; ++q) {
#pragma unroll
        for (int i = 0; i < kPerThread; ++i) av[q][i] = As[kk + q][ty * kPerThread + i];
#pragma unroll
        for (int j = 0; j < kPerThread; ++j) bv[q][j] = Bs[kk + q][tx + 16 * j];
      }
#pragma unroll
      for (int i = 0; i < kPerThread; ++i)
#pragma unroll
        for (int j = 0; j < kPerThread; ++j) {
          F tv[SK];
#pragma unroll
          for (int q = 0; q < SK; ++q) tv[q] = av[q][i] + bv[q][j];
          F mx = tv[0];
#pragma unroll
          for (int q = 1; q < SK; ++q) mx = fmax(mx, tv[q]);   // v_max3 pairs
          lse_raise(mx, m[i][j], nm[i][j], s[i][j]);
          F acc = s[i][j];
#pragma unroll
          for (int q = 0; q < SK; ++q) acc += X::exp2(X::fma(tv[q], X::kLog2e, nm[i][j]));
          s[i][j] = acc;
        }
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < kPerThread; ++i) {
    const unsigned gr = row0 + ty * kPerThread + i;
    if (gr >= N) continue;
#pragma unroll
    for (int j = 0; j < kPerThread; ++j) {
      const unsigned gc = col0 + tx + 16 * j;
      if (gc < M) C[(size_t)gr * M + gc] = (T)(sg * lse_finish(m[i][j], s[i][j]));
    }
  }
}

// NaN-propagating maximum (fmax drops a NaN; the contract does not)
template <typename F> __device__ __forceinline__ F lse_max_nan(F a, F b) { return (a != a || b != b) ? a + b : fmax(a, b); }

// r[e][x] = max_k sg X[e][x][k] for x < R (X row-major R x K), 0 for R <= x < Rp; one workgroup per (element, x)
template <typename T, int RED>
__global__ __launch_bounds__(256) void lse_rowmax_kernel(const T *__restrict__ X, typename LseType<T>::F *__restrict__ R,
                                                         unsigned rows, unsigned K, unsigned rows_p, size_t stride_x,
                                                         size_t stride_r) {
  using F = typename LseType<T>::F;
  constexpr F sg = RED == MM_OP_MIN ? (F)-1 : (F)1;
  __shared__ F part[256];
  const unsigned e = blockIdx.x / rows_p, x = blockIdx.x % rows_p, tid = threadIdx.x;
  F mx = lse_ninf<F>();
  if (x < rows) {
    const T *row = X + e * stride_x + (size_t)x * K;
    for (unsigned k = tid; k < K; k += 256) mx = lse_max_nan(mx, sg * lse_load(row + k));
  }
  part[tid] = mx;
  __syncthreads();
  for (unsigned h = 128; h > 0; h /= 2) {
    if (tid < h) part[tid] = lse_max_nan(part[tid], part[tid + h]);
    __syncthreads();
  }
  if (tid == 0) R[e * stride_r + x] = x < rows ? part[0] : (F)0;
}

// r[e][x] = max_k sg X[e][k][x] for x < R (X row-major K x R), 0 for R <= x < Rp; 32 columns x 8 k-lanes per workgroup
// (one thread per column left a 8192-column B to 32 workgroups: 3.3 ms of an 11.7 ms hybrid call at 8192^3)
template <typename T, int RED>
__global__ __launch_bounds__(256) void lse_colmax_kernel(const T *__restrict__ X, typename LseType<T>::F *__restrict__ R,
                                                         unsigned cols, unsigned K, unsigned cols_p, size_t stride_x,
                                                         size_t stride_r) {
  using F = typename LseType<T>::F;
  constexpr F sg = RED == MM_OP_MIN ? (F)-1 : (F)1;
  __shared__ F part[8][32];
  const unsigned blocks = (cols_p + 31) / 32, e = blockIdx.x / blocks, cx = threadIdx.x % 32, ky = threadIdx.x / 32;
  const unsigned x = (blockIdx.x % blocks) * 32 + cx;
  F mx = lse_ninf<F>();
  if (x < cols) {
    const T *col = X + e * stride_x + x;
#pragma unroll 8
    for (unsigned k = ky; k < K; k += 8) mx = lse_max_nan(mx, sg * lse_load(col + (size_t)k * cols));
  }
  part[ky][cx] = mx;
  __syncthreads();
  if (ky == 0 && x < cols_p) {
#pragma unroll
    for (int q = 1; q < 8; ++q) mx = lse_max_nan(mx, part[q][cx]);
    R[e * stride_r + x] = x < cols ? mx : (F)0;
  }
}

// E[e] = exp(sg X - r) into a zero-padded row-major workspace matrix: out_kmajor ? Kp x Rp : Rp x Kp; X is R x K
// (x_kmajor = false) or K x R.  One thread per element of E.  (XK, OK) = (false, true) is the M x K B of the A x B^T
// call: lanes run along E's rows, so the stores are contiguous and the loads of X are K elements apart.
template <typename T, int RED, bool XK, bool OK>
__global__ __launch_bounds__(256) void lse_expand_kernel(const T *__restrict__ X, const typename LseType<T>::F *__restrict__ R,
                                                         typename LseType<T>::F *__restrict__ E, unsigned rows, unsigned K,
                                                         unsigned rows_p, unsigned k_p, size_t stride_x, size_t stride_r,
                                                         size_t stride_e, unsigned long long total) {
  using F = typename LseType<T>::F;
  using Mth = LseMath<F>;
  constexpr F sg = RED == MM_OP_MIN ? (F)-1 : (F)1;
  const unsigned long long per = (unsigned long long)rows_p * k_p;
  for (unsigned long long g = (unsigned long long)blockIdx.x * 256 + threadIdx.x; g < total;
       g += (unsigned long long)gridDim.x * 256) {
    const unsigned long long e = g / per, w = g - e * per;
    const unsigned hi = (unsigned)(w / (OK ? rows_p : k_p)), lo = (unsigned)(w % (OK ? rows_p : k_p));
    const unsigned x = OK ? lo : hi, k = OK ? hi : lo;
    F v = (F)0;
    if (x < rows && k < K) {
      const T *src = X + e * stride_x + (XK ? (size_t)k * rows + x : (size_t)x * K + k);
      v = Mth::exp(sg * lse_load(src) - R[e * stride_r + x]);
    }
    E[e * stride_e + w] = v;
  }
}

// C from S = EA @ EB: one workgroup per 64 x 64 tile of every element; flags[e * tiles + t] = 1 where the tile goes to
// the fallback (C untouched), else 0 and the tile's C written.
template <typename T, int RED>
__global__ __launch_bounds__(256) void lse_epilogue_kernel(const typename LseType<T>::F *__restrict__ S,
                                                           const typename LseType<T>::F *__restrict__ RA,
                                                           const typename LseType<T>::F *__restrict__ RB, T *__restrict__ C,
                                                           int *__restrict__ flags, unsigned N, unsigned M, unsigned m_p,
                                                           size_t stride_s, size_t stride_ra, size_t stride_rb,
                                                           size_t stride_c, typename LseType<T>::F tau, int seeded, int force) {
  using F = typename LseType<T>::F;
  using X = LseMath<F>;
  constexpr F sg = RED == MM_OP_MIN ? (F)-1 : (F)1;
  const unsigned tid = threadIdx.x, tx = tid % 16, ty = tid / 16;
  const unsigned tiles_m = (M + kTile - 1) / kTile, tiles = tiles_m * ((N + kTile - 1) / kTile);
  const unsigned lin = blockIdx.x, e = lin / tiles, t = lin - e * tiles;
  const unsigned row0 = (t / tiles_m) * kTile, col0 = (t % tiles_m) * kTile;
  S += e * stride_s;
  RA += e * stride_ra;
  RB += e * stride_rb;
  C += e * stride_c;
  F out[kPerThread][kPerThread];
  int bad = 0;
#pragma unroll
  for (int i = 0; i < kPerThread; ++i) {
    const unsigned gr = row0 + ty * kPerThread + i;
#pragma unroll
    for (int j = 0; j < kPerThread; ++j) {
      const unsigned gc = col0 + tx + 16 * j;
      out[i][j] = (F)0;
      if (gr < N && gc < M) {
        const F sv = S[(size_t)gr * m_p + gc];
        F w = RA[gr] + RB[gc] + X::log(sv);
        if (seeded) {   // log-add-exp with C's input, in the Max form
          const F c = sg * lse_load(C + (size_t)gr * M + gc);
          const F hi = fmax(c, w), lo = fmin(c, w);
          w = c != c ? c : (hi == lse_ninf<F>() || hi == -lse_ninf<F>() ? hi : hi + X::log1p(X::exp(lo - hi)));
        }
        out[i][j] = sg * w;
        // S < tau: underflowed terms may matter; a non-finite shift or result: the special-value rules need every term
        bad |= !(sv >= tau) | !(w - w == (F)0);
      }
    }
  }
  const int flag = __syncthreads_or(bad) | force;
  if (tid == 0) flags[lin] = flag ? 1 : 0;
  if (flag) return;
#pragma unroll
  for (int i = 0; i < kPerThread; ++i) {
    const unsigned gr = row0 + ty * kPerThread + i;
    if (gr >= N) continue;
#pragma unroll
    for (int j = 0; j < kPerThread; ++j) {
      const unsigned gc = col0 + tx + 16 * j;
      if (gc < M) C[(size_t)gr * M + gc] = (T)out[i][j];
    }
  }
}

// ---- host side, shared by the units that hold these kernels (mm_lse_fp.hip; mm_lse_nt_fp.hip for an M x K B) -----------
template <typename T, int RED, bool AT, bool BT>
int lse_exact_launch(hipStream_t s, const Problem &p, const int *flags) {
  const unsigned tiles = ((p.m + kTile - 1) / kTile) * ((p.n + kTile - 1) / kTile);
  hipLaunchKernelGGL((lse_exact_kernel<T, RED, AT, BT>), dim3(tiles * p.batch), dim3(256), 0, s, (const T *)p.a,
                     (const T *)p.b, (T *)p.c, p.n, p.k, p.m, p.stride_a, p.stride_b, p.stride_c, p.seed ? 1 : 0, flags);
  return (int)hipGetLastError();
}

template <typename T, int RED, bool XK, bool OK>
int lse_expand_launch(hipStream_t s, const LseOperand &op) {
  using F = typename LseType<T>::F;
  const unsigned long long total = (unsigned long long)op.count * op.rows_p * op.k_p;
  const unsigned long long blocks = (total + 255) / 256;
  hipLaunchKernelGGL((lse_expand_kernel<T, RED, XK, OK>), dim3((unsigned)(blocks < (1ull << 20) ? blocks : 1ull << 20)),
                     dim3(256), 0, s, (const T *)op.x, (const F *)op.r, (F *)op.e, op.rows, op.k, op.rows_p, op.k_p,
                     op.stride_x, op.stride_r, op.stride_e, total);
  return (int)hipGetLastError();
}

// half / float / double x (Add, Min / Max) -> f(Tag<T>, Add, RED)
template <typename Fn>
int lse_dispatch(const mm_config_t &cfg, Fn f) {
  return switch_config<FpTypes, Ops<MM_OP_ADD>, MinMaxOps>(cfg, f);
}

}  // namespace
}  // namespace mm
