// In-place semiring closure (mm_closure_*): the two dependent phases of one round of blocked Floyd-Warshall.  Block
// K = [k0, k0 + bt) of every graph in the launch, Reduce = Min or Max, a winner always a strict improvement (the select of
// Op<RED, T>::apply, as in mm_argreduce.inc), witnesses the global pivot v:
//   * closure_diag_kernel (step 1): for v in K ascending, D[K,K] <- D[K,K] (+) D[K,v] (x) D[v,K], row v and column v taken
//     before the step.  One workgroup per graph holds the block in registers (a TT x TT interleaved sub-block per thread:
//     rows ty + TG * i, columns tx + TG * j) and publishes the pivot row and column through LDS, double-buffered, one
//     barrier per step.  The pivot's register row is i0 = v / TG, so the step loop is unrolled over i0 and every register
//     index is static.  With n <= B this is the whole closure of the graph.
//   * closure_panel_kernel (step 2): row panel D[K,J] <- D[K,J] (+) P (x) D[K,J]_old and column panel
//     D[I,K] <- D[I,K] (+) D[I,K]_old (x) P, over v in K ascending, seeded with the old value (and witness).  One 256-thread
//     workgroup owns a whole panel tile -- all of K by 64 outside rows or columns -- and copies the tile's old values into LDS
//     before anything is written back, so the in-place update is race-free; P streams through LDS in slabs of 16 pivots.
// Both kernels also write the contiguous snapshots step 3 multiplies: Cc = D[:,K] (n x bt) and Rc = D[K,:] (bt x n).
// Included once per element-type group (mm_closure_*.hip); every unit says `#pragma clang fp contract(off)` first.
#include "mm_common.h"

namespace mm {
namespace {

template <int RED, typename T> __device__ __forceinline__ bool cl_takes(T s, T acc) {
  if constexpr (RED == MM_OP_MIN) return s < acc;
  else return acc < s;
}

template <typename T, int MAP, int RED, bool WIT, int TT, int TT2>
__device__ __forceinline__ void cl_update(T (&acc)[TT][TT2], int (&idx)[TT][TT2], const T (&a)[TT], const T (&b)[TT2], int v) {
#pragma unroll
  for (int i = 0; i < TT; ++i)
#pragma unroll
    for (int j = 0; j < TT2; ++j) {
      const T s = Op<MAP, T>::apply(a[i], b[j]);
      const bool t = cl_takes<RED>(s, acc[i][j]);
      acc[i][j] = t ? s : acc[i][j];
      if (WIT) idx[i][j] = t ? v : idx[i][j];
    }
}

// Step 1.  BM: the largest block edge the kernel holds, TT x TT outputs per thread, (BM / TT)^2 threads.
template <typename T, int MAP, int RED, bool WIT, int BM, int TT>
__global__ __launch_bounds__((BM / TT) * (BM / TT)) void closure_diag_kernel(T *__restrict__ D, int *__restrict__ W, unsigned n,
                                                                           size_t stride_d, unsigned k0, unsigned bt,
                                                                           T *__restrict__ Cc, T *__restrict__ Rc,
                                                                           size_t stride_ws, int w_fresh) {
  constexpr int TG = BM / TT;
  __shared__ T colv[2][BM], rowv[2][BM];
  const unsigned e = blockIdx.x, tid = threadIdx.x, tx = tid % TG, ty = tid / TG;
  D += e * stride_d;
  if (WIT) W += e * stride_d;
  T acc[TT][TT];
  int idx[TT][TT];
#pragma unroll
  for (int i = 0; i < TT; ++i)
#pragma unroll
    for (int j = 0; j < TT; ++j) {
      const unsigned r = ty + TG * i, c = tx + TG * j;
      const bool in = r < bt && c < bt;
      const size_t at = (size_t)(k0 + r) * n + k0 + c;
      acc[i][j] = in ? D[at] : (T)0;
      idx[i][j] = (WIT && in && !w_fresh) ? W[at] : -1;
    }
#pragma unroll
  for (int i0 = 0; i0 < TT; ++i0) {
    for (unsigned vv = 0; vv < (unsigned)TG && i0 * TG + vv < bt; ++vv) {
      const unsigned v = i0 * TG + vv, buf = v & 1;
      // row v and column v as they are before step v (buffer buf was last read two steps ago, before the last barrier)
      if (ty == vv) {
#pragma unroll
        for (int j = 0; j < TT; ++j) rowv[buf][tx + TG * j] = acc[i0][j];
      }
      if (tx == vv) {
#pragma unroll
        for (int i = 0; i < TT; ++i) colv[buf][ty + TG * i] = acc[i][i0];
      }
      __syncthreads();
      T a[TT], b[TT];
#pragma unroll
      for (int i = 0; i < TT; ++i) a[i] = colv[buf][ty + TG * i];
#pragma unroll
      for (int j = 0; j < TT; ++j) b[j] = rowv[buf][tx + TG * j];
      cl_update<T, MAP, RED, WIT>(acc, idx, a, b, (int)(k0 + v));
    }
  }
  if (Cc) {
    Cc += e * stride_ws;
    Rc += e * stride_ws;
  }
#pragma unroll
  for (int i = 0; i < TT; ++i)
#pragma unroll
    for (int j = 0; j < TT; ++j) {
      const unsigned r = ty + TG * i, c = tx + TG * j;
      if (r < bt && c < bt) {
        const size_t at = (size_t)(k0 + r) * n + k0 + c;
        D[at] = acc[i][j];
        if (WIT) W[at] = idx[i][j];
        if (Cc) {
          Cc[(size_t)(k0 + r) * bt + c] = acc[i][j];
          Rc[(size_t)r * n + k0 + c] = acc[i][j];
        }
      }
    }
}

constexpr int CL_PW = 64, CL_SLAB = 16;   // panel tile: all of K by CL_PW outside rows / columns; pivots per P slab

template <int BM> struct PanelLds {
  static constexpr int X = (BM * (CL_PW + 1) > CL_PW * (BM + 1) ? BM * (CL_PW + 1) : CL_PW * (BM + 1));
  static constexpr int P = CL_SLAB * (BM + 1);
};

// One panel tile.  COLP = false: the row panel D[K, o0 .. o0+ow) (bt x ow), s = P[r][v] (x) X_old[v][c];
// COLP = true: the column panel D[o0 .. o0+ow, K] (ow x bt), s = X_old[r][v] (x) P[v][c].
template <typename T, int MAP, int RED, bool WIT, int BM, bool COLP>
__device__ __forceinline__ void closure_panel_tile(T *__restrict__ D, int *__restrict__ W, unsigned n, unsigned k0,
                                                   unsigned bt, unsigned o0, unsigned ow, T *__restrict__ Cc,
                                                   T *__restrict__ Rc, T *Xs, T *Ps) {
  constexpr int TY = COLP ? 8 : 32, TX = COLP ? 32 : 8;          // 256 threads
  constexpr int RT = COLP ? 8 : BM / 32, CT = COLP ? BM / 32 : 8;  // outputs per thread
  constexpr int R = COLP ? CL_PW : BM, C = COLP ? BM : CL_PW, XP = C + 1, PP = BM + 1;
  const unsigned rows = COLP ? ow : bt, cols = COLP ? bt : ow;
  const unsigned gr0 = COLP ? o0 : k0, gc0 = COLP ? k0 : o0;
  const unsigned tid = threadIdx.x, tx = tid % TX, ty = tid / TX;
#pragma unroll 1
  for (unsigned q = tid; q < (unsigned)(R * C); q += 256) {
    const unsigned r = q / C, c = q % C;
    Xs[r * XP + c] = (r < rows && c < cols) ? D[(size_t)(gr0 + r) * n + gc0 + c] : (T)0;
  }
  __syncthreads();
  T acc[RT][CT];
  int idx[RT][CT];
#pragma unroll
  for (int i = 0; i < RT; ++i)
#pragma unroll
    for (int j = 0; j < CT; ++j) {
      const unsigned r = ty + TY * i, c = tx + TX * j;
      acc[i][j] = Xs[r * XP + c];
      idx[i][j] = (WIT && r < rows && c < cols) ? W[(size_t)(gr0 + r) * n + gc0 + c] : -1;
    }
#pragma unroll 1
  for (unsigned v0 = 0; v0 < bt; v0 += CL_SLAB) {
    // Ps[kk][x] = P[x][v0 + kk] (row panel: column slab of P) or P[v0 + kk][x] (column panel: row slab)
#pragma unroll 1
    for (unsigned q = tid; q < (unsigned)(CL_SLAB * BM); q += 256) {
      const unsigned kk = COLP ? q / BM : q % CL_SLAB, x = COLP ? q % BM : q / CL_SLAB;
      T val = (T)0;
      if (x < bt && v0 + kk < bt)
        val = COLP ? D[(size_t)(k0 + v0 + kk) * n + k0 + x] : D[(size_t)(k0 + x) * n + k0 + v0 + kk];
      Ps[kk * PP + x] = val;
    }
    __syncthreads();
    const unsigned kmax = min((unsigned)CL_SLAB, bt - v0);
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)   // (the byte types took all 256 VGPRs otherwise)
    for (unsigned kk = 0; kk < kmax; ++kk) {
      const unsigned v = v0 + kk;
      T a[RT], b[CT];
#pragma unroll
      for (int i = 0; i < RT; ++i) a[i] = COLP ? Xs[(ty + TY * i) * XP + v] : Ps[kk * PP + ty + TY * i];
#pragma unroll
      for (int j = 0; j < CT; ++j) b[j] = COLP ? Ps[kk * PP + tx + TX * j] : Xs[v * XP + tx + TX * j];
      cl_update<T, MAP, RED, WIT>(acc, idx, a, b, (int)(k0 + v));
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < RT; ++i)
#pragma unroll
    for (int j = 0; j < CT; ++j) {
      const unsigned r = ty + TY * i, c = tx + TX * j;
      if (r < rows && c < cols) {
        const size_t at = (size_t)(gr0 + r) * n + gc0 + c;
        D[at] = acc[i][j];
        if (WIT) W[at] = idx[i][j];
        if (COLP) Cc[(size_t)(o0 + r) * bt + c] = acc[i][j];
        else Rc[(size_t)r * n + o0 + c] = acc[i][j];
      }
    }
}

// Step 2: per graph, `tiles` row-panel tiles then `tiles` column-panel tiles of CL_PW; those inside K exit at once (k0 and
// every block edge but the last, which ends at n, are multiples of CL_PW).
template <typename T, int MAP, int RED, bool WIT, int BM>
__global__ __launch_bounds__(256) void closure_panel_kernel(T *__restrict__ D, int *__restrict__ W, unsigned n, size_t stride_d,
                                                            unsigned k0, unsigned bt, T *__restrict__ Cc, T *__restrict__ Rc,
                                                            size_t stride_ws, unsigned tiles) {
  __shared__ T Xs[PanelLds<BM>::X];
  __shared__ T Ps[PanelLds<BM>::P];
  const unsigned e = blockIdx.x / (2 * tiles), rest = blockIdx.x % (2 * tiles);
  const bool colp = rest >= tiles;
  const unsigned o0 = (rest % tiles) * CL_PW;
  if (o0 >= k0 && o0 < k0 + bt) return;   // inside K: step 1's block
  const unsigned ow = min((unsigned)CL_PW, n - o0);
  D += e * stride_d;
  if (WIT) W += e * stride_d;
  Cc += e * stride_ws;
  Rc += e * stride_ws;
  if (colp) closure_panel_tile<T, MAP, RED, WIT, BM, true>(D, W, n, k0, bt, o0, ow, Cc, Rc, Xs, Ps);
  else closure_panel_tile<T, MAP, RED, WIT, BM, false>(D, W, n, k0, bt, o0, ow, Cc, Rc, Xs, Ps);
}

// Block classes: the smallest of 64 / 128 / 256 that holds bt.  256 only for value-only elements of at most 4 bytes (an
// 8 x 8 register sub-block per thread); mm_capi.hip never asks for more.
template <typename T, int MAP, int RED, bool WIT>
int cl_launch(hipStream_t s, const ClosureStep &st) {
  T *d = (T *)st.d, *cc = (T *)st.cc, *rc = (T *)st.rc;
  constexpr bool big = !WIT && sizeof(T) <= 4;
  const unsigned cls = st.bt <= 64 ? 64 : st.bt <= 128 ? 128 : 256;
  if (cls == 256 && !big) return kErrNotSupported;
  if (st.panels) {
    const unsigned tiles = (st.n + CL_PW - 1) / CL_PW, grid = 2 * tiles * st.graphs;
    if (cls <= 128)
      hipLaunchKernelGGL((closure_panel_kernel<T, MAP, RED, WIT, 128>), dim3(grid), dim3(256), 0, s, d, st.w, st.n,
                         st.stride_d, st.k0, st.bt, cc, rc, st.stride_ws, tiles);
    else if constexpr (big)
      hipLaunchKernelGGL((closure_panel_kernel<T, MAP, RED, WIT, 256>), dim3(grid), dim3(256), 0, s, d, st.w, st.n,
                         st.stride_d, st.k0, st.bt, cc, rc, st.stride_ws, tiles);
    return (int)hipGetLastError();
  }
  if (cls == 64)
    hipLaunchKernelGGL((closure_diag_kernel<T, MAP, RED, WIT, 64, 4>), dim3(st.graphs), dim3(256), 0, s, d, st.w, st.n,
                       st.stride_d, st.k0, st.bt, cc, rc, st.stride_ws, st.w_fresh);
  else if (cls == 128)
    hipLaunchKernelGGL((closure_diag_kernel<T, MAP, RED, WIT, 128, 4>), dim3(st.graphs), dim3(1024), 0, s, d, st.w, st.n,
                       st.stride_d, st.k0, st.bt, cc, rc, st.stride_ws, st.w_fresh);
  else if constexpr (big)
    hipLaunchKernelGGL((closure_diag_kernel<T, MAP, RED, WIT, 256, 8>), dim3(st.graphs), dim3(1024), 0, s, d, st.w, st.n,
                       st.stride_d, st.k0, st.bt, cc, rc, st.stride_ws, st.w_fresh);
  return (int)hipGetLastError();
}

// TYPES: the element types the including unit instantiates
template <typename TYPES>
int cl_dispatch(hipStream_t s, const mm_config_t &cfg, const ClosureStep &st) {
  return switch_config<TYPES, AllOps, MinMaxOps>(cfg, [&](auto t, auto map, auto red) {
    using T = type_of<decltype(t)>;
    constexpr int MAP = decltype(map)::value, RED = decltype(red)::value;
    return st.w != nullptr ? cl_launch<T, MAP, RED, true>(s, st) : cl_launch<T, MAP, RED, false>(s, st);
  });
}

}  // namespace
}  // namespace mm
