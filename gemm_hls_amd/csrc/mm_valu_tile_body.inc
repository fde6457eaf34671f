// Body of valu_tile_kernel (MM_VT_BATCHED 0), valu_tile_batched_kernel (MM_VT_BATCHED 1) and valu_tile_batched_seeded_kernel
// (MM_VT_BATCHED 1, MM_VT_SEEDED 1): mm_valu_tile.inc includes it once per form, so that the single-problem kernel is the
// same source, and the same machine code, it always was.
  __shared__ __attribute__((aligned(16))) T As[VT_BK][VT_BM + VT_PAD];
  __shared__ __attribute__((aligned(16))) T Bs[VT_BK][VT_BN + VT_PAD];
  const unsigned tid = threadIdx.x, tx = tid % 16, ty = tid / 16;
#if MM_VT_BATCHED
  const unsigned lin = batched_tile(A, B, C, tiles_n * tiles_m, batch, stride_a, stride_b, stride_c);
#else
  const unsigned lin = xcd_remap(blockIdx.x, tiles_n * tiles_m);
#endif
  const unsigned band = lin / (kBand * tiles_m), within = lin % (kBand * tiles_m);
  const unsigned rows_in_band = min(kBand, tiles_n - band * kBand);
  const unsigned row0 = (band * kBand + within % rows_in_band) * VT_BM, col0 = (within / rows_in_band) * VT_BN;

  T acc[8][8];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[i][j] = Op<RED, T>::identity();

  using V = Vec4<T>;
#if MM_VT_SEEDED
  // accumulate: the acc tile starts from C, read with the Vec4 accesses the store below uses (a lane reads exactly what it
  // later writes); the loads are consumed at the first k-step, so they are in flight while the first slab is staged
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const unsigned r = row0 + (i < 4 ? ty * 4 + i : 64 + ty * 4 + (i - 4));
    if (r >= N) continue;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const unsigned c = col0 + h * 64 + tx * 4;
      if (c < M) {
        const V v = *(const V *)(C + (size_t)r * M + c);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[i][h * 4 + e] = v.v[e];
      }
    }
  }
#endif
  for (unsigned k0 = 0; k0 < K; k0 += VT_BK) {
    // ---- stage (K % 4 == 0, so a 4-wide k chunk is entirely inside or entirely outside) ----
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const unsigned idx = tid + 256 * u;
      if (AT) {  // A is K x N: rows of the tile are contiguous
        const unsigned kr = idx / 32, r4 = (idx % 32) * 4;
        V v = {};
        if (k0 + kr < K && row0 + r4 < N) v = *(const V *)(A + (size_t)(k0 + kr) * N + row0 + r4);
        *(V *)&As[kr][r4] = v;
      } else {   // A is N x K: 4 lanes cover one row's 16 k; scatter into the k-major image
        const unsigned r = idx / 4, kc = (idx % 4) * 4;
        V v = {};
        if (row0 + r < N && k0 + kc < K) v = *(const V *)(A + (size_t)(row0 + r) * K + k0 + kc);
#pragma unroll
        for (int e = 0; e < 4; ++e) As[kc + e][r] = v.v[e];
      }
      {
        const unsigned kr = idx / 32, c4 = (idx % 32) * 4;
        V v = {};
        if (k0 + kr < K && col0 + c4 < M) v = *(const V *)(B + (size_t)(k0 + kr) * M + col0 + c4);
        *(V *)&Bs[kr][c4] = v;
      }
    }
    __syncthreads();
    const unsigned kmax = min((unsigned)VT_BK, K - k0);  // multiple of 4
    for (unsigned kk = 0; kk < kmax; kk += 2) {
      T a0[8], b0[8], a1[8], b1[8];
      *(V *)&a0[0] = *(const V *)&As[kk][ty * 4];
      *(V *)&a0[4] = *(const V *)&As[kk][64 + ty * 4];
      *(V *)&b0[0] = *(const V *)&Bs[kk][tx * 4];
      *(V *)&b0[4] = *(const V *)&Bs[kk][64 + tx * 4];
      *(V *)&a1[0] = *(const V *)&As[kk + 1][ty * 4];
      *(V *)&a1[4] = *(const V *)&As[kk + 1][64 + ty * 4];
      *(V *)&b1[0] = *(const V *)&Bs[kk + 1][tx * 4];
      *(V *)&b1[4] = *(const V *)&Bs[kk + 1][64 + tx * 4];
#pragma unroll
      for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const T s0 = FastOp<MAP, T>::apply(a0[i], b0[j]);
          const T s1 = FastOp<MAP, T>::apply(a1[i], b1[j]);
          acc[i][j] = FastOp<RED, T>::apply(FastOp<RED, T>::apply(acc[i][j], s0), s1);  // k, then k+1
        }
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const unsigned r = row0 + (i < 4 ? ty * 4 + i : 64 + ty * 4 + (i - 4));
    if (r >= N) continue;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const unsigned c = col0 + h * 64 + tx * 4;
      if (c < M) {
        V v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v.v[e] = acc[i][h * 4 + e];
        *(V *)(C + (size_t)r * M + c) = v;
      }
    }
  }
