// Body of ordered_kernel (MM_ORDERED_BATCHED 0), ordered_batched_kernel (MM_ORDERED_BATCHED 1) and
// ordered_batched_seeded_kernel (MM_ORDERED_BATCHED 1, MM_ORDERED_SEEDED 1): mm_ordered.hip includes it once per form, so
// that the single-problem kernel is the same source, and the same machine code, it always was.
  __shared__ T As[kBK][kTile + 1];  // [k][row], +1: column reads of a row-major source
  __shared__ T Bs[kBK][kTile];      // [k][col]
  const unsigned tid = threadIdx.x;
  const unsigned tx = tid % 16, ty = tid / 16;
#if MM_ORDERED_BATCHED
  // element e of the batch: XCD-remapped ids e * tiles .. (e + 1) * tiles - 1 (one element's tiles stay on one XCD),
  // row-major over its tile grid; uniform, SGPRs
  const unsigned tiles_m = (M + kTile - 1) / kTile, tiles = tiles_m * ((N + kTile - 1) / kTile);
  const unsigned lin = xcd_remap(blockIdx.x, gridDim.x), e = lin / tiles, t = lin - e * tiles;
  A += e * stride_a;
  B += e * stride_b;
  C += e * stride_c;
  const unsigned row0 = (t / tiles_m) * kTile, col0 = (t % tiles_m) * kTile;
#else
  const unsigned row0 = blockIdx.y * kTile, col0 = blockIdx.x * kTile;
#endif

  ACC acc[kPerThread][kPerThread];
#pragma unroll
  for (int i = 0; i < kPerThread; ++i)
#pragma unroll
    for (int j = 0; j < kPerThread; ++j) acc[i][j] = Op<RED, ACC>::identity();
#if MM_ORDERED_SEEDED
  // accumulate: the value C holds replaces identity() as the start of the chain (Naive with acc = C[i][j]); the loads are
  // only consumed at the first k-step, so they are in flight while the first slab is staged
#pragma unroll
  for (int i = 0; i < kPerThread; ++i) {
    const unsigned gr = row0 + ty * kPerThread + i;
#pragma unroll
    for (int j = 0; j < kPerThread; ++j) {
      const unsigned gc = col0 + tx + 16 * j;
      if (gr < N && gc < M) acc[i][j] = (ACC)C[(size_t)gr * M + gc];
    }
  }
#endif

  for (unsigned k0 = 0; k0 < K; k0 += kBK) {
    // stage A: 64 rows x 16 k
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      unsigned r, kk;
      if (AT) { r = tid % 64; kk = tid / 64 + 4 * i; }   // A is K x N: consecutive lanes along N
      else    { kk = tid % 16; r = tid / 16 + 16 * i; }  // A is N x K: consecutive lanes along K
      const unsigned gr = row0 + r, gk = k0 + kk;
      T v = (T)0;
      if (gr < N && gk < K) v = AT ? A[(size_t)gk * N + gr] : A[(size_t)gr * K + gk];
      As[kk][r] = v;
    }
    // stage B: 16 k x 64 cols
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const unsigned c = tid % 64, kk = tid / 64 + 4 * i;
      const unsigned gc = col0 + c, gk = k0 + kk;
      Bs[kk][c] = (gc < M && gk < K) ? B[(size_t)gk * M + gc] : (T)0;
    }
    __syncthreads();
    const unsigned kmax = (K - k0) < (unsigned)kBK ? (K - k0) : (unsigned)kBK;
    for (unsigned kk = 0; kk < kmax; ++kk) {  // strictly ascending k
      T av[kPerThread], bv[kPerThread];
#pragma unroll
      for (int i = 0; i < kPerThread; ++i) av[i] = As[kk][ty * kPerThread + i];
#pragma unroll
      for (int j = 0; j < kPerThread; ++j) bv[j] = Bs[kk][tx + 16 * j];
#pragma unroll
      for (int i = 0; i < kPerThread; ++i)
#pragma unroll
        for (int j = 0; j < kPerThread; ++j)
          acc[i][j] = Op<RED, ACC>::apply(acc[i][j], Op<MAP, ACC>::apply((ACC)av[i], (ACC)bv[j]));
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
      if (gc < M) C[(size_t)gr * M + gc] = (T)acc[i][j];
    }
  }
