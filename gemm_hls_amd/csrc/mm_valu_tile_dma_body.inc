// Body of valu_tile_dma_kernel (MM_VT_BATCHED 0), valu_tile_dma_batched_kernel (MM_VT_BATCHED 1) and
// valu_tile_dma_batched_seeded_kernel (MM_VT_BATCHED 1, MM_VT_SEEDED 1): mm_valu_tile.inc includes it once per form, so that
// the single-problem kernel is the same source, and the same machine code, it always was.
  static_assert(TI == 8 || TI == 4, "rows per thread");
  constexpr unsigned ES = sizeof(T), EPC = 16 / ES, BK = 64 / ES;   // bytes, elements per 16-B chunk, slab depth
  constexpr unsigned LPR = 8 * ES, KRP = 64 / LPR;                  // lanes per B k-row (128 cols), k-rows per 1-KiB piece
  constexpr unsigned NW = TI == 8 ? 4 : 8, PW = 8 / NW;             // wavefronts; DMA pieces of A (and of B) per wavefront and slab
  static_assert(VT_BN * ES * BK == VTD_A_BYTES && VT_BM == 128 && VT_BN == 128, "byte geometry");
  __shared__ __attribute__((aligned(16))) char smem[2 * VTD_SLAB];
  const unsigned tid = threadIdx.x, tx = tid % 16, ty = tid / 16;
  const unsigned lane = tid & 63u, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
#if MM_VT_BATCHED
  const unsigned lin = batched_tile(A, B, C, tiles_n * tiles_m, batch, stride_a, stride_b, stride_c);
#else
  const unsigned lin = xcd_remap(blockIdx.x, tiles_n * tiles_m);
#endif
  const unsigned band = lin / (kBand * tiles_m), within = lin % (kBand * tiles_m);
  const unsigned rows_in_band = min(kBand, tiles_n - band * kBand);
  const unsigned row0 = (band * kBand + within % rows_in_band) * VT_BM, col0 = (within / rows_in_band) * VT_BN;

  // DMA: 8 A pieces (16 rows x 64 B) and 8 B pieces (KRP k-rows x 128 cols) per slab, PW + PW per wave
  unsigned voff_a[PW], voff_b[PW];
#pragma unroll
  for (unsigned i = 0; i < PW; ++i) {
    const unsigned piece = wave + NW * i;
    const unsigned row = piece * 16 + lane / 4, pc = lane % 4;
    voff_a[i] = (min(row0 + row, N - 1) - row0) * K * ES + (pc ^ ((row >> 2) & 3u)) * 16;
    const unsigned kr = piece * KRP + lane / LPR, c = (lane % LPR) * EPC;
    voff_b[i] = kr * M * ES + (min(col0 + c, M - EPC) - col0) * ES;
  }
  const char *a_base = (const char *)A + (size_t)row0 * K * ES;
  const char *b_base = (const char *)B + (size_t)col0 * ES;
  const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char *)smem;
  const unsigned slabs = (K + BK - 1) / BK;
  auto issue = [&](unsigned t) {  // slab t -> buffer t & 1; the last slab starts at K - BK
    const unsigned k0 = min(t * BK, K - BK);
    const char *ap = a_base + (size_t)k0 * ES;
    const char *bp = b_base + (size_t)k0 * M * ES;
    const unsigned la0 = lds0 + (t & 1u) * VTD_SLAB + wave * 1024, la1 = la0 + 4 * 1024;
    const unsigned lb0 = la0 + VTD_A_BYTES, lb1 = lb0 + 4 * 1024;
    unsigned keep;
    if constexpr (PW == 2) {
      asm volatile("s_mov_b32 %0, m0\n\t" MM_DMA_PIECE("%1", "%5", "%7") MM_DMA_PIECE("%2", "%5", "%8")
                       MM_DMA_PIECE("%3", "%6", "%9") MM_DMA_PIECE("%4", "%6", "%10") "s_mov_b32 m0, %0"
                   : "=&s"(keep)
                   : "v"(voff_a[0]), "v"(voff_a[1]), "v"(voff_b[0]), "v"(voff_b[1]), "s"(ap), "s"(bp), "s"(la0), "s"(la1),
                     "s"(lb0), "s"(lb1)
                   : "memory");
    } else {
      asm volatile("s_mov_b32 %0, m0\n\t" MM_DMA_PIECE("%1", "%3", "%5") MM_DMA_PIECE("%2", "%4", "%6") "s_mov_b32 m0, %0"
                   : "=&s"(keep)
                   : "v"(voff_a[0]), "v"(voff_b[0]), "s"(ap), "s"(bp), "s"(la0), "s"(lb0)
                   : "memory");
    }
  };

  T acc[TI][8];
#pragma unroll
  for (int i = 0; i < TI; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[i][j] = Op<RED, T>::identity();

  using V = Vec4<T>;
  constexpr unsigned KSTEP = ES >= 4 ? 2 : 8 / ES;   // k per A read: 16 B (8-byte types) or 8 B
  struct alignas(KSTEP * sizeof(T)) PK { T v[KSTEP]; };
  // row i of this thread: TI == 8: ty*4 + i, then 64 + ty*4 + (i-4) (ty < 16); TI == 4: ty*4 + i (ty < 32).
  // Either way all of a thread's rows have (row >> 2) & 3 == ty & 3
  auto thread_row = [&](int i) -> unsigned { return TI == 8 ? (i < 4 ? ty * 4 + i : 64 + ty * 4 + (i - 4)) : ty * 4 + i; };
  const unsigned a_swz = ty & 3u;
  issue(0);
#if MM_VT_SEEDED
  // accumulate: the acc tile starts from C, read with the Vec4 accesses the store below uses (a lane reads exactly what it
  // later writes), issued behind the first slab's DMA pieces; the loop's first vmcnt(0) waits for both
#pragma unroll
  for (int i = 0; i < TI; ++i) {
    const unsigned r = row0 + thread_row(i);
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
  for (unsigned t = 0; t < slabs; ++t) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // own pieces of slab t have landed
    __syncthreads();                                  // everybody's have; buffer (t+1)&1 is no longer being read
    if (t + 1 < slabs) issue(t + 1);
    const char *as = smem + (t & 1u) * VTD_SLAB;
    const char *bs = as + VTD_A_BYTES;
    // a full slab uses k 0..BK-1 of the buffer; the (shifted) last slab only its new k
    const unsigned kbeg = t * BK - min(t * BK, K - BK);  // 0 except for a partial last slab
    // one LDS read per row fetches KSTEP consecutive k (8 or 16 bytes: a pair for 4- and 8-byte types, 4 / 8 k for
    // 2- / 1-byte types); the map-reduce steps then go pair by pair, k ascending
    for (unsigned kk = kbeg; kk < BK; kk += KSTEP) {
      PK av[TI];
      const unsigned kb = kk * ES, aoff = (((kb >> 4) ^ a_swz) * 16) + (kb & 15u);
#pragma unroll
      for (int i = 0; i < TI; ++i) av[i] = *(const PK *)(as + thread_row(i) * 64 + aoff);
#pragma unroll
      for (unsigned q = 0; q < KSTEP; q += 2) {
        T b0[8], b1[8];
        *(V *)&b0[0] = *(const V *)(bs + ((kk + q) * VT_BN + tx * 4) * ES);
        *(V *)&b0[4] = *(const V *)(bs + ((kk + q) * VT_BN + 64 + tx * 4) * ES);
        *(V *)&b1[0] = *(const V *)(bs + ((kk + q + 1) * VT_BN + tx * 4) * ES);
        *(V *)&b1[4] = *(const V *)(bs + ((kk + q + 1) * VT_BN + 64 + tx * 4) * ES);
#pragma unroll
        for (int i = 0; i < TI; ++i)
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const T s0 = FastOp<MAP, T>::apply(av[i].v[q], b0[j]);
            const T s1 = FastOp<MAP, T>::apply(av[i].v[q + 1], b1[j]);
            acc[i][j] = FastOp<RED, T>::apply(FastOp<RED, T>::apply(acc[i][j], s0), s1);  // k, then k+1
          }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < TI; ++i) {
    const unsigned r = row0 + thread_row(i);
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
