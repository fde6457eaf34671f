// The kernel of mm_mfma_f64.hip.  F (mm_common.h): the single-problem kernel, its strided-batched form, or the batched form
// that accumulates into C.
template <Form F, typename G, bool AT>
__global__ __launch_bounds__(G::THREADS, G::MIN_WAVES) void mfma_f64_kernel(  // 2 wavefronts per SIMD: <= 256 VGPRs, so that the
                                                                   // 4-wavefront geometry really fits twice on a CU
    const double *__restrict__ A,
                                                              const double *__restrict__ B,
                                                              double *__restrict__ C, unsigned N, unsigned K,
                                                              unsigned M, unsigned tiles_n, unsigned tiles_m, unsigned kBand, unsigned batch,
                                                              size_t stride_a, size_t stride_b, size_t stride_c) {
  constexpr int TM = G::TM, TP = G::TP, BK = G::BK, NS = G::NS, CPR = G::CPR;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const unsigned lane = threadIdx.x & 63u;
  const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const unsigned wm = wave / G::WN, wn = wave % G::WN;
  const unsigned lo = lane & 15u, g4 = lane >> 4;

  const unsigned nwg = tiles_n * tiles_m;
  const unsigned lin = form_tile<F>(A, B, C, nwg, batch, stride_a, stride_b, stride_c);
  unsigned row0, col0;
  band_origin(lin, tiles_n, tiles_m, kBand, G::BM, G::BN, row0, col0);

  size_t a_row_off[G::LA];
  unsigned a_kchunk[G::LA];
#pragma unroll
  for (int i = 0; i < G::LA; ++i) {
    const unsigned slot = (wave + G::NW * i) * 64 + lane;
    if (AT) {  // A stored K x N: slab is [BK][BM] like B's; a_kchunk = k-row, a_row_off = column offset
      a_kchunk[i] = slot / (G::BM / 2);
      a_row_off[i] = min(row0 + (slot % (G::BM / 2)) * 2, N - 2);
    } else {
      const unsigned row = slot / CPR, pc = slot % CPR;
      a_kchunk[i] = pc ^ ((row >> 1) & (CPR - 1));
      a_row_off[i] = (size_t)min(row0 + row, N - 1) * K;
    }
  }
  unsigned b_krow[G::LB], b_col[G::LB];
#pragma unroll
  for (int i = 0; i < G::LB; ++i) {
    const unsigned slot = (wave + G::NW * i) * 64 + lane;
    b_krow[i] = slot / G::BCH;
    b_col[i] = min(col0 + (slot % G::BCH) * 2, M - 2);
  }
  auto stage = [&](unsigned buf, unsigned k0) {
    char *base = smem + buf * G::STAGE_BYTES;
#pragma unroll
    for (int i = 0; i < G::LA; ++i) {
      const double *src = AT ? A + (size_t)min(k0 + a_kchunk[i], K - 1) * N + a_row_off[i]
                             : A + a_row_off[i] + min(k0 + a_kchunk[i] * 2, K - 2);
      __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(base + (wave + G::NW * i) * 1024), 16, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < G::LB; ++i) {
      const unsigned kr = min(k0 + b_krow[i], K - 1);
      __builtin_amdgcn_global_load_lds((gptr_t)(B + (size_t)kr * M + b_col[i]),
                                       (lptr_t)(base + G::A_BYTES + (wave + G::NW * i) * 1024), 16, 0, 0);
    }
  };

  // Scalar-base form of the same DMA (K >= BK): uniform 64-bit base in SGPRs + a constant 32-bit per-lane
  // offset -- one address VGPR per lane instead of two, no per-slab 64-bit VALU address arithmetic.  On the fp32 kernel
  // this removed most of the DMA instructions' issue cost (+2.5 %, mm_mfma_f32.hip).  A slab start past K - BK (beyond
  // the end, or the partial last slab) is clamped to K - BK uniformly: a partial last slab sits in the SECOND half of
  // its buffer (see the last-slab loop).  K < BK never reaches a PIPE geometry (launch_mfma_f64).
  constexpr bool SDMA = G::PIPE;
  unsigned voa[G::LA], vob[G::LB];
  if (SDMA) {
#pragma unroll
    for (int i = 0; i < G::LA; ++i) {
      const unsigned slot = (wave + G::NW * i) * 64 + lane, row = slot / CPR;
      if (AT) voa[i] = a_kchunk[i] * N * 8u + ((unsigned)a_row_off[i] - row0) * 8u;   // K x N: k-row, clamped column
      else voa[i] = (min(row0 + row, N - 1) - row0) * K * 8u + a_kchunk[i] * 16u;
    }
#pragma unroll
    for (int i = 0; i < G::LB; ++i) vob[i] = b_krow[i] * M * 8u + (b_col[i] - col0) * 8u;
  }
  const unsigned lds_base = (unsigned)(size_t)(__attribute__((address_space(3))) char *)smem;
  auto dma_piece_s = [&](unsigned buf, unsigned k0, int i) {
    const unsigned kc = min(k0, K - BK);
    const bool is_a = i < G::LA;
    const int j = is_a ? i : i - G::LA;
    unsigned long long base = !is_a ? (unsigned long long)(B + (size_t)kc * M + col0)
                              : AT ? (unsigned long long)(A + (size_t)kc * N + row0) : (unsigned long long)(A + (size_t)row0 * K + kc);
    const unsigned blo = __builtin_amdgcn_readfirstlane((unsigned)base), bhi = __builtin_amdgcn_readfirstlane((unsigned)(base >> 32));
    base = ((unsigned long long)bhi << 32) | blo;
    const unsigned la = lds_base + buf * G::STAGE_BYTES + (is_a ? 0 : G::A_BYTES) + (wave + G::NW * j) * 1024;
    const unsigned vo = is_a ? voa[j] : vob[j];
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(vo), "s"(base), "s"(la) : "memory");
  };

  // A: row = wm*64 + mi*16 + lo; chunk = (4*kg + g4) ^ swz(lo)
  const unsigned a_swz = (lo >> 1) & (CPR - 1);
  // K x N layout: image [k][row]; a lane reads 2 consecutive rows of k-row 2*g4 + p, so row
  // tiles pair up: tile 2q+t holds rows q*32 + 2*i + t
  const unsigned a_frag_base = AT ? (2 * g4) * (G::BM * 8) + (wm * G::WTM + 2 * lo) * 8 : (wm * G::WTM + lo) * (BK * 8);
  // B: k = kg*8 + 2*g4 + p; col = wn*64 + pair*32 + 2*lo
  const unsigned b_frag_base = G::A_BYTES + (2 * g4) * (G::BN * 8) + (wn * G::WTN + 2 * lo) * 8;

  f64x4 acc[TM][TP][2];
#pragma unroll
  for (int mi = 0; mi < TM; ++mi)
#pragma unroll
    for (int pr = 0; pr < TP; ++pr) {
      acc[mi][pr][0] = (f64x4)0.0;
      acc[mi][pr][1] = (f64x4)0.0;
    }

  auto load_frags = [&](unsigned buf, int kg, f64x2 (&af)[TM], f64x2 (&bf)[2][TP]) {
    const char *base = smem + buf * G::STAGE_BYTES;
    const unsigned achunk = (((unsigned)(4 * kg) + g4) ^ a_swz) * 16;
    if (AT) {
#pragma unroll
      for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int q = 0; q < TM / 2; ++q) {
          const f64x2 v = *(const f64x2 *)(base + a_frag_base + (kg * 8 + p) * (G::BM * 8) + q * 32 * 8);
          af[2 * q][p] = v[0];
          af[2 * q + 1][p] = v[1];
        }
    } else {
#pragma unroll
      for (int mi = 0; mi < TM; ++mi) af[mi] = *(const f64x2 *)(base + a_frag_base + mi * 16 * (BK * 8) + achunk);
    }
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int pr = 0; pr < TP; ++pr)
        bf[p][pr] = *(const f64x2 *)(base + b_frag_base + (kg * 8 + p) * (G::BN * 8) + pr * 32 * 8);
  };
  auto mfma_group = [&](const f64x2 (&af)[TM], const f64x2 (&bf)[2][TP]) {
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int mi = 0; mi < TM; ++mi)
#pragma unroll
        for (int pr = 0; pr < TP; ++pr) {
          acc[mi][pr][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[mi][p], bf[p][pr][0], acc[mi][pr][0], 0, 0, 0);
          acc[mi][pr][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[mi][p], bf[p][pr][1], acc[mi][pr][1], 0, 0, 0);
        }
  };

  const unsigned num_tiles = (K + BK - 1) / BK;
  constexpr int L = G::LA + G::LB;
  constexpr bool sdma = SDMA;          // the launcher sends K < BK to the non-PIPE geometry
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    if constexpr (sdma) {
#pragma unroll
      for (int i = 0; i < L; ++i) dma_piece_s(s, s * BK, i);
    } else {
      stage(s, s * BK);
    }
  }
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NS - 1) * L) : "memory");
  __builtin_amdgcn_s_barrier();

  f64x2 af0[TM], bf0[2][TP], af1[TM], bf1[2][TP];
  load_frags(0, 0, af0, bf0);

  // the two p-halves of a k-group, in mfma_group's order
  auto mfma_half = [&](const f64x2 (&af)[TM], const f64x2 (&bf)[2][TP], int p) {
#pragma unroll
    for (int mi = 0; mi < TM; ++mi)
#pragma unroll
      for (int pr = 0; pr < TP; ++pr) {
        acc[mi][pr][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[mi][p], bf[p][pr][0], acc[mi][pr][0], 0, 0, 0);
        acc[mi][pr][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[mi][p], bf[p][pr][1], acc[mi][pr][1], 0, 0, 0);
      }
  };

  // one full slab with a successor; KG == 2: group 0 from set 0, group 1 from set 1 (see f32 kernel)
  const unsigned steady = num_tiles - 1;
  for (unsigned t = 0; t < steady; ++t) {
    const unsigned buf = t % NS;
    if constexpr (G::PIPE) {
      // Pinned order (round 2).  Written plainly ("read the next group, multiply this one, barrier, refill, ...") the
      // machine scheduler moved BOTH groups' MFMAs behind the barrier: per slab the matrix core then waited for 8
      // fragment reads, the barrier and 6 DMA issues in a row (MfmaUtil 92 %).  Here every fragment is requested 16
      // MFMAs before its first use and the barrier sits between two MFMA halves:
      //   16 MFMAs | reads of group 1 | 16 MFMAs | 16 MFMAs | wait + barrier | (MFMA, DMA piece) x L,
      //   (MFMA, read of slab t+1's group 0) x 8, remaining MFMAs
      constexpr int NM = 4 * TM * TP / 2 * 2 / 2, NR = TM + 2 * TP;  // MFMAs per half group (16), reads per group (8)
      __builtin_amdgcn_sched_barrier(0);
      mfma_half(af0, bf0, 0);
      __builtin_amdgcn_sched_barrier(0);
      load_frags(buf, 1, af1, bf1);
      __builtin_amdgcn_sched_barrier(0);
      mfma_half(af0, bf0, 1);
      mfma_half(af1, bf1, 0);
      __builtin_amdgcn_sched_barrier(0);
      asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"((NS - 2) * L) : "memory");
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
      static_assert(L + NR <= NM, "post-barrier half group too short for the interleave");
      if constexpr (sdma) {
        // the DMA pieces are inline asm (the scheduler cannot classify them): one MFMA, one piece, by hand
        auto mfma_one = [&](int idx) {  // idx-th MFMA of mfma_half(af1, bf1, 1)
          const int mi = idx / (2 * TP), pr = (idx / 2) % TP, h = idx % 2;
          acc[mi][pr][h] = __builtin_amdgcn_mfma_f64_16x16x4f64(af1[mi][1], bf1[1][pr][h], acc[mi][pr][h], 0, 0, 0);
        };
#pragma unroll
        for (int i = 0; i < L; ++i) {
          mfma_one(i);
          dma_piece_s(buf, (t + NS) * BK, i);
          __builtin_amdgcn_sched_barrier(0);
        }
        load_frags((t + 1) % NS, 0, af0, bf0);
#pragma unroll
        for (int i = L; i < NM; ++i) mfma_one(i);
#pragma unroll
        for (int i = 0; i < NR; ++i) {
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
          __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        }
        __builtin_amdgcn_sched_group_barrier(0x008, NM - L - NR, 0);
        __builtin_amdgcn_sched_barrier(0);
        continue;
      }
      stage(buf, (t + NS) * BK);
      load_frags((t + 1) % NS, 0, af0, bf0);
      mfma_half(af1, bf1, 1);
#pragma unroll
      for (int i = 0; i < L; ++i) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
      }
#pragma unroll
      for (int i = 0; i < NR; ++i) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
      }
      __builtin_amdgcn_sched_group_barrier(0x008, NM - L - NR, 0);
      __builtin_amdgcn_sched_barrier(0);
      continue;
    }
    load_frags(buf, 1, af1, bf1);
    mfma_group(af0, bf0);
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"((NS - 2) * L) : "memory");
    __builtin_amdgcn_s_barrier();
    stage(buf, (t + NS) * BK);
    load_frags((t + 1) % NS, 0, af0, bf0);
    mfma_group(af1, bf1);
  }
  {
    const unsigned t = num_tiles - 1;
    const int groups = (int)((K - t * BK) / 8);
    const int shift = sdma ? G::KG - groups : 0;  // scalar-base DMA fetched a partial last slab as the LAST BK k
    for (int kg = 0; kg < groups; ++kg) {
      load_frags(t % NS, kg + shift, af0, bf0);
      mfma_group(af0, bf0);
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // trailing ring refills (clamped, unread)

  // epilogue: lane owns 2 consecutive columns of rows g4 + 4*r
#pragma unroll
  for (int pr = 0; pr < TP; ++pr) {
    const unsigned ccol = col0 + wn * G::WTN + pr * 32 + 2 * lo;
    if (ccol >= M) continue;
#pragma unroll
    for (int mi = 0; mi < TM; ++mi)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const unsigned ri = g4 + 4 * r;
        const unsigned row = row0 + wm * G::WTM + (AT ? (mi >> 1) * 32 + 2 * ri + (mi & 1) : mi * 16 + ri);
        if (row < N) {
          f64x2 v;
          v[0] = acc[mi][pr][0][r];
          v[1] = acc[mi][pr][1][r];
          if constexpr (F == Form::Seeded)
            v += *(const f64x2 *)(C + (size_t)row * M + ccol);   // accumulate: C's value enters here, read by the lane that writes it
          *(f64x2 *)(C + (size_t)row * M + ccol) = v;
        }
      }
  }
}
