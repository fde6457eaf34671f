// fp32 matrix-core family, part 2 of 3: the 64 x 64 geometry for problems below a round of 128 x 128 tiles (its own kernel, the
// per-element arithmetic of tile_body).  Included by mm_mfma_f32.hip inside namespace mm::(anonymous), after mm_mfma_f32_tile.inc.

// ---- small problems (round 3): 64 x 64 tiles, one 32 x 32 accumulator per wavefront -------------------------------------
// Below a round of 128 x 128 tiles the chip has more SIMDs than the problem has wavefront tiles of 32 x 128 (1024^3: 256 for
// 1024 SIMDs), which split-K answers with partial planes and a second kernel.  This geometry instead makes the wavefront
// tile 32 x 32 -- a workgroup of 2 x 2 wavefronts owns 64 x 64 of C, two workgroups per CU (64 KiB of LDS each) --
// so that 1024^3 is 256 workgroups of whole K and no reduction.  The price: twice the L2 -> LDS bytes per flop of the
// 128 x 128 tile, and every MFMA of a wavefront accumulates into the same registers (a dependent chain: 94 % of the
// matrix-core rate with one wavefront per SIMD, 100 % with two -- tools/probes/probe_mfma_chain.hip).
// Arithmetic: per output element exactly the chain of tile_body -- k-groups of 8 ascending, inside a group the MFMA
// pairs (p, p + 4), accumulators flushed into C after every 4096 k that more than 32 k follow -- so the result has the
// bits of the other shipped geometries (tested).  Row-major A only.
//   A slab in LDS: [64 rows][8 chunks of 4 k], chunk index XOR (row >> 1) & 7 (the 16 lanes of a ds_read_b128 service
//     group -- 16 rows, one logical chunk -- hit 16 distinct 16-B slots of the 256-B bank row);
//   B slab in LDS: [32 k][16 chunks of 4 columns], chunk index XOR 8 for k & 4: the MFMA's B operand is one float per
//     lane, B[k = p + 4 * (lane >> 5)][column lane & 31], read with ds_read_b32 -- lanes 0-31 take 32 consecutive dwords
//     of k-row p, lanes 32-63 the same columns of k-row p + 4, which the XOR moves to the other 32 banks.
//   (Both enumerated in tests/test_layouts.py.)  Ring of four stages, one barrier per slab, the order of MFMAs, DMA pieces and
//   fragment reads pinned (below).
template <int NS_>
struct SmallT {
  static constexpr int BM = 64, BN = 64, BK = 32, NS = NS_, NW = 4, THREADS = 256;
  static constexpr int A_BYTES = BM * BK * 4, B_BYTES = BK * BN * 4, STAGE_BYTES = A_BYTES + B_BYTES, LDS_BYTES = NS * STAGE_BYTES;
  static constexpr int PER_CU = 160 * 1024 / LDS_BYTES > 3 ? 3 : 160 * 1024 / LDS_BYTES;
  static constexpr int CHUNK = 128;   // slabs per link of the chain: 4096 k
  static constexpr int L = 4;         // DMA instructions per wavefront per slab: 2 of A, 2 of B
};

using Small = SmallT<4>;

template <typename G>
__global__ __launch_bounds__(G::THREADS, G::PER_CU) void mfma_f32_small_kernel(
    const float *__restrict__ A, const float *__restrict__ B, float *__restrict__ C, unsigned N, unsigned K, unsigned M,
    unsigned tiles_n, unsigned tiles_m, unsigned kBand, unsigned kChunk, float *__restrict__ partials) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const unsigned nwg = tiles_n * tiles_m;
  const unsigned lda = K;
  unsigned bid = blockIdx.x;
  if (kChunk) {   // split-K (few tiles, long K), as in mfma_f32_kernel: copy `split` of the tile grid multiplies its k range into its own plane
    const unsigned split = bid / nwg, kbeg = split * kChunk;
    bid -= split * nwg;
    A += kbeg;
    B += (size_t)kbeg * M;
    C = partials + (size_t)split * N * M;
    K = min(kChunk, K - kbeg);
  }
  const unsigned lin = xcd_remap(bid, nwg);
  unsigned row0, col0;
  band_origin(lin, tiles_n, tiles_m, kBand, G::BM, G::BN, row0, col0);

  const unsigned lane = threadIdx.x & 63u;
  const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const unsigned wm = wave >> 1, wn = wave & 1u, lo = lane & 31u, hi = lane >> 5;

  // per-lane DMA sources (clamped: a slab index past the end, a row past N or a column chunk past M fetch valid bytes
  // that are never multiplied into a stored element)
  size_t a_row_off[2];
  unsigned a_k[2], b_k[2], b_col[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const unsigned slot = (wave + 4 * i) * 64 + lane;
    const unsigned row = slot >> 3, pc = slot & 7u;
    a_k[i] = (pc ^ ((row >> 1) & 7u)) * 4;
    a_row_off[i] = (size_t)min(row0 + row, N - 1) * lda;
    const unsigned k = slot >> 4, pcb = slot & 15u;
    b_k[i] = k;
    b_col[i] = min(col0 + (pcb ^ ((k & 4u) << 1)) * 4, M - 4);
  }
  auto stage = [&](unsigned buf, unsigned k0) {
    char *base = smem + buf * G::STAGE_BYTES;
#pragma unroll
    for (int i = 0; i < 2; ++i)
      __builtin_amdgcn_global_load_lds((gptr_t)(A + a_row_off[i] + min(k0 + a_k[i], K - 4)), (lptr_t)(base + (wave + 4 * i) * 1024), 16, 0, 0);
#pragma unroll
    for (int i = 0; i < 2; ++i)
      __builtin_amdgcn_global_load_lds((gptr_t)(B + (size_t)min(k0 + b_k[i], K - 1) * M + b_col[i]),
                                       (lptr_t)(base + G::A_BYTES + (wave + 4 * i) * 1024), 16, 0, 0);
  };

  // Steady state (K >= 32): the same pieces with a wavefront-uniform 64-bit base in SGPRs and a constant 32-bit per-lane
  // offset (global_load_lds_dwordx4 v, s[base:base+1]) -- no address arithmetic on the vector ALU.  A slab start past K - 32
  // (beyond the end, or the partial last slab) is clamped to K - 32, uniformly: a partial last slab then sits at the END
  // of its stage (see the last-slab loop).  64 rows x K x 4 B and 32 k-rows x M x 4 B stay below 4 GiB (launcher).
  unsigned voa[2], vob[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const unsigned slot = (wave + 4 * i) * 64 + lane;
    voa[i] = (min(row0 + (slot >> 3), N - 1) - row0) * lda * 4u + a_k[i] * 4u;
    vob[i] = b_k[i] * M * 4u + (b_col[i] - col0) * 4u;
  }
  const unsigned lds_base = (unsigned)(size_t)(__attribute__((address_space(3))) char *)smem;
  auto dma_piece = [&](unsigned buf, unsigned k0, int i) {   // i = 0, 1: A; 2, 3: B
    const unsigned kc = min(k0, K - G::BK);
    const bool is_a = i < 2;
    const int j = is_a ? i : i - 2;
    unsigned long long base = is_a ? (unsigned long long)(A + (size_t)row0 * lda + kc) : (unsigned long long)(B + (size_t)kc * M + col0);
    const unsigned blo = __builtin_amdgcn_readfirstlane((unsigned)base), bhi = __builtin_amdgcn_readfirstlane((unsigned)(base >> 32));
    base = ((unsigned long long)bhi << 32) | blo;
    const unsigned la = lds_base + buf * G::STAGE_BYTES + (is_a ? 0 : G::A_BYTES) + (wave + 4 * j) * 1024;
    const unsigned vo = is_a ? voa[j] : vob[j];
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(vo), "s"(base), "s"(la) : "memory");
  };

  // per-lane fragment addresses inside a stage
  const unsigned a_row = wm * 32 + lo;
  const unsigned a_base = a_row * (G::BK * 4), a_swz = hi ^ ((a_row >> 1) & 7u);               // chunk (2 kg + hi) ^ swz(row)
  const unsigned b_base = G::A_BYTES + (4 * hi) * (G::BN * 4) + ((((wn * 32 + lo) >> 2) ^ (8 * hi)) * 16) + (lo & 3u) * 4;

  f32x16 acc = (f32x16)0.0f;
  struct Frags { f32x4 a; float b[4]; };
  auto read_group = [&](unsigned buf, int kg, Frags &f) {
    const char *base = smem + buf * G::STAGE_BYTES;
    f.a = *(const f32x4 *)(base + a_base + (((unsigned)(2 * kg) ^ a_swz) * 16));
#pragma unroll
    for (int p = 0; p < 4; ++p) f.b[p] = *(const float *)(base + b_base + (kg * 8 + p) * (G::BN * 4));
  };
  auto mfma_group = [&](const Frags &f) {
#pragma unroll
    for (int p = 0; p < 4; ++p) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(f.a[p], f.b[p], acc, 0, 0, 0);
  };
  // C (+)= accumulator: lane owns column lo of 16 rows
  auto write_tile = [&](bool accumulate) {
    const unsigned col = col0 + wn * 32 + lo;
    if (col < M) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const unsigned row = row0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
        if (row < N) {
          float *dst = C + (size_t)row * M + col;
          *dst = accumulate ? acc[r] + *dst : acc[r];
        }
      }
    }
  };

  const unsigned num_tiles = (K + G::BK - 1) / G::BK, steady = num_tiles - 1;
  const bool short_k = K < G::BK;   // a single partial slab: the per-lane clamped form, at the start of stage 0
  // prologue: slabs 0 .. NS-2 (slab NS-1 is requested piece by piece during slab 0); wait for slab 0
  if (short_k) {
#pragma unroll
    for (int s = 0; s < G::NS - 1; ++s) stage(s, s * G::BK);
  } else {
#pragma unroll
    for (int s = 0; s < G::NS - 1; ++s)
#pragma unroll
      for (int i = 0; i < G::L; ++i) dma_piece(s, s * G::BK, i);
  }
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"((G::NS - 2) * G::L) : "memory");
  __builtin_amdgcn_s_barrier();

  // One slab that has a successor.  The wavefront's MFMAs are one dependent chain: the second MFMA of a group cannot issue
  // before the first has gone through the pipe, so that is where everything else goes.  After the first MFMA of group g:
  // DMA piece g of slab t+NS-1 (into the stage slab t-1 left at the last hand-over) and the fragment reads of the NEXT
  // group (by that group's first MFMA they are three MFMAs old: the `s_waitcnt lgkmcnt(0)` the compiler puts there is
  // free).  The slab hand-over -- wait for slab t+1 (all but the pieces of the NS-2 slabs requested after it), barrier,
  // first fragments of slab t+1 -- sits in the same place of the fourth group.
  Frags f0, f1;
  read_group(0, 0, f0);
  unsigned buf = 0;
  auto group = [&](const Frags &cur, auto &&meanwhile) {
    __builtin_amdgcn_sched_barrier(0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.a[0], cur.b[0], acc, 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
    meanwhile();
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int p = 1; p < 4; ++p) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.a[p], cur.b[p], acc, 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
  };
  auto slab = [&](unsigned t) {
    const unsigned next = (buf + 1) % G::NS, refill = (buf + G::NS - 1) % G::NS, kr = (t + G::NS - 1) * G::BK;
    group(f0, [&] { dma_piece(refill, kr, 0); read_group(buf, 1, f1); });
    group(f1, [&] { dma_piece(refill, kr, 1); read_group(buf, 2, f0); });
    group(f0, [&] { dma_piece(refill, kr, 2); read_group(buf, 3, f1); });
    group(f1, [&] {
      dma_piece(refill, kr, 3);
      asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"((G::NS - 2) * G::L) : "memory");   // slab t+1 landed; this stage read out
      __builtin_amdgcn_s_barrier();
      read_group(next, 0, f0);
    });
    buf = next;
  };
  bool flushed = false;
  for (unsigned t0 = 0; t0 < steady; t0 += G::CHUNK) {
    const unsigned tend = min(t0 + (unsigned)G::CHUNK, steady);
    for (unsigned t = t0; t < tend; ++t) slab(t);
    if (tend < steady) {   // the flush rule of tile_body (with BK = 32, "more than 32 k follow" == a further steady slab)
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      write_tile(flushed);
      acc = (f32x16)0.0f;
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      flushed = true;
    }
  }
  {
    const int groups = (int)((K - steady * G::BK) / 8);   // the last slab, full or partial
    const int shift = short_k ? 0 : 4 - groups;            // fetched as the LAST 32 k of the matrix: its groups start further in
    for (int kg = 0; kg < groups; ++kg) {
      read_group(buf, kg + shift, f0);
      mfma_group(f0);
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // trailing (clamped, never read) refills
  write_tile(flushed);
}

// (launch_small: after the split-K reduce kernel, which it shares with launch_geo)

