// fp32 matrix-core family, part 3 of 3: stream-K -- the launch forms for problems of a few partial rounds of tiles (single ranges;
// teams with the last-arriver / fix-up-kernel / counter-ticket combines), their kernels, plans and launchers.  Included by
// mm_mfma_f32.hip inside namespace mm::(anonymous), after mm_mfma_f32_tile.inc (every form runs tile_body).

// ---- stream-K (round 3): problems of a few partial rounds of tiles ------------------------------------------------
// A launch runs in whole rounds of resident workgroups, so 2560^3 (400 tiles of 128 x 128 for 512 slots) or 3072^3 (576
// tiles: one full round and an eighth) leave a large part of the chip idle in their last round.  Here the job's
// (tile, 32-deep slab) units are dealt out to `gridDim.x` persistent workgroups in equal contiguous ranges; a workgroup
// walks its range tile by tile.  A tile whose whole K falls into one range is written to C directly; the head and tail
// tiles of a range are written to the workgroup's two 128 x 128 scratch slots, and a second kernel adds the slots of every
// split tile in ascending k -- no atomics, same bits run to run.  Needs K % BK == 0 (whole slabs) and row-major A.
__device__ __forceinline__ unsigned sk_range_begin(unsigned long long units, unsigned w, unsigned nwg) {
  return (unsigned)(units * w / nwg);
}

template <typename G>
__global__ __launch_bounds__(G::THREADS, G::MIN_WAVES) void mfma_f32_streamk_kernel(const float *__restrict__ A,
                                                                                      const float *__restrict__ B,
                                                                                      float *__restrict__ C, unsigned N, unsigned K,
                                                                                      unsigned M, unsigned tiles_n, unsigned tiles_m,
                                                                                      unsigned kBand, unsigned spt,
                                                                                      float *__restrict__ slots) {
  const unsigned nwg = gridDim.x;
  const unsigned w = xcd_remap(blockIdx.x, nwg);   // an XCD's workgroups own one contiguous stretch of the unit order
  const unsigned long long units = (unsigned long long)tiles_n * tiles_m * spt;
  const unsigned u0 = sk_range_begin(units, w, nwg), u1 = sk_range_begin(units, w + 1, nwg);
  const unsigned first_tile = u0 / spt;
  for (unsigned u = u0; u < u1;) {
    const unsigned tile = u / spt, s0 = u - tile * spt, s1 = min(spt, s0 + (u1 - u));
    unsigned row0, col0;
    band_origin(tile, tiles_n, tiles_m, kBand, G::BM, G::BN, row0, col0);
    const unsigned kbeg = s0 * G::BK, klen = (s1 - s0) * G::BK;
    const float *a = A + kbeg, *b = B + (size_t)kbeg * M;
    if (s0 == 0 && s1 == spt) {
      tile_body<G, false>(a, b, C, N, klen, M, K, M, N, M, row0, col0);
    } else {   // head (slot 0) or tail (slot 1) of this workgroup's range: into its scratch slot, addressed like a C with ldc = BN
      float *slot = slots + ((size_t)w * 2 + (tile != first_tile)) * (G::BM * G::BN);
      float *base = (float *)((unsigned long long)slot - ((unsigned long long)row0 * G::BN + col0) * sizeof(float));
      tile_body<G, false>(a, b, base, N, klen, M, K, G::BN, ~0u, ~0u, row0, col0);
    }
    u += s1 - s0;
    __syncthreads();   // the next segment's prologue overwrites the LDS ring
  }
}

// Stream-K in TEAMS (what the shape-adaptive rule and f32_splitk = 0 run; 9 = the single-range form above, kept as an
// independent cross-check).  Same idea of unit ranges, two changes.
//
// Teams.  With one range per workgroup, neighbouring workgroups sit at different k offsets of neighbouring tiles, so no two
// of them ever want the same A or B slab at the same time: the XCD's L2 shares nothing and the launch becomes fabric-bound
// (3968^3: 3.9 GB fetched against 0.93 GB for whole tiles, 133 TF; 4096^3, where the ranges happen to be whole tiles: 0.80
// GB, 146 TF -- profiles/r03w).  So the ranges go to TEAMS of sr x sc workgroups inside one XCD: the tile grid is cut into
// super-tiles of sr x sc tiles, a team walks its range of (super-tile, slab) units with workgroup `lane` of the team on
// tile `lane` of the super-tile, and all of a team are at the same slab at the same time -- each A slab is wanted by sc
// of them and each B slab by sr.  Per lane this is exactly the scheme above with `teams` ranges.  Tiles of a ragged
// super-tile that fall outside the matrix are skipped by their lane (the same lane in every team).
//
// The combine.  Every segment of a tile other than its lowest-k one is the FIRST segment of the workgroup that owns it (a
// range enters a tile from below only at its own start), and the lowest-k segment is the LAST thing its owner does.  A cut
// tile is finished as C = part(t0) + part(t0 + 1) + ... in ascending k, a fixed order, no atomics on data, in one of two
// ways that perform the same additions in the same order (bit-identical; tests compare them on every stream-K shape):
//
// Combine::LastArriver (what MM_PATH_AUTO runs): ONE kernel in which nobody waits.  Every part of a cut tile -- the lowest-k
// one included -- goes to a scratch slot (agent-scope stores: the reader may sit on another XCD) and raises its flag; right
// after raising it, the part's workgroup LOOKS at the flags of the tile's other parts (no loop): whoever finds them all
// raised is (one of) the last to arrive and adds the slots in ascending k into C.  Raising and looking are ordered like a
// sequentially consistent store and load (sc1 store, s_waitcnt vmcnt(0), sc1 loads: how this target implements seq_cst at
// agent scope), so of two parts finishing at the same moment at least one sees the other; if both do, both write the same
// bits to C -- the gather reads slots only, never C, so it is idempotent (which is why the lowest-k part may NOT live in C:
// a second gatherer would read the first one's sum).  No workgroup ever depends on another one being resident, so the form
// is sound next to any other launch of any process, on CU-masked streams, on partitions and in graphs.  A workgroup owns
// two slots and two flags: index 2w for its first segment (a higher part of some tile), 2w + 1 for its last one (the
// lowest-k part of another tile).  A flag is raised when it holds the launch's epoch (flags_alloc, mm_capi.hip): nothing is
// cleared between launches.  Visibility: slot stores sc1 + s_waitcnt vmcnt(0) + __syncthreads before the flag; on the
// gathering side an agent-scope acquire (buffer_inv sc1) + __syncthreads before plain loads (MI355X_MICROARCH.md,
// inter-workgroup visibility: the valid forms); tests/test_isa_contract.py pins the machine code.
//
// Combine::FixupKernel (f32_splitk 11, the cross-check): the lowest-k part of a cut tile goes to C, the other parts to their
// slots (plain stores, no flags), and streamk_teams_fixup_kernel below adds the slots on top of C.  Two kernels, no
// inter-workgroup communication at all; 0-3.5 % slower (profiles/r05f_*).
//
// (Rounds 3-4 ran a third form in which the owner of the lowest-k part WAITED inside the launch for the others' flags.  It
// needed every workgroup of the launch -- and of every other launch of its kind, in any process -- to be resident at once,
// which a library cannot guarantee; the last-arriver form is as fast without waiting, so the waiting form is retired:
// HISTORY.md, round 5.)
//
// Combine::Ticket (f32_splitk 12; round 6, VERDICT r5 next 6): the last-arriver idea written in the LANGUAGE's memory model instead of
// this target's -- the canonical last-block pattern.  Every part stores its slot with plain stores, every thread issues an
// agent-scope release fence, the workgroup meets at a barrier, and one thread takes a TICKET with a single agent-scope acq_rel
// read-modify-write on a COUNTER of the tile (not on data): the part that draws ticket parts - 1 knows -- by release / acquire
// through the counter's modification order -- that every other part's slot is visible to it, and gathers in ascending k.  Exactly
// one gatherer, no flag loads, no inline-asm stores, no s_waitcnt contract; the same additions in the same order, hence the same
// bits.  The counter word carries the launch's epoch in its upper 56 bits (a compare-exchange loop, lock-free: a failed exchange
// means another part got its ticket), so nothing is cleared between launches here either.
enum class Combine { FixupKernel, LastArriver, Ticket };

template <typename G, Combine MODE>
__global__ __launch_bounds__(G::THREADS, G::MIN_WAVES) void mfma_f32_streamk_teams_kernel(
    const float *__restrict__ A, const float *__restrict__ B, float *__restrict__ C, unsigned N, unsigned K, unsigned M,
    unsigned tiles_n, unsigned tiles_m, unsigned spt, unsigned sr, unsigned sc, unsigned teams_per_xcd, unsigned teams,
    float *__restrict__ slots, unsigned long long *__restrict__ flags, unsigned long long epoch) {
  __shared__ unsigned gather_here;   // LastArriver: thread 0's verdict for the workgroup
  const unsigned lanes = sr * sc, xcd = blockIdx.x % 8, place = blockIdx.x / 8;
  const unsigned team_in_xcd = place / lanes, lane = place % lanes;
  const unsigned team = team_in_xcd * 8 + xcd, w = team * lanes + lane;   // consecutive teams on consecutive XCDs: fewer teams than places still use all eight
  if (team_in_xcd >= teams_per_xcd || team >= teams) return;     // teams <= 8 x teams_per_xcd, <= units: no empty range
  const unsigned st_rows = (tiles_n + sr - 1) / sr, st_cols = (tiles_m + sc - 1) / sc;
  const unsigned long long units = (unsigned long long)st_rows * st_cols * spt;   // per lane; teams <= units
  const unsigned u0 = sk_range_begin(units, team, teams), u1 = sk_range_begin(units, team + 1, teams);
  for (unsigned u = u0; u < u1;) {
    const unsigned st = u / spt, s0 = u - st * spt, s1 = min(spt, s0 + (u1 - u));
    const unsigned tile_r = (st % st_rows) * sr + lane % sr, tile_c = (st / st_rows) * sc + lane / sr;
    u += s1 - s0;
    if (tile_r >= tiles_n || tile_c >= tiles_m) continue;        // uniform over the workgroup
    const unsigned row0 = tile_r * G::BM, col0 = tile_c * G::BN;
    const unsigned kbeg = s0 * G::BK, klen = (s1 - s0) * G::BK;
    const float *a = A + kbeg, *b = B + (size_t)kbeg * M;
    if (s0 == 0 && s1 == spt) {
      tile_body<G, false>(a, b, C, N, klen, M, K, M, N, M, row0, col0);
    } else if constexpr (MODE == Combine::Ticket) {
      const unsigned u_lo = st * spt, u_hi = u_lo + spt;
      unsigned t0 = team;
      while (t0 > 0 && sk_range_begin(units, t0, teams) > u_lo) --t0;
      unsigned t_end = team + 1;
      while (t_end < teams && sk_range_begin(units, t_end, teams) < u_hi) ++t_end;
      auto part_index = [&](unsigned o) { return 2u * (o * lanes + lane) + (o == t0 ? 1u : 0u); };
      float *slot = slots + (size_t)part_index(team) * (G::BM * G::BN);
      float *base = (float *)((unsigned long long)slot - ((unsigned long long)row0 * G::BN + col0) * sizeof(float));
      tile_body<G, false>(a, b, base, N, klen, M, K, G::BN, ~0u, ~0u, row0, col0);   // plain stores
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");   // every thread: its slot stores are ordered before whatever follows the barrier
      __syncthreads();
      if (threadIdx.x == 0) {
        // the tile's counter = the flag word of its lowest-k part (one cut tile per workgroup ends there): (epoch tag << 8) | parts arrived
        unsigned long long *counter = flags + part_index(t0);
        const unsigned long long tag = (epoch << 8);
        unsigned long long seen = __hip_atomic_load(counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), want;
        do {
          want = ((seen ^ tag) >> 8) == 0 ? seen + 1 : (tag | 1ull);
        } while (!__hip_atomic_compare_exchange_strong(counter, &seen, want, __ATOMIC_ACQ_REL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        gather_here = (unsigned)(want & 0xffu) == t_end - t0;   // the last ticket of the tile
      }
      __syncthreads();
      if (gather_here) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        constexpr int QUADS = G::BM * G::BN / 4 / G::THREADS;
        f32x4 acc[QUADS];
        const f32x4 *first = (const f32x4 *)(slots + (size_t)part_index(t0) * (G::BM * G::BN));
#pragma unroll
        for (int i = 0; i < QUADS; ++i) acc[i] = first[i * G::THREADS + threadIdx.x];
        for (unsigned o = t0 + 1; o < t_end; ++o) {
          const f32x4 *src = (const f32x4 *)(slots + (size_t)part_index(o) * (G::BM * G::BN));
#pragma unroll
          for (int i = 0; i < QUADS; ++i) acc[i] += src[i * G::THREADS + threadIdx.x];
        }
#pragma unroll
        for (int i = 0; i < QUADS; ++i) {
          const unsigned q = i * G::THREADS + threadIdx.x, row = row0 + q / (G::BN / 4), col = col0 + (q % (G::BN / 4)) * 4;
          if (row < N && col < M) *(f32x4 *)(C + (size_t)row * M + col) = acc[i];
        }
      }
    } else if constexpr (MODE == Combine::LastArriver) {
      // a part of a cut tile.  The tile's parts belong to teams t0 (lowest k: that team's LAST segment, slot / flag 2w' + 1)
      // and t0 + 1 .. t_end - 1 (their FIRST segments, slot / flag 2w'), same lane.
      const unsigned u_lo = st * spt, u_hi = u_lo + spt;
      unsigned t0 = team;
      while (t0 > 0 && sk_range_begin(units, t0, teams) > u_lo) --t0;
      unsigned t_end = team + 1;
      while (t_end < teams && sk_range_begin(units, t_end, teams) < u_hi) ++t_end;
      auto part_index = [&](unsigned o) { return 2u * (o * lanes + lane) + (o == t0 ? 1u : 0u); };
      const unsigned mine = part_index(team);
      float *slot = slots + (size_t)mine * (G::BM * G::BN);
      float *base = (float *)((unsigned long long)slot - ((unsigned long long)row0 * G::BN + col0) * sizeof(float));
      tile_body<G, false, true>(a, b, base, N, klen, M, K, G::BN, ~0u, ~0u, row0, col0);   // slot stores at agent scope
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // every wavefront: its slot stores have reached the agent's coherence point
      __syncthreads();
      if (threadIdx.x == 0) {
        __hip_atomic_store(flags + mine, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // raised = holds this launch's epoch
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the flag is out before the others' flags are looked at (store -> load order)
        unsigned all = 1;
        for (unsigned o = t0; o < t_end; ++o)
          if (o != team && __hip_atomic_load(flags + part_index(o), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != epoch) all = 0;
        if (all) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        gather_here = all;
      }
      __syncthreads();
      if (gather_here) {   // (one of) the last to arrive: C = slot(t0) + slot(t0 + 1) + ... in ascending k, from slots only
        // one slot at a time, all of a thread's quads in flight together: a slot costs one trip to memory, not QUADS of them
        constexpr int QUADS = G::BM * G::BN / 4 / G::THREADS;
        f32x4 acc[QUADS];
        const f32x4 *first = (const f32x4 *)(slots + (size_t)part_index(t0) * (G::BM * G::BN));
#pragma unroll
        for (int i = 0; i < QUADS; ++i) acc[i] = first[i * G::THREADS + threadIdx.x];
        for (unsigned o = t0 + 1; o < t_end; ++o) {
          const f32x4 *src = (const f32x4 *)(slots + (size_t)part_index(o) * (G::BM * G::BN));
#pragma unroll
          for (int i = 0; i < QUADS; ++i) acc[i] += src[i * G::THREADS + threadIdx.x];
        }
#pragma unroll
        for (int i = 0; i < QUADS; ++i) {
          const unsigned q = i * G::THREADS + threadIdx.x, row = row0 + q / (G::BN / 4), col = col0 + (q % (G::BN / 4)) * 4;
          if (row < N && col < M) *(f32x4 *)(C + (size_t)row * M + col) = acc[i];
        }
      }
    } else if (s0 > 0) {   // FixupKernel, not the lowest-k segment: this workgroup's first segment -> its slot
      float *slot = slots + (size_t)w * (G::BM * G::BN);
      float *base = (float *)((unsigned long long)slot - ((unsigned long long)row0 * G::BN + col0) * sizeof(float));
      tile_body<G, false>(a, b, base, N, klen, M, K, G::BN, ~0u, ~0u, row0, col0);
    } else {               // FixupKernel, the lowest-k segment of a split tile: into C; the fix-up kernel adds the others
      tile_body<G, false>(a, b, C, N, klen, M, K, M, N, M, row0, col0);
    }
    __syncthreads();
  }
}

// Team shape for a tile grid: 4, 2 or 1 tiles a side, the largest that divides the grid exactly -- a ragged super-tile idles
// its outside lanes for whole segments and costs more than the sharing returns (profiles/r03w_f32_streamk_teams.txt: 2816^3,
// 22 x 22 tiles, 4 x 4 teams 113 TF against 128; 3584^3, 28 x 28, 140 against 137; 5120^3 146 against 142).  Wider teams
// (8 x 4, 8 x 8) measured no better than 4 x 4 where they divide.
struct TeamShape { unsigned sr, sc; };
static TeamShape streamk_team_shape(unsigned tiles_n, unsigned tiles_m) {
  auto side = [](unsigned t) { return t % 4 == 0 ? 4u : t % 2 == 0 ? 2u : 1u; };
  return {side(tiles_n), side(tiles_m)};
}

// The second kernel of the two-kernel teams form: one workgroup per tile of C.  A tile that one team's range holds whole
// was finished by the main kernel; for a cut tile C already holds the lowest-k part, and the slots of the teams that own
// the other parts (the next teams in range order, same lane) are added on top in ascending k -- the additions of the
// last-arriver form's gather, in its order, by its thread mapping.
template <int BM, int BN, int THREADS>
__global__ __launch_bounds__(THREADS) void streamk_teams_fixup_kernel(const float *__restrict__ slots, float *__restrict__ C, unsigned N,
                                                                       unsigned M, unsigned tiles_n, unsigned tiles_m, unsigned spt,
                                                                       unsigned sr, unsigned sc, unsigned teams) {
  const unsigned tile_r = blockIdx.x % tiles_n, tile_c = blockIdx.x / tiles_n;
  const unsigned lanes = sr * sc, st_rows = (tiles_n + sr - 1) / sr, st_cols = (tiles_m + sc - 1) / sc;
  const unsigned st = (tile_c / sc) * st_rows + tile_r / sr, lane = tile_r % sr + (tile_c % sc) * sr;
  const unsigned long long units = (unsigned long long)st_rows * st_cols * spt;
  const unsigned u_lo = st * spt, u_hi = u_lo + spt;
  unsigned t0 = (unsigned)((unsigned long long)u_lo * teams / units);     // the team whose range holds the tile's first unit
  while (t0 + 1 < teams && sk_range_begin(units, t0 + 1, teams) <= u_lo) ++t0;
  while (t0 > 0 && sk_range_begin(units, t0, teams) > u_lo) --t0;
  unsigned t_end = t0 + 1;
  while (t_end < teams && sk_range_begin(units, t_end, teams) < u_hi) ++t_end;
  if (t_end == t0 + 1) return;                                            // one range holds the whole tile
  const unsigned row0 = tile_r * BM, col0 = tile_c * BN;
  constexpr int QUADS = BM * BN / 4 / THREADS;
  f32x4 acc[QUADS];
#pragma unroll
  for (int i = 0; i < QUADS; ++i) {
    const unsigned q = i * THREADS + threadIdx.x, row = row0 + q / (BN / 4), col = col0 + (q % (BN / 4)) * 4;
    acc[i] = (row < N && col < M) ? *(const f32x4 *)(C + (size_t)row * M + col) : (f32x4)0.0f;
  }
  for (unsigned o = t0 + 1; o < t_end; ++o) {
    const f32x4 *src = (const f32x4 *)(slots + (size_t)(o * lanes + lane) * (BM * BN));
#pragma unroll
    for (int i = 0; i < QUADS; ++i) acc[i] += src[i * THREADS + threadIdx.x];
  }
#pragma unroll
  for (int i = 0; i < QUADS; ++i) {
    const unsigned q = i * THREADS + threadIdx.x, row = row0 + q / (BN / 4), col = col0 + (q % (BN / 4)) * 4;
    if (row < N && col < M) *(f32x4 *)(C + (size_t)row * M + col) = acc[i];
  }
}

// How a problem is dealt out to teams: shared by both forms, so that they cut the same tiles at the same k.
struct TeamPlan { unsigned tiles_n, tiles_m, spt, sr, sc, teams_per_xcd, teams; };
template <typename G>
static TeamPlan streamk_team_plan(const Problem &p) {
  TeamPlan t;
  t.tiles_n = (p.n + G::BM - 1) / G::BM; t.tiles_m = (p.m + G::BN - 1) / G::BN; t.spt = p.k / G::BK;
  const TeamShape ts = streamk_team_shape(t.tiles_n, t.tiles_m);
  t.sr = ts.sr; t.sc = ts.sc;
  t.teams_per_xcd = 64 / (ts.sr * ts.sc);   // 8 XCDs x 64 places
  const unsigned long long super_tiles = (unsigned long long)(t.tiles_n / ts.sr) * (t.tiles_m / ts.sc), units = super_tiles * t.spt;
  // every place gets a team when there is work for it: a team's range is at least 8 slabs (below that the fill and drain
  // of the rings outweigh the slabs -- the chunk floor of split-K) and a tile is cut at most 8 ways (the gather is serial
  // in whoever does it, and a part looks at no more than 7 siblings' flags)
  t.teams = (unsigned)std::max<unsigned long long>(1, std::min<unsigned long long>({8ull * t.teams_per_xcd, units / 8, 8 * super_tiles}));
  return t;
}

// The two-kernel teams form (f32_splitk 11; the cross-check of the default): teams, slots, and the fix-up kernel.  No
// workgroup waits for another one either; the bits of the default form.
template <typename G>
int launch_streamk_teams(hipStream_t s, const Problem &p) {
  const TeamPlan t = streamk_team_plan<G>(p);
  const unsigned nwg = 512;
  static_assert(G::MIN_WAVES == 2, "two workgroups per CU: 64 places per XCD");
  static unsigned long long configured = 0;
  if (int e = ensure_dynamic_lds((const void *)mfma_f32_streamk_teams_kernel<G, Combine::FixupKernel>, G::LDS_BYTES, configured)) return e;
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return (int)e;
  hipMemPool_t pool = nullptr;
  if (int rc = workspace_pool(dev, &pool)) return rc;
  float *slots = nullptr;
  const size_t slot_bytes = (size_t)nwg * G::BM * G::BN * sizeof(float);
  if ((e = hipMallocFromPoolAsync((void **)&slots, slot_bytes, pool, s)) != hipSuccess) return (int)e;
  // debug_poison: NaN in every slot AND in C (pure output: a tile nobody finished then shows as NaN instead of as whatever the buffer held)
  if (tuning(TUNE_DEBUG_POISON) == 1 && ((e = hipMemsetAsync(slots, 0xFF, slot_bytes, s)) != hipSuccess ||
                                         (e = hipMemsetAsync(p.c, 0xFF, (size_t)p.n * p.m * sizeof(float), s)) != hipSuccess)) { (void)hipFreeAsync(slots, s); return (int)e; }
  (void)hipGetLastError();
  hipLaunchKernelGGL((mfma_f32_streamk_teams_kernel<G, Combine::FixupKernel>), dim3(nwg), dim3(G::THREADS), G::LDS_BYTES, s, (const float *)p.a,
                     (const float *)p.b, (float *)p.c, p.n, p.k, p.m, t.tiles_n, t.tiles_m, t.spt, t.sr, t.sc, t.teams_per_xcd, t.teams,
                     slots, (unsigned long long *)nullptr, 0ull);
  int rc = (int)hipGetLastError();
  if (rc == 0 && t.teams > 1) {
    hipLaunchKernelGGL((streamk_teams_fixup_kernel<G::BM, G::BN, G::THREADS>), dim3(t.tiles_n * t.tiles_m), dim3(G::THREADS), 0, s,
                       (const float *)slots, (float *)p.c, p.n, p.m, t.tiles_n, t.tiles_m, t.spt, t.sr, t.sc, t.teams);
    rc = (int)hipGetLastError();
  }
  const hipError_t f = hipFreeAsync(slots, s);
  return rc ? rc : (int)f;
}

// Stream-K as MM_PATH_AUTO runs it (f32_splitk 0): teams, two slots and two flags per workgroup, the last part to arrive
// gathers -- one kernel, no workgroup waits for another one (Combine::LastArriver above).  Flags hold the launch's epoch
// (flags_alloc, mm_capi.hip), so nothing is cleared between launches.
template <typename G, Combine MODE = Combine::LastArriver>
int launch_streamk_arrive(hipStream_t s, const Problem &p) {
  const TeamPlan t = streamk_team_plan<G>(p);
  const unsigned nwg = 512;
  static_assert(G::MIN_WAVES == 2, "two workgroups per CU: 64 places per XCD");
  static unsigned long long configured = 0;
  if (int e = ensure_dynamic_lds((const void *)mfma_f32_streamk_teams_kernel<G, MODE>, G::LDS_BYTES, configured)) return e;
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return (int)e;
  hipMemPool_t pool = nullptr;
  if (int rc = workspace_pool(dev, &pool)) return rc;
  float *slots = nullptr;
  void *flags = nullptr;
  unsigned long long epoch = 0;
  const size_t slot_bytes = (size_t)2 * nwg * G::BM * G::BN * sizeof(float);
  int rc = (int)hipMallocFromPoolAsync((void **)&slots, slot_bytes, pool, s);
  if (rc == 0 && tuning(TUNE_DEBUG_POISON) == 1) rc = (int)hipMemsetAsync(slots, 0xFF, slot_bytes, s);   // debug_poison: NaN in every slot ...
  if (rc == 0 && tuning(TUNE_DEBUG_POISON) == 1) rc = (int)hipMemsetAsync(p.c, 0xFF, (size_t)p.n * p.m * sizeof(float), s);   // ... and in C (pure output): an unfinished tile shows
  if (rc == 0) rc = flags_alloc(dev, s, (size_t)2 * nwg * sizeof(unsigned long long), &flags, &epoch);
  if (rc == 0) {
    (void)hipGetLastError();
    hipLaunchKernelGGL((mfma_f32_streamk_teams_kernel<G, MODE>), dim3(nwg), dim3(G::THREADS), G::LDS_BYTES, s,
                       (const float *)p.a, (const float *)p.b, (float *)p.c, p.n, p.k, p.m, t.tiles_n, t.tiles_m, t.spt, t.sr, t.sc,
                       t.teams_per_xcd, t.teams, slots, (unsigned long long *)flags, epoch);
    rc = (int)hipGetLastError();
  }
  const hipError_t f1 = flags ? hipFreeAsync(flags, s) : hipSuccess, f2 = slots ? hipFreeAsync(slots, s) : hipSuccess;
  return rc ? rc : f1 != hipSuccess ? (int)f1 : (int)f2;
}

// C tile = sum of the scratch slots of the workgroups whose ranges cut it, ascending k.  One workgroup per tile; tiles that
// one range covered whole were written by the main kernel and are skipped.
template <int BM, int BN>
__global__ __launch_bounds__(256) void streamk_fixup_kernel(const float *__restrict__ slots, float *__restrict__ C, unsigned N,
                                                            unsigned M, unsigned tiles_n, unsigned tiles_m, unsigned kBand,
                                                            unsigned spt, unsigned nwg) {
  const unsigned tile = blockIdx.x;
  const unsigned long long units = (unsigned long long)tiles_n * tiles_m * spt;
  const unsigned u_lo = tile * spt, u_hi = u_lo + spt;
  unsigned w = (unsigned)((unsigned long long)u_lo * nwg / units);
  while (w + 1 < nwg && sk_range_begin(units, w + 1, nwg) <= u_lo) ++w;
  while (w > 0 && sk_range_begin(units, w, nwg) > u_lo) --w;
  if (sk_range_begin(units, w + 1, nwg) >= u_hi) return;   // one range holds the whole tile
  unsigned row0, col0;
  band_origin(tile, tiles_n, tiles_m, kBand, BM, BN, row0, col0);
  constexpr int QUADS = BM * BN / 4 / 256;
  f32x4 acc[QUADS];
#pragma unroll
  for (int i = 0; i < QUADS; ++i) acc[i] = (f32x4)0.0f;
  for (; w < nwg && sk_range_begin(units, w, nwg) < u_hi; ++w) {
    if (sk_range_begin(units, w + 1, nwg) == sk_range_begin(units, w, nwg)) continue;   // an empty range (fewer units than workgroups) wrote nothing
    const unsigned first_tile = sk_range_begin(units, w, nwg) / spt;
    const f32x4 *slot = (const f32x4 *)(slots + ((size_t)w * 2 + (tile != first_tile)) * (BM * BN));
#pragma unroll
    for (int i = 0; i < QUADS; ++i) acc[i] += slot[i * 256 + threadIdx.x];
  }
#pragma unroll
  for (int i = 0; i < QUADS; ++i) {
    const unsigned q = i * 256 + threadIdx.x, row = row0 + q / (BN / 4), col = col0 + (q % (BN / 4)) * 4;
    if (row < N && col < M) *(f32x4 *)(C + (size_t)row * M + col) = acc[i];
  }
}

template <typename G>
int launch_streamk(hipStream_t s, const Problem &p) {
  const unsigned tiles_n = (p.n + G::BM - 1) / G::BM, tiles_m = (p.m + G::BN - 1) / G::BN, spt = p.k / G::BK;
  const unsigned nwg = 256 * G::MIN_WAVES;
  static unsigned long long configured = 0;
  if (int e = ensure_dynamic_lds((const void *)mfma_f32_streamk_kernel<G>, G::LDS_BYTES, configured)) return e;
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return (int)e;
  hipMemPool_t pool = nullptr;
  if (int rc = workspace_pool(dev, &pool)) return rc;
  float *slots = nullptr;
  const size_t slot_bytes = (size_t)nwg * 2 * G::BM * G::BN * sizeof(float);
  if ((e = hipMallocFromPoolAsync((void **)&slots, slot_bytes, pool, s)) != hipSuccess) return (int)e;
  // debug_poison: NaN in every slot AND in C (pure output: a tile nobody finished then shows as NaN instead of as whatever the buffer held)
  if (tuning(TUNE_DEBUG_POISON) == 1 && ((e = hipMemsetAsync(slots, 0xFF, slot_bytes, s)) != hipSuccess ||
                                         (e = hipMemsetAsync(p.c, 0xFF, (size_t)p.n * p.m * sizeof(float), s)) != hipSuccess)) { (void)hipFreeAsync(slots, s); return (int)e; }
  (void)hipGetLastError();
  const unsigned kband = band_rows(G::BM, G::BN, G::MIN_WAVES);
  hipLaunchKernelGGL((mfma_f32_streamk_kernel<G>), dim3(nwg), dim3(G::THREADS), G::LDS_BYTES, s, (const float *)p.a, (const float *)p.b,
                     (float *)p.c, p.n, p.k, p.m, tiles_n, tiles_m, kband, spt, slots);
  int rc = (int)hipGetLastError();
  if (rc == 0) {
    hipLaunchKernelGGL((streamk_fixup_kernel<G::BM, G::BN>), dim3(tiles_n * tiles_m), dim3(256), 0, s, (const float *)slots, (float *)p.c,
                       p.n, p.m, tiles_n, tiles_m, kband, spt, nwg);
    rc = (int)hipGetLastError();
  }
  const hipError_t f = hipFreeAsync(slots, s);
  return rc ? rc : (int)f;
}

