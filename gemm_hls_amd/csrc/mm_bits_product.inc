// The mask loop of the packed K x M products, written once: C = COMBINE_k (A AND B) with COMBINE = OR (mm_bits.hip, the
// Boolean semiring) or XOR (mm_bits_gf2.hip, the field GF(2)).  Included inside namespace mm's anonymous namespace, after
// mm_common.h.

constexpr unsigned kThreads = 256;
constexpr unsigned kTileRows = 64;       // rows of C per workgroup: 4 wavefronts x kWaveRows
constexpr unsigned kWaveRows = 16;       // rows per wavefront = accumulator rows per thread
constexpr unsigned kSlab = 32;           // k per slab: one word of A per row

// One workgroup: 64 rows x 64 W words of C.  The lanes of a wavefront span the words (W consecutive words per lane), its 16
// rows are shared by all of them, so A's bit for (row, k) is wave-uniform: the mask is one scalar instruction, and
// acc |= mask & b one vector instruction per W-th of 32 W outputs (XOR: acc ^= mask & b, two).  B's words are read from LDS
// once per k for all 16 rows.
// VEC: B in 16-byte and C in 8-byte accesses wherever a whole access lies inside the row's words (ldb % 4 == 0, ldc % 2 == 0,
// aligned bases and batch strides: the launcher's rule); everything else word by word.  Rows >= N, words >= ceil(M / 32), k
// >= K are predicated: no address outside an operand is formed, no word beyond a row's word count is touched.  Rows of B at
// k >= K are staged as 0 and A's last word is masked, so under XOR too no padding bit of either operand contributes.
template <int W, bool VEC, bool XOR>
__global__ __launch_bounds__(kThreads) void bits_gemm_kernel(const uint32_t *__restrict__ A, const uint32_t *__restrict__ B,
                                                             uint32_t *__restrict__ C, unsigned N, unsigned K, unsigned M,
                                                             size_t lda, size_t ldb, size_t ldc, unsigned tiles_w,
                                                             unsigned tiles, size_t stride_a, size_t stride_b,
                                                             size_t stride_c, int seed) {
  constexpr unsigned TW = 64 * W;                          // words of C per workgroup row
  constexpr unsigned PER = VEC ? 4 : 1;                    // words per staging access
  constexpr unsigned NL = kSlab * TW / PER / kThreads;     // staging accesses per thread and slab
  constexpr unsigned RUN = TW / PER;                       // staging accesses per k row
  __shared__ __attribute__((aligned(16))) uint32_t sB[kSlab][TW];
  __shared__ uint32_t sA[kTileRows];

  const unsigned tid = threadIdx.x, lane = tid & 63;
  const unsigned wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const unsigned e = blockIdx.x / tiles, t = blockIdx.x - e * tiles;
  A += e * stride_a;
  B += e * stride_b;
  C += e * stride_c;
  const unsigned row0 = (t / tiles_w) * kTileRows, w0 = (t % tiles_w) * TW;
  const unsigned mw = (M + 31) / 32, kw = (K + 31) / 32;
  const uint32_t k_tail = (K & 31) ? (1u << (K & 31)) - 1 : ~0u;   // A's padding never contributes

  uint32_t acc[kWaveRows][W];
#pragma unroll
  for (unsigned r = 0; r < kWaveRows; ++r)
#pragma unroll
    for (int j = 0; j < W; ++j) acc[r][j] = 0;

  uint32_t rb[NL][PER];   // the next slab of B, and of A, on their way to LDS
  uint32_t ra = 0;
  auto load = [&](unsigned s) {
#pragma unroll
    for (unsigned i = 0; i < NL; ++i) {
      const unsigned idx = tid + kThreads * i, k = s * kSlab + idx / RUN, w = w0 + (idx % RUN) * PER;
#pragma unroll
      for (unsigned j = 0; j < PER; ++j) rb[i][j] = 0;
      if (k >= K) continue;
      const uint32_t *src = B + (size_t)k * ldb + w;
      if (VEC && w + PER <= mw) {
        const uint4 v = *reinterpret_cast<const uint4 *>(src);
        rb[i][0] = v.x;
        if constexpr (PER == 4) { rb[i][1] = v.y; rb[i][2] = v.z; rb[i][3] = v.w; }
      } else {
#pragma unroll
        for (unsigned j = 0; j < PER; ++j)
          if (w + j < mw) rb[i][j] = src[j];
      }
    }
    if (tid < kTileRows) {
      const unsigned row = row0 + tid;
      ra = row < N ? A[(size_t)row * lda + s] : 0u;
      if (s == kw - 1) ra &= k_tail;
    }
  };

  if (kw) load(0);
  for (unsigned s = 0; s < kw; ++s) {
    __syncthreads();   // the previous slab has been read
#pragma unroll
    for (unsigned i = 0; i < NL; ++i) {
      const unsigned idx = tid + kThreads * i;
      uint32_t *dst = &sB[idx / RUN][(idx % RUN) * PER];
      if constexpr (PER == 4) *reinterpret_cast<uint4 *>(dst) = make_uint4(rb[i][0], rb[i][1], rb[i][2], rb[i][3]);
      else *dst = rb[i][0];
    }
    if (tid < kTileRows) sA[tid] = ra;
    __syncthreads();
    if (s + 1 < kw) load(s + 1);

    uint32_t a[kWaveRows], any = 0;   // scalar registers: the wavefront's 16 words of A
#pragma unroll
    for (unsigned r = 0; r < kWaveRows; ++r) {
      a[r] = __builtin_amdgcn_readfirstlane(sA[wave * kWaveRows + r]);
      any |= a[r];
    }
    // only the k some row of the wavefront has set: all-zero words of A cost nothing (the time depends on the data); a k no
    // row has set contributes nothing under either combine
    // (unrolled over the 32 bits: a constant bit position is what makes the mask one scalar bit-field extract)
#pragma unroll
    for (unsigned bit = 0; bit < kSlab; ++bit) {
      if (!((any >> bit) & 1u)) continue;
      uint32_t b[W];
      if constexpr (W == 2) {
        const uint2 v = *reinterpret_cast<const uint2 *>(&sB[bit][lane * 2]);
        b[0] = v.x;
        b[1] = v.y;
      } else {
        b[0] = sB[bit][lane];
      }
#pragma unroll
      for (unsigned r = 0; r < kWaveRows; ++r) {
        const uint32_t mask = (uint32_t)((int)(a[r] << (31 - bit)) >> 31);   // the bit, sign-extended
#pragma unroll
        for (int j = 0; j < W; ++j) {
          if constexpr (XOR) acc[r][j] ^= mask & b[j];
          else acc[r][j] |= mask & b[j];
        }
      }
    }
  }

  const uint32_t m_tail = (M & 31) ? (1u << (M & 31)) - 1 : ~0u;   // C's padding is written 0
  const unsigned w = w0 + lane * W;
  if (w >= mw) return;   // (no barrier follows)
#pragma unroll
  for (unsigned r = 0; r < kWaveRows; ++r) {
    const unsigned row = row0 + wave * kWaveRows + r;
    if (row >= N) break;
    uint32_t *cp = C + (size_t)row * ldc + w;
    if constexpr (VEC && W == 2) {
      if (w + 2 <= mw) {
        uint2 v = make_uint2(acc[r][0], acc[r][1]);
        if (seed) {
          const uint2 o = *reinterpret_cast<const uint2 *>(cp);
          if constexpr (XOR) { v.x ^= o.x; v.y ^= o.y; }
          else { v.x |= o.x; v.y |= o.y; }
        }
        if (w + 2 == mw) v.y &= m_tail;
        *reinterpret_cast<uint2 *>(cp) = v;
        continue;
      }
    }
#pragma unroll
    for (int j = 0; j < W; ++j) {
      if (w + j >= mw) break;
      uint32_t v = acc[r][j];
      if (seed) v = XOR ? v ^ cp[j] : v | cp[j];
      if (w + j == mw - 1) v &= m_tail;
      cp[j] = v;
    }
  }
}

template <int W, bool VEC, bool XOR>
int launch_gemm(hipStream_t s, const BitsProblem &p) {
  const unsigned tiles_w = ((p.m + 31) / 32 + 64 * W - 1) / (64 * W), tiles_r = (p.n + kTileRows - 1) / kTileRows;
  const unsigned long long grid = (unsigned long long)tiles_w * tiles_r * p.batch;
  if (grid > 0x7fffffffull) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL((bits_gemm_kernel<W, VEC, XOR>), dim3((unsigned)grid), dim3(kThreads), 0, s, p.a, p.b, p.c, p.n, p.k, p.m,
                     p.lda, p.ldb, p.ldc, tiles_w, tiles_w * tiles_r, p.stride_a, p.stride_b, p.stride_c, p.seed ? 1 : 0);
  return (int)hipGetLastError();
}
