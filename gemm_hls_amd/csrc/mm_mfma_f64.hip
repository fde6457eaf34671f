// fp64 (Multiply, Add) fast path for gfx950: C[N x M] = A[N x K] . B[K x M], row-major, on
// v_mfma_f64_16x16x4_f64.  Same organisation as the fp32 kernel (mm_mfma_f32.hip: resident output
// tile in accumulation registers for the whole K loop -- kernel/Compute.cpp:58-60 -- A row-panel /
// B column-panel k-slabs DMA'd to an LDS ring -- the role of kernel/Memory.cpp's ReadA/ReadB/FeedB),
// with the fragment shapes of the f64 instruction:
//   operands: lane l supplies A[i = l&15][k = l>>4] and B[k = l>>4][j = l&15] (one f64 each);
//   result:   4 f64 per lane, column l&15, rows (l>>4) + 4*r   (NOT the f32 row map).
// Workgroup = WM x WN wavefronts, each owning 64 x 64 of C as 4 x 4 accumulators (128 registers).
// K slab = 16 doubles: an A row is 128 B = 8 chunks of 16 B, XOR-swizzled with (row>>1)&7 on the
// DMA source address so that every ds_read_b128 service group touches 16 distinct 16-B slots.
// Fragment reads (all ds_read_b128 = 2 doubles):
//   A: lane reads A[row = l&15][2 consecutive k at k-offset 2*(l>>4)] -> feeds 2 MFMAs of an
//      8-deep k-group, MFMA p using k = {2g+p : g = 0..3};
//   B: lane reads B[k = 2*(l>>4)+p][2 consecutive columns 2*(l&15)..+1] -> feeds 2 column
//      accumulators (accumulator t holds columns 2*j+t), so the epilogue stores 16 B per lane.
// Accumulation: one f64 fma chain per element (k order 0,2,4,6,1,3,5,7 inside each group).
// Edges: N arbitrary, M % 2 == 0, K % 8 == 0 (the reference's own contract for double is
// K % 8 == 0 and M % 8 == 0, host/RunHardware.cpp:50-61); other shapes -> predicated kernels.
#include <cstdlib>

#include "mm_common.h"

namespace mm {
namespace {

using f64x2 = __attribute__((ext_vector_type(2))) double;
using f64x4 = __attribute__((ext_vector_type(4))) double;
typedef const __attribute__((address_space(1))) void *gptr_t;
typedef __attribute__((address_space(3))) void *lptr_t;

template <int WM_, int WN_, int NS_, bool PIPE_ = true, int TM_ = 4, int TP_ = 2, int MIN_WAVES_ = 2>
struct GeoD {
  static constexpr int WM = WM_, WN = WN_, NS = NS_;
  static constexpr bool PIPE = PIPE_;  // pinned, software-pipelined fragment reads (see the main loop)
  static constexpr int TM = TM_, TP = TP_;           // row tiles x pairs of column tiles of 16 (4 x 2: a 64 x 64 wavefront tile)
  static constexpr int MIN_WAVES = MIN_WAVES_;       // wavefronts per SIMD the kernel is compiled for
  static constexpr int NW = WM * WN, THREADS = NW * 64;
  static constexpr int WTM = TM * 16, WTN = TP * 32;  // the wavefront's tile
  static constexpr int BM = WM * WTM, BN = WN * WTN, BK = 16;
  static constexpr int CPR = 8;                      // 16-B chunks per A row (16 doubles)
  static constexpr int A_BYTES = BM * BK * 8, B_BYTES = BK * BN * 8;
  static constexpr int STAGE_BYTES = A_BYTES + B_BYTES, LDS_BYTES = NS * STAGE_BYTES;
  static constexpr int NA = A_BYTES / 1024, NB = B_BYTES / 1024;
  static constexpr int LA = NA / NW, LB = NB / NW;
  static constexpr int KG = BK / 8;
  static constexpr int BCH = BN / 2;                 // 16-B chunks per B k-row
  static_assert(NA % NW == 0 && NB % NW == 0, "DMA split");
  static_assert(LDS_BYTES <= 160 * 1024, "LDS");
};

#include "mm_mfma_f64_kernels.inc"

using D0 = GeoD<4, 2, 2>;  // 256 x 128 tile, 8 wavefronts (2 per SIMD), 96 KiB LDS
using D1 = GeoD<2, 2, 2>;  // 128 x 128 tile, 4 wavefronts, 64 KiB LDS: two workgroups per CU (small / mid-size shapes)
using D0R1 = GeoD<4, 2, 2, false>;  // the same tiles with the compiler-placed schedule they first shipped with (f64_variant 2 / 3)
using D1R1 = GeoD<2, 2, 2, false>;
// Problems below a round of 128 x 128 tiles (round 3): a 32 x 32 wavefront tile (2 x 1 x 2 accumulators), 64 x 64 per workgroup,
// 32 KiB of LDS, compiled for four wavefronts per SIMD.  Same fma chain per element as the others: identical bits.
using DS = GeoD<2, 2, 2, false, 2, 1, 4>;

// The table: one row per answer of resolve(), read by the names and mm_kernel_info; launch_resolved pairs each with its geometry.
// Efficiency: pinned schedule + scalar-base DMA, 76.4 TF of 78.6 (profiles/r02z_f64_scalar_base_dma.log)
constexpr KernelRow kTable[] = {
    kernel_row<D0>("mfma_f64_256x128x16_w8", nullptr, 16, 4, 0.97),
    kernel_row<D1>("mfma_f64_128x128x16_w4x2", nullptr, 16, 4, 0.97),
    kernel_row<D0R1>("mfma_f64_256x128x16_w8_compiler_placed", nullptr, 16, 4, 0.97),
    kernel_row<D1R1>("mfma_f64_128x128x16_w4x2_compiler_placed", nullptr, 16, 4, 0.97),
    kernel_row<DS>("mfma_f64_64x64x16_w4x4", nullptr, 16, 4, 0.97),
};

}  // namespace

bool mfma_f64_serves(const Problem &p) {
  if (!(p.n >= 1 && p.m >= 2 && p.k >= 8 && p.m % 2 == 0 && p.k % 8 == 0)) return false;
  return !p.a_transposed || (p.n >= 2 && p.n % 2 == 0);
}

// One launch of mfma_f64_kernel<F, G, AT>: the problem at (a, b, c), or (F != Form::Single) the p.batch elements of p
template <Form F, typename G, bool AT>
static int launch_at(hipStream_t s, const Problem &p) {
  const unsigned tiles_n = (p.n + G::BM - 1) / G::BM, tiles_m = (p.m + G::BN - 1) / G::BN;
  const unsigned grid = tiles_n * tiles_m * (F == Form::Single ? 1u : p.batch);
  const unsigned band = band_rows(G::BM, G::BN, G::BM * G::BN <= 64 * 64 ? 4 : G::BM * G::BN <= 128 * 128 ? 2 : 1);
  static unsigned long long configured = 0;   // one per instantiation of this function, so one per kernel
  if (int e = ensure_dynamic_lds((const void *)mfma_f64_kernel<F, G, AT>, G::LDS_BYTES, configured)) return e;
  hipLaunchKernelGGL((mfma_f64_kernel<F, G, AT>), dim3(grid), dim3(G::THREADS), G::LDS_BYTES, s, (const double *)p.a,
                     (const double *)p.b, (double *)p.c, p.n, p.k, p.m, tiles_n, tiles_m, band,
                     F == Form::Single ? 1u : p.batch, p.stride_a, p.stride_b, p.stride_c);
  return (int)hipGetLastError();
}

template <Form F, typename G>
static int launch_d(hipStream_t s, const Problem &p) {
  return p.a_transposed ? launch_at<F, G, true>(s, p) : launch_at<F, G, false>(s, p);
}

static int mfma_f64_tile(const Problem &p) {  // 0: 256x128, 1: 128x128, 4: 64x64
  const int v = tuning(TUNE_F64_VARIANT);
  if (v == 4) return 4;
  if (v >= 0) return v & 1;
  // measured (profiles/r02z_f64_pinned_schedule.log): with two workgroups per CU the small tile sustains the same
  // 74.6 TF as the large one at 16384^3; the large one is kept on ties (fewer, larger DMA streams per CU)
  // 64 x 64 (round 3): compiler-placed, four workgroups per CU; efficiency fitted to profiles/r03y_f64_small_tile.txt
  static const TileCandidate cands[] = {{0, 256, 128, 1, 1.00}, {1, 128, 128, 2, 0.995}, {4, 64, 64, 4, 0.90}};
  return pick_tile(cands, 3, p.n, p.m, nullptr, p.batch);   // (a batched launch: its elements' tiles together)
}

// One resolver for mm_kernel_name and the launcher: bit 0 = the 128 x 128 tile, bit 1 = the compiler-placed schedule
// with per-lane 64-bit DMA addresses (f64_variant 2 / 3, and every problem beyond the scalar-base DMA's reach).
static int resolve(const Problem &p) {
  if (!mfma_f64_serves(p) || tuning(TUNE_F64_VARIANT) > 4) return -1;   // f64_variant: -1 (by shape), 0 .. 4
  // scalar-base DMA: 32-bit byte offsets inside a tile's rows (256 rows x K x 8 B, 16 k-rows x M x 8 B) and K >= BK
  const bool sdma_fits = p.k >= 16 && 256ull * (p.a_transposed ? 1ull : p.k) * 8ull < (1ull << 32) &&
                         16ull * (p.m > p.n ? p.m : p.n) * 8ull < (1ull << 32);
  const int tile = mfma_f64_tile(p);
  if (tile == 4) return 4;   // its own (per-lane 64-bit) DMA addresses: no reach limit
  return tile | ((tuning(TUNE_F64_VARIANT) >= 2 || !sdma_fits) ? 2 : 0);
}

const char *mfma_f64_name(const Problem &p) {
  const int r = resolve(p);
  return r < 0 ? "unsupported" : kTable[r].name;
}
const KernelRow &mfma_f64_row(const Problem &p) { return kTable[resolve(p) < 0 ? 0 : resolve(p)]; }   // (unsupported: the default tile)

template <Form F>
static int launch_resolved(hipStream_t s, const Problem &p, int r) {   // r: resolve()'s answer
  switch (r) {
    case 0: return launch_d<F, D0>(s, p);
    case 1: return launch_d<F, D1>(s, p);
    case 2: return launch_d<F, D0R1>(s, p);
    case 3: return launch_d<F, D1R1>(s, p);
    case 4: return launch_d<F, DS>(s, p);
  }
  return kErrNotSupported;
}

// Batched (mm_gemm_batched_*): the same resolver on the whole batch (Problem::batch copies of the tile grid; every f64
// geometry gives the same bits), the kernels' batched forms (Form::Seeded for p.seed); no workspace is involved in any f64 launch.
int mfma_f64_batched_resolve(const Problem &p) { return resolve(p); }
const char *mfma_f64_batched_name(const Problem &p) { return mfma_f64_name(p); }
int launch_mfma_f64_batched(hipStream_t s, const Problem &p, int r) {
  return p.seed ? launch_resolved<Form::Seeded>(s, p, r) : launch_resolved<Form::Batched>(s, p, r);
}

int launch_mfma_f64(hipStream_t s, const Problem &p) { return launch_resolved<Form::Single>(s, p, resolve(p)); }

}  // namespace mm
