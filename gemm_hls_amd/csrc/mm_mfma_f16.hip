// half (Multiply, Add) fast path for gfx950: C[N x M] = A[N x K] . B[K x M], row-major binary16
// in and out, on the f16 matrix-core instructions (v_mfma_f32_16x16x32_f16 / v_mfma_f32_32x32x16_f16).
//
// Numerical contract: products of two binary16 values are exact in f32;
// they are accumulated in f32 by the matrix core and rounded to binary16 ONCE on store.  The
// reference's HLS kernel accumulates in half (and overflows to inf beyond K ~ 2000 on its own
// [1,10) inputs); the k-ordered kernel (MM_PATH_ORDERED) reproduces that behaviour exactly.
//
// Kernels in this file (what MM_PATH_AUTO can dispatch, plus one cross-check):
//   pingpong_16x16x32   default: 256 x 256 tile, ping-pong schedule, A in full-line double slabs, the 16x16x32
//                       instruction (K % 64 == 0, K >= 256, row-major A)
//   pingpong_32x32x16   the same tile / rings / protocol on the 32x32x16 instruction: the independently written
//                       cross-check of the default (f16_variant 100); also what round 2 shipped
//   pingpong_k32        32-deep slabs with 64-byte A rows (K % 32 == 0, K >= 128), row-major and K x N A
//   slab64              one barrier per 64-deep slab (K % 16 == 0; any N; 256 x 256, or 128 x 256 for small problems)
// The two pingpong_NxNxK kernels share their protocol and geometry with the int8 pair: mm_pingpong2.h.
// Each is one row of kTable at the end of mm_mfma_f16_kernels.inc (name, wide twin, geometry, instruction, efficiency); this unit
// holds the rules that pick a row (resolve) and launches it through the include's launch_kind.
// The schedules and ablations these went through (lock step, early barrier, DMA cache policies, no-DMA / no-read power
// breakdown, the 384 x 256 tile) live in tools/lab/lab_mfma_f16.hip -> tools/lab/libmm_gemm_amd_lab.so.
//
// Common organisation (as mm_mfma_f32.hip: resident output tile, LDS ring fed by global_load_lds):
//   B fragment: B is K x M row-major, the operand wants consecutive k of ONE column, so the
//     LDS image stays row-major [k][256 cols] and the operand is gathered by two
//     ds_read_b64_tr_b16 (hardware 4 x 16 transpose: lane i of a 16-lane group receives column i
//     of the [4 k][16 col] block whose rows the group's lanes point at;
//     out[i][j] = in[4j + (i>>2)][i&3], profiles/r01_probe_ds_read_b64_tr_b16.txt).
//     A B k-row is 512 B, so the 4 rows of a block would share banks; the 16-B chunk index is
//     XORed with (k&3)<<2 on the DMA source side, which spreads the 4 rows over the 4 quadrants
//     of the 256-B bank row: each half-wave then reads 256 distinct bytes.
// Edges: N arbitrary, K % 16 == 0, M % 8 == 0 (reference contract for half: K % 32, M % 32).
#include <cstdlib>
#include <type_traits>

#include "mm_common.h"
#include "mm_pingpong2.h"

namespace mm {
namespace {

#include "mm_mfma_f16_kernels.inc"

}  // namespace

bool mfma_f16_serves(const Problem &p) {
  if (!(p.n >= 1 && p.m >= 8 && p.k >= 16 && p.m % 8 == 0 && p.k % 16 == 0)) return false;
  return !p.a_transposed || (p.n >= 8 && p.n % 8 == 0);
}

// The DMA addresses a tile's rows with 32-bit byte offsets from a uniform 64-bit base: 256 rows x K x 2 B, and 64 k-rows
// x M (or N, K x N layout) x 2 B, must stay below 4 GiB; longer rows are served by the slab64 kernel (64-bit addresses).
static bool pp_reach(const Problem &p) {
  return 256ull * (p.a_transposed ? 1ull : p.k) * 2ull < (1ull << 32) && 64ull * (p.m > p.n ? p.m : p.n) * 2ull < (1ull << 32);
}
static bool ppk32_serves(const Problem &p) {
  const bool shape = p.k % 32 == 0 && p.k >= 128 && p.m % 8 == 0 && p.m >= 8 && pp_reach(p);
  return p.a_transposed ? shape && p.n % 8 == 0 && p.n >= 8 : shape && p.n >= 1;
}
static bool pp64_serves(const Problem &p) { return !p.a_transposed && ppk32_serves(p) && p.k % 64 == 0 && p.k >= 256; }

int mfma_f16_tile(const Problem &p) {  // 0: 256x256, 4: 128x256, 5: 64x256
  static const TileCandidate cands[] = {{0, 256, 256, 1, 1.00}, {4, 128, 256, 1, 0.80}, {5, 64, 256, 1, 0.60}};
  return p.a_transposed ? 0 : pick_tile(cands, 3, p.n, p.m, nullptr, p.batch);   // (batched: all elements' tiles)
}

// The one place that decides which kernel a (problem, f16_variant knob) pair runs; mm_kernel_name and the launcher
// both go through it.  f16_variant: -1 the best the shape allows; 0 slab64; 4 / 5 slab64 on the 128 x 256 / 64 x 256 tile;
// 11 pingpong_k32; 100 pingpong_32x32x16; 200 pingpong_16x16x32.  A pinned kernel that cannot serve the shape falls
// through to the next one down (as the default does), so a knob never turns a servable problem into an error.
// K x N A (MM_TRANSPOSED_A) of a wide problem under the shape-adaptive pick: transposed into a stream-ordered workspace
// first (mm_transpose.hip), then the row-major default with its bits.  A pinned f16_variant keeps the K x N kernels.
static bool transposes_first(const Problem &p) {
  if (tuning(TUNE_F16_VARIANT) >= 0 || !transposes_first_small(p, 2)) return false;
  Problem q = p;
  q.a_transposed = false;
  return pp64_serves(q) && mfma_f16_tile(q) == 0;
}

static Kind resolve(const Problem &p) {
  if (!mfma_f16_serves(p)) return K_NONE;
  const int v = tuning(TUNE_F16_VARIANT);
  if (!(v < 0 || v == 0 || v == 4 || v == 5 || v == 11 || v == 100 || v == 200)) return K_NONE;   // lab ids are not in this library
  if (transposes_first(p)) return K_PP16;
  if (p.a_transposed) return (v != 0 && ppk32_serves(p)) ? K_PPK32_AT : K_SLAB64_AT;
  if (v == 5 || (v < 0 && mfma_f16_tile(p) == 5)) return K_SLAB64_64;
  if (v == 4 || (v < 0 && mfma_f16_tile(p) == 4)) return K_SLAB64_128;
  if (v == 0) return K_SLAB64;
  if ((v < 0 || v == 200) && pp64_serves(p)) return K_PP16;   // +7 % over pingpong_32x32x16 (profiles/r03c_*)
  if (v == 100 && pp64_serves(p)) return K_PP32;              // round 2's default: +2-4 % over pingpong_k32 (profiles/r02h_*)
  if (ppk32_serves(p)) return K_PPK32;
  return K_SLAB64;
}

const char *mfma_f16_name(const Problem &p) { return kTable[resolve(p)].name; }
const KernelRow &mfma_f16_row(const Problem &p) { return kTable[resolve(p)]; }

// A K x N A served where it lies (no workspace): the ping-pong K x N kernel where its shape rules allow, else slab64's
static int launch_kxn_in_place(hipStream_t s, const Problem &p) {
  return launch_kind<Form::Single, _Float16>(s, p, tuning(TUNE_F16_VARIANT) != 0 && ppk32_serves(p) ? K_PPK32_AT : K_SLAB64_AT);
}

int launch_mfma_f16(hipStream_t s, const Problem &p) {
  if (transposes_first(p)) return launch_transposed_first(s, p, 2, launch_mfma_f16, launch_kxn_in_place);
  return launch_kind<Form::Single, _Float16>(s, p, resolve(p));
}

// Batched (mm_gemm_batched_*): whole tiles of the in-place kernels, decided on the whole batch (Problem::batch copies of the
// tile grid).  The instruction schedule -- and with it the bits -- depends on the element's shape only: where a ping-pong
// kernel serves, it runs whatever the batch; the tile pick among the slab kernels counts the whole batch.  A K x N A that
// the single launch would transpose first (workspace) is not served here: -1, and the caller takes the VALU families.
static Kind resolve_batched(const Problem &p) {
  if (!mfma_f16_serves(p) || transposes_first(p)) return K_NONE;
  const int v = tuning(TUNE_F16_VARIANT);
  if (v < 0 && !p.a_transposed && pp64_serves(p)) return K_PP16;
  if (v < 0 && !p.a_transposed && ppk32_serves(p)) return K_PPK32;
  return resolve(p);
}
int mfma_f16_batched_resolve(const Problem &p) { const Kind k = resolve_batched(p); return k == K_NONE ? -1 : (int)k; }
const char *mfma_f16_batched_name(const Problem &p) { return kTable[resolve_batched(p)].name; }
int launch_mfma_f16_batched(hipStream_t s, const Problem &p, int kind) {
  if (kind < 0 || kind >= (int)K_NONE) return kErrNotSupported;
  // an accumulating launch (p.seed): the same kernel with C's value in its epilogue
  return p.seed ? launch_kind<Form::Seeded, _Float16>(s, p, (Kind)kind) : launch_kind<Form::Batched, _Float16>(s, p, (Kind)kind);
}

}  // namespace mm
