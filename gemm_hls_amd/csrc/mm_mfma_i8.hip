// int8_t / uint8_t (Multiply, Add) fast path for gfx950 on the int8 matrix-core instructions
// (v_mfma_i32_16x16x64_i8 / v_mfma_i32_32x32x32_i8).
//
// Why the signed-int8 matrix core serves BOTH element types exactly: the reference's semiring on
// an 8-bit Data_t wraps every product and every sum to 8 bits (hlslib::op::Multiply/Add return
// Data_t), i.e. the result is sum_k a*b taken mod 2^8.  uint8 and int8 bit patterns are congruent
// mod 2^8, products and sums of congruent numbers stay congruent, and the i32 accumulator wraps mod
// 2^32 (a multiple of 2^8), so (int8)(i32 accumulator) is bit-identical to Naive
// (include/Utility.h:18-42) for int8_t and for uint8_t (the type the reference special-cases at
// CMakeLists.txt:46-47).  Checked against the oracle in tests/test_gpu_parity.py.
//
// Kernels in this file, as in mm_mfma_f16.hip: pingpong_16x16x64 (default: K % 128 == 0, K >= 512, row-major A),
// pingpong_32x32x32 (cross-check, i8_variant 100), pingpong_k64 (K % 64 == 0; row-major and K x N A), slab128 (K % 32 == 0).
// The two pingpong_NxNxK kernels share their protocol and geometry with the half pair: mm_pingpong2.h.
// Each is one row of kTable at the end of mm_mfma_i8_kernels.inc; this unit picks the row (resolve) and launches it through the
// include's launch_kind.  Lock-step ablations: tools/lab/lab_mfma_i8.hip.
// Organisation of slab128 as mm_mfma_f16.hip's slab64: 256 x 256 x 128(bytes) slabs, 8 wavefronts of 64 x 128, A operand
// by one ds_read_b128 (16 consecutive k of a row, rows swizzled with (row>>1)&7), B operand (16
// consecutive k of ONE column of the row-major B) by two ds_read_b64_tr_b8: lane i of a 16-lane
// group receives column i of the [8 k][16 col] block whose rows the group's lanes point at,
// out[i][j] = in[2j + (i>>3)][i&7] (profiles/r01_probe_ds_read_b64_tr_b8_and_mfma_i8.txt).  A B
// k-row is 256 B = one bank row, so the 16-B chunk index is XORed with (k&7)<<1 on the DMA source
// side: the 8 rows of a block then sit in 8 different chunk pairs and a half-wave reads 256
// distinct bytes.  Operand layout of the MFMA (same probe): lane l, byte b <-> k = 16*(l>>5) + b.
// Edges: N arbitrary, K % 32 == 0, M % 16 == 0 (reference contract for 1-byte types: K % 64,
// M % 64); a K x N A (N % 16 == 0) is gathered like B; other shapes go to the predicated kernels.
#include <cstdlib>
#include <type_traits>

#include "mm_common.h"
#include "mm_pingpong2.h"

namespace mm {
namespace {

#include "mm_mfma_i8_kernels.inc"

}  // namespace

bool mfma_i8_serves(const Problem &p) {
  if (!(p.n >= 1 && p.m >= 16 && p.k >= 32 && p.m % 16 == 0 && p.k % 32 == 0)) return false;
  return !p.a_transposed || (p.n >= 16 && p.n % 16 == 0);
}

// 32-bit byte offsets inside a tile's rows (see mm_mfma_f16.hip): 256 rows x K B and 128 k-rows x max(M, N) B below 4 GiB
static bool pp_reach(const Problem &p) {
  return 256ull * (p.a_transposed ? 1ull : p.k) < (1ull << 32) && 128ull * (p.m > p.n ? p.m : p.n) < (1ull << 32);
}
static bool ppk64_serves(const Problem &p) {
  const bool shape = p.k % 64 == 0 && p.k >= 256 && p.m % 16 == 0 && p.m >= 16 && pp_reach(p);
  return p.a_transposed ? shape && p.n % 16 == 0 && p.n >= 16 : shape && p.n >= 1;
}
static bool pp128_serves(const Problem &p) { return !p.a_transposed && ppk64_serves(p) && p.k % 128 == 0 && p.k >= 512; }

// Below a round of 256 x 256 tiles the slab128 kernel's 64 x 256 tile gives four times the workgroups (1024^3: 64 instead
// of 16 for 256 CUs); efficiency relative to the ping-pong kernel fitted to profiles/r03y_i8_small_tile.txt.
static int mfma_i8_tile(const Problem &p) {  // 0: 256x256, 5: 64x256
  static const TileCandidate cands[] = {{0, 256, 256, 1, 1.00}, {5, 64, 256, 1, 0.45}};
  return p.a_transposed ? 0 : pick_tile(cands, 2, p.n, p.m, nullptr, p.batch);   // (batched: all elements' tiles)
}

// i8_variant: -1 the best the shape allows; 0 slab128; 5 slab128 on the 64 x 256 tile; 10 pingpong_k64; 100 pingpong_32x32x32;
// 200 pingpong_16x16x64 (one resolver for mm_kernel_name and the launcher; a pinned kernel that cannot serve the shape
// falls through).
// K x N A of a wide problem under the shape-adaptive pick: transposition pre-pass (mm_transpose.hip), then the row-major default
static bool transposes_first(const Problem &p) {
  if (tuning(TUNE_I8_VARIANT) >= 0 || !transposes_first_small(p, 1)) return false;
  Problem q = p;
  q.a_transposed = false;
  return pp128_serves(q) && mfma_i8_tile(q) == 0;
}

static Kind resolve(const Problem &p) {
  if (!mfma_i8_serves(p)) return K_NONE;
  const int v = tuning(TUNE_I8_VARIANT);
  if (!(v < 0 || v == 0 || v == 5 || v == 10 || v == 100 || v == 200)) return K_NONE;   // lab ids are not in this library
  if (transposes_first(p)) return K_PP16;
  if (p.a_transposed) return (v != 0 && ppk64_serves(p)) ? K_PPK64_AT : K_SLAB128_AT;
  if (v == 5 || (v < 0 && mfma_i8_tile(p) == 5)) return K_SLAB128_64;
  if (v == 0) return K_SLAB128;
  if ((v < 0 || v == 200) && pp128_serves(p)) return K_PP16;  // +7.6 % over pingpong_32x32x32 (profiles/r03e_*)
  if (v == 100 && pp128_serves(p)) return K_PP32;
  if (ppk64_serves(p)) return K_PPK64;
  return K_SLAB128;
}

const char *mfma_i8_name(const Problem &p) { return kTable[resolve(p)].name; }
const KernelRow &mfma_i8_row(const Problem &p) { return kTable[resolve(p)]; }

// A K x N A served where it lies (no workspace): the ping-pong K x N kernel where its shape rules allow, else slab128's
static int launch_kxn_in_place(hipStream_t s, const Problem &p) {
  return launch_kind<Form::Single, signed char>(s, p, tuning(TUNE_I8_VARIANT) != 0 && ppk64_serves(p) ? K_PPK64_AT : K_SLAB128_AT);
}

int launch_mfma_i8(hipStream_t s, const Problem &p) {
  if (transposes_first(p)) return launch_transposed_first(s, p, 1, launch_mfma_i8, launch_kxn_in_place);
  return launch_kind<Form::Single, signed char>(s, p, resolve(p));
}

// Batched (mm_gemm_batched_*): whole tiles of the in-place kernels, decided on the whole batch (Problem::batch copies of the
// tile grid).  The instruction schedule -- and with it the bits -- depends on the element's shape only: where a ping-pong
// kernel serves, it runs whatever the batch; the tile pick among the slab kernels counts the whole batch.  A K x N A that
// the single launch would transpose first (workspace) is not served here: -1, and the caller takes the VALU families.
static Kind resolve_batched(const Problem &p) {
  if (!mfma_i8_serves(p) || transposes_first(p)) return K_NONE;
  const int v = tuning(TUNE_I8_VARIANT);
  if (v < 0 && !p.a_transposed && pp128_serves(p)) return K_PP16;
  if (v < 0 && !p.a_transposed && ppk64_serves(p)) return K_PPK64;
  return resolve(p);
}
int mfma_i8_batched_resolve(const Problem &p) { const Kind k = resolve_batched(p); return k == K_NONE ? -1 : (int)k; }
const char *mfma_i8_batched_name(const Problem &p) { return kTable[resolve_batched(p)].name; }
int launch_mfma_i8_batched(hipStream_t s, const Problem &p, int kind) {
  if (kind < 0 || kind >= (int)K_NONE) return kErrNotSupported;
  // an accumulating launch (p.seed): the same kernel with C's value in its epilogue
  return p.seed ? launch_kind<Form::Seeded, signed char>(s, p, (Kind)kind) : launch_kind<Form::Batched, signed char>(s, p, (Kind)kind);
}

}  // namespace mm
