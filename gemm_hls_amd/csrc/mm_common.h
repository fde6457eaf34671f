// Shared device-side vocabulary of the gfx950 kernels: element types, the (map, reduce)
// operator functors and launch descriptors.  Mirrors what the reference gets from
// include/Config.h.in:15,34-35 (Data_t, OperatorMap, OperatorReduce) and from
// hlslib::op::{Add,Multiply,And,Min,Max} (third-party header, absent from the reference tree;
// semantics: Apply(a,b) and identity(), used at kernel/Compute.cpp:129,133 and
// include/Utility.h:29,37).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include <type_traits>

#include "../../include/mm_gemm.h"

namespace mm {

using half_t = _Float16;

// ---- operators -------------------------------------------------------------------------------
template <typename T> struct Limits;
template <> struct Limits<float> {
  __host__ __device__ static constexpr float max() { return 3.40282346638528859812e+38f; }
  __host__ __device__ static constexpr float lowest() { return -3.40282346638528859812e+38f; }
};
template <> struct Limits<double> {
  __host__ __device__ static constexpr double max() { return 1.79769313486231570815e+308; }
  __host__ __device__ static constexpr double lowest() { return -1.79769313486231570815e+308; }
};
template <> struct Limits<half_t> {
  __host__ __device__ static constexpr half_t max() { return (half_t)65504.0f; }
  __host__ __device__ static constexpr half_t lowest() { return (half_t)-65504.0f; }
};
#define MM_INT_LIMITS(T, LO, HI)                                       \
  template <> struct Limits<T> {                                       \
    __host__ __device__ static constexpr T max() { return HI; }        \
    __host__ __device__ static constexpr T lowest() { return LO; }     \
  };
MM_INT_LIMITS(int8_t, INT8_MIN, INT8_MAX)
MM_INT_LIMITS(uint8_t, 0, UINT8_MAX)
MM_INT_LIMITS(int16_t, INT16_MIN, INT16_MAX)
MM_INT_LIMITS(uint16_t, 0, UINT16_MAX)
MM_INT_LIMITS(int32_t, INT32_MIN, INT32_MAX)
MM_INT_LIMITS(uint32_t, 0, UINT32_MAX)
MM_INT_LIMITS(int64_t, INT64_MIN, INT64_MAX)
MM_INT_LIMITS(uint64_t, 0, UINT64_MAX)
#undef MM_INT_LIMITS

// Integer Add / Multiply wrap mod 2^width (include/mm_gemm.h): they are computed in an unsigned type at least as wide as
// unsigned int, where wrapping is defined.  In T itself a signed overflow -- or a uint16_t product, promoted to int --
// is undefined behaviour, and the compiler does exploit it: (Multiply, And) on int / long took products that wrap to 0
// (INT_MIN * 2) for nonzero (tests/test_gpu_value_ranges.py).  Floating types: T.
template <typename T, bool = std::is_integral<T>::value> struct WrapType { using type = T; };
template <typename T> struct WrapType<T, true> { using type = decltype(0u + (typename std::make_unsigned<T>::type)0); };

template <int OP, typename T> struct Op;
template <typename T> struct Op<MM_OP_ADD, T> {
  using W = typename WrapType<T>::type;
  __device__ static __forceinline__ T apply(T a, T b) { return (T)((W)a + (W)b); }
  __host__ __device__ static constexpr T identity() { return (T)0; }
};
template <typename T> struct Op<MM_OP_MULTIPLY, T> {
  using W = typename WrapType<T>::type;
  __device__ static __forceinline__ T apply(T a, T b) { return (T)((W)a * (W)b); }
  __host__ __device__ static constexpr T identity() { return (T)1; }
};
template <typename T> struct Op<MM_OP_AND, T> {
  __device__ static __forceinline__ T apply(T a, T b) { return (T)((a != (T)0) && (b != (T)0)); }
  __host__ __device__ static constexpr T identity() { return (T)1; }
};
template <typename T> struct Op<MM_OP_MIN, T> {
  __device__ static __forceinline__ T apply(T a, T b) { return b < a ? b : a; }  // std::min
  __host__ __device__ static constexpr T identity() { return Limits<T>::max(); }
};
template <typename T> struct Op<MM_OP_MAX, T> {
  __device__ static __forceinline__ T apply(T a, T b) { return a < b ? b : a; }  // std::max
  __host__ __device__ static constexpr T identity() { return Limits<T>::lowest(); }
};

// ---- problem descriptor handed to every kernel launcher --------------------------------------
struct Problem {
  const void *a;   // N x K row-major (or K x N when a_transposed)
  const void *b;   // K x M row-major
  void *c;         // N x M row-major, pure output
  unsigned n, k, m;
  bool a_transposed;
  // rows of the whole job when this launch is one row slab of it (the host-pointer pipeline, the N-split over GPUs);
  // 0 = n.  Decisions that change the summation order (split-K) are taken on the whole job, so that a row's bits do
  // not depend on how the rows were dealt out.
  unsigned n_total = 0;
  // strided batch (mm_gemm_batched_*): `batch` problems of this shape, element e at a + e * stride_a, b + e * stride_b,
  // c + e * stride_c (strides in elements; 0 = one operand shared by every element).  Only the *_batched launchers read
  // these; every other launcher runs the one problem at (a, b, c).
  unsigned batch = 1;
  size_t stride_a = 0, stride_b = 0, stride_c = 0;
  // accumulate (mm_gemm_*accumulate_*): C <- C (+) (A (x) B), each output's reduction starts at the value C holds instead
  // of identity().  Only the *_batched launchers read it (they then run the kernels' Form::Seeded instantiations).
  bool seed = false;
  // A x B^T (mm_gemm_nt_*, mm_gemm_argreduce_nt_*, mm_gemm_logsumexp_nt_*): b is M x K row-major per element (Bt[j][k];
  // stride_b counts its elements), never together with a_transposed.  Only the *_nt launchers, launch_argreduce and
  // launch_lse_exact are handed such a problem; nothing else reads this.
  bool b_transposed = false;
};

// Batched launches: `p.batch` copies of the tile grid in ONE launch; the kernel derives the element from the workgroup id
// (XCD-remapped linear id = element * tiles + tile, so one element's tiles stay contiguous on an XCD) and moves the A, B and
// C bases by it.  No workspace, no split of K.  Grid-size limits are the caller's (mm_capi.hip splits the batch).
int launch_ordered_batched(hipStream_t s, const mm_config_t &cfg, const Problem &p);
int launch_half_wide_batched(hipStream_t s, const Problem &p);
int launch_valu_tile_batched(hipStream_t s, const mm_config_t &cfg, const Problem &p);
int launch_valu_tile_exact_batched(hipStream_t s, const mm_config_t &cfg, const Problem &p);
int mfma_f32_batched_resolve(const Problem &p, int variant);   // 33 / 8 / 35 (row-major), 8 (K x N A); -1 = unsupported
int launch_mfma_f32_batched(hipStream_t s, const Problem &p, int resolved_variant);
// the other matrix-core families: resolve once on the whole batch (-1: not served batched -- e.g. a K x N A the single
// launch would transpose first), then launch each chunk with that kernel
int mfma_f64_batched_resolve(const Problem &p);
int mfma_f16_batched_resolve(const Problem &p);
int mfma_i8_batched_resolve(const Problem &p);
const char *mfma_f64_batched_name(const Problem &p);
const char *mfma_f16_batched_name(const Problem &p);
const char *mfma_i8_batched_name(const Problem &p);
int launch_mfma_f64_batched(hipStream_t s, const Problem &p, int resolved);
int launch_mfma_f16_batched(hipStream_t s, const Problem &p, int resolved);
int launch_mfma_i8_batched(hipStream_t s, const Problem &p, int resolved);
// Widening (mm_gemm_widen_*): the kernel mfma_*_batched_name(p) names, instantiated with a wide C (int for int8_t, float for
// half; p.c and p.stride_c are of that type) -- mm_mfma_i8_wide.hip, mm_mfma_f16_wide.hip.  resolve: -1 where the narrow
// batched resolver names no kernel of this library; name: that kernel's name + "_wide", null for -1.
int mfma_i8_wide_resolve(const Problem &p);
int mfma_f16_wide_resolve(const Problem &p);
const char *mfma_i8_wide_name(const Problem &p);
const char *mfma_f16_wide_name(const Problem &p);
int launch_mfma_i8_wide(hipStream_t s, const Problem &p, int resolved);
int launch_mfma_f16_wide(hipStream_t s, const Problem &p, int resolved);
// "widen_ordered" (mm_widen_ordered.hip): k ascending, one accumulator in the wide type, fully predicated; dtype is the operands'.
// blocked (half only): the terms summed in blocks of k instead -- MM_PATH_AUTO's bound where a misaligned launch was demoted
int launch_widen_ordered(hipStream_t s, mm_dtype_t dtype, const Problem &p, bool blocked);

// A x B^T (mm_gemm_nt_*): the p.batch elements of p, p.b M x K row-major per element, p.seed accumulating into C.
// "ordered_nt" (mm_ordered_nt.hip): Naive on Bt[j][k], k ascending, one accumulator, unfused; any shape, any element-aligned
// pointer.  launch_half_wide_nt: its half (Multiply, Add) instantiation with an f32 accumulator (one rounding on store).
int launch_ordered_nt(hipStream_t s, const mm_config_t &cfg, const Problem &p);
int launch_half_wide_nt(hipStream_t s, const Problem &p);
// "valu_tile_nt" (mm_valu_tile_nt.inc): serves by configuration and shape (maps {Multiply, Add, Min, Max}, reductions {Add, Min,
// Max}, K >= 64 bytes, K a multiple of 16 bytes, 128 rows of K below 4 GiB); the launch also needs every element's A and
// Bt 16-byte aligned.  kErrNotSupported where it does not serve.
bool valu_tile_nt_serves(const mm_config_t &cfg, const Problem &p);
int launch_valu_tile_nt(hipStream_t s, const mm_config_t &cfg, const Problem &p);

// Launchers (one translation unit each).  Return hipError_t as int; hipErrorNotSupported (801)
// means "this family does not serve this (config, shape)".
int launch_ordered(hipStream_t s, const mm_config_t &cfg, const Problem &p);
int launch_half_wide(hipStream_t s, const Problem &p);  // half (x,+), f32 accumulate, any shape
int launch_valu_tile(hipStream_t s, const mm_config_t &cfg, const Problem &p);
bool valu_tile_serves(const mm_config_t &cfg, const Problem &p);
// The same register-tiled kernels under the k-ORDERED contract ("ordered_tile"): floating-point types from the unit compiled
// with contraction off and Op<> to the letter (mm_valu_tile_fp_exact.hip); the integer types' kernels are bit-identical to
// Naive as they are.  Serves whenever valu_tile_serves() and the operands are 16-byte aligned.
int launch_valu_tile_exact(hipStream_t s, const mm_config_t &cfg, const Problem &p);
// Min / Max reductions with the winning k (mm_gemm_argreduce_*, mm_argreduce_*.hip): the p.batch elements of p, C and the
// int32 index matrix `index` with the same element strides (p.stride_c); p.seed starts from C and `index`.  tile: the
// register-tiled argreduce_tile kernel (valu_tile_serves() and 16-byte aligned operands), else the predicated argreduce.
// p.b_transposed: launch_argreduce_nt, their M x K B instantiations "argreduce_tile_nt" and "argreduce_nt"
// (mm_argreduce_nt_*.hip).
int launch_argreduce(hipStream_t s, const mm_config_t &cfg, const Problem &p, int *index, int index_base, bool tile);
int launch_argreduce_nt(hipStream_t s, const mm_config_t &cfg, const Problem &p, int *index, int index_base, bool tile);
// One launch of a closure round (mm_closure_*.hip): block K = [k0, k0 + bt) of `graphs` graphs at d + e * stride_d, n x n
// each; w (int32, D's strides) null for the value-only form.  panels = false: step 1 (closure_diag_kernel, one workgroup per
// graph; w_fresh: start the witnesses at -1 instead of reading w); true: step 2 (closure_panel_kernel).  cc / rc: the
// snapshots D[:,K] (n x bt) and D[K,:] (bt x n) at cc + e * stride_ws, rc + e * stride_ws (null in step 1 of an on-chip
// closure).  bt <= 128, or <= 256 for value-only elements of at most 4 bytes.
struct ClosureStep {
  void *d;
  int *w;
  unsigned n, graphs, k0, bt;
  size_t stride_d;
  void *cc, *rc;
  size_t stride_ws;
  bool panels;
  int w_fresh;
};
int launch_closure(hipStream_t s, const mm_config_t &cfg, const ClosureStep &st);
// Bit-packed Boolean product (mm_bits_gemm_*, mm_bits.hip): the p.batch elements of p, every ld and batch stride in words;
// seed: C <- C | A B.  tile: "bits_tile" (bits_tile_serves() on the ld's, b 16-byte and c 8-byte aligned per element), else
// "bits_plain" (anything).
struct BitsProblem {
  const uint32_t *a, *b;
  uint32_t *c;
  unsigned n, k, m;
  size_t lda, ldb, ldc;
  unsigned batch;
  size_t stride_a, stride_b, stride_c;
  bool seed;
};
bool bits_tile_serves(size_t ldb, size_t ldc);   // the ld half of the serving rule; the M half is mm_capi.hip's (a knob lifts it)
int launch_bits_gemm(hipStream_t s, const BitsProblem &p, bool tile);
// Bit-packed product over GF(2) (mm_bits_gf2_*, mm_bits_gf2.hip): BitsProblem as for launch_bits_gemm; seed: C <- C ^ A B.
// tile: "bits_gf2_tile" (bits_gf2_tile_serves() on the ld's, b and c 8-byte aligned per element), else
// "bits_gf2_plain" (anything).
bool bits_gf2_tile_serves(size_t ldb, size_t ldc);   // the ld half of the serving rule; the shape half is mm_capi.hip's (a knob lifts it)
int launch_bits_gf2(hipStream_t s, const BitsProblem &p, bool tile);
// pack: src bytes -> dst words; unpack: src words -> dst bytes (0 / 1).  ld and batch strides in each side's own unit.
struct BitsConvert {
  const void *src;
  void *dst;
  unsigned rows, cols;
  size_t ld_src, ld_dst;
  unsigned batch;
  size_t stride_src, stride_dst;
};
int launch_bits_pack(hipStream_t s, const BitsConvert &c);
int launch_bits_unpack(hipStream_t s, const BitsConvert &c);
// Bit-packed counting product (mm_bits_count_*, mm_bits_count.hip): C[i][j] = sum_k (A[i][k] op Bt[j][k]), op AND or XOR, as
// int32.  p.b is Bt, M x K packed along K (ldb = ldbt, words); p.c is N x M int32 (ldc and stride_c in elements); seed: C +=.
// tile: "bits_count_tile" (bits_count_tile_serves() on the ld's, 16-byte aligned bases and batch strides), else
// "bits_count_plain" (anything).
bool bits_count_tile_serves(size_t lda, size_t ldbt, size_t ldc);   // the ld half of the rule; the tile-count half is mm_capi.hip's
int launch_bits_count(hipStream_t s, const BitsProblem &p, bool xor_op, bool tile);
// src rows x cols -> dst cols x rows, both packed (ld and batch strides in words); dst's padding bits are written 0.
int launch_bits_transpose(hipStream_t s, const BitsConvert &c);
// The wavefront kernel of the packed closure (mm_bits_closure.hip): closes block [k0, k0 + min(64, n - k0)) of `graphs` graphs
// at d + e * stride_d.  pstar null: writes the closed block back into D (the on-chip closure, k0 = 0, n <= 64); else leaves D
// alone and writes P | I as 64 rows x 2 words at pstar + e * stride_p.
int launch_bits_closure_diag(hipStream_t s, uint32_t *d, unsigned n, size_t ldd, unsigned graphs, size_t stride_d, unsigned k0,
                             uint32_t *pstar, size_t stride_p);
// Log-semiring product (mm_gemm_logsumexp_*, mm_lse_fp.hip).  launch_lse_exact: the exact kernel over the p.batch elements of
// p (p.seed: C's input is one more term); flags != null: the hybrid's fallback, tile t of element e runs only where
// flags[e * tiles + t] != 0 (64 x 64 tiles); p.b_transposed: launch_lse_exact_nt, "lse_exact_nt" (mm_lse_nt_fp.hip).  The hybrid's prepass transforms `count` elements of one operand: r = the
// per-line maxima (NaN-propagating; Min: of the negated operand) and e = exp(X - r), zero-padded to rows_p x k_p
// (out_kmajor: k_p x rows_p), in f32 (f64 for double).  X is rows x k row-major, or k x rows when x_kmajor.
struct LseOperand {
  const void *x;
  size_t stride_x;
  unsigned count, rows, k, rows_p, k_p;
  bool x_kmajor, out_kmajor;
  void *e, *r;
  size_t stride_e, stride_r;
};
// The epilogue: C from S (n_p x m_p per element, row stride m_p), ra and rb; one flag per 64 x 64 tile of each element.
struct LseEpilogue {
  const void *s, *ra, *rb;
  void *c;
  int *flags;
  unsigned n, m, m_p, batch;
  size_t stride_s, stride_ra, stride_rb, stride_c;
  bool seed, force;
};
int launch_lse_exact(hipStream_t s, const mm_config_t &cfg, const Problem &p, const int *flags);
int launch_lse_exact_nt(hipStream_t s, const mm_config_t &cfg, const Problem &p, const int *flags);
int launch_lse_expand_nt(hipStream_t s, const mm_config_t &cfg, const LseOperand &op);   // e of an M x K B: !x_kmajor, out_kmajor
int launch_lse_prepass(hipStream_t s, const mm_config_t &cfg, const LseOperand &op);
int launch_lse_epilogue(hipStream_t s, const mm_config_t &cfg, const LseEpilogue &ep);
int launch_mfma_f32(hipStream_t s, const Problem &p, int variant);
int launch_mfma_f64(hipStream_t s, const Problem &p);
int launch_mfma_f16(hipStream_t s, const Problem &p);
int launch_mfma_i8(hipStream_t s, const Problem &p);
int launch_mfma_f32_split(hipStream_t s, const Problem &p, int variant);  // MM_PATH_SPLIT (mm_mfma_f32_split.hip)
bool mfma_f32_split_serves(const Problem &p);
size_t mfma_f32_split_workspace_bytes(const Problem &p);
int mfma_f32_split_tile(const Problem &p, int variant);  // 256 or 128
int workspace_pool(int device, hipMemPool_t *pool);      // the library-owned, stream-ordered workspace pool of `device` (mm_capi.hip)
int workspace_release(int device);                       // hands its cached memory back to the driver
// `bytes` of epoch flags for one stream-K launch on `stream` (free with hipFreeAsync), and the launch's epoch: mm_capi.hip
int flags_alloc(int device, hipStream_t stream, size_t bytes, void **flags, unsigned long long *epoch);
int device_compute_units(int device);                    // as reported by the device when the library initialised
int mfma_f32_splitk(const Problem &p, int variant);      // K chunks the fp32 MFMA launcher uses for (problem, resolved variant)
const char *mfma_f32_launch_name(const Problem &p, int variant);   // what that pair runs: the geometry's name, or its split-K / stream-K form's
bool mfma_f32_serves(const Problem &p);
bool mfma_f64_serves(const Problem &p);
bool mfma_f16_serves(const Problem &p);
bool mfma_i8_serves(const Problem &p);
const char *mfma_f32_name(int variant);
void mfma_f32_geometry(int variant, unsigned *bm, unsigned *bn, unsigned *bk, unsigned *waves);
int mfma_f32_num_variants();
int mfma_f32_variant_id(int index);                      // the valid f32_variant values, 0 <= index < num_variants
int mfma_f32_resolve(const Problem &p, int variant);     // variant id a (problem, knob) pair runs, -1 = unsupported
const char *mfma_f16_name(const Problem &p);
const char *mfma_f64_name(const Problem &p);
const char *mfma_i8_name(const Problem &p);
// One row of a matrix-core family's kernel table (mm_mfma_*_kernels.inc): the one place that describes a kernel.  The launch,
// the names, the wide twin and mm_kernel_info all read it.
struct KernelRow {
  const char *name, *wide_name;   // literals; wide_name: the instantiation with a wide C (mm_gemm_widen_*), null where there is none
  unsigned tile_n, tile_m, tile_k, wavefronts, inst_n, inst_m, inst_k;
  double measured_issue_efficiency;
};
// The row of the kernel mfma_*_name(p) names; where it names none ("unsupported": a knob value the library does not have),
// the row of the family's catch-all kernel.
const KernelRow &mfma_f16_row(const Problem &p);
const KernelRow &mfma_f64_row(const Problem &p);
const KernelRow &mfma_i8_row(const Problem &p);
int mfma_f32_auto_variant(const Problem &p);
int mfma_f16_tile(const Problem &p);  // 0: 256x256, 4: 128x256  // shape-adaptive pick (variant < 0)
// dst[n][k] = src[k][n] for 1- and 2-byte elements (mm_transpose.hip); N and K multiples of 16 bytes' worth of elements
int launch_transpose_kxn(hipStream_t s, const void *src, void *dst, unsigned K, unsigned N, unsigned elem_size);
// The same for 1-, 2-, 4- and 8-byte elements over `count` matrices at src + e * stride_src, dst + e * stride_dst (elements)
int launch_transpose_batched(hipStream_t s, const void *src, void *dst, unsigned K, unsigned N, unsigned elem_size, unsigned count,
                             size_t stride_src, size_t stride_dst);
bool transposes_first_small(const Problem &p, unsigned elem_size);   // K x N A of half / int8: pre-pass + the row-major default
// That pre-pass: A into N x K pool workspace, row_major() on the copy, free.  A full pool is no error: in_place() serves the K x N A.
typedef int (*ProblemLauncher)(hipStream_t s, const Problem &p);
int launch_transposed_first(hipStream_t s, const Problem &p, unsigned elem_size, ProblemLauncher row_major, ProblemLauncher in_place);
int launch_fill(hipStream_t s, mm_dtype_t dtype, void *ptr, size_t elements, unsigned long long seed);

constexpr int kErrNotSupported = 801;  // hipErrorNotSupported

// ---- host dispatch: a config's run-time dtype, map and reduce to template arguments -----------
// switch_dtype<Types<...>>(dtype, f) returns f(Tag<T>{}) for the element type T of `dtype`; switch_op<Ops<...>>(op, f)
// returns f(std::integral_constant<int, OP>{}) (map_op and reduce_op are one enum, so one switch serves both).  A value
// the list does not hold is kErrNotSupported and instantiates nothing: the lists a compile unit names are the kernels
// it holds.
template <typename T> struct Tag { using type = T; };
template <typename TAG> using type_of = typename TAG::type;
template <typename... Ts> struct Types {
  template <typename T> static constexpr bool has = (std::is_same<T, Ts>::value || ...);
};
template <int... OPS> struct Ops {
  template <int OP> static constexpr bool has = ((OP == OPS) || ...);
};
using FpTypes = Types<float, double, half_t>;
using NarrowIntTypes = Types<int8_t, uint8_t, int16_t, uint16_t>;
using WideIntTypes = Types<int32_t, uint32_t, int64_t, uint64_t>;
using AllTypes = Types<float, double, half_t, int8_t, uint8_t, int16_t, uint16_t, int32_t, uint32_t, int64_t, uint64_t>;
using AllOps = Ops<MM_OP_ADD, MM_OP_MULTIPLY, MM_OP_AND, MM_OP_MIN, MM_OP_MAX>;
using MinMaxOps = Ops<MM_OP_MIN, MM_OP_MAX>;

// In both switches a case the list does not hold leaves the switch (`else break`) for the kErrNotSupported below; it must be
// the `else` of the `if constexpr`, so that f is not instantiated for it.
template <typename TYPES, typename Fn>
int switch_dtype(int dtype, Fn f) {
  switch (dtype) {
#define MM_CASE(D, T) \
  case D:             \
    if constexpr (TYPES::template has<T>) return f(Tag<T>{}); else break;
    MM_CASE(MM_DTYPE_F32, float)
    MM_CASE(MM_DTYPE_F64, double)
    MM_CASE(MM_DTYPE_F16, half_t)
    MM_CASE(MM_DTYPE_I8, int8_t)
    MM_CASE(MM_DTYPE_U8, uint8_t)
    MM_CASE(MM_DTYPE_I16, int16_t)
    MM_CASE(MM_DTYPE_U16, uint16_t)
    MM_CASE(MM_DTYPE_I32, int32_t)
    MM_CASE(MM_DTYPE_U32, uint32_t)
    MM_CASE(MM_DTYPE_I64, int64_t)
    MM_CASE(MM_DTYPE_U64, uint64_t)
#undef MM_CASE
  }
  return kErrNotSupported;
}

template <typename OPS, typename Fn>
int switch_op(int op, Fn f) {
  switch (op) {
#define MM_CASE(OP) \
  case OP:          \
    if constexpr (OPS::template has<OP>) return f(std::integral_constant<int, OP>{}); else break;
    MM_CASE(MM_OP_ADD)
    MM_CASE(MM_OP_MULTIPLY)
    MM_CASE(MM_OP_AND)
    MM_CASE(MM_OP_MIN)
    MM_CASE(MM_OP_MAX)
#undef MM_CASE
  }
  return kErrNotSupported;
}

// f(Tag<T>, map, reduce) for cfg's (dtype, map_op, reduce_op), each from its list
template <typename TYPES, typename MAPS, typename REDS, typename Fn>
int switch_config(const mm_config_t &cfg, Fn f) {
  return switch_dtype<TYPES>(cfg.dtype, [&](auto t) {
    return switch_op<MAPS>(cfg.map_op, [&](auto map) {
      return switch_op<REDS>(cfg.reduce_op, [&](auto red) { return f(t, map, red); });
    });
  });
}

// Kernels that need more than 64 KiB of dynamic LDS must opt in once per (function, device).
// `mask` is a per-kernel static bitmask of devices already configured.
inline int ensure_dynamic_lds(const void *func, int bytes, unsigned long long &mask) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return (int)e;
  const unsigned long long bit = 1ull << (dev & 63);
  if (__atomic_load_n(&mask, __ATOMIC_ACQUIRE) & bit) return 0;
  e = hipFuncSetAttribute(func, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e != hipSuccess) return (int)e;
  __atomic_fetch_or(&mask, bit, __ATOMIC_RELEASE);
  return 0;
}

// Tuning knobs (sweeps and ablations only; defaults are the measured best).  Each one is read
// ONCE from its environment variable when the library initialises and can be changed afterwards
// through mm_tuning_set() -- the launch path itself never calls getenv.  -1 = unset.
enum Tunable {
  TUNE_F32_VARIANT = 0,  // MM_F32_VARIANT  geometry of the fp32 MFMA kernel (mm_mfma_f32.hip)
  TUNE_F64_VARIANT,      // MM_F64_VARIANT
  TUNE_F16_VARIANT,      // MM_F16_VARIANT
  TUNE_I8_VARIANT,       // MM_I8_VARIANT
  TUNE_BAND_ROWS,        // MM_BAND_ROWS    tile-rows per rasterisation band
  TUNE_VALU_VARIANT,     // MM_VALU_VARIANT 0 = synchronous valu_tile kernel, else (default) the DMA-staged one
  TUNE_SPLIT_VARIANT,    // MM_SPLIT_VARIANT schedule / product count of the MM_PATH_SPLIT kernel (mm_mfma_f32_split.hip)
  TUNE_F32_SPLITK,       // MM_F32_SPLITK   fp32 MFMA path: -1 by shape (small problems only), 1 never, 2..8 that many K chunks
  TUNE_ABLATIONS,        // MM_ABLATIONS    1 = allow the variants that skip work on purpose (power breakdown
                         //                 measurements; they produce WRONG results and are refused otherwise)
  TUNE_DEBUG_POISON,     // MM_DEBUG_POISON 1 = fill scratch the kernels hand data through (stream-K slots) with NaN before
                         //                 every launch: a read of anything this launch did not write shows up in C
  TUNE_KXN_PREPASS_MIN_M,  // MM_KXN_PREPASS_MIN_M  half / int8 with a K x N A: M from which the transposition pre-pass is taken (-1: 6144)
  TUNE_MD_VIRTUAL_DEVICES, // MM_MD_VIRTUAL_DEVICES  G > 0: mm_gemm_multi_device accepts device_count <= G and deals its logical devices
                           //                 out over the physical ones round-robin (tests: every g > 0 branch on a 1-GPU box)
  TUNE_ORDERED_VARIANT,    // MM_ORDERED_VARIANT  0 = MM_PATH_ORDERED always runs the 64 x 64 kernel of mm_ordered.hip (the cross-check);
                           //                 else (default) the register-tiled k-ordered kernel wherever it serves -- same bits
  TUNE_HALF_CONTRACT,      // MM_HALF_CONTRACT  1 / "reference": half (Multiply, Add) under MM_PATH_AUTO keeps the REFERENCE's arithmetic
                           //                 (binary16 products and binary16 accumulation, k ascending: kernel/Compute.cpp:129-133) on the
                           //                 k-ordered tile kernel instead of the matrix cores' f32 accumulation; 0 / "wide" / unset: f32
  TUNE_BATCH_CHUNK,        // MM_BATCH_CHUNK  mm_gemm_batched_*: at most this many elements per launch (tests); -1: only the grid limits
  TUNE_CLOSURE_BLOCK,      // MM_CLOSURE_BLOCK  block size B of mm_closure_* (64, 128, or 256 where the form allows it); -1: the default
  TUNE_LSE_VARIANT,        // MM_LSE_VARIANT  mm_gemm_logsumexp_*: 0 exact kernel only, 1 hybrid, 2 hybrid with every tile sent to
                           //                 the fallback (the cross-check); -1: the default (hybrid)
  TUNE_BITS_VARIANT,       // MM_BITS_VARIANT  mm_bits_gemm_*: 0 bits_plain always, 1 bits_tile wherever its ld rule holds (any M);
                           //                 -1: the default (bits_tile for M > 2048)
  TUNE_BITS_COUNT_VARIANT, // MM_BITS_COUNT_VARIANT  mm_bits_count_*: 0 bits_count_plain always, 1 bits_count_tile wherever its ld rule
                           //                 holds (any shape); -1: the default (bits_count_tile from 256 tiles of 128 x 128)
  TUNE_BITS_GF2_VARIANT,   // MM_BITS_GF2_VARIANT  mm_bits_gf2_*: 0 bits_gf2_plain always, 1 bits_gf2_tile wherever its ld rule holds (any
                           //                 shape); -1: the default (bits_gf2_tile from N >= 128 and M >= 128)
  TUNE_COUNT
};
int tuning(Tunable t);  // mm_capi.hip

// Tile rasterisation: after the XCD remap, workgroups are ordered in bands of `band_rows` tile-rows
// (column-major inside a band), so the T = 32 x per_cu workgroups an XCD runs at once cover
// band_rows x (T / band_rows) tiles and share A row-panels / B column-panels in that XCD's L2.  What the XCD then
// pulls through the fabric per round is band_rows x BM rows of A plus (T / band_rows) x BN columns of B: the default is
// the power of two that minimises that sum (ties: the smaller band).  256 x 256 tiles, one per CU: 4 (measured on the
// fp32 kernel: fabric fetch 30 GB per 16384^3 launch vs 51 GB at 8 and 100 GB at 16, profiles/r01_band_rows_sweep.txt);
// 128-row tiles running two workgroups per CU: 8 (round 3: the 128 x 256 fp32 default fetched 50 GB with bands of 4).
inline unsigned band_rows(unsigned bm = 256, unsigned bn = 256, unsigned per_cu = 1) {
  const int v = tuning(TUNE_BAND_ROWS);
  if (v > 0) return (unsigned)v;
  const unsigned t = 32u * per_cu;
  unsigned best = 4, cost = ~0u;
  for (unsigned r = 1; r <= t; r *= 2) {
    const unsigned c = r * bm + (t / r) * bn;
    if (c < cost) { cost = c; best = r; }
  }
  return best;
}

// Shape-adaptive tile choice shared by the MFMA families.  A launch runs in rounds of resident
// workgroups (256 CUs x per_cu), so a big tile loses up to a round to quantisation on mid-size
// problems and leaves CUs idle on small ones.  Estimated time of a candidate ~ (workgroups the
// busiest CU runs) x tile area / relative efficiency; the smallest wins.
struct TileCandidate { int id; unsigned bm, bn, per_cu; double eff; };
// `copies`: copies of the N x M tile grid the launch runs side by side (the elements of a batched launch).
inline int pick_tile(const TileCandidate *cands, int count, unsigned n, unsigned m, double *best_time = nullptr,
                     unsigned long long copies = 1) {
  double best = 0;
  int pick = cands[0].id;
  for (int i = 0; i < count; ++i) {
    const TileCandidate &c = cands[i];
    const unsigned long long tiles = (unsigned long long)((n + c.bm - 1) / c.bm) * ((m + c.bn - 1) / c.bn) * copies;
    const unsigned long long slots = 256ull * c.per_cu, full = tiles / slots, rem = tiles % slots;
    const double t = ((double)full * c.per_cu + (double)((rem + 255) / 256)) * c.bm * c.bn / c.eff;
    if (best == 0 || t < best * 0.999) { best = t; pick = c.id; }
  }
  if (best_time) *best_time = best;
  return pick;
}

// XCD-aware remap of a 1-D workgroup id: the dispatcher places workgroup b on XCD b % 8
// (observed, used for speed only); give every XCD one contiguous chunk of the tile order so that
// tiles sharing A row-panels / B column-panels meet in the same private L2.  Bijective for any
// grid size.
__device__ __forceinline__ unsigned xcd_remap(unsigned bid, unsigned nwg) {
  constexpr unsigned kXcds = 8;
  const unsigned q = nwg / kXcds, r = nwg % kXcds;
  const unsigned xcd = bid % kXcds, slot = bid / kXcds;
  const unsigned base = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  return base + slot;
}

// The band rasterisation above, on the device: the first row and column of the bm x bn tile that linear tile id `lin` names in
// a grid of tiles_n x tiles_m tiles with bands of kBand tile-rows.  bm = bn = 1: the tile's row and column index.
__device__ __forceinline__ void band_origin(unsigned lin, unsigned tiles_n, unsigned tiles_m, unsigned kBand, unsigned bm,
                                            unsigned bn, unsigned &row0, unsigned &col0) {
  const unsigned band = lin / (kBand * tiles_m), within = lin % (kBand * tiles_m);
  const unsigned rows_in_band = min(kBand, tiles_n - band * kBand);
  row0 = (band * kBand + within % rows_in_band) * bm, col0 = (within / rows_in_band) * bn;
}

// One LDS-DMA piece of an asm statement that saves and restores m0: 64 lanes x 16 B from (uniform base sb + per-lane offset vo) to LDS at la
#define MM_DMA_PIECE(vo, sb, la) "s_mov_b32 m0, " la "\n\ts_nop 0\n\tglobal_load_lds_dwordx4 " vo ", " sb "\n\t"

// The three forms every kernel of the older families exists in, a template parameter of the kernel: the single launch,
// the strided-batched launch, and the batched launch whose reduction starts at the value C holds (Problem::seed; Seeded
// implies batched).  Every form takes the batched argument list (..., batch, stride_a, stride_b, stride_c); Form::Single
// never reads that tail, so its machine code is that of a kernel without it.
enum class Form { Single, Batched, Seeded };

// One launch of KERN, the form-F instantiation of a half / int8 matrix-core kernel with geometry G, operands of type T and a C of
// type CT: the problem at (a, b, c), or (F != Form::Single) p.batch copies of the tile grid over the elements of p.
template <Form F, typename G, auto KERN, typename T, typename CT>
int launch_tile(hipStream_t s, const Problem &p) {
  const unsigned tiles_n = (p.n + G::BM - 1) / G::BM, tiles_m = (p.m + G::BN - 1) / G::BN;
  static unsigned long long configured = 0;   // one per instantiation of this function, so one per kernel
  if (int e = ensure_dynamic_lds((const void *)KERN, G::LDS_BYTES, configured)) return e;
  hipLaunchKernelGGL(KERN, dim3(tiles_n * tiles_m * (F == Form::Single ? 1u : p.batch)), dim3(G::THREADS), G::LDS_BYTES, s,
                     (const T *)p.a, (const T *)p.b, (CT *)p.c, p.n, p.k, p.m, tiles_n, tiles_m, band_rows(G::BM, G::BN, 1),
                     F == Form::Single ? 1u : p.batch, p.stride_a, p.stride_b, p.stride_c);
  return (int)hipGetLastError();
}

// A table row from the kernel's geometry struct G, its instruction shape (inst x inst x inst_k) and its measured efficiency
template <typename G>
constexpr KernelRow kernel_row(const char *name, const char *wide_name, unsigned inst, unsigned inst_k, double efficiency) {
  return {name, wide_name, G::BM, G::BN, G::BK, G::THREADS / 64, inst, inst, inst_k, efficiency};
}

// Batched launches (Form::Batched, Form::Seeded): `batch` elements of one shape, `batch` copies of the tile grid in one
// launch.  The XCD-remapped linear id is decomposed as (element, tile), so one element's tiles stay contiguous in an XCD's
// chunk of the grid (a broadcast B, or one element's A panels, stays in that XCD's L2); the element index is uniform across
// the workgroup (SGPRs) and moves the A, B and C bases before anything else.  Returns the element's linear tile id.
template <typename PA, typename PB, typename PC>
__device__ __forceinline__ unsigned batched_tile(PA &A, PB &B, PC &C, unsigned tiles, unsigned batch, size_t stride_a,
                                                 size_t stride_b, size_t stride_c) {
  const unsigned g = xcd_remap(blockIdx.x, tiles * batch), e = g / tiles;
  A += e * stride_a;
  B += e * stride_b;
  C += e * stride_c;
  return g - e * tiles;
}

// The workgroup's linear tile id in a kernel of form F: the XCD-remapped workgroup id of a single launch, or the
// element's tile of a batched one (A, B and C then move to that element).
template <Form F, typename PA, typename PB, typename PC>
__device__ __forceinline__ unsigned form_tile(PA &A, PB &B, PC &C, unsigned tiles, unsigned batch, size_t stride_a,
                                              size_t stride_b, size_t stride_c) {
  if constexpr (F == Form::Single) return xcd_remap(blockIdx.x, tiles);
  else return batched_tile(A, B, C, tiles, batch, stride_a, stride_b, stride_c);
}

// ---- wide epilogue of the int8 / half matrix-core kernels (mm_gemm_widen_*) ------------------------------------------------
// The accumulators leave in their own type (int, float), straight from the C/D register layout: a lane holds ONE column, so
// each store instruction writes whole 64- or 128-byte runs of rows (DESIGN.md 3.10 for why not through LDS).  Form::Seeded
// adds C's input value first, in the wide type; a lane reads exactly the elements it then writes.  Rows >= N and columns
// >= M are masked.
__device__ __forceinline__ int wide_add(int a, int b) { return (int)((unsigned)a + (unsigned)b); }   // mod 2^32
__device__ __forceinline__ float wide_add(float a, float b) { return a + b; }

// Registers of one column: register i of `acc` is row grow + row_of(i).  wide_seed_column adds C's input value to them,
// wide_store_column stores them; a kernel seeds a whole block of accumulators before it stores them, so the loads are in flight together.
template <int R, typename CT, typename V, typename RowOf>
__device__ __forceinline__ void wide_seed_column(const CT *C, unsigned N, unsigned M, unsigned grow, unsigned gcol, V &acc, RowOf row_of) {
  if (gcol >= M) return;
#pragma unroll
  for (int i = 0; i < R; ++i) {
    const unsigned row = grow + row_of(i);
    if (row < N) acc[i] = wide_add(acc[i], C[(size_t)row * M + gcol]);
  }
}
template <int R, typename CT, typename V, typename RowOf>
__device__ __forceinline__ void wide_store_column(CT *C, unsigned N, unsigned M, unsigned grow, unsigned gcol, const V &acc, RowOf row_of) {
  if (gcol >= M) return;
#pragma unroll
  for (int i = 0; i < R; ++i) {
    const unsigned row = grow + row_of(i);
    if (row < N) C[(size_t)row * M + gcol] = acc[i];
  }
}
// a 32 x 32 accumulator (32x32 instructions): lane = column lo + 32 * hi, register rr = row (rr & 3) + 8 * (rr >> 2) + 4 * hi;
// a 16 x 16 accumulator (16x16 instructions): lane = column l15 + 16 * g, register i = row 4 * g + i.  grow includes 4 * hi / 4 * g.
struct WideRows32 { __device__ unsigned operator()(int rr) const { return (unsigned)((rr & 3) + 8 * (rr >> 2)); } };
struct WideRows16 { __device__ unsigned operator()(int i) const { return (unsigned)i; } };
template <typename CT, typename V>
__device__ __forceinline__ void wide_seed_32x32(const CT *C, unsigned N, unsigned M, unsigned grow, unsigned gcol, V &acc) {
  wide_seed_column<16>(C, N, M, grow, gcol, acc, WideRows32{});
}
template <typename CT, typename V>
__device__ __forceinline__ void wide_store_32x32(CT *C, unsigned N, unsigned M, unsigned grow, unsigned gcol, const V &acc) {
  wide_store_column<16>(C, N, M, grow, gcol, acc, WideRows32{});
}
template <typename CT, typename V>
__device__ __forceinline__ void wide_seed_16x16(const CT *C, unsigned N, unsigned M, unsigned grow, unsigned gcol, V &acc) {
  wide_seed_column<4>(C, N, M, grow, gcol, acc, WideRows16{});
}
template <typename CT, typename V>
__device__ __forceinline__ void wide_store_16x16(CT *C, unsigned N, unsigned M, unsigned grow, unsigned gcol, const V &acc) {
  wide_store_column<4>(C, N, M, grow, gcol, acc, WideRows16{});
}

}  // namespace mm
