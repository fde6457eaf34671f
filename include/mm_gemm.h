/*
 * mm_gemm.h -- C ABI of the MI355X (gfx950) implementation of gemm_hls's hot path
 *              C = A (map, reduce) B,  A: N x K, B: K x M, C: N x M, all row-major.
 *
 * Plain C, plain pointers and sizes.  One shared library (libmm_gemm_amd.so) exports all
 * of it.  Every entry point names the reference interface it replaces (paths relative to the
 * reference repository).  Unless stated otherwise a function returns 0 on success and a
 * non-zero status otherwise, with a human-readable message available from mm_last_error();
 * nothing throws across this boundary.  There is NO CPU fallback anywhere behind this ABI:
 * without a usable gfx950 device every compute call fails with MM_ERR_NO_DEVICE.
 */
#ifndef MM_GEMM_H
#define MM_GEMM_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Element type == the reference's build-time MM_DATA_TYPE / Data_t
 * (CMakeLists.txt:17, include/Config.h.in:15; "half" and "uint8_t" special-cased at
 * CMakeLists.txt:40-50). */
typedef enum {
  MM_DTYPE_F32 = 0, /* float          */
  MM_DTYPE_F64 = 1, /* double         */
  MM_DTYPE_F16 = 2, /* half (IEEE binary16).  (Multiply, Add) under MM_PATH_AUTO: exact products,
                       f32 accumulation, ONE rounding on store, for EVERY shape (matrix cores when
                       K % 16 == 0 and M % 8 == 0, a plain wide-accumulate kernel otherwise);
                       MM_PATH_ORDERED accumulates in binary16 exactly like the reference
                       (kernel/Compute.cpp:129-133), and so does MM_PATH_AUTO once the process asked for
                       the REFERENCE's half contract: mm_tuning_set("half_contract", 1) /
                       MM_HALF_CONTRACT=reference -- the result the reference's hosts compare with
                       EXACTLY (test/TestSimulation.cpp:80-85, host/RunHardware.cpp:214-218) */
  MM_DTYPE_I8 = 3,  /* int8_t         */
  MM_DTYPE_U8 = 4,  /* uint8_t        */
  MM_DTYPE_I16 = 5, /* short          */
  MM_DTYPE_U16 = 6, /* unsigned short */
  MM_DTYPE_I32 = 7, /* int            */
  MM_DTYPE_U32 = 8, /* unsigned       */
  MM_DTYPE_I64 = 9, /* long           */
  MM_DTYPE_U64 = 10 /* unsigned long  */
} mm_dtype_t;

/* == the reference's MM_MAP_OP / MM_REDUCE_OP, i.e. hlslib::op::<Name><Data_t>
 * (CMakeLists.txt:33-34, include/Config.h.in:34-35; applied at kernel/Compute.cpp:129,133 and
 * include/Utility.h:29,37).  identity(): Add 0, Multiply 1, And 1, Min max(), Max lowest().
 * hlslib's Operators.h is an absent submodule of the reference tree, so these seeds are NOT pinned by a
 * reference file: Add / Multiply / And / Min are what any identity of those reductions must be; Max lowest()
 * is THIS LIBRARY'S CHOICE (the mathematical identity).  The published hlslib is believed to seed Max with
 * numeric_limits<T>::min() -- for floating types the smallest POSITIVE value -- which differs from lowest()
 * only when every mapped value of an output is negative; on the reference's own inputs ([1,10]) both give
 * the same bits, which is all that parity is pinned on.
 * Integer types: Add and Multiply wrap mod 2^width for EVERY integer type, signed ones included (two's complement, as
 * the unsigned type of the same width computes them); Min / Max are typed compares (std::min / std::max); And gives 0 / 1.
 * Floating-point Min / Max: MM_PATH_ORDERED is std::min / std::max to the letter (b < a ? b : a; NaN and signed-zero
 * ties follow from that); MM_PATH_AUTO's register-tiled kernel uses IEEE minNum / maxNum instead (a NaN operand is
 * dropped; which zero a (+0, -0) tie returns is unspecified) -- the same value for every pair of numbers.
 * A Min reduction whose mapped values are all +inf (or NaN) returns max(), not inf: the identity max() is never
 * replaced by a value that is not below it -- Naive's semantics (e.g. (Add, Min) over a row of A that is all +inf). */
typedef enum {
  MM_OP_ADD = 0,
  MM_OP_MULTIPLY = 1,
  MM_OP_AND = 2,
  MM_OP_MIN = 3,
  MM_OP_MAX = 4
} mm_op_t;

/* Which kernel family serves a launch.
 *   MM_PATH_AUTO     the fast path for the configuration (MFMA for (Multiply,Add) on
 *                    float/half/double, register-tiled VALU otherwise); == RunHardware "hw".
 *   MM_PATH_ORDERED  the plain GPU kernel that evaluates every output as the reference's
 *                    Naive does -- acc = identity; for k ascending: acc = Reduce(acc, Map(a,b)),
 *                    multiply and add NOT fused -- bit-identical to include/Utility.h:18-42
 *                    for every dtype; == RunHardware "hw_emu" (a slower, independently written
 *                    execution of the same contract on the same device).  Two kernels with the same
 *                    bits serve it: "ordered_tile", 128 x 128 register tiles (K % 4 == 0, M % 4 == 0,
 *                    16-byte aligned operands; half 74, float 58, double 29 TOp/s at 8192^3), and
 *                    "ordered", fully predicated 64 x 64 tiles, for everything else ("ordered_variant"
 *                    = 0 forces it: the cross-check).
 *   MM_PATH_SPLIT    float (Multiply, Add) only, opt-in: fp32 operands split into three bf16
 *                    planes (all 24 significand bits for magnitudes >= 2^-108), six bf16 matrix-core
 *                    products per element pair accumulated in fp32 -- each product good to ~2^-25,
 *                    i.e. at least as fine as an fp32 multiply; 1.7x the fp32 matrix-core peak.  Any
 *                    N, K, M and any element-aligned pointers; needs 6 bytes of stream-ordered
 *                    workspace per element of A and B (hipMallocAsync on the launch stream).
 *                    Error bound: |C - AB| <= 2^-19 (|A||B|) elementwise when every nonzero operand
 *                    is finite and 2^-112 <= |x| < 2^127.  Below 2^-112 the second and third
 *                    planes fall into bf16's subnormal range (quantum 2^-133) and lose bits: each
 *                    operand is then represented to within 2^-134 ABSOLUTE, and the bound is
 *                    2^-19 (|A||B|)_ij + 2^-134 (sum_k |a_ik| + sum_k |b_kj|) -- e.g. A ~ 2^-120
 *                    next to B ~ 2^120 gives ~1e-5 normwise, fp32-subnormal A much more; the
 *                    default fp32 path has no such limit.  An inf/nan operand still gives
 *                    non-finite results, but +inf may become nan.  Any other configuration:
 *                    MM_ERR_UNSUPPORTED.  RunHardware: MM_PATH=split with "hw".  See mm_release_workspace(). */
typedef enum { MM_PATH_AUTO = 0, MM_PATH_ORDERED = 1, MM_PATH_SPLIT = 2 } mm_path_t;

/* Layout of A: row-major N x K (default) or K x N == the reference's MM_TRANSPOSED_A
 * (CMakeLists.txt:30, include/Utility.h:31-35, kernel/Memory.cpp:205-261). */
typedef enum { MM_A_ROW_MAJOR = 0, MM_A_TRANSPOSED = 1 } mm_layout_a_t;

enum {
  MM_OK = 0,
  MM_ERR_NO_DEVICE = 1,   /* no gfx950 device / HIP runtime unusable            */
  MM_ERR_BAD_ARGUMENT = 2,/* null pointer, unknown enum, device index out of range */
  MM_ERR_UNSUPPORTED = 3, /* (dtype, map, reduce) not compiled into this library */
  MM_ERR_HIP = 4          /* a HIP call failed; see mm_last_error()             */
};

typedef struct {
  mm_dtype_t dtype;
  mm_op_t map_op;
  mm_op_t reduce_op;
  mm_path_t path;
  mm_layout_a_t layout_a;
} mm_config_t;

/* ---- device management: replaces hlslib::ocl::Context / MakeBuffer / CopyFromHost /
 *      CopyToHost as used by host/RunHardware.cpp:116-145,187-190 ----------------------------- */

/* hlslib::ocl::Context context; (RunHardware.cpp:116-117).  Reports the number of usable
 * gfx950 devices. */
int mm_init(int *device_count);

/* context.MakeBuffer<...>(DDR bank, elements) (RunHardware.cpp:122-138).  The caller owns the
 * returned device pointer and releases it with mm_free. */
int mm_alloc(int device, size_t bytes, void **device_ptr);
int mm_free(int device, void *device_ptr);

/* buffer.CopyFromHost / CopyToHost (RunHardware.cpp:142-144,189).  Blocking. */
/* Stream-ordered workspace (MM_PATH_SPLIT: 6 bytes per element of A and B of the largest launch so far; the fp32
 * default path: the partial planes / scratch slots of its split-K and stream-K launches, a few MiB, and for a K x N A
 * that does not fill rounds of the K x N kernel's tiles its N x K copy, 4 bytes per element, at most 2 GiB) is cached
 * between launches in a memory pool this library owns -- never in the process's default pool.  This waits for the device and
 * hands that memory back to the driver; the next launch that needs workspace allocates again. */
int mm_release_workspace(int device);

/* The PCI address ("0000:c1:00.0") of HIP device `device`, for tools that must find the same physical GPU through
 * an interface that does not honour HIP_VISIBLE_DEVICES / ROCR_VISIBLE_DEVICES (ROCm SMI, sysfs): the runner's
 * power meter (the reference's PowerMeter role, host/RunHardware.cpp:156-172). */
int mm_device_pci_bus_id(int device, char *buffer, int length);

/* The largest gridDim.y HIP device `device` launches (hipDeviceAttributeMaxGridDimY): the limit the 2-D launches of this
 * library stay under -- taller problems go to 1-D grids -- and the one its tests cross. */
int mm_device_max_grid_dim_y(int device, int *value);

int mm_copy_to_device(int device, void *device_dst, const void *host_src, size_t bytes);
int mm_copy_to_host(int device, void *host_dst, const void *device_src, size_t bytes);

/* Fill a device buffer with the reference's input distribution (uniform in [1,10], values
 * drawn on the device, NOT the seed-5 host stream): for `verify off` timing runs, where the
 * reference leaves its device buffers uninitialised (RunHardware.cpp:99,140). */
int mm_fill_device(int device, mm_dtype_t dtype, void *device_ptr, size_t elements,
                   unsigned long long seed);

/* ---- the kernel: replaces program.MakeKernel("MatrixMultiplicationKernel", a, b, c, N, K, M)
 *      + kernel.ExecuteTask() (RunHardware.cpp:148-162).  C is pure output (kernel/Top.cpp
 *      never reads it).  Sizes follow the reference's contract (RunHardware.cpp:50-61): K and
 *      M multiples of the 64-byte bus in elements; other sizes are served by a slower,
 *      fully predicated kernel rather than rejected. ----------------------------------------- */

/* Blocking launch on `device`; *elapsed_seconds (may be NULL) receives the kernel time
 * measured with HIP events on the launch stream == ExecuteTask()'s elapsed.first.
 * MM_PATH_AUTO needs a, b and c 16-byte aligned (any allocator's result; the reference's host
 * vectors are 4096-byte aligned, include/Utility.h:48) and returns MM_ERR_BAD_ARGUMENT for an
 * offset view; MM_PATH_ORDERED takes any element-aligned pointer.
 * Thread safety: every entry point may be called concurrently from several host threads (on the
 * same or on different devices / streams); mm_last_error() is per thread. */
int mm_gemm_launch(int device, const mm_config_t *cfg, const void *a_dev, const void *b_dev,
                   void *c_dev, unsigned size_n, unsigned size_k, unsigned size_m,
                   double *elapsed_seconds);

/* Asynchronous launch on a caller-provided hipStream_t (passed as void*; NULL = the default
 * stream) of the CURRENT device.  No synchronisation, no timing: for callers that own streams,
 * events and graphs (bench.py, multi-stream pipelines). */
int mm_gemm_enqueue(void *hip_stream, const mm_config_t *cfg, const void *a_dev,
                    const void *b_dev, void *c_dev, unsigned size_n, unsigned size_k,
                    unsigned size_m);

/* Strided batch: `batch` independent problems of one shape in one call (torch.bmm's role).  Element e is the single
 * problem at a_dev + e * stride_a, b_dev + e * stride_b, c_dev + e * stride_c; strides count ELEMENTS, each matrix is
 * dense row-major (A: N x K, or K x N with MM_A_TRANSPOSED).  stride_a or stride_b 0 = one operand shared by every
 * element (broadcast).  With batch > 1, stride_c < N * M is refused (MM_ERR_BAD_ARGUMENT: the outputs would overlap).
 * batch, N or M 0: nothing to do, MM_OK; K 0: refused.  Every argument is checked before any device is touched.
 * Alignment per element as for the single launch: MM_PATH_AUTO needs every element's a, b and c 16-byte aligned (bases,
 * and each stride times the element size a multiple of 16), else MM_ERR_BAD_ARGUMENT; MM_PATH_ORDERED takes any
 * element-aligned pointer and strides.  MM_PATH_SPLIT: MM_ERR_UNSUPPORTED (it needs workspace).  A batched launch never
 * allocates workspace and never splits K: per element, MM_PATH_ORDERED gives Naive's bits, integer types and Min / Max /
 * And reductions under MM_PATH_AUTO the bits of mm_gemm_launch on that element alone, floating (Multiply, Add) the same
 * contract and error bound as the single launch in a summation order that may differ from it.  An element's bits do not
 * depend on its position, the other elements, the strides or how the batch is split into launches ("batch_chunk").
 * Batches beyond a grid limit run as consecutive launches on the same stream.
 * _enqueue: asynchronous on a caller-provided hipStream_t of the CURRENT device (like mm_gemm_enqueue); _launch: blocking,
 * *elapsed_seconds (may be NULL) = the whole batch, all launches, timed with HIP events. */
int mm_gemm_batched_enqueue(void *hip_stream, const mm_config_t *cfg, const void *a_dev, const void *b_dev, void *c_dev,
                            unsigned size_n, unsigned size_k, unsigned size_m, unsigned batch,
                            size_t stride_a, size_t stride_b, size_t stride_c);
int mm_gemm_batched_launch(int device, const mm_config_t *cfg, const void *a_dev, const void *b_dev, void *c_dev,
                           unsigned size_n, unsigned size_k, unsigned size_m, unsigned batch,
                           size_t stride_a, size_t stride_b, size_t stride_c, double *elapsed_seconds);

/* Accumulate: C <- C (+) (A (x) B) in place -- for each output the value C holds replaces identity() as the start of the
 * reduction; nothing else about it changes (D <- min(D, A + B) of min-plus relaxation, BLAS beta = 1 / torch.addmm_ of
 * (Multiply, Add), a K split the caller drives itself).
 *   MM_PATH_ORDERED: Naive (include/Utility.h:18-42) with acc = C[i][j] in place of acc = identity(), bit for bit, every dtype
 *     -- so a Min reduction seeded with +inf whose mapped values are all +inf returns +inf (not max()), and a NaN seed
 *     follows from b < a ? b : a.
 *   MM_PATH_AUTO, integer types and Min / Max / And reductions: the bits of the seeded MM_PATH_ORDERED result (floating Min /
 *     Max for non-NaN operands, with the minNum / maxNum caveat above).  (Multiply, Add) on the matrix cores: float, double and
 *     half (wide contract) keep the single launch's error bound with |C_in| + |A||B| in place of |A||B| (half: one rounding
 *     on store); int8 / uint8 add the seed to the i32 sums and keep the low 8 bits (exact); half_contract = reference
 *     accumulates in binary16 from the seed.
 * Arguments as for mm_gemm_batched_* (strides in elements, 0 = broadcast, stride_c >= N * M when batch > 1, 16-byte
 * alignment per element for the fast families under MM_PATH_AUTO, MM_PATH_SPLIT: MM_ERR_UNSUPPORTED; batch, N or M 0:
 * MM_OK), all checked before any device is touched, with two differences: K = 0 is accepted and leaves C unchanged
 * (MM_OK), and C must not overlap A or B -- a conservative span test, [base, base + ((batch - 1) * stride + extent)
 * elements) per operand, else MM_ERR_BAD_ARGUMENT.  C is read and written by the same thread: in place is safe.
 * An accumulating launch runs exactly the kernel mm_kernel_name_batched(cfg, n, k, m, batch) names, batch = 1 included: no
 * workspace, no split of K, no stream-K (mid-size fp32 shapes run whole tiles -- slower than mm_gemm_launch there).
 * _enqueue: asynchronous on a hipStream_t of the CURRENT device; _launch: blocking, *elapsed_seconds (may be NULL) timed
 * with HIP events.  The single forms are the batched ones with batch = 1. */
int mm_gemm_accumulate_enqueue(void *hip_stream, const mm_config_t *cfg, const void *a_dev, const void *b_dev, void *c_dev,
                               unsigned size_n, unsigned size_k, unsigned size_m);
int mm_gemm_accumulate_launch(int device, const mm_config_t *cfg, const void *a_dev, const void *b_dev, void *c_dev,
                              unsigned size_n, unsigned size_k, unsigned size_m, double *elapsed_seconds);
int mm_gemm_batched_accumulate_enqueue(void *hip_stream, const mm_config_t *cfg, const void *a_dev, const void *b_dev,
                                       void *c_dev, unsigned size_n, unsigned size_k, unsigned size_m, unsigned batch,
                                       size_t stride_a, size_t stride_b, size_t stride_c);
int mm_gemm_batched_accumulate_launch(int device, const mm_config_t *cfg, const void *a_dev, const void *b_dev, void *c_dev,
                                      unsigned size_n, unsigned size_k, unsigned size_m, unsigned batch, size_t stride_a,
                                      size_t stride_b, size_t stride_c, double *elapsed_seconds);

/* Argmin / argmax: a Min- or Max-reduced product that also returns, per output, the k that produced it (the witness:
 * predecessor matrices of shortest paths, Viterbi backpointers, bottleneck paths) -- torch.min(x, dim)'s (values, indices).
 * For output (e, i, j) of the batch, with Reduce = cfg->reduce_op in {Min, Max}:
 *     acc = accumulate ? C[e,i,j] : Reduce::identity();   idx = accumulate ? I[e,i,j] : -1
 *     for k = 0 .. K-1 ascending:
 *         s = Map(A[e,i,k], B[e,k,j])                     (Op<MAP, T>::apply; integers wrap as everywhere)
 *         if (Min: s < acc  /  Max: acc < s) { acc = s; idx = index_base + k; }
 *     C[e,i,j] = acc;  I[e,i,j] = idx
 * So C is bit for bit what MM_PATH_ORDERED's mm_gemm_batched_launch (plain) / mm_gemm_batched_accumulate_launch
 * (accumulate) returns, NaN, +-inf and +-0 included, under MM_PATH_AUTO too (no minNum / maxNum here, and
 * MM_HALF_CONTRACT does not apply); ties keep the smallest k; a NaN mapped value is never taken; -1 = no k improved on
 * the identity (e.g. every path +inf, or max()); when accumulating, an index whose seed survives is left exactly as it was.
 * c_index: int32, the same shape and element strides (stride_c) as C.  index_base >= 0 shifts the recorded k (a blocked
 * or K-split caller records global k: A[:, K1:], B[K1:] with index_base = K1); index_base + K - 1 must not exceed
 * INT32_MAX.  Every other argument as for mm_gemm_batched_* (strides in elements, 0 = broadcast, stride_c >= N * M when
 * batch > 1; batch, N or M 0: MM_OK).  K = 0: MM_ERR_BAD_ARGUMENT in the plain form, MM_OK (nothing changes) when
 * accumulating.  Refused before any device is touched: a reduction other than Min / Max and MM_PATH_SPLIT
 * (MM_ERR_UNSUPPORTED); a null pointer, a bad index_base, and the span of C or of I overlapping A, B or each other (the
 * span test of the accumulating calls; MM_ERR_BAD_ARGUMENT).
 * Kernels (mm_kernel_name_argreduce): "argreduce_tile" (register-tiled, 128 x 128 outputs per workgroup) under
 * MM_PATH_AUTO where valu_tile serves -- K % 4 == 0, M % 4 == 0 (and N % 4 == 0 for a K x N A), a map other than And --
 * for elements of at most 4 bytes; "argreduce" (fully predicated, any shape, any element-aligned pointer) otherwise --
 * double, long and unsigned long always -- and always under MM_PATH_ORDERED.
 * The name is decided by shape and path alone: a launch whose a, b, c, c_index (or element strides) are not 16-byte
 * aligned runs "argreduce" instead -- the same bits, no error.  The batch is split into launches as for the batched calls.
 * _enqueue: asynchronous on a hipStream_t of the CURRENT device; _launch: blocking, *elapsed_seconds (may be NULL) timed
 * with HIP events.  A single problem is batch = 1. */
int mm_gemm_argreduce_enqueue(void *hip_stream, const mm_config_t *cfg, const void *a_dev, const void *b_dev, void *c_dev,
                              int *c_index, unsigned size_n, unsigned size_k, unsigned size_m, unsigned batch,
                              size_t stride_a, size_t stride_b, size_t stride_c, int index_base, int accumulate);
int mm_gemm_argreduce_launch(int device, const mm_config_t *cfg, const void *a_dev, const void *b_dev, void *c_dev,
                             int *c_index, unsigned size_n, unsigned size_k, unsigned size_m, unsigned batch,
                             size_t stride_a, size_t stride_b, size_t stride_c, int index_base, int accumulate,
                             double *elapsed_seconds);
/* Name of the kernel mm_gemm_argreduce_* runs for this shape ("argreduce_tile", "argreduce"; "unsupported" for a reduction
 * other than Min / Max or MM_PATH_SPLIT; "invalid" for a bad configuration).  Static string, pure arithmetic. */
const char *mm_kernel_name_argreduce(const mm_config_t *cfg, unsigned size_n, unsigned size_k, unsigned size_m,
                                     unsigned batch);

/* Log semiring: the smooth form of the (Add, Max) product -- HMM forward algorithm, CRF partition functions, CTC,
 * inside-outside; with Min, the soft-min of soft-DTW and smoothed shortest paths.  For output (e, i, j) of a strided batch
 * the terms are s_k = A[e,i,k] + B[e,k,j], k < K, each one rounded sum in the computation type (f32 for half and float, f64
 * for double); when accumulating, C's input value is one more term.  cfg->reduce_op picks
 *     MM_OP_MAX:  C = log sum_k exp(s_k)          MM_OP_MIN:  C = -log sum_k exp(-s_k)
 * Special values follow torch.logsumexp over the terms, exactly.  Max: a NaN term (a NaN operand in a pair, or +inf + -inf)
 * gives NaN; otherwise a +inf term gives +inf; otherwise all terms -inf give -inf.  Min is the mirror image.  A finite result
 * beyond the output type's range (half) becomes +-inf.  Terms of magnitude beyond 2^127 / log2(e) (float and half) or
 * 2^1023 / log2(e) (double) lie outside the contract: their exponent shift is clamped and the result may overflow.
 * Finite outputs: with ra_i = max_k A[i,k], rb_j = max_k B[k,j] (Min: of the negated operands), u = 2^-24 (half, float) or
 * 2^-53 (double) and C* the exact value,
 *     |C - C*| <= u (4 (|ra_i| + |rb_j|) + 4 |C*| + 2 K + 512)        (+ 2^-11 |C*| for half: the rounding on store)
 * on both kernels (derivation: DESIGN.md 3.9).  A call gives the same bits on every run, and an element's bits depend on
 * neither its position in the batch nor the other elements.
 * Kernels (mm_kernel_name_logsumexp):
 *   "lse_exact"  a register-tiled VALU kernel: every output keeps a running (max, scaled sum) pair; exp2 on v_exp_f32 (f64:
 *                one library exp2 per term, slow).  MM_PATH_ORDERED, and the knob "lse_variant" = 0.
 *   "lse_hybrid" MM_PATH_AUTO: a prepass takes ra, rb and EA = exp(A - ra), EB = exp(B - rb) (zero-padded to multiples of 64,
 *                f32 / f64) into the library's stream-ordered workspace; S = EA @ EB runs on the fp32 / fp64 matrix cores;
 *                an epilogue writes C = ra_i + rb_j + log S and flags every 64 x 64 tile holding an output with S < 2^-64
 *                (f64: 2^-512), a non-finite shift or result; the exact kernel then recomputes the flagged tiles only.  No
 *                host synchronisation, no atomics; the batch is chunked to keep the workspace near 256 MiB.
 * Knob "lse_variant" (MM_LSE_VARIANT): -1 default, 0 exact kernel only, 1 hybrid, 2 hybrid with every tile sent to the
 * fallback (the cross-check); any other value makes the calls return MM_ERR_BAD_ARGUMENT.
 * Arguments as for mm_gemm_argreduce_* without the index: strides in elements, 0 = broadcast, stride_c >= N * M when
 * batch > 1, any element-aligned pointer or stride.  Refused before any device is touched: a dtype other than half, float
 * and double, a map other than Add, a reduction other than Min / Max, MM_PATH_SPLIT (MM_ERR_UNSUPPORTED); a bad knob value,
 * a null pointer, overlapping outputs and C's span overlapping A's or B's (MM_ERR_BAD_ARGUMENT).  batch, N or M 0: MM_OK;
 * K = 0: MM_ERR_BAD_ARGUMENT in the plain form, MM_OK (C unchanged) when accumulating.
 * _enqueue: asynchronous on a hipStream_t of the CURRENT device, never synchronises the host; _launch: blocking,
 * *elapsed_seconds (may be NULL) timed with HIP events. */
int mm_gemm_logsumexp_enqueue(void *hip_stream, const mm_config_t *cfg, const void *a_dev, const void *b_dev, void *c_dev,
                              unsigned size_n, unsigned size_k, unsigned size_m, unsigned batch,
                              size_t stride_a, size_t stride_b, size_t stride_c, int accumulate);
int mm_gemm_logsumexp_launch(int device, const mm_config_t *cfg, const void *a_dev, const void *b_dev, void *c_dev,
                             unsigned size_n, unsigned size_k, unsigned size_m, unsigned batch,
                             size_t stride_a, size_t stride_b, size_t stride_c, int accumulate, double *elapsed_seconds);
/* "lse_hybrid", "lse_exact"; "unsupported" for a configuration the calls refuse with MM_ERR_UNSUPPORTED; "invalid" for a bad
 * configuration or knob value.  Pure arithmetic. */
const char *mm_kernel_name_logsumexp(const mm_config_t *cfg, unsigned size_n, unsigned size_k, unsigned size_m,
                                     unsigned batch);

/* Widening product: the matrix cores' own sums.  cfg->dtype is the OPERAND type, half or int8_t; C has the type
 * mm_widen_dtype() names -- float for half, int for int8_t -- and cfg is otherwise (Multiply, Add).  The narrow entry points keep
 * the reference's single Data_t: they store (int8_t)sum, defined mod 2^8 only, and (half)sum, 11 of the 24 bits the
 * accumulator holds, rounded again on every pass of a K-split through mm_gemm_accumulate_*.  Here nothing is discarded.
 * For output (e, i, j) of a strided batch, with acc's start C's input value when accumulating and 0 otherwise:
 *   int8_t -> int    C = start + sum_k (int)A[e,i,k] * (int)B[e,k,j], taken mod 2^32: the same bits on every kernel and path,
 *                    for every batch position and chunking.  No wrap can occur in the plain form while K <= 131071
 *                    (131071 * 2^14 < 2^31).
 *   half -> float    MM_PATH_ORDERED: acc = start; for k ascending: acc = acc + (float)a * (float)b in f32.  A product of two
 *                    binary16 values is exact in f32, so fused and unfused evaluation give the same bits and a float32 loop
 *                    on the host reproduces C bit for bit.
 *                    MM_PATH_AUTO: exact products, f32 accumulation in an unspecified fixed order, NO rounding on store:
 *                    |C - C*| <= 1e-6 (|C_in| + |A||B|)_ij -- the f32-accumulation term of the half family's bound without
 *                    its 2^-11 store rounding.  The same bits on every run, independent of batch position and chunking.  In
 *                    the plain form, rounding C once to binary16 gives bit for bit what mm_gemm_batched_launch returns for
 *                    the same operands: the same kernel and schedule with a different store.  A launch demoted for
 *                    misalignment (below) sums the same terms in blocks of k and keeps this bound.  One exception, stated
 *                    because it is one: a SHAPE the matrix cores do not take (K % 16 != 0 or M % 8 != 0) runs k ascending
 *                    like MM_PATH_ORDERED -- the order of the narrow call's own fallback on that shape, so that rounding C
 *                    to binary16 still gives the narrow call's bits -- and is bounded by (K - 1) 2^-24 (|C_in| + |A||B|); it
 *                    stays within 1e-6 while K is a few hundred (1.02e-6 was measured at K = 512 on same-sign operands).
 *   Non-finite half operands: the result follows IEEE arithmetic on the f32 sum.
 * uint8_t is refused on purpose: the signed-int8 matrix core serves uint8_t in the narrow calls only because their result is
 * taken mod 2^8, where both types agree; unsigned 32-bit sums need a bias correction with the row sums of A and the column
 * sums of B -- a different kernel, not this one.  The "half_contract" knob does not apply: it picks between two NARROW contracts.
 * Kernels (mm_kernel_name_widen): under MM_PATH_AUTO the kernel mm_kernel_name_batched(cfg, n, k, m, batch) names for the
 * narrow type -- for batch = 1 too, as in the accumulating calls -- instantiated with the wide output: that name + "_wide";
 * no workspace, no transposition pre-pass, no split of K.  "widen_ordered" (k ascending, one wide accumulator, fully
 * predicated: any shape, any element-aligned pointer or stride) serves MM_PATH_ORDERED, every shape for which the narrow
 * batched resolver names no matrix-core kernel, and -- silently, same contract; the name is decided by shape and path --
 * MM_PATH_AUTO launches where some element's A, B or C is not 16-byte aligned.  A K x N A that the narrow single launch would
 * transpose into workspace first (M >= 6144, knob "kxn_prepass_min_m") has no batched matrix-core kernel either: such a call
 * runs widen_ordered, at VALU speed -- transpose A once and call with a row-major A instead.
 * Arguments as for mm_gemm_logsumexp_*: strides count elements of each buffer's own type, 0 = broadcast, stride_c >= N * M
 * when batch > 1.  Refused before any device is touched: a dtype other than half and int8_t, a (map, reduce) other than
 * (Multiply, Add), MM_PATH_SPLIT (MM_ERR_UNSUPPORTED); a null pointer, overlapping outputs and C's span overlapping A's or
 * B's (MM_ERR_BAD_ARGUMENT).  batch, N or M 0: MM_OK; K = 0: MM_ERR_BAD_ARGUMENT in the plain form, MM_OK (C unchanged) when
 * accumulating.  The batch is launched in chunks (knob "batch_chunk"); the kernel is resolved once on the whole batch.
 * _enqueue: asynchronous on a hipStream_t of the CURRENT device, never synchronises the host; _launch: blocking,
 * *elapsed_seconds (may be NULL) timed with HIP events. */
int mm_gemm_widen_enqueue(void *hip_stream, const mm_config_t *cfg, const void *a_dev, const void *b_dev, void *c_dev,
                          unsigned size_n, unsigned size_k, unsigned size_m, unsigned batch,
                          size_t stride_a, size_t stride_b, size_t stride_c, int accumulate);
int mm_gemm_widen_launch(int device, const mm_config_t *cfg, const void *a_dev, const void *b_dev, void *c_dev,
                         unsigned size_n, unsigned size_k, unsigned size_m, unsigned batch,
                         size_t stride_a, size_t stride_b, size_t stride_c, int accumulate, double *elapsed_seconds);
/* A "..._wide" matrix-core kernel or "widen_ordered"; "unsupported" for a configuration the calls refuse with
 * MM_ERR_UNSUPPORTED; "invalid" for a bad configuration.  Static string, pure arithmetic. */
const char *mm_kernel_name_widen(const mm_config_t *cfg, unsigned size_n, unsigned size_k, unsigned size_m, unsigned batch);
/* C's mm_dtype_t for operands of `dtype`: MM_DTYPE_F32 for half, MM_DTYPE_I32 for int8_t; -1 for every other type. */
int mm_widen_dtype(mm_dtype_t dtype);

/* A x B^T: C[e,i,j] = reduce_k map(A[e,i,k], Bt[e,j,k]) -- B stored M x K row-major, k contiguous in BOTH operands: pairwise
 * products between two row-stored point or state sets (min-plus A (x) A^T, Gram matrices, Viterbi steps with a "to-state
 * major" transition matrix) and the dA = G B^T half of a backward pass (dB = A^T G is MM_A_TRANSPOSED's), without the
 * K x M copy and the extra pass of a transposition by the caller.  bt_dev: M x K row-major per element; stride_b counts ITS
 * elements, 0 = broadcast.  accumulate != 0: C <- C (+) (A (x) Bt^T), each chain starting at the value C holds.
 * Kernels (mm_kernel_name_nt), from the family mm_gemm_batched_* would run on (n, k, m, batch) -- for batch = 1 too:
 *   "nt_prepass"    (Multiply, Add) on the matrix cores (float, double, half, int8_t / uint8_t) where the narrow batched
 *                   resolver names a kernel and K, M are multiples of 16 bytes' worth of elements: Bt is transposed into the
 *                   library's stream-ordered workspace (about 256 MiB per chunk of the batch, a broadcast Bt once) and that
 *                   kernel runs on the copy, resolved once on the whole batch: bit for bit what mm_gemm_batched_* /
 *                   mm_gemm_batched_accumulate_* returns on a materialised transpose, with that family's contract.
 *   "valu_tile_nt"  every other configuration under MM_PATH_AUTO with map in {Multiply, Add, Min, Max} and reduce in {Add, Min,
 *                   Max}, where K >= 64 bytes of elements, K is a multiple of 16 bytes of elements and 128 rows of K stay
 *                   below 4 GiB; nothing is asked of N or M.  MM_PATH_AUTO's contract as "valu_tile" keeps it: k ascending on
 *                   one accumulator, so integer and Min / Max results are Naive's bits; floating Min / Max are minNum /
 *                   maxNum (a NaN operand is dropped, +0 / -0 ties unspecified); floating (x, Add) may fuse.
 *   "ordered_nt"    MM_PATH_ORDERED, half_contract = 1, and every shape or operator the rows above do not take: Naive on
 *                   Bt[j][k] -- k ascending, one accumulator, unfused -- bit-identical to the reference's Naive on the transposed
 *                   operand for all 275 configurations; any shape, any element-aligned pointer or stride.  ONE exception, as
 *                   in the row-major calls: half (Multiply, Add) under MM_PATH_AUTO (half_contract unset) accumulates in f32
 *                   and rounds once on store -- the matrix cores' contract, kept on every shape.
 * The name is decided by configuration, shape and path.  A launch whose A or Bt ("nt_prepass": or C) -- base or element stride --
 * is not 16-byte aligned runs ordered_nt instead, silently and under the same contract, as does "nt_prepass" when the pool
 * cannot give the workspace.
 * Arguments as for mm_gemm_widen_*: strides count elements, stride_c >= N * M when batch > 1.  Refused before any device is
 * touched: MM_PATH_SPLIT and MM_A_TRANSPOSED (MM_ERR_UNSUPPORTED: A^T B^T is not served); a null pointer, C's span overlapping
 * A's or Bt's (MM_ERR_BAD_ARGUMENT).  A and Bt may be the same buffer (A (x) A^T).  batch, N or M 0: MM_OK; K = 0:
 * MM_ERR_BAD_ARGUMENT in the plain form, MM_OK (C unchanged) when accumulating.  The batch is launched in chunks (knob
 * "batch_chunk"); an element's bits do not depend on the chunk it falls in.
 * _enqueue: asynchronous on a hipStream_t of the CURRENT device, never synchronises the host; _launch: blocking,
 * *elapsed_seconds (may be NULL) timed with HIP events. */
int mm_gemm_nt_enqueue(void *hip_stream, const mm_config_t *cfg, const void *a_dev, const void *bt_dev, void *c_dev,
                       unsigned size_n, unsigned size_k, unsigned size_m, unsigned batch,
                       size_t stride_a, size_t stride_b, size_t stride_c, int accumulate);
int mm_gemm_nt_launch(int device, const mm_config_t *cfg, const void *a_dev, const void *bt_dev, void *c_dev,
                      unsigned size_n, unsigned size_k, unsigned size_m, unsigned batch,
                      size_t stride_a, size_t stride_b, size_t stride_c, int accumulate, double *elapsed_seconds);
/* "nt_prepass", "valu_tile_nt" or "ordered_nt"; "unsupported" for a configuration the calls refuse with MM_ERR_UNSUPPORTED;
 * "invalid" for a bad configuration.  Static string, pure arithmetic. */
const char *mm_kernel_name_nt(const mm_config_t *cfg, unsigned size_n, unsigned size_k, unsigned size_m, unsigned batch);

/* A x B^T forms of the two derived products: mm_gemm_argreduce_* and mm_gemm_logsumexp_* with B stored M x K row-major, as
 * in mm_gemm_nt_* -- the backpointers of a Viterbi step and the forward / partition-function step over a "to-state major"
 * transition matrix, without the K x M copy of a transposition by the caller.  bt_dev: M x K row-major per element; stride_b
 * counts ITS elements, 0 = broadcast.  Each contract is the row-major call's with B[e,k,j] read as Bt[e,j,k]; every other
 * argument (c_index, index_base, accumulate, the strides, the "batch_chunk" chunking) is the row-major call's.
 * Argmin / argmax.  For output (e, i, j), with Reduce = cfg->reduce_op in {Min, Max}:
 *     acc = accumulate ? C[e,i,j] : Reduce::identity();   idx = accumulate ? I[e,i,j] : -1
 *     for k = 0 .. K-1 ascending:
 *         s = Map(A[e,i,k], Bt[e,j,k])
 *         if (Min: s < acc  /  Max: acc < s) { acc = s; idx = index_base + k; }
 *     C[e,i,j] = acc;  I[e,i,j] = idx
 * C and I are bit for bit what mm_gemm_argreduce_* returns on a materialised transpose, on both kernels and under both
 * paths, NaN, +-inf and +-0 included: ties keep the smallest k, a NaN mapped value is never taken, a surviving seed keeps its
 * index.  Kernels (mm_kernel_name_argreduce_nt): "argreduce_tile_nt" (the register-tiled kernel, Bt staged the way it stages
 * an N x K A) under MM_PATH_AUTO for elements of at most 4 bytes with a map in {Add, Multiply, Min, Max}, K % 4 == 0 and
 * M % 4 == 0; "argreduce_nt" (fully predicated, any shape, any element-aligned pointer, every map) for everything else --
 * the 8-byte types, the And map, any other shape -- and always under MM_PATH_ORDERED.  The name is decided by
 * configuration, shape and path alone: a tile launch whose a, bt, c or c_index -- base, or element stride in bytes -- is not
 * 16-byte aligned runs "argreduce_nt" instead, the same bits, no error.
 * Log semiring.  The terms are s_k = A[e,i,k] + Bt[e,j,k]; the error bound (with rb_j = max_k Bt[j,k]), the special-value
 * rules and the determinism of mm_gemm_logsumexp_* hold unchanged.  Kernels (mm_kernel_name_logsumexp_nt), chosen exactly as
 * mm_kernel_name_logsumexp chooses, "lse_variant" included: "lse_exact_nt" has the row-major exact kernel's per-output
 * sequence and gives its bits on a materialised transpose; "lse_hybrid_nt" takes rb and EB from Bt as it lies (EB still
 * K-major in the workspace), runs the same product and epilogue, and falls back to lse_exact_nt on the flagged tiles: the
 * row-major hybrid's values, where only the sign of a zero may differ, because the maxima of Bt are reduced in another
 * order.  Workspace, chunking and "never synchronises the host" as for the row-major hybrid.
 * Refused before any device is touched: MM_A_TRANSPOSED (MM_ERR_UNSUPPORTED, as in mm_gemm_nt_*) and everything the
 * row-major call of the product refuses, with its status: MM_PATH_SPLIT, a reduction other than Min / Max, for the log
 * semiring a dtype other than half, float and double or a map other than Add (MM_ERR_UNSUPPORTED); a bad "lse_variant" or
 * index_base, a null pointer, overlapping outputs, and the span of C (or of I) overlapping A's or Bt's
 * (MM_ERR_BAD_ARGUMENT).  A and Bt may be the same buffer.  batch, N or M 0: MM_OK; K = 0: MM_ERR_BAD_ARGUMENT in the plain
 * form, MM_OK (nothing written) when accumulating.
 * _enqueue: asynchronous on a hipStream_t of the CURRENT device, never synchronises the host; _launch: blocking,
 * *elapsed_seconds (may be NULL) timed with HIP events. */
int mm_gemm_argreduce_nt_enqueue(void *hip_stream, const mm_config_t *cfg, const void *a_dev, const void *bt_dev, void *c_dev,
                                 int *c_index, unsigned size_n, unsigned size_k, unsigned size_m, unsigned batch,
                                 size_t stride_a, size_t stride_b, size_t stride_c, int index_base, int accumulate);
int mm_gemm_argreduce_nt_launch(int device, const mm_config_t *cfg, const void *a_dev, const void *bt_dev, void *c_dev,
                                int *c_index, unsigned size_n, unsigned size_k, unsigned size_m, unsigned batch,
                                size_t stride_a, size_t stride_b, size_t stride_c, int index_base, int accumulate,
                                double *elapsed_seconds);
/* "argreduce_tile_nt" or "argreduce_nt"; "unsupported" for a configuration the calls refuse with MM_ERR_UNSUPPORTED;
 * "invalid" for a bad configuration.  Static string, pure arithmetic. */
const char *mm_kernel_name_argreduce_nt(const mm_config_t *cfg, unsigned size_n, unsigned size_k, unsigned size_m,
                                        unsigned batch);
int mm_gemm_logsumexp_nt_enqueue(void *hip_stream, const mm_config_t *cfg, const void *a_dev, const void *bt_dev, void *c_dev,
                                 unsigned size_n, unsigned size_k, unsigned size_m, unsigned batch,
                                 size_t stride_a, size_t stride_b, size_t stride_c, int accumulate);
int mm_gemm_logsumexp_nt_launch(int device, const mm_config_t *cfg, const void *a_dev, const void *bt_dev, void *c_dev,
                                unsigned size_n, unsigned size_k, unsigned size_m, unsigned batch,
                                size_t stride_a, size_t stride_b, size_t stride_c, int accumulate, double *elapsed_seconds);
/* "lse_hybrid_nt" or "lse_exact_nt"; "unsupported" for a configuration the calls refuse with MM_ERR_UNSUPPORTED; "invalid"
 * for a bad configuration or knob value.  Pure arithmetic. */
const char *mm_kernel_name_logsumexp_nt(const mm_config_t *cfg, unsigned size_n, unsigned size_k, unsigned size_m,
                                        unsigned batch);

/* Closure: all-pairs shortest / widest / longest paths and transitive closure -- blocked Floyd-Warshall, in place.
 * D is n x n, row-major; graph e of the batch starts at d_dev + e * stride_d (elements; stride_d >= n * n when batch > 1).
 * The call runs the recurrence D[i][j] <- D[i][j] (+) D[i][v] (x) D[v][j] over every v, with Reduce = cfg->reduce_op in
 * {Min, Max} and Map = cfg->map_op (every dtype, every map: 110 configurations).  No identity is added to the diagonal, so the
 * result is A+ (paths of one or more edges); for A* the caller first sets the diagonal to the map's identity (0 for Add, 1 for
 * Multiply and And, ...).
 * The caller's obligation: the result equals plain Floyd-Warshall only where the semiring is absorptive on the input,
 * x (+) (d_kk (x) x) == x.  Min-plus needs no negative cycles; integer sums must not overflow, so "no edge" is a sentinel such
 * as max() / 2, not max(); max-plus needs no positive cycles (a DAG); (Min, Max), (Max, Min) are always absorptive, and so is
 * (And, Max) on 0 / 1.  Outside that, the result is still fully defined by the blocked algorithm, bit for bit:
 *   block t covers K = [tB, min(n, (t + 1)B)); for t ascending:
 *   1. for v in K ascending: D[K,K] <- D[K,K] (+) D[K,v] (x) D[v,K] (row v and column v read before the step) -- call it P;
 *   2. row panel D[K,J] <- D[K,J] (+) P (x) D[K,J]_old for J outside K, column panel D[I,K] <- D[I,K] (+) D[I,K]_old (x) P for
 *      I outside K: reductions over v in K from the old value as seed;
 *   3. D <- D (+) Cc (x) Rc over the whole matrix, Cc = D[:,K] and Rc = D[K,:] as steps 1 and 2 left them.
 *   With n <= B only step 1 runs (one workgroup per graph, on chip: many small graphs in one launch).
 * A winner is always a strict improvement (Min: s < acc, Max: acc < s, the select of the k-ordered contract), ties keep the
 * first v.  Min / Max are exact and each map value is rounded once in the element type, so D's bits follow (NaN and signed
 * zeros aside: step 3 under MM_PATH_AUTO, value-only, runs valu_tile's minNum / maxNum) and are the same from run to run.
 * witness_dev (int32, D's shape and strides; may be NULL): fully written; the intermediate vertex v of the last strict
 * improvement of (i, j), or -1 where D[i][j] kept its input value.  Expanding (i, w, j) recursively gives the path.
 * B: 256 for the value-only form of elements of at most 4 bytes, 128 otherwise; the tuning knob "closure_block" (-1 =
 * default) takes 64, 128, and 256 where the form allows it -- any other value makes the call return MM_ERR_BAD_ARGUMENT.
 * Step 3 runs what mm_kernel_name_batched (value-only, accumulating; under MM_PATH_AUTO a D not 16-byte aligned per graph runs
 * the k-ordered kernel, the same values) or mm_kernel_name_argreduce (witnesses, index_base = tB) names for (n, B, n); the
 * snapshots live in the library's stream-ordered workspace pool (2 n B elements per graph, the batch chunked to stay near
 * 256 MiB).  Refused before any device is touched: reductions other than Min / Max (Add, Multiply and And are not idempotent:
 * no closure) and MM_PATH_SPLIT (MM_ERR_UNSUPPORTED); MM_A_TRANSPOSED, a null d_dev, stride_d < n * n with batch > 1 and a
 * witness span overlapping D's (MM_ERR_BAD_ARGUMENT).  n or batch 0: MM_OK, nothing done (_launch reports 0 s).
 * _enqueue: asynchronous on a hipStream_t of the CURRENT device, never synchronises the host; _launch: blocking,
 * *elapsed_seconds (may be NULL) timed with HIP events. */
int mm_closure_enqueue(void *hip_stream, const mm_config_t *cfg, void *d_dev, int *witness_dev, unsigned n, unsigned batch,
                       size_t stride_d);
int mm_closure_launch(int device, const mm_config_t *cfg, void *d_dev, int *witness_dev, unsigned n, unsigned batch,
                      size_t stride_d, double *elapsed_seconds);
/* "closure_onchip" (n <= B) or "closure_blocked"; "unsupported" for a reduction other than Min / Max or MM_PATH_SPLIT;
 * "invalid" for a bad configuration, MM_A_TRANSPOSED or a closure_block this form does not take.  Pure arithmetic. */
const char *mm_kernel_name_closure(const mm_config_t *cfg, unsigned n, unsigned batch, int with_witness);

/* ---- bit-packed Boolean semiring: (AND, OR) on one bit per element -------------------------------------------------------
 * Storage format (the contract of every mm_bits_* call).  A Boolean rows x cols matrix is `rows` rows of 32-bit words:
 * column j is bit (j & 31) of word (j >> 5), least significant bit first -- on the host
 * np.packbits(x, axis=-1, bitorder="little"), padded to a multiple of 4 bytes and viewed as uint32.  Each operand has a row
 * stride ld in WORDS, ld >= ceil(cols / 32), so a column slice of a packed matrix (whole words) and a panel of a larger
 * matrix are operands as they lie.  Padding bits -- positions >= cols in a row's last word -- are ignored in every input,
 * whatever they hold, and written as 0 in every output.  The words of a row beyond ceil(cols / 32), up to ld, are never
 * read and never written.  Pointers are 4-byte aligned; batch strides count words.
 *
 * Product: C[e,i,j] = OR_k (A[e,i,k] AND B[e,k,j]); a: N x K packed along K, b: K x M packed along M, c: N x M packed along
 * M.  accumulate != 0: C <- C | A B (the valid bits of C's input are kept, its padding bits are dropped).  stride_a or
 * stride_b 0 = one operand shared by the batch; with batch > 1, stride_c >= (N - 1) ldc + ceil(M / 32).  batch, N or M 0:
 * MM_OK, nothing done (_launch reports 0 s); so is K = 0 when accumulating; K = 0 in the plain form writes C = 0, the
 * empty OR (a and b are then not read and may be null).  Refused with MM_ERR_BAD_ARGUMENT before any device is touched: a
 * null pointer, an ld below its row's word count, outputs of the batch that would overlap, and a span of C -- [base, base +
 * (batch - 1) stride + (rows - 1) ld + words) -- that overlaps A's or B's.
 * Kernels (mm_kernel_name_bits_gemm; pure arithmetic, the launcher's own resolver):
 *   "bits_tile"   64 rows x 128 words of C per workgroup, K streamed through LDS in slabs of 32; a thread holds 16 rows x 2
 *                 words, forms each row's mask from A's bit with one scalar instruction and does acc |= mask & b.  Serves
 *                 M > 2048 with ldb % 4 == 0 and ldc % 2 == 0 (16-byte loads of B, 8-byte loads and stores of C).
 *   "bits_plain"  the same loop on 64 rows x 64 words with one-word accesses: every shape, every ld, any 4-byte aligned
 *                 pointer.
 * Knob "bits_variant" (MM_BITS_VARIANT): -1 the rule above, 0 bits_plain always, 1 bits_tile wherever its ld rule holds,
 * whatever M; any other value: MM_ERR_BAD_ARGUMENT ("invalid" as a name).  The name is decided by shape and ld alone: a
 * bits_tile launch whose b is not 16-byte aligned or whose c is not 8-byte aligned -- base, or batch stride -- runs
 * bits_plain instead, the same bits, no error.  All-zero words of A are skipped: the time depends on the data, the result
 * does not.  The batch is launched in chunks (knob "batch_chunk").
 * _enqueue: asynchronous on a hipStream_t of the CURRENT device, never synchronises the host; _launch: blocking,
 * *elapsed_seconds (may be NULL) timed with HIP events. */
int mm_bits_gemm_enqueue(void *hip_stream, const void *a_dev, const void *b_dev, void *c_dev, unsigned size_n, unsigned size_k,
                         unsigned size_m, size_t lda, size_t ldb, size_t ldc, unsigned batch, size_t stride_a,
                         size_t stride_b, size_t stride_c, int accumulate);
int mm_bits_gemm_launch(int device, const void *a_dev, const void *b_dev, void *c_dev, unsigned size_n, unsigned size_k,
                        unsigned size_m, size_t lda, size_t ldb, size_t ldc, unsigned batch, size_t stride_a,
                        size_t stride_b, size_t stride_c, int accumulate, double *elapsed_seconds);
const char *mm_kernel_name_bits_gemm(unsigned size_n, unsigned size_k, unsigned size_m, size_t lda, size_t ldb, size_t ldc,
                                     unsigned batch);

/* Product over the field GF(2), C = XOR_k (A AND B) on this format (mm_bits_gf2_*): "mm_bits_gf2.h", a header of its own,
 * included at the end of this one. */

/* Transitive closure, in place: D <- D+, (i, j) set when a path of one or more edges leads from i to j.  No identity is
 * added to the diagonal, as in mm_closure_*.  OR is idempotent, so the result does not depend on the algorithm.  d: n x n
 * packed, row stride ldd >= ceil(n / 32) words; graph e at d_dev + e * stride_d (stride_d >= (n - 1) ldd + ceil(n / 32)
 * when batch > 1).  Kernels (mm_kernel_name_bits_closure): "bits_closure_onchip" for n <= 64 -- one wavefront per graph,
 * one row per lane, the pivot row by broadcast; four graphs per workgroup, 2^20 graphs per launch -- else
 * "bits_closure_blocked": blocked Warshall over blocks K of 64 vertices; per block the wavefront kernel closes D[K,K] into P
 * and writes P | I to workspace, the product kernels take R = (P | I) D[K,:] and Cc = D[:,K] (P | I) into workspace (the
 * panels as the round leaves them), and D <- D | Cc R runs as the accumulating product with ld = ldd.  The workspace (about
 * 66 ceil(n / 32) + 2 n words per graph) comes from the library's stream-ordered pool; the batch is chunked to keep it near
 * 256 MiB and by "batch_chunk".  Refused before any device is touched: a null d_dev, ldd < ceil(n / 32), overlapping graphs
 * (MM_ERR_BAD_ARGUMENT).  n or batch 0: MM_OK, nothing done.  _enqueue / _launch as above. */
int mm_bits_closure_enqueue(void *hip_stream, void *d_dev, unsigned n, size_t ldd, unsigned batch, size_t stride_d);
int mm_bits_closure_launch(int device, void *d_dev, unsigned n, size_t ldd, unsigned batch, size_t stride_d,
                           double *elapsed_seconds);
const char *mm_kernel_name_bits_closure(unsigned n, unsigned batch);

/* Conversions between a row-major matrix of one-byte elements (bool, uint8_t; row stride ld in BYTES, batch stride in bytes)
 * and the packed form (row stride and batch stride in words).  pack: a nonzero byte is 1, padding bits are written 0;
 * unpack writes 0 or 1.  Only ceil(cols / 32) words and cols bytes of a row are touched.  Refused before any device is
 * touched: a null pointer, an ld below its row, a destination whose rows or batch elements would overlap, and a
 * destination span overlapping the source's (MM_ERR_BAD_ARGUMENT).  rows, cols or batch 0: MM_OK, nothing done. */
int mm_bits_pack_enqueue(void *hip_stream, const void *bytes_dev, void *packed_dev, unsigned rows, unsigned cols,
                         size_t ld_bytes, size_t ld_packed, unsigned batch, size_t stride_bytes, size_t stride_packed);
int mm_bits_pack_launch(int device, const void *bytes_dev, void *packed_dev, unsigned rows, unsigned cols, size_t ld_bytes,
                        size_t ld_packed, unsigned batch, size_t stride_bytes, size_t stride_packed, double *elapsed_seconds);
int mm_bits_unpack_enqueue(void *hip_stream, const void *packed_dev, void *bytes_dev, unsigned rows, unsigned cols,
                           size_t ld_packed, size_t ld_bytes, unsigned batch, size_t stride_packed, size_t stride_bytes);
int mm_bits_unpack_launch(int device, const void *packed_dev, void *bytes_dev, unsigned rows, unsigned cols, size_t ld_packed,
                          size_t ld_bytes, unsigned batch, size_t stride_packed, size_t stride_bytes, double *elapsed_seconds);

/* Counting products on the packed format, A x B^T: C[e,i,j] = sum_k (A[e,i,k] op Bt[e,j,k]) as int32, op AND (common
 * neighbours, set intersections, binarised dot products) or XOR (Hamming distances) on single bits.  A count over k needs
 * both operands packed along k: a is N x K with lda >= ceil(K / 32) words, bt is M x K with ldbt >= ceil(K / 32) words --
 * sets of row-stored codes as they lie (mm_bits_transpose_* below converts a K x M operand of mm_bits_gemm_*).  c is N x M
 * row-major int32: ldc >= M and stride_c count ELEMENTS; elements of a row beyond M, up to ldc, and the space between batch
 * elements are never written.  Padding bits of a and bt are ignored, whatever they hold -- under XOR too, where a padding
 * bit set in one operand alone must not count -- and words of a row beyond ceil(K / 32) are never read.  accumulate != 0:
 * C += counts, mod 2^32 like the library's integer Add.  stride_a or stride_bt 0 = one operand shared by the batch; with
 * batch > 1, stride_c >= (N - 1) ldc + M.  batch, N or M 0: MM_OK, nothing done (_launch reports 0 s); so is K = 0 when
 * accumulating; K = 0 in the plain form writes C = 0 (a and bt are then not read and may be null).  Refused with
 * MM_ERR_BAD_ARGUMENT before any device is touched: an op outside mm_bits_count_op_t, a null pointer, an ld below its row,
 * outputs of the batch that would overlap, and a span of C in bytes -- [base, base + 4 ((batch - 1) stride + (rows - 1) ld
 * + M)) -- that overlaps A's or Bt's.
 * Kernels (mm_kernel_name_bits_count; pure arithmetic, the launcher's own resolver):
 *   "bits_count_tile"   128 x 128 outputs per workgroup, 8 x 8 int32 accumulators per thread, K streamed through LDS in slabs
 *                       of 8 words (256 k) stored k-major, so a thread's 8 rows of A and 8 rows of Bt are two 16-byte LDS
 *                       reads each per word; per output and word one AND / XOR and one accumulating population count.
 *                       Serves lda % 4 == 0, ldbt % 4 == 0, ldc % 4 == 0 (16-byte loads of A and Bt, 16-byte loads and
 *                       stores of C) from ceil(N / 128) ceil(M / 128) >= 256 tiles, one per compute unit.
 *   "bits_count_plain"  the same loop on 64 x 64 outputs, 4 x 4 per thread, with one-word / one-element accesses: every
 *                       shape, every ld, any 4-byte aligned pointer.
 * Knob "bits_count_variant" (MM_BITS_COUNT_VARIANT): -1 the rule above, 0 bits_count_plain always, 1 bits_count_tile
 * wherever its ld rule holds, whatever the shape; any other value: MM_ERR_BAD_ARGUMENT ("invalid" as a name).  The name is
 * decided by shape and ld alone: a bits_count_tile launch whose a, bt or c is not 16-byte aligned -- base, or a batch stride
 * that is no multiple of 4 -- runs bits_count_plain instead, the same values, no error.  The time does not depend on the
 * data.  The batch is launched in chunks (knob "batch_chunk").  _enqueue / _launch as for mm_bits_gemm_*. */
typedef enum { MM_BITS_COUNT_AND = 0, MM_BITS_COUNT_XOR = 1 } mm_bits_count_op_t;
int mm_bits_count_enqueue(void *hip_stream, int op, const void *a_dev, const void *bt_dev, void *c_dev, unsigned size_n,
                          unsigned size_k, unsigned size_m, size_t lda, size_t ldbt, size_t ldc, unsigned batch,
                          size_t stride_a, size_t stride_bt, size_t stride_c, int accumulate);
int mm_bits_count_launch(int device, int op, const void *a_dev, const void *bt_dev, void *c_dev, unsigned size_n,
                         unsigned size_k, unsigned size_m, size_t lda, size_t ldbt, size_t ldc, unsigned batch,
                         size_t stride_a, size_t stride_bt, size_t stride_c, int accumulate, double *elapsed_seconds);
const char *mm_kernel_name_bits_count(unsigned size_n, unsigned size_k, unsigned size_m, size_t lda, size_t ldbt, size_t ldc,
                                      unsigned batch);

/* Packed transpose: src is rows x cols packed along cols (ld_src >= ceil(cols / 32) words), dst is cols x rows packed along
 * rows (ld_dst >= ceil(rows / 32) words), dst[j, i] = src[i, j]; batch strides in words.  Padding bits of src are ignored,
 * padding bits of dst are written 0, the words of a row beyond its word count are never touched on either side.  One
 * wavefront takes one word from each of 64 consecutive source rows and 32 ballots, one per bit position: two words of 32
 * destination rows.  Refused before any device is touched: a null pointer, an ld below its row, a destination whose rows or
 * batch elements would overlap, and a destination span overlapping the source's -- there is no in-place form
 * (MM_ERR_BAD_ARGUMENT).  rows, cols or batch 0: MM_OK, nothing done. */
int mm_bits_transpose_enqueue(void *hip_stream, const void *src_dev, void *dst_dev, unsigned rows, unsigned cols,
                              size_t ld_src, size_t ld_dst, unsigned batch, size_t stride_src, size_t stride_dst);
int mm_bits_transpose_launch(int device, const void *src_dev, void *dst_dev, unsigned rows, unsigned cols, size_t ld_src,
                             size_t ld_dst, unsigned batch, size_t stride_src, size_t stride_dst, double *elapsed_seconds);

/* One node, `device_count` GPUs, rows of C split into contiguous slabs (device g gets the rows mm_row_slab() names), B
 * replicated, no collective: every outer tile of C is independent (kernel/Compute.cpp:53-60, kernel/Memory.cpp:114-127,
 * 272-286, 367-391).  Host pointers in, host pointer out; copies are outside the timed region exactly as in
 * RunHardware.cpp:140-190.  *elapsed_seconds = the longest of the devices' kernel times, each measured with HIP events on that
 * device's stream (mm_gemm_multi_device_timed also hands out the per-device figures and the host clock).  New functionality
 * (the reference is single-device).  A K x N A (MM_A_TRANSPOSED == MM_TRANSPOSED_A, kernel/Memory.cpp:205-261)
 * is split along its columns (one strided copy per device).  With device_count = 1 (or N within one slab) the launch is
 * mm_gemm_launch's.  The kernel FAMILY and every decision that changes a row's summation order (split-K of small fp32
 * problems) are taken on the whole job, so a split gives the one-device bits -- except for the mid-size fp32 shapes a
 * single device runs as stream-K (one to two rounds of 128 x 128 tiles), which slabs run as whole tiles: same contract,
 * different summation order.
 * Tests only: "md_virtual_devices" = V (MM_MD_VIRTUAL_DEVICES) lets device_count go up to V LOGICAL devices dealt out over
 * the physical ones round-robin, so that every per-device branch runs on a 1-GPU box. */
int mm_gemm_multi_device(int device_count, const mm_config_t *cfg, const void *a_host,
                         const void *b_host, void *c_host, unsigned size_n, unsigned size_k,
                         unsigned size_m, double *elapsed_seconds);
/* The same call, saying where the time went ("max over devices of kernel time").  Every
 * device's launch is bracketed by HIP events on its own stream: *elapsed_seconds = the MAX over devices of that kernel time
 * (== what mm_gemm_multi_device reports), per_device_seconds[g] (device_count entries, may be NULL) = device g's own kernel
 * time, 0 for a trailing device that got no rows, *host_wall_seconds (may be NULL) = the host clock from the first dispatch
 * to the last completion, a cross-check that also contains the G launch latencies.  `MM_GPUS=G RunHardware.exe` prints them. */
int mm_gemm_multi_device_timed(int device_count, const mm_config_t *cfg, const void *a_host, const void *b_host,
                               void *c_host, unsigned size_n, unsigned size_k, unsigned size_m, double *elapsed_seconds,
                               double *per_device_seconds, double *host_wall_seconds);
/* The row partition mm_gemm_multi_device uses, for callers that drive one process per GPU themselves (bench.py):
 * slabs of ceil(N / G) rows rounded up to whole tile rows of the kernel that will run on them (mm_kernel_info's tile_n),
 * so only the last busy device owns a ragged tile row; trailing devices may get *rows = 0.  Pure arithmetic: works
 * without a device. */
int mm_row_slab(const mm_config_t *cfg, unsigned size_n, unsigned size_k, unsigned size_m, int device_count, int rank,
                unsigned *row0, unsigned *rows);

/* extern "C" void MatrixMultiplicationKernel(MemoryPackK_t const a[], MemoryPackM_t const b[],
 * MemoryPackM_t c[], unsigned size_n, unsigned size_k, unsigned size_m)
 * (include/MatrixMultiplication.h:155-171, kernel/Top.cpp:6-18; called directly by
 * test/TestSimulation.cpp:66-67).  Host pointers; DataPack arrays are layout-compatible with
 * plain row-major Data_t arrays (include/Utility.h:44-63).  Uses device 0 and the
 * configuration set by mm_set_default_config (initially float, Multiply, Add == the
 * reference's CMake defaults).  Errors are reported on stderr and abort(), because the
 * reference's symbol returns void. */
#ifndef MM_GEMM_NO_KERNEL_SYMBOL /* defined by translation units that declare the reference's typed
                                    or 3-pointer form themselves (host/KernelShim.cpp and its callers) */
void MatrixMultiplicationKernel(const void *a, const void *b, void *c, unsigned size_n,
                                unsigned size_k, unsigned size_m);
#endif
int mm_set_default_config(const mm_config_t *cfg);
/* The same host-pointer call with an explicit configuration and a status instead of abort().
 * This is what the build-time-configured kernel shim (gemm_hls_amd/host/KernelShim.cpp: one
 * library per MM_DATA_TYPE / MM_MAP_OP / MM_REDUCE_OP / MM_TRANSPOSED_A / MM_DYNAMIC_SIZES choice,
 * exporting the reference's exact symbol incl. the 3-pointer static-size form,
 * include/MatrixMultiplication.h:155-171) forwards to. */
int mm_gemm_host(const mm_config_t *cfg, const void *a, const void *b, void *c, unsigned size_n,
                 unsigned size_k, unsigned size_m);

/* ---- introspection ------------------------------------------------------------------------ */
size_t mm_dtype_size(mm_dtype_t dtype);
/* 1 if (dtype, map, reduce) is compiled in, else 0. */
int mm_config_supported(const mm_config_t *cfg);
/* Name of the kernel family that mm_gemm_launch would run for this problem (static string),
 * e.g. "mfma_f32_128x256x32", "valu_tile", "ordered". */
const char *mm_kernel_name(const mm_config_t *cfg, unsigned size_n, unsigned size_k, unsigned size_m);
/* Name of the kernel family mm_gemm_batched_launch would run for `batch` elements of this shape (static string; pure
 * arithmetic, the batched launcher's own resolver). */
const char *mm_kernel_name_batched(const mm_config_t *cfg, unsigned size_n, unsigned size_k, unsigned size_m, unsigned batch);
/* Geometry of the kernel family that would serve this problem: the GPU counterpart of the
 * constants src/PrintSpecifications.cpp prints for the FPGA build (memory tile = the output tile a
 * workgroup keeps resident, compute tile = what one wavefront instruction computes). */
typedef struct {
  unsigned tile_n, tile_m, tile_k;     /* resident C tile (rows x cols) and k-slab per workgroup  */
  unsigned wavefronts;                 /* wavefronts per workgroup                               */
  unsigned inst_n, inst_m, inst_k;     /* shape of one matrix/vector instruction (1x64x1 = VALU) */
  double ops_per_clk_per_cu;           /* peak map+reduce operations per clock per compute unit  */
  unsigned compute_units;              /* 256 on MI355X                                          */
  double max_clock_mhz;                /* 2400 on MI355X                                         */
  double measured_issue_efficiency;    /* fraction of issue slots the family sustains at BASELINE
                                          size (rocprofv3 MfmaUtil, profiles/), 0 if not measured */
} mm_kernel_info_t;
int mm_kernel_info(const mm_config_t *cfg, unsigned size_n, unsigned size_k, unsigned size_m,
                   mm_kernel_info_t *info);
/* Tuning knobs for sweeps ("f32_variant", "f64_variant", "f16_variant", "i8_variant", "valu_variant", "split_variant",
 * "band_rows", "f32_splitk", "ordered_variant", "batch_chunk" = the most elements one batched launch holds, for tests;
 * -1 = the library's own choice) and ONE contract knob, "half_contract"
 * (MM_HALF_CONTRACT = reference | wide; 1 = reference: half (Multiply, Add) under MM_PATH_AUTO is evaluated like the reference's
 * kernel -- binary16 products, binary16 accumulation, k ascending -- on the k-ordered tile kernel; unset / 0: f32 accumulation on
 * the matrix cores).  Kernel ids of this library: f32_variant 33 / 8 / 35 / 64 (the
 * geometries of the shape-adaptive pick) and 0 / 3 (cross-checks); f16_variant 200 / 100 / 11 / 0 / 4 / 5; i8_variant 200 /
 * 100 / 10 / 5 / 0; f64_variant 0-4 (4: the 64 x 64 geometry for small problems); f32_splitk 1 whole tiles, 2-8 K chunks,
 * 0 stream-K as MM_PATH_AUTO runs it: teams of workgroups, every part of a tile that a range boundary cuts goes to a scratch
 * slot and raises a flag, and the LAST part to arrive adds the slots in ascending k into C -- one kernel in which no workgroup
 * ever waits for another one, so it is sound next to anything else on the device (other streams, other processes), on
 * CU-masked streams, on partitions and in graphs; 11 the same with a small fix-up kernel doing the gather (cross-check, the
 * bits of 0); 12 the same again with the hand-over written as the canonical last-block pattern -- a release fence, ONE agent-scope acq_rel
 * read-modify-write per part on a per-tile counter, the last ticket gathers: correct by the language's memory model alone, the bits of 0,
 * 0.2-30 % slower (its release fence writes the L2 back; profiles/r06d_*), kept as the cross-check of the shipped flag protocol; 9 stream-K in
 * single ranges with its own fix-up kernel (cross-check, its own bits).
 * "closure_block": the block size of mm_closure_* (see there).  "lse_variant": the kernels of mm_gemm_logsumexp_* (see there).
 * "bits_variant": the kernels of mm_bits_gemm_* (see there).  "bits_count_variant": the kernels of mm_bits_count_* (see there).
 * "bits_gf2_variant": the kernels of mm_bits_gf2_* (see there).
 * "debug_poison" = 1 fills the scratch that kernels hand partial tiles through, and C itself (pure output), with NaN before
 * every stream-K launch: a read of anything the launch did not write, or a tile nobody finished, then shows in C (tests only).  "md_virtual_devices": see mm_gemm_multi_device.  Any
 * other id is refused: the retired schedules and the work-skipping ablations of the measurement history exist only in the
 * lab build (tools/lab/libmm_gemm_amd_lab.so, built on request, where "ablations" = 1 unlocks the latter).  Each knob is
 * initialised ONCE from its environment variable (MM_F32_VARIANT, ...) and changed only through this call afterwards; the
 * launch path never reads the environment.  The reference's counterpart is the build-time tile knob
 * (CMakeLists.txt:18-20), which the host binaries honour through -DMM_MEMORY_TILE_SIZE_N / _M (host/HostConfig.h:
 * ApplyBuildTimeTile). */
int mm_tuning_set(const char *name, int value);
int mm_tuning_get(const char *name, int *value);
/* Message of the last failing call on this thread (static or thread-local storage). */
const char *mm_last_error(void);

#ifdef __cplusplus
}
#endif
#include "mm_bits_gf2.h"
#endif /* MM_GEMM_H */
