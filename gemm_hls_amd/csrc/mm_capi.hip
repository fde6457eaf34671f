// C ABI of libmm_gemm_amd.so (declared in include/mm_gemm.h): device management, dispatch to
// the gfx950 kernel families, the timed blocking launch that replaces hlslib's
// Kernel::ExecuteTask() (host/RunHardware.cpp:161-162), the N-split multi-device driver and the
// reference's own entry point MatrixMultiplicationKernel (kernel/Top.cpp:6-18).
// There is no CPU compute path in this file or anywhere in this library.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <random>
#include <unordered_map>
#include <vector>

#include "mm_common.h"

namespace {

thread_local char g_error[512] = "";

int fail(int code, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_error, sizeof(g_error), fmt, ap);
  va_end(ap);
  return code;
}

int hip_fail(hipError_t e, const char *what) {
  return fail(e == hipErrorNoDevice || e == hipErrorInvalidDevice ? MM_ERR_NO_DEVICE : MM_ERR_HIP,
              "%s: %s (%d)", what, hipGetErrorString(e), (int)e);
}

#define MM_HIP(call)                                   \
  do {                                                 \
    hipError_t e_ = (call);                            \
    if (e_ != hipSuccess) return hip_fail(e_, #call);  \
  } while (0)

// ---- process-wide state: initialised exactly once, read-only afterwards (safe for concurrent
// calls from any number of host threads; g_error above is per thread) -------------------------
std::once_flag g_init_once;
int g_device_count = 0;
int g_device_cus[64] = {};   // compute units each device reports (MI355X in SPX mode: 256; a CPX partition: 32)
int g_init_status = MM_ERR_NO_DEVICE;
char g_init_error[512] = "";

void init_once() {
  auto init_fail = [](const char *fmt, auto... args) {
    snprintf(g_init_error, sizeof(g_init_error), fmt, args...);
    g_device_count = 0;
    g_init_status = MM_ERR_NO_DEVICE;
  };
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0)
    return init_fail("hipGetDeviceCount: %s; this library needs an MI355X (gfx950), there is no CPU fallback",
                     e == hipSuccess ? "0 devices" : hipGetErrorString(e));
  // device indices are HIP's, so every visible device must be usable (mask others out with
  // HIP_VISIBLE_DEVICES); a mixed box is reported, not half-used.
  for (int d = 0; d < n; ++d) {
    hipDeviceProp_t prop;
    e = hipGetDeviceProperties(&prop, d);
    if (e != hipSuccess) return init_fail("hipGetDeviceProperties(%d): %s", d, hipGetErrorString(e));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
      return init_fail("device %d is %s; the kernels in this library are built for gfx950 only "
                       "(hide other devices with HIP_VISIBLE_DEVICES)", d, prop.gcnArchName);
    if (d < 64) g_device_cus[d] = prop.multiProcessorCount;
  }
  g_device_count = n;
  g_init_status = MM_OK;
}

int ensure_init() {
  std::call_once(g_init_once, init_once);
  return g_init_status == MM_OK ? MM_OK : fail(g_init_status, "%s", g_init_error);
}

std::mutex g_default_cfg_mutex;
mm_config_t g_default_cfg = {MM_DTYPE_F32, MM_OP_MULTIPLY, MM_OP_ADD, MM_PATH_AUTO, MM_A_ROW_MAJOR};
mm_config_t default_cfg() {
  std::lock_guard<std::mutex> lock(g_default_cfg_mutex);
  return g_default_cfg;
}

// ---- tuning knobs: environment read once, then only mm_tuning_set() changes them --------------
std::once_flag g_tuning_once;
std::atomic<int> g_tuning[mm::TUNE_COUNT];
const char *const kTuneName[mm::TUNE_COUNT] = {"f32_variant", "f64_variant", "f16_variant", "i8_variant", "band_rows",
                                               "valu_variant", "split_variant", "f32_splitk", "ablations", "debug_poison", "kxn_prepass_min_m",
                                               "md_virtual_devices", "ordered_variant", "half_contract", "batch_chunk",
                                               "closure_block", "lse_variant", "bits_variant", "bits_count_variant", "bits_gf2_variant"};
const char *const kTuneEnv[mm::TUNE_COUNT] = {"MM_F32_VARIANT", "MM_F64_VARIANT", "MM_F16_VARIANT", "MM_I8_VARIANT",
                                              "MM_BAND_ROWS", "MM_VALU_VARIANT", "MM_SPLIT_VARIANT", "MM_F32_SPLITK", "MM_ABLATIONS", "MM_DEBUG_POISON", "MM_KXN_PREPASS_MIN_M",
                                              "MM_MD_VIRTUAL_DEVICES", "MM_ORDERED_VARIANT", "MM_HALF_CONTRACT", "MM_BATCH_CHUNK",
                                              "MM_CLOSURE_BLOCK", "MM_LSE_VARIANT", "MM_BITS_VARIANT", "MM_BITS_COUNT_VARIANT",
                                              "MM_BITS_GF2_VARIANT"};
void tuning_init() {
  for (int i = 0; i < mm::TUNE_COUNT; ++i) {
    const char *e = getenv(kTuneEnv[i]);
    int v = (e && *e) ? atoi(e) : -1;
    if (i == mm::TUNE_HALF_CONTRACT && e && *e) {   // the one knob with words for values: MM_HALF_CONTRACT=reference | wide
      if (strcmp(e, "reference") == 0) v = 1;
      else if (strcmp(e, "wide") == 0) v = 0;
    }
    g_tuning[i].store(v, std::memory_order_relaxed);
  }
}

int check_device(int device) {
  int rc = ensure_init();
  if (rc) return rc;
  if (device < 0 || device >= g_device_count)
    return fail(MM_ERR_BAD_ARGUMENT, "device %d out of range [0, %d)", device, g_device_count);
  return MM_OK;
}

bool valid_cfg(const mm_config_t *cfg) {
  return cfg && cfg->dtype >= MM_DTYPE_F32 && cfg->dtype <= MM_DTYPE_U64 && cfg->map_op >= MM_OP_ADD &&
         cfg->map_op <= MM_OP_MAX && cfg->reduce_op >= MM_OP_ADD && cfg->reduce_op <= MM_OP_MAX &&
         (cfg->path == MM_PATH_AUTO || cfg->path == MM_PATH_ORDERED || cfg->path == MM_PATH_SPLIT) &&
         (cfg->layout_a == MM_A_ROW_MAJOR || cfg->layout_a == MM_A_TRANSPOSED);
}

// fp32 geometry: 256x256x16, 8 wavefronts, accumulators flushed into C every 4096 k (146 TF at
// 16384^3, max rel err 2.7e-6 over the full matrix: profiles/r01_f32_precision_full_matrix.txt).
// The f32_variant knob selects another one for sweeps (tools/sweep.py); -1 = shape-adaptive choice
// among the flush-capable geometries (mm_mfma_f32.hip).
int f32_variant() { return mm::tuning(mm::TUNE_F32_VARIANT); }
int f32_variant_for(const mm::Problem &p) { return mm::mfma_f32_resolve(p, f32_variant()); }  // what the launcher runs; -1: none

enum Family { FAM_ORDERED, FAM_ORDERED_TILE, FAM_VALU_TILE, FAM_MFMA_F32, FAM_MFMA_F64, FAM_MFMA_F16, FAM_MFMA_I8, FAM_HALF_WIDE,
              FAM_F32_SPLIT, FAM_NONE };

// The family is a property of the JOB: a row slab of a bigger job (Problem::n_total) runs the family the whole job would
// run, so that a split never changes which arithmetic a row gets.  (Row-major slabs qualify for whatever the job
// qualifies for -- the families only ask n >= 1; a K x N A asks for N % 4 / 2 / 8 / 16 == 0, which tile-aligned slabs of
// an N that has it keep, the last one included.)
Family choose(const mm_config_t &cfg, const mm::Problem &slab) {
  mm::Problem p = slab;
  if (slab.n_total) { p.n = slab.n_total; p.n_total = 0; }
  const bool mul_add = cfg.map_op == MM_OP_MULTIPLY && cfg.reduce_op == MM_OP_ADD;
  // The k-ordered contract (Naive's: include/Utility.h:18-42) has two kernels with the same bits: the register-tiled one
  // wherever it serves, the fully predicated 64 x 64 one for everything else (and always under ordered_variant = 0).
  // half (Multiply, Add) under AUTO joins it when the process asked for the REFERENCE's half arithmetic (half_contract = 1:
  // binary16 accumulating in binary16, kernel/Compute.cpp:129-133 -- what its hosts compare with exactly).
  const bool reference_half = cfg.path == MM_PATH_AUTO && mul_add && cfg.dtype == MM_DTYPE_F16 && mm::tuning(mm::TUNE_HALF_CONTRACT) == 1;
  if (cfg.path == MM_PATH_ORDERED || reference_half)
    return mm::tuning(mm::TUNE_ORDERED_VARIANT) != 0 && mm::valu_tile_serves(cfg, p) ? FAM_ORDERED_TILE : FAM_ORDERED;
  if (cfg.path == MM_PATH_SPLIT)  // an explicit request is never re-routed: fp32 (x,+) or nothing
    return mul_add && cfg.dtype == MM_DTYPE_F32 && mm::mfma_f32_split_serves(p) ? FAM_F32_SPLIT : FAM_NONE;
  if (mul_add && cfg.dtype == MM_DTYPE_F32 && mm::mfma_f32_serves(p)) return FAM_MFMA_F32;
  if (mul_add && cfg.dtype == MM_DTYPE_F64 && mm::mfma_f64_serves(p)) return FAM_MFMA_F64;
  // half (x,+) keeps ONE numerical contract under AUTO (exact products, f32 accumulation, one
  // rounding): shapes the matrix-core kernel does not take run the wide-accumulate plain kernel,
  // never the half-accumulating ones (which would overflow to inf beyond K ~ 2000 on [1,10) data)
  if (mul_add && cfg.dtype == MM_DTYPE_F16) return mm::mfma_f16_serves(p) ? FAM_MFMA_F16 : FAM_HALF_WIDE;
  if (mul_add && (cfg.dtype == MM_DTYPE_I8 || cfg.dtype == MM_DTYPE_U8) && mm::mfma_i8_serves(p)) return FAM_MFMA_I8;
  return mm::valu_tile_serves(cfg, p) ? FAM_VALU_TILE : FAM_ORDERED;
}

// The fast families move 16 bytes per lane (global_load_lds_dwordx4, 16-B vector stores): their
// operands must be 16-B aligned, which every allocator gives (hipMalloc 256 B; the reference's
// host vectors are 4096-B aligned, include/Utility.h:48).  An offset view is refused loudly; the
// ordered path takes any element-aligned pointer.
bool aligned16(const mm::Problem &p) {
  return (((uintptr_t)p.a | (uintptr_t)p.b | (uintptr_t)p.c) & 15u) == 0;
}

// A launcher's status as this library's: kErrNotSupported (the configuration's kernel is not compiled in) is
// MM_ERR_UNSUPPORTED, any other non-zero value the HIP error of `what`.  `family` ("", "argreduce ", ...) and, when
// non-zero, `block` name the kernel in the message.
int launch_status(int e, const mm_config_t &cfg, const char *family, const char *what, unsigned block = 0) {
  if (e == mm::kErrNotSupported) {
    char b[32] = "";
    if (block) snprintf(b, sizeof(b), ", block %u", block);
    return fail(MM_ERR_UNSUPPORTED, "%sconfiguration (dtype %d, map %d, reduce %d%s) is not compiled into this library", family,
                (int)cfg.dtype, (int)cfg.map_op, (int)cfg.reduce_op, b);
  }
  return e ? hip_fail((hipError_t)e, what) : MM_OK;
}

int dispatch(hipStream_t s, const mm_config_t &cfg, const mm::Problem &p) {
  if (p.n == 0 || p.m == 0) return MM_OK;  // nothing to write
  Family fam = choose(cfg, p);
  if (fam == FAM_NONE)
    return fail(MM_ERR_UNSUPPORTED, "MM_PATH_SPLIT serves float (Multiply, Add) only (got dtype %d, map %d, reduce %d)",
                (int)cfg.dtype, (int)cfg.map_op, (int)cfg.reduce_op);
  if (fam == FAM_ORDERED_TILE && !aligned16(p)) fam = FAM_ORDERED;   // the k-ordered contract takes any element-aligned pointer
  if (fam != FAM_ORDERED && fam != FAM_HALF_WIDE && fam != FAM_F32_SPLIT && !aligned16(p))
    return fail(MM_ERR_BAD_ARGUMENT, "a, b and c must be 16-byte aligned for the fast path (got %p, %p, %p); "
                "use an aligned allocation or MM_PATH_ORDERED", p.a, p.b, p.c);
  // the launchers report hipGetLastError() after their launch: a stale (sticky-until-read) error of the application's own
  // earlier HIP calls on this thread must not be reported as this launch's
  (void)hipGetLastError();
  int e;
  switch (fam) {
    case FAM_MFMA_F32: e = mm::launch_mfma_f32(s, p, f32_variant()); break;
    case FAM_MFMA_F64: e = mm::launch_mfma_f64(s, p); break;
    case FAM_MFMA_F16: e = mm::launch_mfma_f16(s, p); break;
    case FAM_MFMA_I8: e = mm::launch_mfma_i8(s, p); break;
    case FAM_HALF_WIDE: e = mm::launch_half_wide(s, p); break;
    case FAM_F32_SPLIT: e = mm::launch_mfma_f32_split(s, p, mm::tuning(mm::TUNE_SPLIT_VARIANT)); break;
    case FAM_VALU_TILE:
      e = mm::launch_valu_tile(s, cfg, p);
      if (e == mm::kErrNotSupported) e = mm::launch_ordered(s, cfg, p);  // still the GPU
      break;
    case FAM_ORDERED_TILE:
      e = mm::launch_valu_tile_exact(s, cfg, p);
      if (e == mm::kErrNotSupported) e = mm::launch_ordered(s, cfg, p);  // the same bits
      break;
    default: e = mm::launch_ordered(s, cfg, p); break;
  }
  return launch_status(e, cfg, "", "kernel launch");
}

int check_problem(const mm_config_t *cfg, const void *a, const void *b, void *c, unsigned n, unsigned k, unsigned m) {
  if (!valid_cfg(cfg)) return fail(MM_ERR_BAD_ARGUMENT, "invalid mm_config_t");
  if (k == 0) return fail(MM_ERR_BAD_ARGUMENT, "size_k must be positive");
  if (n && m && (!a || !b || !c)) return fail(MM_ERR_BAD_ARGUMENT, "null matrix pointer");
  return MM_OK;
}

// ---- one row per matrix-core family: its batched kernels' resolver (once per call, on the whole batch; -1: none serves), launcher
// (a chunk of the batch on the resolved kernel) and name.  mm_gemm_batched_*, the A x B^T pre-pass, the logsumexp hybrid's product
// and mm_kernel_name_batched all go through it: a new family is a new row.  The fp32 row binds the f32_variant knob.
struct MatrixCore {
  int (*resolve)(const mm::Problem &whole);
  int (*launch)(hipStream_t s, const mm::Problem &chunk, int kernel);
  const char *(*name)(const mm::Problem &whole);
};
int f32_batched_resolve(const mm::Problem &p) { return mm::mfma_f32_batched_resolve(p, f32_variant()); }
const char *f32_batched_name(const mm::Problem &p) {
  const int v = f32_batched_resolve(p);
  return v < 0 ? "unsupported" : mm::mfma_f32_name(v);
}
const MatrixCore kMatrixCore[] = {   // by Family, from FAM_MFMA_F32 on
    {f32_batched_resolve, mm::launch_mfma_f32_batched, f32_batched_name},
    {mm::mfma_f64_batched_resolve, mm::launch_mfma_f64_batched, mm::mfma_f64_batched_name},
    {mm::mfma_f16_batched_resolve, mm::launch_mfma_f16_batched, mm::mfma_f16_batched_name},
    {mm::mfma_i8_batched_resolve, mm::launch_mfma_i8_batched, mm::mfma_i8_batched_name},
};
static_assert(FAM_MFMA_F64 == FAM_MFMA_F32 + 1 && FAM_MFMA_F16 == FAM_MFMA_F32 + 2 && FAM_MFMA_I8 == FAM_MFMA_F32 + 3, "kMatrixCore's order");
const MatrixCore *matrix_core(Family f) {   // null: not a matrix-core family
  return f >= FAM_MFMA_F32 && f <= FAM_MFMA_I8 ? &kMatrixCore[f - FAM_MFMA_F32] : nullptr;
}

// ---- strided batches (mm_gemm_batched_*) -----------------------------------------------------------------------------
// The family a batched launch runs: the single launch's, each matrix-core family through its batched resolver (decided on
// the whole batch), except where that family would need workspace (split-K planes, stream-K scratch, a K x N transposition
// pre-pass): those shapes go to the family with the same contract -- fp32 (Multiply, Add) to its whole-tile geometries
// (K x N A: the direct K x N kernel), half (Multiply, Add) to half_wide (f32 accumulation, one rounding: mfma_f16's
// contract), the 8-bit products to the register-tiled VALU kernel (exact).  Pure arithmetic: no device is touched.
Family choose_batched(const mm_config_t &cfg, const mm::Problem &p) {
  const Family f = choose(cfg, p);
  if (f == FAM_F32_SPLIT) return FAM_NONE;   // MM_PATH_SPLIT needs workspace: not batched
  const MatrixCore *mc = matrix_core(f);
  if (!mc || mc->resolve(p) >= 0) return f;   // (a library built without the batched fp32 kernels -- tools/lab -- resolves none)
  if (f == FAM_MFMA_F16) return FAM_HALF_WIDE;
  return mm::valu_tile_serves(cfg, p) ? FAM_VALU_TILE : FAM_ORDERED;
}

// Every element meets the single launch's alignment rule: the fast families need each element's a, b and c 16-byte aligned.
bool batch_aligned16(const mm::Problem &p, size_t es) {
  const size_t strides = p.batch > 1 ? ((p.stride_a | p.stride_b | p.stride_c) * es) : 0;
  return aligned16(p) && (strides & 15u) == 0;
}

// ---- the rules every batched call shares --------------------------------------------------------------------------------
bool empty_batch(const mm::Problem &p) { return p.batch == 0 || p.n == 0 || p.m == 0; }   // nothing to write

int check_stride_c(const mm::Problem &p) {
  if (p.batch > 1 && p.stride_c < (size_t)p.n * p.m)
    return fail(MM_ERR_BAD_ARGUMENT, "stride_c %zu < N * M = %zu: the outputs of the batch would overlap", p.stride_c,
                (size_t)p.n * p.m);
  return MM_OK;
}

// Bytes an operand of the batch can touch: [base, base + ((batch - 1) * stride + extent) * es), extent = its elements.
size_t batch_span(size_t extent, size_t stride, unsigned batch, size_t es) {
  return extent ? ((size_t)(batch - 1) * stride + extent) * es : 0;
}
bool spans_overlap(const void *x, size_t xbytes, const void *y, size_t ybytes) {
  const uintptr_t x0 = (uintptr_t)x, y0 = (uintptr_t)y;
  return xbytes && ybytes && x0 < y0 + ybytes && y0 < x0 + xbytes;
}

// Whether C overlaps A or B, or (given) the int32 index I, laid out as C, overlaps A, B or C -- over the bytes the whole
// batch can touch.  A conservative test: the kernels read A and B while other workgroups already write C and I.
// c_es: C's element size where it is not the operands' (mm_gemm_widen_*).
bool outputs_overlap(const mm::Problem &p, size_t es, const int *index = nullptr, size_t c_es = 0) {
  const size_t nm = (size_t)p.n * p.m;
  const size_t a_bytes = batch_span((size_t)p.n * p.k, p.stride_a, p.batch, es);
  const size_t b_bytes = batch_span((size_t)p.k * p.m, p.stride_b, p.batch, es);
  const size_t c_bytes = batch_span(nm, p.stride_c, p.batch, c_es ? c_es : es), i_bytes = batch_span(nm, p.stride_c, p.batch, sizeof(int));
  return spans_overlap(p.c, c_bytes, p.a, a_bytes) || spans_overlap(p.c, c_bytes, p.b, b_bytes) ||
         (index && (spans_overlap(index, i_bytes, p.a, a_bytes) || spans_overlap(index, i_bytes, p.b, b_bytes) ||
                    spans_overlap(index, i_bytes, p.c, c_bytes)));
}

// What the checks of the products that may be seeded (p.seed: mm_gemm_logsumexp_*, mm_gemm_widen_*, mm_gemm_nt_*) end in, after
// the call's own rules -- the configurations it serves, its knob.  A refusal's status; else *go: whether there is anything to
// launch -- not for an empty batch, nor when accumulating over K = 0, where C keeps its value.  es, c_es: A and B's and C's
// element sizes.  (mm_gemm_argreduce_* has this order too, but index checks in between and A, B and the index required at K = 0.)
int check_seeded(const mm::Problem &p, size_t es, size_t c_es, bool *go) {
  *go = false;
  if (p.k == 0 && !p.seed) return fail(MM_ERR_BAD_ARGUMENT, "size_k must be positive");
  if (empty_batch(p)) return MM_OK;
  if (!p.c || (p.k && (!p.a || !p.b))) return fail(MM_ERR_BAD_ARGUMENT, "null matrix pointer");   // (K = 0: A, B unread)
  if (int rc = check_stride_c(p)) return rc;
  if (outputs_overlap(p, es, nullptr, c_es))   // (B's extent is K * M in either layout)
    return fail(MM_ERR_BAD_ARGUMENT, "c overlaps a or b (bases %p, %p, %p)", p.a, p.b, p.c);
  *go = p.k > 0;
  return MM_OK;
}

// Elements [e0, e0 + count) of the batch.
mm::Problem batch_slice(const mm::Problem &p, unsigned e0, unsigned count, size_t es) {
  mm::Problem q = p;
  q.batch = count;
  q.a = (const char *)p.a + (size_t)e0 * p.stride_a * es;
  q.b = (const char *)p.b + (size_t)e0 * p.stride_b * es;
  q.c = (char *)p.c + (size_t)e0 * p.stride_c * es;
  return q;
}

// fn(slice, e0) over consecutive slices of at most `chunk` elements; stops at the first non-zero status.
template <class F> int for_each_chunk(const mm::Problem &p, size_t es, unsigned chunk, F &&fn) {
  for (unsigned e0 = 0; e0 < p.batch; e0 += chunk)
    if (int rc = fn(batch_slice(p, e0, std::min(chunk, p.batch - e0), es), e0)) return rc;
  return MM_OK;
}

// Stream-ordered workspace of one call, from the current device's library pool: allocated on the call's stream and freed on it
// with hipFreeAsync, so the host never waits.  A dispatcher allocates, enqueues its work keeping its status, and returns
// release(status); an exit without release() frees in the destructor.
struct Workspace {
  hipStream_t s;
  const char *free_failed;   // the caller's words for a failed release: "hipFreeAsync (closure workspace)"
  void *p = nullptr;
  ~Workspace() { if (p) (void)hipFreeAsync(p, s); }
  char *bytes() const { return (char *)p; }

  // `size` bytes; *e: the allocation's own status.  Non-zero: the device's pool could not be had.
  int from_pool(size_t size, hipError_t *e) {
    *e = hipSuccess;
    int dev = 0;
    MM_HIP(hipGetDevice(&dev));
    hipMemPool_t pool = nullptr;
    if (int rc = mm::workspace_pool(dev, &pool)) return hip_fail((hipError_t)rc, "workspace pool");
    if ((*e = hipMallocFromPoolAsync(&p, size, pool, s)) != hipSuccess) p = nullptr;
    return MM_OK;
  }
  // A failed allocation fails the call, under the caller's words for it
  int allocate(size_t size, const char *failed) {
    hipError_t e;
    const int rc = from_pool(size, &e);
    return rc == MM_OK && e != hipSuccess ? hip_fail(e, failed) : rc;
  }
  // A failed allocation is reported in *full, the sticky error cleared: for a caller with a kernel that needs no workspace
  int try_allocate(size_t size, bool *full) {
    hipError_t e;
    const int rc = from_pool(size, &e);
    if ((*full = e != hipSuccess)) (void)hipGetLastError();
    return rc;
  }

  // `rc`, the status of the work enqueued since allocate(), or -- when that is MM_OK -- a failed free's
  int release(int rc) {
    const hipError_t f = hipFreeAsync(p, s);
    p = nullptr;
    return rc == MM_OK && f != hipSuccess ? hip_fail(f, free_failed) : rc;
  }
};

// All argument checks of a batched call, before any device is touched.  *fam: the family that will run (FAM_NONE: an empty
// batch, a no-op).
int check_batched(const mm_config_t *cfg, const mm::Problem &p, Family *fam) {
  if (!valid_cfg(cfg)) return fail(MM_ERR_BAD_ARGUMENT, "invalid mm_config_t");
  if (p.k == 0) return fail(MM_ERR_BAD_ARGUMENT, "size_k must be positive");
  if (cfg->path == MM_PATH_SPLIT) return fail(MM_ERR_UNSUPPORTED, "MM_PATH_SPLIT has no batched form (it needs workspace)");
  *fam = FAM_NONE;
  if (empty_batch(p)) return MM_OK;
  if (!p.a || !p.b || !p.c) return fail(MM_ERR_BAD_ARGUMENT, "null matrix pointer");
  if (int rc = check_stride_c(p)) return rc;
  Family f = choose_batched(*cfg, p);
  if (f == FAM_NONE) return fail(MM_ERR_UNSUPPORTED, "no batched kernel serves this configuration");
  const bool aligned = batch_aligned16(p, mm_dtype_size(cfg->dtype));
  if (f == FAM_ORDERED_TILE && !aligned) f = FAM_ORDERED;   // the k-ordered contract takes any element-aligned pointer
  if (f != FAM_ORDERED && f != FAM_HALF_WIDE && !aligned)
    return fail(MM_ERR_BAD_ARGUMENT, "every element's a, b and c must be 16-byte aligned for the fast path (bases %p, %p, %p; "
                "strides %zu, %zu, %zu elements); use aligned strides or MM_PATH_ORDERED", p.a, p.b, p.c, p.stride_a,
                p.stride_b, p.stride_c);
  *fam = f;
  return MM_OK;
}

// Elements per launch of a batch whose elements take `tiles` workgroups each: the batch_chunk knob, and a grid of at most
// 2^22 workgroups (of at most 512 threads).  An element bigger than that runs alone, as a single launch would.
unsigned chunk_of_tiles(unsigned long long tiles, unsigned batch) {
  unsigned long long chunk = std::max(1ull, (1ull << 22) / tiles);
  const int knob = mm::tuning(mm::TUNE_BATCH_CHUNK);
  if (knob > 0) chunk = std::min<unsigned long long>(chunk, (unsigned)knob);
  return (unsigned)std::min<unsigned long long>(chunk, batch);
}

// ... of a product, counted in 64 x 64 tiles of C, the smallest any family uses
unsigned batch_chunk(const mm::Problem &p) {
  return chunk_of_tiles((unsigned long long)((p.n + 63) / 64) * ((p.m + 63) / 64), p.batch);
}

// Launches the batch as consecutive launches of at most batch_chunk() elements on `s`.  The family and the fp32 geometry
// are decided once, on the whole batch, so that an element's kernel does not depend on how the batch was chunked.
int dispatch_batched(hipStream_t s, const mm_config_t &cfg, const mm::Problem &p, Family fam) {
  if (empty_batch(p)) return MM_OK;
  const MatrixCore *mc = matrix_core(fam);
  const int kernel = mc ? mc->resolve(p) : -1;
  (void)hipGetLastError();   // a stale error of the application's own calls must not be reported as this launch's
  return for_each_chunk(p, mm_dtype_size(cfg.dtype), batch_chunk(p), [&](const mm::Problem &q, unsigned) {
    if (mc) return launch_status(mc->launch(s, q, kernel), cfg, "", "batched kernel launch");
    int e;
    switch (fam) {
      case FAM_HALF_WIDE: e = mm::launch_half_wide_batched(s, q); break;
      case FAM_VALU_TILE:
        e = mm::launch_valu_tile_batched(s, cfg, q);
        if (e == mm::kErrNotSupported) e = mm::launch_ordered_batched(s, cfg, q);
        break;
      case FAM_ORDERED_TILE:
        e = mm::launch_valu_tile_exact_batched(s, cfg, q);
        if (e == mm::kErrNotSupported) e = mm::launch_ordered_batched(s, cfg, q);
        break;
      default: e = mm::launch_ordered_batched(s, cfg, q); break;
    }
    return launch_status(e, cfg, "", "batched kernel launch");
  });
}

mm::Problem batched_problem(const mm_config_t *cfg, const void *a, const void *b, void *c, unsigned n, unsigned k,
                            unsigned m, unsigned batch, size_t stride_a, size_t stride_b, size_t stride_c, bool seed = false) {
  mm::Problem p{a, b, c, n, k, m, cfg && cfg->layout_a == MM_A_TRANSPOSED};
  p.batch = batch;
  p.stride_a = stride_a;
  p.stride_b = stride_b;
  p.stride_c = stride_c;
  p.seed = seed;
  return p;
}

// ---- accumulate (mm_gemm_*accumulate_*): C <- C (+) (A (x) B) -------------------------------------------------------
// The batched call's checks (check_batched), K = 0 accepted, and C refused where it overlaps A or B.  *fam = FAM_NONE:
// nothing to launch (an empty batch, or K = 0: C keeps its value).
int check_accumulate(const mm_config_t *cfg, const mm::Problem &p, Family *fam) {
  *fam = FAM_NONE;
  if (!valid_cfg(cfg)) return fail(MM_ERR_BAD_ARGUMENT, "invalid mm_config_t");
  if (p.k > 0) {
    int rc = check_batched(cfg, p, fam);
    if (rc || *fam == FAM_NONE) return rc;
  } else {   // K = 0: the same checks on a problem that has no k, then nothing to do
    mm::Problem q = p;
    q.k = 1;
    Family f;
    if (int rc = check_batched(cfg, q, &f)) return rc;
    if (f == FAM_NONE) return MM_OK;
  }
  if (outputs_overlap(p, mm_dtype_size(cfg->dtype))) {
    *fam = FAM_NONE;
    return fail(MM_ERR_BAD_ARGUMENT, "c overlaps a or b (bases %p, %p, %p): an accumulating call updates C in place and reads "
                "A and B meanwhile; pass a copy", p.a, p.b, p.c);
  }
  return MM_OK;
}

// The A x B^T forms (p.b_transposed: mm_gemm_nt_*, mm_gemm_argreduce_nt_*, mm_gemm_logsumexp_nt_*) serve a row-major A only
bool bt_refused(const mm_config_t &cfg, const mm::Problem &p) { return p.b_transposed && cfg.layout_a == MM_A_TRANSPOSED; }
int fail_bt(const mm_config_t &cfg) {
  return fail(MM_ERR_UNSUPPORTED, "the A x B^T calls serve a row-major A (got layout_a %d): A^T B^T is not served", (int)cfg.layout_a);
}

// ---- argreduce (mm_gemm_argreduce_*, mm_gemm_argreduce_nt_*): Min / Max with the winning k ---------------------------
enum ArKernel { AR_NONE, AR_PLAIN, AR_TILE };

// The kernel by configuration and shape alone (mm_kernel_name_argreduce, mm_kernel_name_argreduce_nt); alignment may still
// demote AR_TILE at launch.  An M x K B asks what a K x M B asks: K % 4 == 0 for the 4-wide loads of A and Bt, M % 4 == 0
// for the 4-wide stores of C and I.
ArKernel argreduce_kernel_for(const mm_config_t &cfg, const mm::Problem &p) {
  if (bt_refused(cfg, p)) return AR_NONE;
  if (cfg.reduce_op != MM_OP_MIN && cfg.reduce_op != MM_OP_MAX) return AR_NONE;
  if (cfg.path == MM_PATH_SPLIT) return AR_NONE;
  if (cfg.path == MM_PATH_ORDERED) return AR_PLAIN;
  // the tile holds 8 x 8 values per thread: instantiated for elements of at most 4 bytes (mm_argreduce.inc)
  return mm::valu_tile_serves(cfg, p) && mm_dtype_size(cfg.dtype) <= 4 ? AR_TILE : AR_PLAIN;
}

// All argument checks of an argreduce call, before any device is touched.  *ker = AR_NONE: nothing to launch (an empty
// batch, or K = 0 when accumulating).
int check_argreduce(const mm_config_t *cfg, const mm::Problem &p, const int *index, int index_base, ArKernel *ker) {
  *ker = AR_NONE;
  if (!valid_cfg(cfg)) return fail(MM_ERR_BAD_ARGUMENT, "invalid mm_config_t");
  if (bt_refused(*cfg, p)) return fail_bt(*cfg);
  if (cfg->reduce_op != MM_OP_MIN && cfg->reduce_op != MM_OP_MAX)
    return fail(MM_ERR_UNSUPPORTED, "argreduce needs a Min or Max reduction (got reduce %d)", (int)cfg->reduce_op);
  if (cfg->path == MM_PATH_SPLIT) return fail(MM_ERR_UNSUPPORTED, "MM_PATH_SPLIT has no argreduce form");
  if (p.k == 0 && !p.seed) return fail(MM_ERR_BAD_ARGUMENT, "size_k must be positive");
  if (index_base < 0) return fail(MM_ERR_BAD_ARGUMENT, "index_base %d is negative", index_base);
  if (p.k > 0 && (long long)index_base + p.k - 1 > (long long)INT32_MAX)
    return fail(MM_ERR_BAD_ARGUMENT, "index_base %d + K - 1 (K = %u) does not fit an int32 index", index_base, p.k);
  if (empty_batch(p)) return MM_OK;
  if (!p.a || !p.b || !p.c || !index) return fail(MM_ERR_BAD_ARGUMENT, "null matrix or index pointer");
  if (int rc = check_stride_c(p)) return rc;
  const size_t es = mm_dtype_size(cfg->dtype);
  if (outputs_overlap(p, es, index))
    return fail(MM_ERR_BAD_ARGUMENT, "c or c_index overlaps a, b or each other (bases %p, %p, %p, %p)", p.a, p.b, p.c,
                (const void *)index);
  if (p.k == 0) return MM_OK;   // accumulating over no k: C and I keep their values
  *ker = argreduce_kernel_for(*cfg, p);
  // the tile kernel moves 16 bytes per lane: every element's a, b, c and index 16-byte aligned, else the predicated kernel
  if (*ker == AR_TILE && (!batch_aligned16(p, es) || ((uintptr_t)index & 15u) != 0 ||
                          (p.batch > 1 && (p.stride_c * sizeof(int)) % 16 != 0)))
    *ker = AR_PLAIN;
  return MM_OK;
}

// Launches the batch as consecutive launches of at most batch_chunk() elements on `s`, C and I advancing together.
int dispatch_argreduce(hipStream_t s, const mm_config_t &cfg, const mm::Problem &p, int *index, int index_base,
                       ArKernel ker) {
  (void)hipGetLastError();   // a stale error of the application's own calls must not be reported as this launch's
  return for_each_chunk(p, mm_dtype_size(cfg.dtype), batch_chunk(p), [&](const mm::Problem &q, unsigned e0) {
    return launch_status(mm::launch_argreduce(s, cfg, q, index + (size_t)e0 * p.stride_c, index_base, ker == AR_TILE), cfg,
                         "argreduce ", "argreduce kernel launch");
  });
}

// ---- closure (mm_closure_*): blocked Floyd-Warshall in place -------------------------------------------------------
// Block size B: the closure_block knob -- 64, 128, or 256 for the value-only form of elements of at most 4 bytes (the
// kernels' register sub-blocks, mm_closure.inc) -- else 256 for that form and 128 for the others.  0: the knob holds a value
// this form does not take.
unsigned closure_block(const mm_config_t &cfg, bool witness) {
  const bool big = !witness && mm_dtype_size(cfg.dtype) <= 4;
  const int knob = mm::tuning(mm::TUNE_CLOSURE_BLOCK);
  if (knob == -1) return big ? 256 : 128;
  return (knob == 64 || knob == 128 || (knob == 256 && big)) ? (unsigned)knob : 0;
}

// All argument checks of a closure call, before any device is touched.  *block = 0: nothing to do (n or batch 0).
int check_closure(const mm_config_t *cfg, const void *d, const int *w, unsigned n, unsigned batch, size_t stride_d,
                  unsigned *block) {
  *block = 0;
  if (!valid_cfg(cfg)) return fail(MM_ERR_BAD_ARGUMENT, "invalid mm_config_t");
  if (cfg->reduce_op != MM_OP_MIN && cfg->reduce_op != MM_OP_MAX)
    return fail(MM_ERR_UNSUPPORTED, "a closure needs an idempotent reduction, Min or Max (got reduce %d)", (int)cfg->reduce_op);
  if (cfg->path == MM_PATH_SPLIT) return fail(MM_ERR_UNSUPPORTED, "MM_PATH_SPLIT has no closure form");
  if (cfg->layout_a == MM_A_TRANSPOSED) return fail(MM_ERR_BAD_ARGUMENT, "a closure has no A operand to transpose");
  const unsigned b = closure_block(*cfg, w != nullptr);
  if (!b)
    return fail(MM_ERR_BAD_ARGUMENT, "closure_block %d is not a block size of this form (64, 128%s)",
                mm::tuning(mm::TUNE_CLOSURE_BLOCK), !w && mm_dtype_size(cfg->dtype) <= 4 ? " or 256" : "");
  if (n == 0 || batch == 0) return MM_OK;   // nothing to do
  if (!d) return fail(MM_ERR_BAD_ARGUMENT, "null matrix pointer");
  const size_t nn = (size_t)n * n;
  if (batch > 1 && stride_d < nn)
    return fail(MM_ERR_BAD_ARGUMENT, "stride_d %zu < n * n = %zu: the graphs of the batch would overlap", stride_d, nn);
  if (w && spans_overlap(d, batch_span(nn, stride_d, batch, mm_dtype_size(cfg->dtype)), w,
                         batch_span(nn, stride_d, batch, sizeof(int))))
    return fail(MM_ERR_BAD_ARGUMENT, "witness overlaps d (bases %p, %p)", d, (const void *)w);
  *block = b;
  return MM_OK;
}

// Snapshot workspace of one chunk of the batch stays below this; a graph that alone needs more runs alone.
constexpr size_t kClosureWorkspaceCap = 256ull << 20;

// Step 3 of a round: D <- D (+) Cc (x) Rc over every graph of the chunk, seeded, on the existing kernels.  Value-only: the
// accumulating batched call's kernel (a D that is not 16-byte aligned per graph runs the k-ordered one under
// MM_PATH_AUTO: the same values); with witnesses: the seeded argreduce kernel, index_base = k0.
int closure_rank_update(hipStream_t s, const mm_config_t &cfg, mm::Problem q, int *w, unsigned k0) {
  q.seed = true;
  if (w) {
    ArKernel ker;
    int rc = check_argreduce(&cfg, q, w, (int)k0, &ker);
    return rc ? rc : dispatch_argreduce(s, cfg, q, w, (int)k0, ker);
  }
  mm_config_t c3 = cfg;
  if (cfg.path == MM_PATH_AUTO && !batch_aligned16(q, mm_dtype_size(cfg.dtype))) c3.path = MM_PATH_ORDERED;
  Family fam;
  int rc = check_accumulate(&c3, q, &fam);
  return rc ? rc : dispatch_batched(s, c3, q, fam);
}

int closure_step(hipStream_t s, const mm_config_t &cfg, const mm::ClosureStep &st) {
  return launch_status(mm::launch_closure(s, cfg, st), cfg, "closure ",
                       st.panels ? "closure panel kernel launch" : "closure diagonal kernel launch", st.bt);
}

// The closure on stream `s`, never synchronising the host.  n <= B: one on-chip launch per chunk of graphs.  Otherwise, per
// chunk of graphs, rounds of (diagonal, panels, rank-B update) with the snapshots in stream-ordered workspace.
int dispatch_closure(hipStream_t s, const mm_config_t &cfg, void *d, int *w, unsigned n, unsigned batch, size_t stride_d,
                     unsigned B) {
  const size_t es = mm_dtype_size(cfg.dtype), nn = (size_t)n * n;
  if (batch == 1) stride_d = nn;
  (void)hipGetLastError();   // a stale error of the application's own calls must not be reported as this launch's
  mm::ClosureStep st{};
  st.n = n;
  st.stride_d = stride_d;
  if (n <= B) {
    const unsigned chunk = 1u << 20;   // workgroups per launch (of up to 1024 threads)
    for (unsigned e0 = 0; e0 < batch; e0 += chunk) {
      st.d = (char *)d + (size_t)e0 * stride_d * es;
      st.w = w ? w + (size_t)e0 * stride_d : nullptr;
      st.graphs = std::min(chunk, batch - e0);
      st.bt = n;
      st.w_fresh = 1;
      if (int rc = closure_step(s, cfg, st)) return rc;
    }
    return MM_OK;
  }
  const size_t sn = ((size_t)n * B + 63) & ~(size_t)63;   // elements of one snapshot: 16-byte aligned for every element size
  const unsigned chunk = (unsigned)std::min<size_t>(batch, std::max<size_t>(1, kClosureWorkspaceCap / (2 * sn * es)));
  Workspace ws{s, "hipFreeAsync (closure workspace)"};
  int rc = ws.allocate(2 * sn * chunk * es, "hipMallocFromPoolAsync(&ws, 2 * sn * chunk * es, pool, s)");
  if (rc) return rc;
  st.cc = ws.bytes();
  st.rc = ws.bytes() + sn * chunk * es;
  st.stride_ws = sn;
  for (unsigned e0 = 0; e0 < batch && rc == MM_OK; e0 += chunk) {
    st.graphs = std::min(chunk, batch - e0);
    st.d = (char *)d + (size_t)e0 * stride_d * es;
    st.w = w ? w + (size_t)e0 * stride_d : nullptr;
    if (st.w) {   // every witness starts at -1
      const hipError_t e = hipMemset2DAsync(st.w, stride_d * sizeof(int), 0xFF, nn * sizeof(int), st.graphs, s);
      if (e != hipSuccess) rc = hip_fail(e, "hipMemset2DAsync (witness)");
    }
    for (unsigned k0 = 0; k0 < n && rc == MM_OK; k0 += B) {
      st.k0 = k0;
      st.bt = std::min(B, n - k0);
      st.panels = false;
      st.w_fresh = 0;
      if ((rc = closure_step(s, cfg, st))) break;
      st.panels = true;
      if ((rc = closure_step(s, cfg, st))) break;
      const mm::Problem q = batched_problem(&cfg, st.cc, st.rc, st.d, n, st.bt, n, st.graphs, sn, sn, stride_d);
      rc = closure_rank_update(s, cfg, q, st.w, k0);
    }
  }
  return ws.release(rc);
}

// ---- bit-packed Boolean semiring (mm_bits_*) ----------------------------------------------------------------------------
enum BitsKernel { BITS_NONE, BITS_PLAIN, BITS_TILE, BITS_INVALID };

size_t bits_words(unsigned cols) { return ((size_t)cols + 31) / 32; }
// Units (words, or bytes for the unpacked side) an operand of the batch can touch: rows of `row` units, ld apart.
size_t bits_span(unsigned rows, size_t row, size_t ld, unsigned batch, size_t stride) {
  return rows && row && batch ? (size_t)(batch - 1) * stride + (size_t)(rows - 1) * ld + row : 0;
}

// A kernel knob of the packed products: -1 the product's own rule (by_shape), 0 the plain kernel always, 1 the tile kernel
// wherever its ld rule holds (serves); alignment may still demote BITS_TILE at launch.
BitsKernel bits_kernel_by_knob(mm::Tunable knob, bool serves, bool by_shape) {
  const int v = mm::tuning(knob);
  if (v < -1 || v > 1) return BITS_INVALID;
  if (v == 0 || !serves) return BITS_PLAIN;
  return v == 1 || by_shape ? BITS_TILE : BITS_PLAIN;
}

// The kernel by shape, ld and knob alone (mm_kernel_name_bits_gemm).
BitsKernel bits_kernel_for(unsigned m, size_t ldb, size_t ldc) {
  // below 65 words the tile's second word per lane would be idle
  return bits_kernel_by_knob(mm::TUNE_BITS_VARIANT, mm::bits_tile_serves(ldb, ldc), m > 2048);
}

constexpr unsigned long long kBitsCountTileMin = 256;   // 128 x 128 tiles of C from which bits_count_tile serves: one per CU

// The kernel by shape, ld and knob alone (mm_kernel_name_bits_count).
BitsKernel bits_count_kernel_for(unsigned n, unsigned m, size_t lda, size_t ldbt, size_t ldc) {
  const unsigned long long tiles = (unsigned long long)(((size_t)n + 127) / 128) * (((size_t)m + 127) / 128);
  return bits_kernel_by_knob(mm::TUNE_BITS_COUNT_VARIANT, mm::bits_count_tile_serves(lda, ldbt, ldc), tiles >= kBitsCountTileMin);
}

constexpr unsigned kBitsGf2TileMin = 128;    // N and M from which bits_gf2_tile serves (profiles/bits_gf2_sweep_mi355x.txt)

// The kernel by shape, ld and knob alone (mm_kernel_name_bits_gf2).
BitsKernel bits_gf2_kernel_for(unsigned n, unsigned m, size_t ldb, size_t ldc) {
  return bits_kernel_by_knob(mm::TUNE_BITS_GF2_VARIANT, mm::bits_gf2_tile_serves(ldb, ldc), n >= kBitsGf2TileMin && m >= kBitsGf2TileMin);
}

// What is a packed product's own in its argument checks; everything else the three products share (check_bits_product).
struct BitsProduct {
  mm::Tunable knob;        // the knob of its kernels
  BitsKernel ker;          // its kernel by shape, ld and knob
  unsigned b_rows;         // B as it is stored: K x ceil(M / 32) words, or (Bt) M x ceil(K / 32) words
  size_t b_row;
  size_t c_row;            // a row of C: ceil(M / 32) words, or M int32 elements -- 4 bytes each either way
  unsigned align[3];       // bytes to which the tile kernel needs a, b and c aligned, base and batch stride (0: to nothing)
  const char *b_name, *c_row_text, *ld_text;
};

BitsProduct bits_gemm_rules(const mm::BitsProblem &p) {
  const size_t mw = bits_words(p.m);
  return {mm::TUNE_BITS_VARIANT, bits_kernel_for(p.m, p.ldb, p.ldc), p.k, mw, mw, {0, 16, 8}, "b", "ceil(M / 32)",
          "a row stride is below its row's words: lda %zu (needs %zu), ldb %zu (%zu), ldc %zu (%zu)"};
}

BitsProduct bits_gf2_rules(const mm::BitsProblem &p) {   // the Boolean product's operands and texts; its own knob and kernels
  BitsProduct r = bits_gemm_rules(p);
  r.knob = mm::TUNE_BITS_GF2_VARIANT;
  r.ker = bits_gf2_kernel_for(p.n, p.m, p.ldb, p.ldc);
  r.align[1] = 8;   // bits_gf2_tile's accesses of B and of C are 8 bytes wide
  return r;
}

BitsProduct bits_count_rules(const mm::BitsProblem &p) {   // p.b: Bt, M x K
  return {mm::TUNE_BITS_COUNT_VARIANT, bits_count_kernel_for(p.n, p.m, p.lda, p.ldb, p.ldc), p.m, bits_words(p.k), p.m, {16, 16, 16},
          "bt", "M", "a row stride is below its row: lda %zu (needs %zu words), ldbt %zu (%zu words), ldc %zu (%zu elements)"};
}

// The launch-time half of the serving rule: the tile kernel's wide accesses, for every element of the batch.
BitsKernel bits_demote(const mm::BitsProblem &p, BitsKernel ker, const unsigned (&align)[3]) {
  if (ker != BITS_TILE) return ker;
  const void *const base[3] = {p.a, p.b, p.c};
  const size_t stride[3] = {p.stride_a, p.stride_b, p.stride_c};
  for (int i = 0; i < 3; ++i)
    if (align[i] && (((uintptr_t)base[i] & (align[i] - 1)) != 0 || (p.batch > 1 && stride[i] % (align[i] / 4) != 0))) return BITS_PLAIN;
  return BITS_TILE;
}

// All argument checks of a packed product, before any device is touched.  *ker = BITS_NONE: nothing to launch.
int check_bits_product(const mm::BitsProblem &p, const BitsProduct &r, BitsKernel *ker) {
  *ker = BITS_NONE;
  if (r.ker == BITS_INVALID) return fail(MM_ERR_BAD_ARGUMENT, "%s %d is not one of -1, 0, 1", kTuneName[r.knob], mm::tuning(r.knob));
  if (p.batch == 0 || p.n == 0 || p.m == 0) return MM_OK;
  if (!p.c || (p.k && (!p.a || !p.b))) return fail(MM_ERR_BAD_ARGUMENT, "null matrix pointer");   // (K = 0: A, B unread)
  const size_t kw = bits_words(p.k);
  if (p.lda < kw || p.ldc < r.c_row || (r.b_rows && p.ldb < r.b_row))
    return fail(MM_ERR_BAD_ARGUMENT, r.ld_text, p.lda, kw, p.ldb, r.b_row, p.ldc, r.c_row);
  const size_t c_units = bits_span(p.n, r.c_row, p.ldc, 1, 0);
  if (p.batch > 1 && p.stride_c < c_units)
    return fail(MM_ERR_BAD_ARGUMENT, "stride_c %zu < (N - 1) ldc + %s = %zu: the outputs of the batch would overlap", p.stride_c,
                r.c_row_text, c_units);
  const size_t a_bytes = 4 * bits_span(p.n, kw, p.lda, p.batch, p.stride_a);
  const size_t b_bytes = 4 * bits_span(r.b_rows, r.b_row, p.ldb, p.batch, p.stride_b);
  const size_t c_bytes = 4 * bits_span(p.n, r.c_row, p.ldc, p.batch, p.stride_c);
  if (spans_overlap(p.c, c_bytes, p.a, a_bytes) || spans_overlap(p.c, c_bytes, p.b, b_bytes))
    return fail(MM_ERR_BAD_ARGUMENT, "c overlaps a or %s (bases %p, %p, %p)", r.b_name, (const void *)p.a, (const void *)p.b,
                (void *)p.c);
  if (p.k == 0 && p.seed) return MM_OK;   // accumulating over no k: C keeps its value
  *ker = bits_demote(p, r.ker, r.align);
  return MM_OK;
}

int check_bits_count(int op, const mm::BitsProblem &p, BitsKernel *ker) {
  *ker = BITS_NONE;
  if (op != MM_BITS_COUNT_AND && op != MM_BITS_COUNT_XOR)
    return fail(MM_ERR_BAD_ARGUMENT, "op %d is not MM_BITS_COUNT_AND (0) or MM_BITS_COUNT_XOR (1)", op);
  return check_bits_product(p, bits_count_rules(p), ker);
}

// The packed twin of for_each_chunk: fn(slice) over the batch in launches of at most 2^22 workgroups -- `tiles` per element,
// counted in the smaller of a product's two tiles -- and batch_chunk elements.
template <class F> int for_each_bits_chunk(const mm::BitsProblem &p, unsigned long long tiles, F &&fn) {
  const unsigned chunk = chunk_of_tiles(tiles, p.batch);
  (void)hipGetLastError();   // a stale error of the application's own calls must not be reported as this launch's
  for (unsigned e0 = 0; e0 < p.batch; e0 += chunk) {
    mm::BitsProblem q = p;
    q.batch = std::min(chunk, p.batch - e0);
    q.a += (size_t)e0 * p.stride_a;
    q.b += (size_t)e0 * p.stride_b;
    q.c += (size_t)e0 * p.stride_c;
    if (int rc = fn(q)) return rc;
  }
  return MM_OK;
}

int dispatch_bits_gemm(hipStream_t s, const mm::BitsProblem &p, BitsKernel ker) {   // tiles of 64 x 64 words
  return for_each_bits_chunk(p, (unsigned long long)((p.n + 63) / 64) * ((bits_words(p.m) + 63) / 64), [&](const mm::BitsProblem &q) {
    const int e = mm::launch_bits_gemm(s, q, ker == BITS_TILE);
    return e ? hip_fail((hipError_t)e, "packed product kernel launch") : MM_OK;
  });
}

int dispatch_bits_gf2(hipStream_t s, const mm::BitsProblem &p, BitsKernel ker) {   // tiles of 64 x 64 words (bits_gf2_tile's are larger)
  return for_each_bits_chunk(p, (unsigned long long)((p.n + 63) / 64) * ((bits_words(p.m) + 63) / 64), [&](const mm::BitsProblem &q) {
    const int e = mm::launch_bits_gf2(s, q, ker == BITS_TILE);
    return e ? hip_fail((hipError_t)e, "packed GF(2) product kernel launch") : MM_OK;
  });
}

int dispatch_bits_count(hipStream_t s, int op, const mm::BitsProblem &p, BitsKernel ker) {   // tiles of 64 x 64 elements
  return for_each_bits_chunk(p, (unsigned long long)((p.n + 63) / 64) * ((p.m + 63) / 64), [&](const mm::BitsProblem &q) {
    const int e = mm::launch_bits_count(s, q, op == MM_BITS_COUNT_XOR, ker == BITS_TILE);
    return e ? hip_fail((hipError_t)e, "packed counting kernel launch") : MM_OK;
  });
}

// ---- pack, unpack and the packed transpose: one check, each side given as it is stored ---------------------------------------
enum BitsConversion { BITS_PACK, BITS_UNPACK, BITS_TRANSPOSE };
struct BitsSide {
  unsigned rows;
  size_t row, unit;   // units of a row, bytes of a unit: bytes of the unpacked form, words of the packed one
};

// *nothing: an empty call
int check_bits_convert(const mm::BitsConvert &c, const BitsSide &src, const BitsSide &dst, bool *nothing) {
  *nothing = c.rows == 0 || c.cols == 0 || c.batch == 0;
  if (*nothing) return MM_OK;
  if (!c.src || !c.dst) return fail(MM_ERR_BAD_ARGUMENT, "null matrix pointer");
  if (c.ld_src < src.row || c.ld_dst < dst.row)
    return fail(MM_ERR_BAD_ARGUMENT, "a row stride is below its row: source %zu (needs %zu), destination %zu (%zu)", c.ld_src,
                src.row, c.ld_dst, dst.row);
  if (c.batch > 1 && c.stride_dst < bits_span(dst.rows, dst.row, c.ld_dst, 1, 0))
    return fail(MM_ERR_BAD_ARGUMENT, "destination batch stride %zu: the outputs of the batch would overlap", c.stride_dst);
  if (spans_overlap(c.dst, dst.unit * bits_span(dst.rows, dst.row, c.ld_dst, c.batch, c.stride_dst), c.src,
                    src.unit * bits_span(src.rows, src.row, c.ld_src, c.batch, c.stride_src)))
    return fail(MM_ERR_BAD_ARGUMENT, "the destination overlaps the source (bases %p, %p)", c.src, c.dst);
  return MM_OK;
}

int dispatch_bits_convert(hipStream_t s, const mm::BitsConvert &c, BitsConversion how) {
  static constexpr struct {
    int (*launch)(hipStream_t, const mm::BitsConvert &);
    const char *what;
  } kConversions[] = {{mm::launch_bits_pack, "pack kernel launch"},
                      {mm::launch_bits_unpack, "unpack kernel launch"},
                      {mm::launch_bits_transpose, "packed transpose kernel launch"}};
  (void)hipGetLastError();
  const int e = kConversions[how].launch(s, c);
  return e ? hip_fail((hipError_t)e, kConversions[how].what) : MM_OK;
}

constexpr unsigned kBitsClosureBlock = 64;   // one wavefront closes a diagonal block: one row of 64 bits per lane

int check_bits_closure(const void *d, unsigned n, size_t ldd, unsigned batch, size_t stride_d, bool *nothing) {
  *nothing = n == 0 || batch == 0;
  if (*nothing) return MM_OK;
  if (!d) return fail(MM_ERR_BAD_ARGUMENT, "null matrix pointer");
  const size_t nw = bits_words(n);
  if (ldd < nw) return fail(MM_ERR_BAD_ARGUMENT, "ldd %zu is below the row's %zu words", ldd, nw);
  if (batch > 1 && stride_d < bits_span(n, nw, ldd, 1, 0))
    return fail(MM_ERR_BAD_ARGUMENT, "stride_d %zu < (n - 1) ldd + ceil(n / 32) = %zu: the graphs of the batch would overlap",
                stride_d, bits_span(n, nw, ldd, 1, 0));
  return MM_OK;
}

// One product of a closure round on the graphs of a chunk: the library's own operands, no argument checks.
int bits_closure_product(hipStream_t s, const mm::BitsProblem &p) {
  const BitsProduct r = bits_gemm_rules(p);
  return dispatch_bits_gemm(s, p, bits_demote(p, r.ker == BITS_INVALID ? BITS_PLAIN : r.ker, r.align));
}

// The packed closure on stream `s`, never synchronising the host.  n <= 64: the wavefront kernel in place, 2^20 graphs per
// launch.  Otherwise, per chunk of graphs and per block K of 64 vertices: P | I of the closed diagonal block, the panels
// R = (P | I) D[K,:] and Cc = D[:,K] (P | I) into workspace -- nothing reads a word of D that the same launch writes -- and
// D <- D | Cc R.  (P | I)(P | I) = P | I, so Cc R = D[:,K] (P | I) D[K,:]: every path whose inner vertices lie in K.
int dispatch_bits_closure(hipStream_t s, uint32_t *d, unsigned n, size_t ldd, unsigned batch, size_t stride_d) {
  (void)hipGetLastError();
  if (batch == 1) stride_d = 0;
  if (n <= kBitsClosureBlock) {
    const unsigned chunk = 1u << 20;
    for (unsigned e0 = 0; e0 < batch; e0 += chunk)
      if (int e = mm::launch_bits_closure_diag(s, d + (size_t)e0 * stride_d, n, ldd, std::min(chunk, batch - e0), stride_d, 0, nullptr, 0))
        return hip_fail((hipError_t)e, "packed closure kernel launch");
    return MM_OK;
  }
  const size_t nw = bits_words(n), ldr = (nw + 3) & ~(size_t)3;   // R's rows 16-byte aligned: the tile kernel's B
  const size_t p_words = 2 * kBitsClosureBlock, r_words = kBitsClosureBlock * ldr, c_words = ((size_t)2 * n + 3) & ~(size_t)3;
  const size_t per_graph = p_words + r_words + c_words;
  size_t chunk = std::min<size_t>(batch, std::max<size_t>(1, kClosureWorkspaceCap / (per_graph * 4)));
  const int knob = mm::tuning(mm::TUNE_BATCH_CHUNK);
  if (knob > 0) chunk = std::min<size_t>(chunk, (unsigned)knob);
  Workspace ws{s, "hipFreeAsync (packed closure workspace)"};
  int rc = ws.allocate(per_graph * chunk * 4, "hipMallocFromPoolAsync(&ws, per_graph * chunk * 4, pool, s)");
  if (rc) return rc;
  uint32_t *pstar = (uint32_t *)ws.bytes(), *rp = pstar + p_words, *cp = rp + r_words;   // per graph: [P | I, R, Cc], per_graph words apart
  for (unsigned e0 = 0; e0 < batch && rc == MM_OK; e0 += (unsigned)chunk) {
    const unsigned graphs = (unsigned)std::min<size_t>(chunk, batch - e0);
    uint32_t *dg = d + (size_t)e0 * stride_d;
    for (unsigned k0 = 0; k0 < n && rc == MM_OK; k0 += kBitsClosureBlock) {
      const unsigned bt = std::min(kBitsClosureBlock, n - k0);
      if (int e = mm::launch_bits_closure_diag(s, dg, n, ldd, graphs, stride_d, k0, pstar, per_graph)) {
        rc = hip_fail((hipError_t)e, "packed closure kernel launch");
        break;
      }
      const mm::BitsProblem row{pstar, dg + (size_t)k0 * ldd, rp, bt, bt, n, 2, ldd, ldr, graphs, per_graph, stride_d, per_graph, false};
      const mm::BitsProblem col{dg + k0 / 32, pstar, cp, n, bt, bt, ldd, 2, 2, graphs, stride_d, per_graph, per_graph, false};
      const mm::BitsProblem all{cp, rp, dg, n, bt, n, 2, ldr, ldd, graphs, per_graph, per_graph, stride_d, true};
      if ((rc = bits_closure_product(s, row)) || (rc = bits_closure_product(s, col))) break;
      rc = bits_closure_product(s, all);
    }
  }
  return ws.release(rc);
}

// ---- log semiring (mm_gemm_logsumexp_*, mm_gemm_logsumexp_nt_*): log sum exp (A + B) --------------------------------------
enum LseKernel { LSE_NONE, LSE_EXACT, LSE_HYBRID };

// The kernel by configuration and knob alone (mm_kernel_name_logsumexp).  *bad_knob: lse_variant holds a value it does not take.
LseKernel lse_kernel_for(const mm_config_t &cfg, bool *bad_knob) {
  const int v = mm::tuning(mm::TUNE_LSE_VARIANT);
  *bad_knob = v < -1 || v > 2;
  if (cfg.dtype != MM_DTYPE_F32 && cfg.dtype != MM_DTYPE_F64 && cfg.dtype != MM_DTYPE_F16) return LSE_NONE;
  if (cfg.map_op != MM_OP_ADD || (cfg.reduce_op != MM_OP_MIN && cfg.reduce_op != MM_OP_MAX)) return LSE_NONE;
  if (cfg.path == MM_PATH_SPLIT) return LSE_NONE;
  if (cfg.path == MM_PATH_ORDERED || v == 0) return LSE_EXACT;
  return LSE_HYBRID;
}

// All argument checks of a logsumexp call, before any device is touched.  *ker = LSE_NONE: nothing to launch (an empty
// batch, or K = 0 when accumulating).
int check_lse(const mm_config_t *cfg, const mm::Problem &p, LseKernel *ker) {
  *ker = LSE_NONE;
  if (!valid_cfg(cfg)) return fail(MM_ERR_BAD_ARGUMENT, "invalid mm_config_t");
  if (bt_refused(*cfg, p)) return fail_bt(*cfg);
  bool bad_knob;
  const LseKernel k = lse_kernel_for(*cfg, &bad_knob);
  if (k == LSE_NONE)
    return fail(MM_ERR_UNSUPPORTED, "logsumexp serves half, float and double with map Add and reduce Min or Max, under "
                "MM_PATH_AUTO or MM_PATH_ORDERED (got dtype %d, map %d, reduce %d, path %d)", (int)cfg->dtype,
                (int)cfg->map_op, (int)cfg->reduce_op, (int)cfg->path);
  if (bad_knob)
    return fail(MM_ERR_BAD_ARGUMENT, "lse_variant %d is not one of -1, 0, 1, 2", mm::tuning(mm::TUNE_LSE_VARIANT));
  bool go;
  const size_t es = mm_dtype_size(cfg->dtype);
  if (int rc = check_seeded(p, es, es, &go)) return rc;
  if (go) *ker = k;
  return MM_OK;
}

// The exact kernel over the batch, in launches of at most batch_chunk() elements; flags (per element: the 64 x 64 tiles of
// one element) restrict it to the flagged tiles.
int lse_exact_chunks(hipStream_t s, const mm_config_t &cfg, const mm::Problem &p, const int *flags) {
  const size_t tiles = (size_t)((p.n + 63) / 64) * ((p.m + 63) / 64);
  return for_each_chunk(p, mm_dtype_size(cfg.dtype), batch_chunk(p), [&](const mm::Problem &q, unsigned e0) {
    return launch_status(mm::launch_lse_exact(s, cfg, q, flags ? flags + e0 * tiles : nullptr), cfg, "logsumexp ",
                         "logsumexp kernel launch");
  });
}

// Workspace of one chunk of the hybrid stays near this; an element that alone needs more runs alone.
constexpr size_t kLseWorkspaceCap = 256ull << 20;

// The hybrid, never synchronising the host: per chunk of the batch, prepass (row maxima of A, column maxima of B -- row maxima
// of an M x K B: "lse_hybrid_nt", whose EB is K-major in the workspace all the same --, EA and EB
// zero-padded to multiples of 64 in f32 / f64), S = EA @ EB on the matrix cores, the epilogue (C and one flag per tile) and
// the exact kernel over the flagged tiles.  A broadcast operand is transformed once.  The product's kernel is resolved once on
// the whole batch, so an element's bits do not depend on the chunk it falls in.
int dispatch_lse_hybrid(hipStream_t s, const mm_config_t &cfg, const mm::Problem &p) {
  const bool dbl = cfg.dtype == MM_DTYPE_F64;
  const size_t fs = dbl ? 8 : 4, es = mm_dtype_size(cfg.dtype);
  const auto up = [](size_t x) { return (x + 63) & ~(size_t)63; };
  const unsigned np = (unsigned)up(p.n), kp = (unsigned)up(p.k), mp = (unsigned)up(p.m);
  const size_t tiles = (size_t)(np / 64) * (mp / 64);
  const bool a_shared = p.batch > 1 && p.stride_a == 0, b_shared = p.batch > 1 && p.stride_b == 0;
  const size_t ea = up((size_t)np * kp), eb = up((size_t)kp * mp), sz = up((size_t)np * mp), ra = up(np), rb = up(mp);
  const size_t per = (a_shared ? 0 : ea + ra) + (b_shared ? 0 : eb + rb) + sz;   // F elements per element of the batch
  const size_t fixed = (a_shared ? ea + ra : 0) + (b_shared ? eb + rb : 0);
  unsigned chunk = (unsigned)std::min<size_t>(p.batch, std::max<size_t>(1, kLseWorkspaceCap / ((per + tiles) * fs)));
  chunk = std::min(chunk, batch_chunk(p));
  const size_t fl = up(tiles * chunk);                                          // int32 flags, one per tile
  const size_t bytes = (fixed + per * chunk) * fs + fl * sizeof(int);
  Workspace ws{s, "hipFreeAsync (logsumexp workspace)"};
  int rc = ws.allocate(bytes, "hipMallocFromPoolAsync((void **)&ws, bytes, pool, s)");
  if (rc) return rc;
  if (mm::tuning(mm::TUNE_DEBUG_POISON) == 1) {   // every F of the workspace NaN: a read of an unwritten element shows up
    const hipError_t e = hipMemsetAsync(ws.bytes(), 0xFF, bytes, s);
    if (e != hipSuccess) rc = hip_fail(e, "hipMemsetAsync (logsumexp workspace)");
  }
  const auto launched = [&](int e, const char *what) { return launch_status(e, cfg, "logsumexp ", what); };
  // layout: [EA][EB][S][ra][rb] in F, then the flags
  char *const pea = ws.bytes(), *const peb = pea + (a_shared ? ea : ea * chunk) * fs, *const ps = peb + (b_shared ? eb : eb * chunk) * fs;
  char *const pra = ps + sz * chunk * fs, *const prb = pra + (a_shared ? ra : ra * chunk) * fs;
  int *const flags = (int *)(prb + (b_shared ? rb : rb * chunk) * fs);
  const size_t sea = a_shared ? 0 : ea, seb = b_shared ? 0 : eb, sra = a_shared ? 0 : ra, srb = b_shared ? 0 : rb;
  mm::LseOperand opa{}, opb{};
  opa.rows = p.n; opa.k = p.k; opa.rows_p = np; opa.k_p = kp; opa.x_kmajor = p.a_transposed; opa.out_kmajor = false;
  opa.e = pea; opa.r = pra; opa.stride_x = p.stride_a; opa.stride_e = ea; opa.stride_r = ra;
  opb.rows = p.m; opb.k = p.k; opb.rows_p = mp; opb.k_p = kp; opb.x_kmajor = !p.b_transposed; opb.out_kmajor = true;
  opb.e = peb; opb.r = prb; opb.stride_x = p.stride_b; opb.stride_e = eb; opb.stride_r = rb;
  if (rc == MM_OK && a_shared) {
    opa.x = p.a; opa.count = 1;
    rc = launched(mm::launch_lse_prepass(s, cfg, opa), "logsumexp prepass launch");
  }
  if (rc == MM_OK && b_shared) {
    opb.x = p.b; opb.count = 1;
    rc = launched(mm::launch_lse_prepass(s, cfg, opb), "logsumexp prepass launch");
  }
  // S = EA @ EB: (Multiply, Add) in F on the matrix cores; one element: the single launch's kernel, else the batched one
  // resolved on the whole batch
  const mm_config_t gcfg{dbl ? MM_DTYPE_F64 : MM_DTYPE_F32, MM_OP_MULTIPLY, MM_OP_ADD, MM_PATH_AUTO, MM_A_ROW_MAJOR};
  mm::Problem whole = batched_problem(&gcfg, pea, peb, ps, np, kp, mp, p.batch, sea, seb, sz);
  const MatrixCore &mc = *matrix_core(dbl ? FAM_MFMA_F64 : FAM_MFMA_F32);
  const int gk = mc.resolve(whole);
  if (rc == MM_OK && p.batch > 1 && gk < 0) rc = fail(MM_ERR_UNSUPPORTED, "no batched matrix-core kernel for the logsumexp product");
  for (unsigned e0 = 0; e0 < p.batch && rc == MM_OK; e0 += chunk) {
    const unsigned ce = std::min(chunk, p.batch - e0);
    const mm::Problem q = batch_slice(p, e0, ce, es);   // this chunk's elements
    if (!a_shared) {
      opa.x = q.a; opa.count = ce;
      if ((rc = launched(mm::launch_lse_prepass(s, cfg, opa), "logsumexp prepass launch"))) break;
    }
    if (!b_shared) {
      opb.x = q.b; opb.count = ce;
      if ((rc = launched(mm::launch_lse_prepass(s, cfg, opb), "logsumexp prepass launch"))) break;
    }
    mm::Problem g = batched_problem(&gcfg, pea, peb, ps, np, kp, mp, ce, sea, seb, sz);
    if (p.batch == 1) {
      if ((rc = dispatch(s, gcfg, g))) break;
    } else if ((rc = launch_status(mc.launch(s, g, gk), gcfg, "logsumexp ", "logsumexp product launch"))) {   // (the product's own)
      break;
    }
    mm::LseEpilogue ep{};
    ep.s = ps; ep.ra = pra; ep.rb = prb; ep.c = q.c; ep.flags = flags;
    ep.n = p.n; ep.m = p.m; ep.m_p = mp; ep.batch = ce;
    ep.stride_s = sz; ep.stride_ra = sra; ep.stride_rb = srb; ep.stride_c = p.stride_c;
    ep.seed = p.seed; ep.force = mm::tuning(mm::TUNE_LSE_VARIANT) == 2;
    if ((rc = launched(mm::launch_lse_epilogue(s, cfg, ep), "logsumexp epilogue launch"))) break;
    // the fallback: the exact kernel over the flagged tiles of this chunk
    if ((rc = launched(mm::launch_lse_exact(s, cfg, q, flags), "logsumexp fallback launch"))) break;
  }
  return ws.release(rc);
}

int dispatch_lse(hipStream_t s, const mm_config_t &cfg, const mm::Problem &p, LseKernel ker) {
  (void)hipGetLastError();   // a stale error of the application's own calls must not be reported as this launch's
  mm::Problem q = p;
  if (q.batch == 1) q.stride_a = q.stride_b = q.stride_c = 0;
  return ker == LSE_HYBRID ? dispatch_lse_hybrid(s, cfg, q) : lse_exact_chunks(s, cfg, q, nullptr);
}

// ---- widening (mm_gemm_widen_*): int8_t operands to int sums, half operands to float sums -------------------------------------
enum WidenKernel { WD_NONE, WD_ORDERED, WD_ORDERED_BLOCKED, WD_MFMA };   // BLOCKED: a misaligned matrix-core launch, demoted

bool widen_serves(const mm_config_t &cfg) {
  return (cfg.dtype == MM_DTYPE_F16 || cfg.dtype == MM_DTYPE_I8) && cfg.map_op == MM_OP_MULTIPLY && cfg.reduce_op == MM_OP_ADD &&
         cfg.path != MM_PATH_SPLIT;
}

// The wide instantiation of the kernel the narrow batched resolver names, by shape and path alone (mm_kernel_name_widen);
// null: widen_ordered.  The half_contract knob does not apply: it chooses between two narrow contracts.
const char *widen_mfma_name(const mm_config_t &cfg, const mm::Problem &p) {
  if (cfg.path != MM_PATH_AUTO) return nullptr;
  return cfg.dtype == MM_DTYPE_I8 ? mm::mfma_i8_wide_name(p) : mm::mfma_f16_wide_name(p);
}

// All argument checks of a widening call, before any device is touched.  *ker = WD_NONE: nothing to launch (an empty batch,
// or K = 0 when accumulating).
int check_widen(const mm_config_t *cfg, const mm::Problem &p, WidenKernel *ker) {
  *ker = WD_NONE;
  if (!valid_cfg(cfg)) return fail(MM_ERR_BAD_ARGUMENT, "invalid mm_config_t");
  if (!widen_serves(*cfg))
    return fail(MM_ERR_UNSUPPORTED, "widening serves half and int8_t with (Multiply, Add), under MM_PATH_AUTO or MM_PATH_ORDERED "
                "(got dtype %d, map %d, reduce %d, path %d)", (int)cfg->dtype, (int)cfg->map_op, (int)cfg->reduce_op,
                (int)cfg->path);
  const size_t es = mm_dtype_size(cfg->dtype), ws = mm_dtype_size((mm_dtype_t)mm_widen_dtype(cfg->dtype));
  bool go;
  if (int rc = check_seeded(p, es, ws, &go)) return rc;
  if (!go) return MM_OK;
  *ker = widen_mfma_name(*cfg, p) ? WD_MFMA : WD_ORDERED;
  // the matrix-core kernels move 16 bytes per lane of A and B, and C is written in 64-byte runs: every element's a, b and c
  // 16-byte aligned, else widen_ordered summing in blocks: MM_PATH_AUTO's contract, bound included
  const size_t strides = p.batch > 1 ? ((p.stride_a | p.stride_b) * es) | (p.stride_c * ws) : 0;
  if (*ker == WD_MFMA && (!aligned16(p) || (strides & 15u) != 0)) *ker = WD_ORDERED_BLOCKED;
  return MM_OK;
}

// Launches the batch as consecutive launches of at most batch_chunk() elements on `s`; the matrix-core kernel is resolved
// once, on the whole batch, so an element's kernel does not depend on how the batch was chunked.
int dispatch_widen(hipStream_t s, const mm_config_t &cfg, const mm::Problem &p, WidenKernel ker) {
  (void)hipGetLastError();   // a stale error of the application's own calls must not be reported as this launch's
  mm::Problem q = p;
  if (q.batch == 1) q.stride_a = q.stride_b = q.stride_c = 0;
  const bool i8 = cfg.dtype == MM_DTYPE_I8;
  const int kernel = ker != WD_MFMA ? -1 : i8 ? mm::mfma_i8_wide_resolve(q) : mm::mfma_f16_wide_resolve(q);
  const size_t ws = mm_dtype_size((mm_dtype_t)mm_widen_dtype(cfg.dtype));
  return for_each_chunk(q, mm_dtype_size(cfg.dtype), batch_chunk(q), [&](mm::Problem r, unsigned e0) {
    r.c = (char *)q.c + (size_t)e0 * q.stride_c * ws;   // C advances in its own type
    const int e = ker != WD_MFMA ? mm::launch_widen_ordered(s, cfg.dtype, r, ker == WD_ORDERED_BLOCKED)
                  : i8 ? mm::launch_mfma_i8_wide(s, r, kernel) : mm::launch_mfma_f16_wide(s, r, kernel);
    return launch_status(e, cfg, "widen ", "widen kernel launch");
  });
}

// ---- A x B^T (mm_gemm_nt_*): B stored M x K row-major -----------------------------------------------------------------------
enum NtKernel { NT_NONE, NT_ORDERED, NT_ORDERED_WIDE, NT_VALU_TILE, NT_PREPASS };   // ORDERED_WIDE: ordered_nt's ACC = float half form

bool nt_serves(const mm_config_t &cfg) { return cfg.path != MM_PATH_SPLIT && cfg.layout_a != MM_A_TRANSPOSED; }

// half (Multiply, Add) under MM_PATH_AUTO keeps ONE contract on every shape and alignment: exact products, f32 sums, one rounding
bool nt_half_wide(const mm_config_t &cfg) {
  return cfg.path == MM_PATH_AUTO && cfg.dtype == MM_DTYPE_F16 && cfg.map_op == MM_OP_MULTIPLY && cfg.reduce_op == MM_OP_ADD &&
         mm::tuning(mm::TUNE_HALF_CONTRACT) != 1;
}

// The kernel by configuration, shape and path alone (mm_kernel_name_nt): the family the narrow batched call would run on
// (n, k, m, batch), mapped.  A matrix-core family (its batched resolver names a kernel) with K and M multiples of the 16-byte
// chunk: the transposition pre-pass and that kernel; the k-ordered contract (MM_PATH_ORDERED, half_contract = 1): ordered_nt;
// half (Multiply, Add) otherwise: ordered_nt accumulating in f32; everything else: valu_tile_nt where it serves -- by ITS rule,
// which asks nothing of M -- else ordered_nt.  Alignment and a full workspace pool may still demote at launch.
NtKernel nt_kernel_for(const mm_config_t &cfg, const mm::Problem &p) {
  if (!nt_serves(cfg)) return NT_NONE;
  const bool mul_add = cfg.map_op == MM_OP_MULTIPLY && cfg.reduce_op == MM_OP_ADD;
  // the k-ordered contract, as choose() reads it: asked for by path, or by half_contract = 1 for half (Multiply, Add)
  if (cfg.path == MM_PATH_ORDERED || (mul_add && cfg.dtype == MM_DTYPE_F16 && mm::tuning(mm::TUNE_HALF_CONTRACT) == 1)) return NT_ORDERED;
  const auto valu_or_ordered = [&] {
    return nt_half_wide(cfg) ? NT_ORDERED_WIDE : mm::valu_tile_nt_serves(cfg, p) ? NT_VALU_TILE : NT_ORDERED;
  };
  switch (choose_batched(cfg, p)) {
    case FAM_MFMA_F32: case FAM_MFMA_F64: case FAM_MFMA_F16: case FAM_MFMA_I8: {
      const unsigned epc = (unsigned)(16 / mm_dtype_size(cfg.dtype));
      return p.k % epc == 0 && p.m % epc == 0 ? NT_PREPASS : valu_or_ordered();
    }
    case FAM_NONE: case FAM_F32_SPLIT: return NT_NONE;
    // FAM_HALF_WIDE; FAM_VALU_TILE; and FAM_ORDERED, which under MM_PATH_AUTO only means that the row-major kernel's K % 4 /
    // M % 4 rule, or an operator it does not hold, sent the narrow call there
    default: return valu_or_ordered();
  }
}

// What a launch that cannot run its fast kernel (misaligned operands, no workspace) runs instead: the same contract
NtKernel nt_demoted(const mm_config_t &cfg) { return nt_half_wide(cfg) ? NT_ORDERED_WIDE : NT_ORDERED; }

// All argument checks of an A x B^T call, before any device is touched.  *ker = NT_NONE: nothing to launch (an empty batch,
// or K = 0 when accumulating).  A and Bt may be the same buffer.
int check_nt(const mm_config_t *cfg, const mm::Problem &p, NtKernel *ker) {
  *ker = NT_NONE;
  if (!valid_cfg(cfg)) return fail(MM_ERR_BAD_ARGUMENT, "invalid mm_config_t");
  if (!nt_serves(*cfg))
    return fail(MM_ERR_UNSUPPORTED, "the A x B^T calls serve a row-major A under MM_PATH_AUTO or MM_PATH_ORDERED (got path %d, "
                "layout_a %d)", (int)cfg->path, (int)cfg->layout_a);
  const size_t es = mm_dtype_size(cfg->dtype);
  bool go;
  if (int rc = check_seeded(p, es, es, &go)) return rc;
  if (!go) return MM_OK;
  *ker = nt_kernel_for(*cfg, p);
  // valu_tile_nt moves 16 bytes per lane of A and Bt (C goes element by element); the pre-pass and the matrix-core kernels
  // 16 bytes of C as well: else ordered_nt, any element-aligned pointer
  const size_t in_strides = p.batch > 1 ? (p.stride_a | p.stride_b) * es : 0;
  const bool in_aligned = ((((uintptr_t)p.a | (uintptr_t)p.b) | in_strides) & 15u) == 0;
  if ((*ker == NT_VALU_TILE && !in_aligned) || (*ker == NT_PREPASS && !batch_aligned16(p, es))) *ker = nt_demoted(*cfg);
  return MM_OK;
}

// `ker` over the batch in launches of at most batch_chunk() elements
int nt_chunks(hipStream_t s, const mm_config_t &cfg, const mm::Problem &p, NtKernel ker) {
  return for_each_chunk(p, mm_dtype_size(cfg.dtype), batch_chunk(p), [&](const mm::Problem &q, unsigned) {
    int e;
    switch (ker) {
      case NT_VALU_TILE:
        e = mm::launch_valu_tile_nt(s, cfg, q);
        if (e == mm::kErrNotSupported) e = mm::launch_ordered_nt(s, cfg, q);   // still the GPU
        break;
      case NT_ORDERED_WIDE: e = mm::launch_half_wide_nt(s, q); break;
      default: e = mm::launch_ordered_nt(s, cfg, q); break;
    }
    return launch_status(e, cfg, "A x B^T ", "A x B^T kernel launch");
  });
}

// Transposed copies of one chunk of the batch stay near this; an element that alone needs more runs alone.
constexpr size_t kNtWorkspaceCap = 256ull << 20;

// "nt_prepass", never synchronising the host: B = Bt^T (K x M per element) into stream-ordered workspace, then the batched
// matrix-core kernel on it -- resolved once on the whole batch, so the bits are those of mm_gemm_batched_* /
// mm_gemm_batched_accumulate_* on a materialised transpose, whatever the chunking.  A broadcast Bt is transposed once.
// A full pool is no error: ordered_nt serves the call without extra memory, same contract.
int dispatch_nt_prepass(hipStream_t s, const mm_config_t &cfg, const mm::Problem &p) {
  const size_t es = mm_dtype_size(cfg.dtype), km = (size_t)p.k * p.m;   // (km * es is a multiple of 16: K and M are chunk multiples)
  const bool b_shared = p.batch == 1 || p.stride_b == 0;
  const unsigned chunk = b_shared ? p.batch : (unsigned)std::min<size_t>(p.batch, std::max<size_t>(1, kNtWorkspaceCap / (km * es)));
  mm::Problem whole = p;   // the row-major problem the kernels see
  whole.b_transposed = false;
  whole.stride_b = b_shared ? 0 : km;
  const MatrixCore *mc = matrix_core(choose_batched(cfg, whole));
  const int kernel = mc ? mc->resolve(whole) : -1;
  if (kernel < 0) return nt_chunks(s, cfg, p, nt_demoted(cfg));   // (a knob changed between the check and here)
  Workspace ws{s, "hipFreeAsync (A x B^T workspace)"};
  bool full;
  int rc = ws.try_allocate((b_shared ? 1 : chunk) * km * es, &full);
  if (rc) return rc;
  if (full) return nt_chunks(s, cfg, p, nt_demoted(cfg));
  for (unsigned e0 = 0; e0 < p.batch && rc == MM_OK; e0 += chunk) {
    const mm::Problem src = batch_slice(p, e0, std::min(chunk, p.batch - e0), es);   // this chunk's elements
    if (e0 == 0 || !b_shared)
      rc = launch_status(mm::launch_transpose_batched(s, src.b, ws.bytes(), p.m, p.k, (unsigned)es, b_shared ? 1 : src.batch, p.stride_b, km),
                         cfg, "A x B^T ", "transposition pre-pass launch");
    if (rc) break;
    mm::Problem g = src;
    g.b = ws.bytes();
    g.b_transposed = false;
    g.stride_b = whole.stride_b;
    rc = for_each_chunk(g, es, batch_chunk(g), [&](const mm::Problem &q, unsigned) {
      return launch_status(mc->launch(s, q, kernel), cfg, "A x B^T ", "A x B^T product launch");
    });
  }
  return ws.release(rc);
}

int dispatch_nt(hipStream_t s, const mm_config_t &cfg, const mm::Problem &p, NtKernel ker) {
  (void)hipGetLastError();   // a stale error of the application's own calls must not be reported as this launch's
  mm::Problem q = p;
  if (q.batch == 1) q.stride_a = q.stride_b = q.stride_c = 0;
  return ker == NT_PREPASS ? dispatch_nt_prepass(s, cfg, q) : nt_chunks(s, cfg, q, ker);
}

// The kernel of a family that is one kernel whatever the shape (the matrix-core families name theirs by shape)
const char *family_name(Family f) {
  switch (f) {
    case FAM_HALF_WIDE: return "ordered_wide_f16";
    case FAM_VALU_TILE: return "valu_tile";
    case FAM_ORDERED_TILE: return "ordered_tile";   // k ascending, one accumulator, unfused: Naive's bits on 128 x 128 register tiles
    case FAM_NONE: return "unsupported";
    default: return "ordered";
  }
}

// hipEvent_t with a destructor: no exit path of the timed launch can leak one
struct Event {
  hipEvent_t e = nullptr;
  ~Event() { if (e) (void)hipEventDestroy(e); }
};

// The enqueue forms, once their arguments are checked: `nothing` to do returns without initialising the library, else
// dispatch(stream).
template <class F> int enqueue_on(void *stream, bool nothing, F &&dispatch) {
  if (nothing) return MM_OK;
  if (int rc = ensure_init()) return rc;
  return dispatch((hipStream_t)stream);
}

// The blocking forms (mm_*_launch), once their arguments are checked: `nothing` to do reports 0 s and touches no device,
// else dispatch(null stream) on `device` between two HIP events, synchronised; *elapsed = the time between them.
template <class F> int launch_timed(int device, bool nothing, double *elapsed, F &&dispatch) {
  if (nothing) {
    if (elapsed) *elapsed = 0.0;
    return MM_OK;
  }
  if (int rc = check_device(device)) return rc;
  MM_HIP(hipSetDevice(device));
  Event start, stop;
  MM_HIP(hipEventCreate(&start.e));
  MM_HIP(hipEventCreate(&stop.e));
  MM_HIP(hipEventRecord(start.e, nullptr));
  if (int rc = dispatch((hipStream_t)nullptr)) return rc;
  MM_HIP(hipEventRecord(stop.e, nullptr));
  MM_HIP(hipEventSynchronize(stop.e));
  if (elapsed) {
    float ms = 0.f;
    MM_HIP(hipEventElapsedTime(&ms, start.e, stop.e));
    *elapsed = 1e-3 * (double)ms;
  }
  return MM_OK;
}

// Where a checked call runs: the caller's stream (mm_*_enqueue), or `device`'s null stream, timed (mm_*_launch).  Each entry-point
// pair writes its body once, against a Target.
struct Target {
  bool timed;
  void *stream;
  int device;
  double *elapsed;
};
Target on_stream(void *stream) { return {false, stream, 0, nullptr}; }
Target timed_on(int device, double *elapsed) { return {true, nullptr, device, elapsed}; }
template <class F> int run(const Target &t, bool nothing, F &&dispatch) {
  return t.timed ? launch_timed(t.device, nothing, t.elapsed, dispatch) : enqueue_on(t.stream, nothing, dispatch);
}

// ---- the entry points' bodies: checks first (no device is touched before they pass), then the dispatch on the target -------------
int run_gemm(const Target &t, const mm_config_t *cfg, const void *a, const void *b, void *c, unsigned n, unsigned k, unsigned m) {
  if (int rc = t.timed ? check_device(t.device) : ensure_init()) return rc;   // (mm_gemm_launch: the device first, then the arguments)
  if (int rc = check_problem(cfg, a, b, c, n, k, m)) return rc;
  const mm::Problem p{a, b, c, n, k, m, cfg->layout_a == MM_A_TRANSPOSED};
  return run(t, false, [&](hipStream_t s) { return dispatch(s, *cfg, p); });
}

int run_batched(const Target &t, const mm_config_t *cfg, const mm::Problem &p) {   // p.seed: the accumulating calls
  Family fam;
  if (int rc = p.seed ? check_accumulate(cfg, p, &fam) : check_batched(cfg, p, &fam)) return rc;
  return run(t, fam == FAM_NONE, [&](hipStream_t s) { return dispatch_batched(s, *cfg, p, fam); });
}

// bt: the A x B^T form of the call (p.b is M x K per element)
int run_argreduce(const Target &t, const mm_config_t *cfg, mm::Problem p, int *c_index, int index_base, bool bt = false) {
  p.b_transposed = bt;
  ArKernel ker;
  if (int rc = check_argreduce(cfg, p, c_index, index_base, &ker)) return rc;
  return run(t, ker == AR_NONE, [&](hipStream_t s) { return dispatch_argreduce(s, *cfg, p, c_index, index_base, ker); });
}

int run_lse(const Target &t, const mm_config_t *cfg, mm::Problem p, bool bt = false) {
  p.b_transposed = bt;
  LseKernel ker;
  if (int rc = check_lse(cfg, p, &ker)) return rc;
  return run(t, ker == LSE_NONE, [&](hipStream_t s) { return dispatch_lse(s, *cfg, p, ker); });
}

int run_widen(const Target &t, const mm_config_t *cfg, const mm::Problem &p) {
  WidenKernel ker;
  if (int rc = check_widen(cfg, p, &ker)) return rc;
  return run(t, ker == WD_NONE, [&](hipStream_t s) { return dispatch_widen(s, *cfg, p, ker); });
}

int run_nt(const Target &t, const mm_config_t *cfg, mm::Problem p) {
  p.b_transposed = true;
  NtKernel ker;
  if (int rc = check_nt(cfg, p, &ker)) return rc;
  return run(t, ker == NT_NONE, [&](hipStream_t s) { return dispatch_nt(s, *cfg, p, ker); });
}

int run_closure(const Target &t, const mm_config_t *cfg, void *d, int *witness, unsigned n, unsigned batch, size_t stride_d) {
  unsigned block;   // 0: n or batch 0, nothing to do
  if (int rc = check_closure(cfg, d, witness, n, batch, stride_d, &block)) return rc;
  return run(t, block == 0, [&](hipStream_t s) { return dispatch_closure(s, *cfg, d, witness, n, batch, stride_d, block); });
}

int run_bits_gemm(const Target &t, const mm::BitsProblem &p) {
  BitsKernel ker;
  if (int rc = check_bits_product(p, bits_gemm_rules(p), &ker)) return rc;
  return run(t, ker == BITS_NONE, [&](hipStream_t s) { return dispatch_bits_gemm(s, p, ker); });
}

int run_bits_gf2(const Target &t, const mm::BitsProblem &p) {
  BitsKernel ker;
  if (int rc = check_bits_product(p, bits_gf2_rules(p), &ker)) return rc;
  return run(t, ker == BITS_NONE, [&](hipStream_t s) { return dispatch_bits_gf2(s, p, ker); });
}

int run_bits_count(const Target &t, int op, const mm::BitsProblem &p) {
  BitsKernel ker;
  if (int rc = check_bits_count(op, p, &ker)) return rc;
  return run(t, ker == BITS_NONE, [&](hipStream_t s) { return dispatch_bits_count(s, op, p, ker); });
}

// c.src rows x cols; c.dst the same in the other form, or (the transpose) cols x rows packed
int run_bits_convert(const Target &t, const mm::BitsConvert &c, BitsConversion how) {
  const BitsSide bytes{c.rows, c.cols, 1}, words{c.rows, bits_words(c.cols), 4}, turned{c.cols, bits_words(c.rows), 4};
  bool nothing;
  if (int rc = check_bits_convert(c, how == BITS_PACK ? bytes : words, how == BITS_PACK ? words : how == BITS_UNPACK ? bytes : turned,
                                  &nothing))
    return rc;
  return run(t, nothing, [&](hipStream_t s) { return dispatch_bits_convert(s, c, how); });
}

int run_bits_closure(const Target &t, void *d, unsigned n, size_t ldd, unsigned batch, size_t stride_d) {
  bool nothing;
  if (int rc = check_bits_closure(d, n, ldd, batch, stride_d, &nothing)) return rc;
  return run(t, nothing, [&](hipStream_t s) { return dispatch_bits_closure(s, (uint32_t *)d, n, ldd, batch, stride_d); });
}

}  // namespace

// One library-owned memory pool per device for stream-ordered workspace (the packed planes of MM_PATH_SPLIT, the
// partial tiles of the fp32 split-K launches): freed workspace stays cached between launches (release threshold
// "never") without touching the process's default pool, whose settings belong to the application.
// mm_release_workspace() trims it.
static hipMemPool_t g_workspace_pool[64] = {};
static std::mutex g_workspace_mu;
static int make_pool(int dev, hipMemPool_t &pool) {   // under g_workspace_mu
  if (pool) return 0;
  hipMemPoolProps props = {};
  props.allocType = hipMemAllocationTypePinned;
  props.handleTypes = hipMemHandleTypeNone;
  props.location.type = hipMemLocationTypeDevice;
  props.location.id = dev;
  hipError_t e = hipMemPoolCreate(&pool, &props);
  if (e != hipSuccess) { pool = nullptr; return (int)e; }
  unsigned long long keep = ~0ull;
  return (int)hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &keep);
}
int mm::workspace_pool(int dev, hipMemPool_t *out) {
  std::lock_guard<std::mutex> lock(g_workspace_mu);
  hipMemPool_t &pool = g_workspace_pool[dev & 63];
  if (int rc = make_pool(dev, pool)) return rc;
  *out = pool;
  return 0;
}

// Flags of the stream-K launches (mm_mfma_f32_streamk.inc: launch_streamk_arrive).  A flag is "raised" when it holds the
// launch's EPOCH, a process-wide 64-bit count that no two launches share, so flags never have to be lowered -- provided the
// memory they live in has never held anything but zeros and epochs.  Hence a second pool of this library's own that
// serves nothing else, every block of it cleared (stream-ordered) the first time its address is handed out.  That saves
// the fill kernel and its dependency gap in front of every launch (~10 us: 4 % of a 2560^3 product).  While the stream is
// being captured into a graph the block is cleared every time: a replay repeats the epoch it was captured with.
static hipMemPool_t g_flags_pool[64] = {};
static std::unordered_map<unsigned long long, size_t> g_flags_seen[64];   // address -> bytes cleared there
static unsigned long long g_flags_reserved[64] = {};                    // the pool's reserved bytes when last looked at
// Epochs start from a random 64-bit base per process: what is left in recycled memory -- a small integer,
// an index buffer, an epoch of another process -- cannot plausibly equal a live epoch even if a block were ever missed.
static unsigned long long flags_epoch_base() {
  std::random_device rd;
  return (((unsigned long long)rd() << 32) ^ (unsigned long long)rd() ^ (unsigned long long)std::chrono::steady_clock::now().time_since_epoch().count()) | (1ull << 62);
}
static std::atomic<unsigned long long> g_flags_epoch{flags_epoch_base()};
int mm::flags_alloc(int dev, hipStream_t s, size_t bytes, void **out, unsigned long long *epoch) {
  std::lock_guard<std::mutex> lock(g_workspace_mu);
  hipMemPool_t &pool = g_flags_pool[dev & 63];
  if (int rc = make_pool(dev, pool)) return rc;
  hipError_t e = hipMallocFromPoolAsync(out, bytes, pool, s);
  if (e != hipSuccess) return (int)e;
  hipStreamCaptureStatus capture = hipStreamCaptureStatusNone;
  if ((e = hipStreamIsCapturing(s, &capture)) != hipSuccess) { (void)hipFreeAsync(*out, s); return (int)e; }
  *epoch = g_flags_epoch.fetch_add(1, std::memory_order_relaxed);
  // The pool mapped or unmapped memory since the last look (the runtime may trim a pool by itself when the device runs
  // out of memory): an address seen before may be backed by fresh physical memory now -- forget what was cleared.
  unsigned long long reserved = 0;
  if (hipMemPoolGetAttribute(pool, hipMemPoolAttrReservedMemCurrent, &reserved) == hipSuccess && reserved != g_flags_reserved[dev & 63]) {
    g_flags_reserved[dev & 63] = reserved;
    g_flags_seen[dev & 63].clear();
  }
  // (a block handed out during capture is not recorded: whether the graph ever runs and clears it is not known here)
  const bool capturing = capture != hipStreamCaptureStatusNone;
  bool clear = capturing;
  if (!capturing) {
    size_t &cleared = g_flags_seen[dev & 63][(unsigned long long)(size_t)*out];   // 0 when the address is new
    if (cleared < bytes) { cleared = bytes; clear = true; }                        // new, or seen with fewer bytes
  }
  if (clear) {
    if ((e = hipMemsetAsync(*out, 0, bytes, s)) != hipSuccess) { (void)hipFreeAsync(*out, s); return (int)e; }
  }
  return 0;
}

int mm::device_compute_units(int dev) { return dev >= 0 && dev < 64 && g_device_cus[dev] > 0 ? g_device_cus[dev] : 256; }

int mm::workspace_release(int dev) {
  std::lock_guard<std::mutex> lock(g_workspace_mu);
  int rc = 0;
  if (hipMemPool_t pool = g_workspace_pool[dev & 63]) rc = (int)hipMemPoolTrimTo(pool, 0);
  if (hipMemPool_t pool = g_flags_pool[dev & 63]) {
    g_flags_seen[dev & 63].clear();   // what comes back from the driver after this is fresh memory again
    const int rf = (int)hipMemPoolTrimTo(pool, 0);
    if (!rc) rc = rf;
  }
  return rc;
}

int mm::tuning(mm::Tunable t) {
  std::call_once(g_tuning_once, tuning_init);
  return g_tuning[t].load(std::memory_order_relaxed);
}

static void kernel_info_for(const mm_config_t *cfg, const mm::Problem &p, mm_kernel_info_t *info);

extern "C" {

const char *mm_last_error(void) { return g_error; }

int mm_tuning_set(const char *name, int value) {
  std::call_once(g_tuning_once, tuning_init);
  for (int i = 0; name && i < mm::TUNE_COUNT; ++i)
    if (strcmp(name, kTuneName[i]) == 0) { g_tuning[i].store(value, std::memory_order_relaxed); return MM_OK; }
  return fail(MM_ERR_BAD_ARGUMENT, "unknown tuning knob '%s'", name ? name : "(null)");
}

int mm_tuning_get(const char *name, int *value) {
  for (int i = 0; name && value && i < mm::TUNE_COUNT; ++i)
    if (strcmp(name, kTuneName[i]) == 0) { *value = mm::tuning((mm::Tunable)i); return MM_OK; }
  return fail(MM_ERR_BAD_ARGUMENT, "unknown tuning knob '%s'", name ? name : "(null)");
}

size_t mm_dtype_size(mm_dtype_t dtype) {
  static const size_t sz[] = {4, 8, 2, 1, 1, 2, 2, 4, 4, 8, 8};
  return (dtype >= MM_DTYPE_F32 && dtype <= MM_DTYPE_U64) ? sz[dtype] : 0;
}

int mm_init(int *device_count) {
  int rc = ensure_init();
  if (device_count) *device_count = g_device_count;
  return rc;
}

int mm_alloc(int device, size_t bytes, void **device_ptr) {
  if (!device_ptr) return fail(MM_ERR_BAD_ARGUMENT, "device_ptr is null");
  int rc = check_device(device);
  if (rc) return rc;
  MM_HIP(hipSetDevice(device));
  MM_HIP(hipMalloc(device_ptr, bytes ? bytes : 1));
  return MM_OK;
}

int mm_free(int device, void *device_ptr) {
  int rc = check_device(device);
  if (rc) return rc;
  MM_HIP(hipSetDevice(device));
  MM_HIP(hipFree(device_ptr));
  return MM_OK;
}

int mm_release_workspace(int device) {
  int rc = check_device(device);
  if (rc) return rc;
  MM_HIP(hipSetDevice(device));
  MM_HIP(hipDeviceSynchronize());   // stream-ordered frees are complete: everything the pool holds is reclaimable
  MM_HIP((hipError_t)mm::workspace_release(device));
  return MM_OK;
}

int mm_device_pci_bus_id(int device, char *buffer, int length) {
  int rc = check_device(device);
  if (rc) return rc;
  if (!buffer || length < 13) return fail(MM_ERR_BAD_ARGUMENT, "mm_device_pci_bus_id needs a buffer of at least 13 bytes");
  MM_HIP(hipDeviceGetPCIBusId(buffer, length, device));
  return MM_OK;
}

int mm_device_max_grid_dim_y(int device, int *value) {
  int rc = check_device(device);
  if (rc) return rc;
  if (!value) return fail(MM_ERR_BAD_ARGUMENT, "mm_device_max_grid_dim_y needs a place for the value");
  MM_HIP(hipDeviceGetAttribute(value, hipDeviceAttributeMaxGridDimY, device));
  return MM_OK;
}

int mm_copy_to_device(int device, void *dst, const void *src, size_t bytes) {
  int rc = check_device(device);
  if (rc) return rc;
  if (bytes && (!dst || !src)) return fail(MM_ERR_BAD_ARGUMENT, "null pointer in copy");
  MM_HIP(hipSetDevice(device));
  MM_HIP(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
  return MM_OK;
}

int mm_copy_to_host(int device, void *dst, const void *src, size_t bytes) {
  int rc = check_device(device);
  if (rc) return rc;
  if (bytes && (!dst || !src)) return fail(MM_ERR_BAD_ARGUMENT, "null pointer in copy");
  MM_HIP(hipSetDevice(device));
  MM_HIP(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
  return MM_OK;
}

int mm_fill_device(int device, mm_dtype_t dtype, void *ptr, size_t elements, unsigned long long seed) {
  int rc = check_device(device);
  if (rc) return rc;
  if (!mm_dtype_size(dtype) || (elements && !ptr)) return fail(MM_ERR_BAD_ARGUMENT, "bad fill arguments");
  MM_HIP(hipSetDevice(device));
  int e = mm::launch_fill(nullptr, dtype, ptr, elements, seed);
  if (e) return hip_fail((hipError_t)e, "fill launch");
  MM_HIP(hipDeviceSynchronize());
  return MM_OK;
}

int mm_gemm_enqueue(void *hip_stream, const mm_config_t *cfg, const void *a, const void *b, void *c, unsigned n,
                    unsigned k, unsigned m) {
  return run_gemm(on_stream(hip_stream), cfg, a, b, c, n, k, m);
}

int mm_gemm_launch(int device, const mm_config_t *cfg, const void *a, const void *b, void *c, unsigned n, unsigned k,
                   unsigned m, double *elapsed_seconds) {
  return run_gemm(timed_on(device, elapsed_seconds), cfg, a, b, c, n, k, m);
}

int mm_gemm_batched_enqueue(void *hip_stream, const mm_config_t *cfg, const void *a, const void *b, void *c, unsigned n,
                            unsigned k, unsigned m, unsigned batch, size_t stride_a, size_t stride_b, size_t stride_c) {
  return run_batched(on_stream(hip_stream), cfg, batched_problem(cfg, a, b, c, n, k, m, batch, stride_a, stride_b, stride_c));
}

int mm_gemm_batched_launch(int device, const mm_config_t *cfg, const void *a, const void *b, void *c, unsigned n,
                           unsigned k, unsigned m, unsigned batch, size_t stride_a, size_t stride_b, size_t stride_c,
                           double *elapsed_seconds) {
  return run_batched(timed_on(device, elapsed_seconds), cfg, batched_problem(cfg, a, b, c, n, k, m, batch, stride_a, stride_b, stride_c));
}

int mm_gemm_batched_accumulate_enqueue(void *hip_stream, const mm_config_t *cfg, const void *a, const void *b, void *c,
                                       unsigned n, unsigned k, unsigned m, unsigned batch, size_t stride_a, size_t stride_b,
                                       size_t stride_c) {
  return run_batched(on_stream(hip_stream), cfg, batched_problem(cfg, a, b, c, n, k, m, batch, stride_a, stride_b, stride_c, true));
}

int mm_gemm_batched_accumulate_launch(int device, const mm_config_t *cfg, const void *a, const void *b, void *c, unsigned n,
                                      unsigned k, unsigned m, unsigned batch, size_t stride_a, size_t stride_b,
                                      size_t stride_c, double *elapsed_seconds) {
  return run_batched(timed_on(device, elapsed_seconds), cfg,
                     batched_problem(cfg, a, b, c, n, k, m, batch, stride_a, stride_b, stride_c, true));
}

// The single accumulating launch is a batch of one: the batched kernel mm_kernel_name_batched(cfg, n, k, m, 1) names.
int mm_gemm_accumulate_enqueue(void *hip_stream, const mm_config_t *cfg, const void *a, const void *b, void *c, unsigned n,
                               unsigned k, unsigned m) {
  return mm_gemm_batched_accumulate_enqueue(hip_stream, cfg, a, b, c, n, k, m, 1, 0, 0, 0);
}

int mm_gemm_accumulate_launch(int device, const mm_config_t *cfg, const void *a, const void *b, void *c, unsigned n,
                              unsigned k, unsigned m, double *elapsed_seconds) {
  return mm_gemm_batched_accumulate_launch(device, cfg, a, b, c, n, k, m, 1, 0, 0, 0, elapsed_seconds);
}

int mm_gemm_argreduce_enqueue(void *hip_stream, const mm_config_t *cfg, const void *a, const void *b, void *c, int *c_index,
                              unsigned n, unsigned k, unsigned m, unsigned batch, size_t stride_a, size_t stride_b,
                              size_t stride_c, int index_base, int accumulate) {
  return run_argreduce(on_stream(hip_stream), cfg,
                       batched_problem(cfg, a, b, c, n, k, m, batch, stride_a, stride_b, stride_c, accumulate != 0), c_index, index_base);
}

int mm_gemm_argreduce_launch(int device, const mm_config_t *cfg, const void *a, const void *b, void *c, int *c_index,
                             unsigned n, unsigned k, unsigned m, unsigned batch, size_t stride_a, size_t stride_b,
                             size_t stride_c, int index_base, int accumulate, double *elapsed_seconds) {
  return run_argreduce(timed_on(device, elapsed_seconds), cfg,
                       batched_problem(cfg, a, b, c, n, k, m, batch, stride_a, stride_b, stride_c, accumulate != 0), c_index, index_base);
}

int mm_gemm_logsumexp_enqueue(void *hip_stream, const mm_config_t *cfg, const void *a, const void *b, void *c, unsigned n,
                              unsigned k, unsigned m, unsigned batch, size_t stride_a, size_t stride_b, size_t stride_c,
                              int accumulate) {
  return run_lse(on_stream(hip_stream), cfg, batched_problem(cfg, a, b, c, n, k, m, batch, stride_a, stride_b, stride_c, accumulate != 0));
}

int mm_gemm_logsumexp_launch(int device, const mm_config_t *cfg, const void *a, const void *b, void *c, unsigned n,
                             unsigned k, unsigned m, unsigned batch, size_t stride_a, size_t stride_b, size_t stride_c,
                             int accumulate, double *elapsed_seconds) {
  return run_lse(timed_on(device, elapsed_seconds), cfg,
                 batched_problem(cfg, a, b, c, n, k, m, batch, stride_a, stride_b, stride_c, accumulate != 0));
}

int mm_widen_dtype(mm_dtype_t dtype) { return dtype == MM_DTYPE_F16 ? (int)MM_DTYPE_F32 : dtype == MM_DTYPE_I8 ? (int)MM_DTYPE_I32 : -1; }

int mm_gemm_widen_enqueue(void *hip_stream, const mm_config_t *cfg, const void *a, const void *b, void *c, unsigned n,
                          unsigned k, unsigned m, unsigned batch, size_t stride_a, size_t stride_b, size_t stride_c,
                          int accumulate) {
  return run_widen(on_stream(hip_stream), cfg, batched_problem(cfg, a, b, c, n, k, m, batch, stride_a, stride_b, stride_c, accumulate != 0));
}

int mm_gemm_widen_launch(int device, const mm_config_t *cfg, const void *a, const void *b, void *c, unsigned n, unsigned k,
                         unsigned m, unsigned batch, size_t stride_a, size_t stride_b, size_t stride_c, int accumulate,
                         double *elapsed_seconds) {
  return run_widen(timed_on(device, elapsed_seconds), cfg,
                   batched_problem(cfg, a, b, c, n, k, m, batch, stride_a, stride_b, stride_c, accumulate != 0));
}

int mm_gemm_nt_enqueue(void *hip_stream, const mm_config_t *cfg, const void *a, const void *bt, void *c, unsigned n, unsigned k,
                       unsigned m, unsigned batch, size_t stride_a, size_t stride_b, size_t stride_c, int accumulate) {
  return run_nt(on_stream(hip_stream), cfg, batched_problem(cfg, a, bt, c, n, k, m, batch, stride_a, stride_b, stride_c, accumulate != 0));
}

int mm_gemm_nt_launch(int device, const mm_config_t *cfg, const void *a, const void *bt, void *c, unsigned n, unsigned k,
                      unsigned m, unsigned batch, size_t stride_a, size_t stride_b, size_t stride_c, int accumulate,
                      double *elapsed_seconds) {
  return run_nt(timed_on(device, elapsed_seconds), cfg,
                batched_problem(cfg, a, bt, c, n, k, m, batch, stride_a, stride_b, stride_c, accumulate != 0));
}

int mm_gemm_argreduce_nt_enqueue(void *hip_stream, const mm_config_t *cfg, const void *a, const void *bt, void *c, int *c_index,
                                 unsigned n, unsigned k, unsigned m, unsigned batch, size_t stride_a, size_t stride_b,
                                 size_t stride_c, int index_base, int accumulate) {
  return run_argreduce(on_stream(hip_stream), cfg,
                       batched_problem(cfg, a, bt, c, n, k, m, batch, stride_a, stride_b, stride_c, accumulate != 0), c_index, index_base, true);
}

int mm_gemm_argreduce_nt_launch(int device, const mm_config_t *cfg, const void *a, const void *bt, void *c, int *c_index,
                                unsigned n, unsigned k, unsigned m, unsigned batch, size_t stride_a, size_t stride_b,
                                size_t stride_c, int index_base, int accumulate, double *elapsed_seconds) {
  return run_argreduce(timed_on(device, elapsed_seconds), cfg,
                       batched_problem(cfg, a, bt, c, n, k, m, batch, stride_a, stride_b, stride_c, accumulate != 0), c_index, index_base, true);
}

int mm_gemm_logsumexp_nt_enqueue(void *hip_stream, const mm_config_t *cfg, const void *a, const void *bt, void *c, unsigned n,
                                 unsigned k, unsigned m, unsigned batch, size_t stride_a, size_t stride_b, size_t stride_c,
                                 int accumulate) {
  return run_lse(on_stream(hip_stream), cfg, batched_problem(cfg, a, bt, c, n, k, m, batch, stride_a, stride_b, stride_c, accumulate != 0), true);
}

int mm_gemm_logsumexp_nt_launch(int device, const mm_config_t *cfg, const void *a, const void *bt, void *c, unsigned n,
                                unsigned k, unsigned m, unsigned batch, size_t stride_a, size_t stride_b, size_t stride_c,
                                int accumulate, double *elapsed_seconds) {
  return run_lse(timed_on(device, elapsed_seconds), cfg,
                 batched_problem(cfg, a, bt, c, n, k, m, batch, stride_a, stride_b, stride_c, accumulate != 0), true);
}

int mm_closure_enqueue(void *hip_stream, const mm_config_t *cfg, void *d, int *witness, unsigned n, unsigned batch,
                       size_t stride_d) {
  return run_closure(on_stream(hip_stream), cfg, d, witness, n, batch, stride_d);
}

int mm_closure_launch(int device, const mm_config_t *cfg, void *d, int *witness, unsigned n, unsigned batch, size_t stride_d,
                      double *elapsed_seconds) {
  return run_closure(timed_on(device, elapsed_seconds), cfg, d, witness, n, batch, stride_d);
}

int mm_bits_gemm_enqueue(void *hip_stream, const void *a, const void *b, void *c, unsigned n, unsigned k, unsigned m, size_t lda,
                         size_t ldb, size_t ldc, unsigned batch, size_t stride_a, size_t stride_b, size_t stride_c,
                         int accumulate) {
  return run_bits_gemm(on_stream(hip_stream), {(const uint32_t *)a, (const uint32_t *)b, (uint32_t *)c, n, k, m, lda, ldb, ldc, batch,
                                               stride_a, stride_b, stride_c, accumulate != 0});
}

int mm_bits_gemm_launch(int device, const void *a, const void *b, void *c, unsigned n, unsigned k, unsigned m, size_t lda, size_t ldb,
                        size_t ldc, unsigned batch, size_t stride_a, size_t stride_b, size_t stride_c, int accumulate,
                        double *elapsed_seconds) {
  return run_bits_gemm(timed_on(device, elapsed_seconds), {(const uint32_t *)a, (const uint32_t *)b, (uint32_t *)c, n, k, m, lda, ldb,
                                                           ldc, batch, stride_a, stride_b, stride_c, accumulate != 0});
}

int mm_bits_gf2_enqueue(void *hip_stream, const void *a, const void *b, void *c, unsigned n, unsigned k, unsigned m, size_t lda,
                        size_t ldb, size_t ldc, unsigned batch, size_t stride_a, size_t stride_b, size_t stride_c, int accumulate) {
  return run_bits_gf2(on_stream(hip_stream), {(const uint32_t *)a, (const uint32_t *)b, (uint32_t *)c, n, k, m, lda, ldb, ldc, batch,
                                              stride_a, stride_b, stride_c, accumulate != 0});
}

int mm_bits_gf2_launch(int device, const void *a, const void *b, void *c, unsigned n, unsigned k, unsigned m, size_t lda, size_t ldb,
                       size_t ldc, unsigned batch, size_t stride_a, size_t stride_b, size_t stride_c, int accumulate,
                       double *elapsed_seconds) {
  return run_bits_gf2(timed_on(device, elapsed_seconds), {(const uint32_t *)a, (const uint32_t *)b, (uint32_t *)c, n, k, m, lda, ldb,
                                                          ldc, batch, stride_a, stride_b, stride_c, accumulate != 0});
}

int mm_bits_closure_enqueue(void *hip_stream, void *d, unsigned n, size_t ldd, unsigned batch, size_t stride_d) {
  return run_bits_closure(on_stream(hip_stream), d, n, ldd, batch, stride_d);
}

int mm_bits_closure_launch(int device, void *d, unsigned n, size_t ldd, unsigned batch, size_t stride_d, double *elapsed_seconds) {
  return run_bits_closure(timed_on(device, elapsed_seconds), d, n, ldd, batch, stride_d);
}

int mm_bits_pack_enqueue(void *hip_stream, const void *bytes, void *packed, unsigned rows, unsigned cols, size_t ld_bytes,
                         size_t ld_packed, unsigned batch, size_t stride_bytes, size_t stride_packed) {
  return run_bits_convert(on_stream(hip_stream), {bytes, packed, rows, cols, ld_bytes, ld_packed, batch, stride_bytes, stride_packed}, BITS_PACK);
}

int mm_bits_pack_launch(int device, const void *bytes, void *packed, unsigned rows, unsigned cols, size_t ld_bytes, size_t ld_packed,
                        unsigned batch, size_t stride_bytes, size_t stride_packed, double *elapsed_seconds) {
  return run_bits_convert(timed_on(device, elapsed_seconds),
                          {bytes, packed, rows, cols, ld_bytes, ld_packed, batch, stride_bytes, stride_packed}, BITS_PACK);
}

int mm_bits_count_enqueue(void *hip_stream, int op, const void *a, const void *bt, void *c, unsigned n, unsigned k, unsigned m,
                          size_t lda, size_t ldbt, size_t ldc, unsigned batch, size_t stride_a, size_t stride_bt, size_t stride_c,
                          int accumulate) {
  return run_bits_count(on_stream(hip_stream), op, {(const uint32_t *)a, (const uint32_t *)bt, (uint32_t *)c, n, k, m, lda, ldbt, ldc,
                                                    batch, stride_a, stride_bt, stride_c, accumulate != 0});
}

int mm_bits_count_launch(int device, int op, const void *a, const void *bt, void *c, unsigned n, unsigned k, unsigned m, size_t lda,
                         size_t ldbt, size_t ldc, unsigned batch, size_t stride_a, size_t stride_bt, size_t stride_c, int accumulate,
                         double *elapsed_seconds) {
  return run_bits_count(timed_on(device, elapsed_seconds), op, {(const uint32_t *)a, (const uint32_t *)bt, (uint32_t *)c, n, k, m, lda,
                                                                ldbt, ldc, batch, stride_a, stride_bt, stride_c, accumulate != 0});
}

int mm_bits_transpose_enqueue(void *hip_stream, const void *src, void *dst, unsigned rows, unsigned cols, size_t ld_src,
                              size_t ld_dst, unsigned batch, size_t stride_src, size_t stride_dst) {
  return run_bits_convert(on_stream(hip_stream), {src, dst, rows, cols, ld_src, ld_dst, batch, stride_src, stride_dst}, BITS_TRANSPOSE);
}

int mm_bits_transpose_launch(int device, const void *src, void *dst, unsigned rows, unsigned cols, size_t ld_src, size_t ld_dst,
                             unsigned batch, size_t stride_src, size_t stride_dst, double *elapsed_seconds) {
  return run_bits_convert(timed_on(device, elapsed_seconds), {src, dst, rows, cols, ld_src, ld_dst, batch, stride_src, stride_dst},
                          BITS_TRANSPOSE);
}

int mm_bits_unpack_enqueue(void *hip_stream, const void *packed, void *bytes, unsigned rows, unsigned cols, size_t ld_packed,
                           size_t ld_bytes, unsigned batch, size_t stride_packed, size_t stride_bytes) {
  return run_bits_convert(on_stream(hip_stream), {packed, bytes, rows, cols, ld_packed, ld_bytes, batch, stride_packed, stride_bytes}, BITS_UNPACK);
}

int mm_bits_unpack_launch(int device, const void *packed, void *bytes, unsigned rows, unsigned cols, size_t ld_packed, size_t ld_bytes,
                          unsigned batch, size_t stride_packed, size_t stride_bytes, double *elapsed_seconds) {
  return run_bits_convert(timed_on(device, elapsed_seconds),
                          {packed, bytes, rows, cols, ld_packed, ld_bytes, batch, stride_packed, stride_bytes}, BITS_UNPACK);
}

// Rows per device of the N split: ceil(N / G) rounded up to whole tile rows of the kernel that will run on a slab of that
// height (mm_kernel_info's tile_n: 256 for the large fp32 default, 128 / 64 for the smaller geometries), so that only the last busy
// device owns a ragged tile row.  The one place this arithmetic lives: mm_row_slab() hands it to bench.py and partition.py.
static unsigned md_slab_rows(const mm_config_t &cfg, unsigned n, unsigned k, unsigned m, int device_count) {
  if (n == 0) return 0;
  const size_t base = ((size_t)n + device_count - 1) / device_count;
  // The tile height is a property of the kernel that runs on a slab of the FINAL height, which the rounding itself changes
  // (ADVICE r5): iterate to a fixed point -- tile of a slab of `rows` rows -> rows = ceil(N / G) rounded up to it -> ... -- and
  // if the geometry choice flips back and forth, round to the largest tile any candidate uses (256), which every smaller
  // one divides.  Depends on (configuration, shape, knobs) only: not on the current device, so that every rank of a
  // one-process-per-GPU job computes the same partition.
  auto tile_for = [&](unsigned rows) -> size_t {
    mm_kernel_info_t info = {};
    const mm::Problem p{nullptr, nullptr, nullptr, rows, k, m, cfg.layout_a == MM_A_TRANSPOSED, rows == n ? 0u : n};
    kernel_info_for(&cfg, p, &info);
    return info.tile_n ? info.tile_n : 128;
  };
  unsigned rows = (unsigned)std::min<size_t>(n, (base + 127) / 128 * 128);
  for (int it = 0; it < 4; ++it) {
    const size_t tile = tile_for(rows);
    const unsigned next = (unsigned)std::min<size_t>(n, (base + tile - 1) / tile * tile);
    if (next == rows) return rows;
    rows = next;
  }
  return (unsigned)std::min<size_t>(n, (base + 255) / 256 * 256);
}

int mm_row_slab(const mm_config_t *cfg, unsigned n, unsigned k, unsigned m, int device_count, int rank, unsigned *row0,
                unsigned *rows) {
  if (!valid_cfg(cfg) || !row0 || !rows) return fail(MM_ERR_BAD_ARGUMENT, "invalid arguments to mm_row_slab");
  if (device_count < 1 || rank < 0 || rank >= device_count)
    return fail(MM_ERR_BAD_ARGUMENT, "rank %d not in [0, device_count = %d)", rank, device_count);
  const unsigned slab = md_slab_rows(*cfg, n, k ? k : 1, m, device_count);
  *row0 = (unsigned)std::min<size_t>((size_t)rank * slab, n);
  *rows = std::min(slab, n - *row0);
  return MM_OK;
}

namespace {
// What one logical device of the N split owns; everything is released by the destructor, on every path.
struct SplitDevice {
  int phys = 0;                       // the HIP device this logical device runs on
  void *a = nullptr, *b = nullptr, *c = nullptr;
  unsigned row0 = 0, rows = 0;
  hipStream_t s = nullptr;
  hipEvent_t start = nullptr, stop = nullptr;   // around this device's launch, on its stream
  ~SplitDevice() {
    if (!a && !b && !c && !s && !start && !stop) return;
    (void)hipSetDevice(phys);
    if (s) (void)hipStreamSynchronize(s);
    if (start) (void)hipEventDestroy(start);
    if (stop) (void)hipEventDestroy(stop);
    if (a) (void)hipFree(a);
    if (b) (void)hipFree(b);
    if (c) (void)hipFree(c);
    if (s) (void)hipStreamDestroy(s);
  }
};
}  // namespace

int mm_gemm_multi_device(int device_count, const mm_config_t *cfg, const void *a_host, const void *b_host,
                         void *c_host, unsigned n, unsigned k, unsigned m, double *elapsed_seconds) {
  return mm_gemm_multi_device_timed(device_count, cfg, a_host, b_host, c_host, n, k, m, elapsed_seconds, nullptr, nullptr);
}

int mm_gemm_multi_device_timed(int device_count, const mm_config_t *cfg, const void *a_host, const void *b_host,
                               void *c_host, unsigned n, unsigned k, unsigned m, double *elapsed_seconds,
                               double *per_device_seconds, double *host_wall_seconds) {
  int rc = ensure_init();
  if (rc) return rc;
  rc = check_problem(cfg, a_host, b_host, c_host, n, k, m);
  if (rc) return rc;
  // MM_MD_VIRTUAL_DEVICES / "md_virtual_devices" = V > 0 (tests): up to V LOGICAL devices, dealt out over the physical ones
  // round-robin -- on a 1-GPU box all of them on device 0, each with its own stream, slabs and copy of B, the B fan-out
  // taking the peer-copy branch (device 0 -> device 0).  Every line below is the one a real G-GPU node runs.
  const int virt = mm::tuning(mm::TUNE_MD_VIRTUAL_DEVICES);
  const int limit = virt > 0 ? virt : g_device_count;
  if (device_count < 1 || device_count > limit)
    return fail(MM_ERR_BAD_ARGUMENT, "device_count %d not in [1, %d]", device_count, limit);
  if (per_device_seconds) std::fill(per_device_seconds, per_device_seconds + device_count, 0.0);
  if (host_wall_seconds) *host_wall_seconds = 0.0;
  if (n == 0 || m == 0) {   // an empty C: nothing to copy, launch or time (the single-device entry points do the same)
    if (elapsed_seconds) *elapsed_seconds = 0.0;
    return MM_OK;
  }
  const size_t es = mm_dtype_size(cfg->dtype);
  const bool kxn = cfg->layout_a == MM_A_TRANSPOSED;
  const unsigned slab = md_slab_rows(*cfg, n, k, m, device_count);
  std::vector<SplitDevice> devs(device_count);
  // independent row slabs: logical device g owns C[row0 : row0+rows, :] = A[row0 : row0+rows, :] . B
  // (kernel/Compute.cpp:53-60: no outer tile of C depends on another one)
  for (int g = 0; g < device_count; ++g) {
    SplitDevice &d = devs[g];
    d.phys = g % g_device_count;
    d.row0 = (unsigned)std::min<size_t>((size_t)g * slab, n);
    d.rows = std::min(slab, n - d.row0);
    MM_HIP(hipSetDevice(d.phys));
    MM_HIP(hipStreamCreateWithFlags(&d.s, hipStreamNonBlocking));
    if (!d.rows) continue;          // a trailing device without rows takes no part (and no copy of B)
    MM_HIP(hipEventCreate(&d.start));
    MM_HIP(hipEventCreate(&d.stop));
    MM_HIP(hipMalloc(&d.b, (size_t)k * m * es));
    MM_HIP(hipMalloc(&d.a, (size_t)d.rows * k * es));
    MM_HIP(hipMalloc(&d.c, (size_t)d.rows * m * es));
  }
  // B crosses PCIe ONCE (host -> device 0) and is then fanned out device 0 -> device g over xGMI
  // (every GPU has its own link to GPU 0, so the G-1 peer copies run concurrently), instead of G
  // pageable host copies through one root complex; the A slabs go up meanwhile.  A device that
  // cannot take the peer copy gets B from the host as before.
  Event b_on_dev0;
  MM_HIP(hipSetDevice(devs[0].phys));
  MM_HIP(hipEventCreateWithFlags(&b_on_dev0.e, hipEventDisableTiming));
  MM_HIP(hipMemcpyAsync(devs[0].b, b_host, (size_t)k * m * es, hipMemcpyHostToDevice, devs[0].s));
  MM_HIP(hipEventRecord(b_on_dev0.e, devs[0].s));
  for (int g = 0; g < device_count; ++g) {
    SplitDevice &d = devs[g];
    if (!d.rows) continue;
    MM_HIP(hipSetDevice(d.phys));
    if (g > 0) {
      bool peer = d.phys == devs[0].phys;          // the same physical device (virtual devices): a peer copy onto itself
      if (!peer) {
        int can = 0;
        peer = hipDeviceCanAccessPeer(&can, d.phys, devs[0].phys) == hipSuccess && can;
        if (peer) {
          const hipError_t en = hipDeviceEnablePeerAccess(devs[0].phys, 0);
          peer = en == hipSuccess || en == hipErrorPeerAccessAlreadyEnabled;
        }
        (void)hipGetLastError();  // "already enabled" / "no peer" are not errors of this call
      }
      if (peer) {
        MM_HIP(hipStreamWaitEvent(d.s, b_on_dev0.e, 0));
        MM_HIP(hipMemcpyPeerAsync(d.b, d.phys, devs[0].b, devs[0].phys, (size_t)k * m * es, d.s));
      } else {
        MM_HIP(hipMemcpyAsync(d.b, b_host, (size_t)k * m * es, hipMemcpyHostToDevice, d.s));
      }
    }
    if (!kxn) {   // rows [row0, row0 + rows) of a row-major A: one contiguous block
      MM_HIP(hipMemcpyAsync(d.a, (const char *)a_host + (size_t)d.row0 * k * es, (size_t)d.rows * k * es,
                            hipMemcpyHostToDevice, d.s));
    } else {      // the same rows of a K x N A (MM_TRANSPOSED_A, kernel/Memory.cpp:205-261): COLUMNS [row0, row0 + rows) of every
                  // one of its K rows -> a dense K x rows matrix on the device
      MM_HIP(hipMemcpy2DAsync(d.a, (size_t)d.rows * es, (const char *)a_host + (size_t)d.row0 * es, (size_t)n * es,
                              (size_t)d.rows * es, k, hipMemcpyHostToDevice, d.s));
    }
  }
  for (SplitDevice &d : devs) { MM_HIP(hipSetDevice(d.phys)); MM_HIP(hipStreamSynchronize(d.s)); }
  // untimed warm-up pass of the same launch: the first dispatch on a device loads the code object,
  // opts the kernel into its LDS size and ramps the clocks; paying that outside the timed region
  // makes this figure comparable with mm_gemm_launch's (whose callers warm up the same way).
  // pass 1 is the timed region (copies excluded, as RunHardware.cpp:161-180 does).  Every device's launch is bracketed by HIP
  // events on ITS stream: the job's time is the MAX over devices of that kernel time -- what ExecuteTask() would
  // report on the slowest device -- and the per-device figures say which device that was.  The host clock from the first
  // dispatch to the last completion is kept as a cross-check (it adds G launch latencies and G stream synchronisations).
  double elapsed = 0.0, wall = 0.0;
  for (int pass = 0; pass < 2; ++pass) {
    const auto t0 = std::chrono::steady_clock::now();
    for (SplitDevice &d : devs) {
      if (!d.rows) continue;
      MM_HIP(hipSetDevice(d.phys));
      // a row slab of the n-row job (n_total 0: the slab IS the job -- the same launch as mm_gemm_launch's)
      const mm::Problem p{d.a, d.b, d.c, d.rows, k, m, kxn, d.rows == n ? 0u : n};
      MM_HIP(hipEventRecord(d.start, d.s));
      rc = dispatch(d.s, *cfg, p);
      if (rc) return rc;
      MM_HIP(hipEventRecord(d.stop, d.s));
    }
    for (SplitDevice &d : devs) { MM_HIP(hipSetDevice(d.phys)); MM_HIP(hipStreamSynchronize(d.s)); }
    wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  }
  for (int g = 0; g < device_count; ++g) {
    SplitDevice &d = devs[g];
    if (!d.rows) continue;
    MM_HIP(hipSetDevice(d.phys));
    float ms = 0.f;
    MM_HIP(hipEventElapsedTime(&ms, d.start, d.stop));
    if (per_device_seconds) per_device_seconds[g] = 1e-3 * (double)ms;
    elapsed = std::max(elapsed, 1e-3 * (double)ms);
  }
  if (host_wall_seconds) *host_wall_seconds = wall;
  if (elapsed_seconds) *elapsed_seconds = elapsed;
  for (SplitDevice &d : devs) {
    if (!d.rows) continue;
    MM_HIP(hipSetDevice(d.phys));
    MM_HIP(hipMemcpy((char *)c_host + (size_t)d.row0 * m * es, d.c, (size_t)d.rows * m * es, hipMemcpyDeviceToHost));
  }
  return MM_OK;
}

int mm_set_default_config(const mm_config_t *cfg) {
  if (!valid_cfg(cfg)) return fail(MM_ERR_BAD_ARGUMENT, "invalid mm_config_t");
  std::lock_guard<std::mutex> lock(g_default_cfg_mutex);
  g_default_cfg = *cfg;
  return MM_OK;
}

// Host-pointer entry point.  Rows of C are independent (kernel/Compute.cpp:53-60), so large problems
// are pipelined in row slabs: while slab i is multiplied on a non-blocking stream, slab i+1 of A is
// copied in and finished slabs of C are copied out, hiding most of the PCIe time behind the kernel
// (float 16384^3: 120 ms one-shot -> see profiles/).  The arithmetic of a slab is the arithmetic of
// the same rows in a single launch (tests: row-slab property), so results do not depend on slabbing.
static int mm_run_host_pointers(const mm_config_t &cfg, const void *a, const void *b, void *c, unsigned n, unsigned k,
                                unsigned m) {
  int rc = check_device(0);
  if (rc) return rc;
  rc = check_problem(&cfg, a, b, c, n, k, m);
  if (rc) return rc;
  if (n == 0 || m == 0) return MM_OK;
  const size_t es = mm_dtype_size(cfg.dtype);
  MM_HIP(hipSetDevice(0));
  void *ad = nullptr, *bd = nullptr, *cd = nullptr;
  hipStream_t stream = nullptr;
  std::vector<hipEvent_t> done;
  auto cleanup = [&]() {
    for (hipEvent_t e : done) (void)hipEventDestroy(e);
    if (stream) (void)hipStreamDestroy(stream);
    if (ad) (void)hipFree(ad);
    if (bd) (void)hipFree(bd);
    if (cd) (void)hipFree(cd);
  };
#define MM_HIP_HP(call)                                               \
  do {                                                                \
    hipError_t e_ = (call);                                           \
    if (e_ != hipSuccess) { cleanup(); return hip_fail(e_, #call); }  \
  } while (0)
  MM_HIP_HP(hipMalloc(&ad, (size_t)n * k * es));
  MM_HIP_HP(hipMalloc(&bd, (size_t)k * m * es));
  MM_HIP_HP(hipMalloc(&cd, (size_t)n * m * es));
  MM_HIP_HP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
  MM_HIP_HP(hipMemcpy(bd, b, (size_t)k * m * es, hipMemcpyHostToDevice));
  // a K x N A is not row-sliceable; small problems are not worth slicing
  bool pipelined = cfg.layout_a == MM_A_ROW_MAJOR && (double)n * k * m >= 64.0 * 1024 * 1024 * 1024 && n >= 2048;
  if (pipelined) {   // a job that one launch would run as stream-K stays one launch: slabs could not reproduce its unit ranges
    const mm::Problem whole{nullptr, nullptr, nullptr, n, k, m, false};
    if (choose(cfg, whole) == FAM_MFMA_F32) {
      const int v = f32_variant_for(whole);
      if (v >= 0 && mm::mfma_f32_splitk(whole, v) == 0) pipelined = false;
    }
  }
  const unsigned slabs = pipelined ? 8 : 1;
  const unsigned slab_rows = ((n + slabs - 1) / slabs + 255) / 256 * 256;
  for (unsigned r0 = 0; r0 < n; r0 += slab_rows) {
    const unsigned rows = std::min(slab_rows, n - r0);
    const char *a_src = (const char *)a + (cfg.layout_a == MM_A_ROW_MAJOR ? (size_t)r0 * k * es : 0);
    char *a_dst = (char *)ad + (cfg.layout_a == MM_A_ROW_MAJOR ? (size_t)r0 * k * es : 0);
    MM_HIP_HP(hipMemcpy(a_dst, a_src, (size_t)(slabs == 1 ? n : rows) * k * es, hipMemcpyHostToDevice));
    mm::Problem p{a_dst, bd, (char *)cd + (size_t)r0 * m * es, slabs == 1 ? n : rows, k, m,
                  cfg.layout_a == MM_A_TRANSPOSED, slabs == 1 ? 0u : n};   // a row slab of the n-row job (or all of it)
    rc = dispatch(stream, cfg, p);
    if (rc) { cleanup(); return rc; }
    hipEvent_t e;
    MM_HIP_HP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    done.push_back(e);
    MM_HIP_HP(hipEventRecord(e, stream));
    if (slabs == 1) break;
  }
  size_t idx = 0;
  for (unsigned r0 = 0; r0 < n; r0 += slab_rows, ++idx) {
    const unsigned rows = slabs == 1 ? n : std::min(slab_rows, n - r0);
    MM_HIP_HP(hipEventSynchronize(done[idx]));
    MM_HIP_HP(hipMemcpy((char *)c + (size_t)r0 * m * es, (char *)cd + (size_t)r0 * m * es, (size_t)rows * m * es,
                        hipMemcpyDeviceToHost));
    if (slabs == 1) break;
  }
#undef MM_HIP_HP
  cleanup();
  return MM_OK;
}

int mm_gemm_host(const mm_config_t *cfg, const void *a, const void *b, void *c, unsigned n, unsigned k, unsigned m) {
  if (!valid_cfg(cfg)) return fail(MM_ERR_BAD_ARGUMENT, "invalid mm_config_t");
  return mm_run_host_pointers(*cfg, a, b, c, n, k, m);
}

void MatrixMultiplicationKernel(const void *a, const void *b, void *c, unsigned n, unsigned k, unsigned m) {
  const int rc = mm_run_host_pointers(default_cfg(), a, b, c, n, k, m);
  if (rc) {
    fprintf(stderr, "MatrixMultiplicationKernel failed: %s\n", mm_last_error());
    abort();  // the reference's symbol returns void; failing silently would fake a result
  }
}

int mm_config_supported(const mm_config_t *cfg) {
  if (!valid_cfg(cfg)) return 0;
  if (cfg->path == MM_PATH_SPLIT)
    return cfg->dtype == MM_DTYPE_F32 && cfg->map_op == MM_OP_MULTIPLY && cfg->reduce_op == MM_OP_ADD;
  return 1;
}

const char *mm_kernel_name(const mm_config_t *cfg, unsigned n, unsigned k, unsigned m) {
  if (!valid_cfg(cfg)) return "invalid";
  mm::Problem p{nullptr, nullptr, nullptr, n, k, m, cfg->layout_a == MM_A_TRANSPOSED};
  switch (const Family fam = choose(*cfg, p)) {
    // every family answers through the same resolver its launcher uses, so the name IS the kernel that runs
    case FAM_MFMA_F32: {
      const int v = f32_variant_for(p);
      return v < 0 ? "unsupported" : mm::mfma_f32_launch_name(p, v);
    }
    case FAM_MFMA_F64: return mm::mfma_f64_name(p);
    case FAM_MFMA_F16: return mm::mfma_f16_name(p);
    case FAM_MFMA_I8: return mm::mfma_i8_name(p);
    case FAM_F32_SPLIT: return "mfma_f32_split_bf16x3";
    default: return family_name(fam);
  }
}

const char *mm_kernel_name_batched(const mm_config_t *cfg, unsigned n, unsigned k, unsigned m, unsigned batch) {
  if (!valid_cfg(cfg)) return "invalid";
  const mm::Problem p = batched_problem(cfg, nullptr, nullptr, nullptr, n, k, m, batch ? batch : 1, 0, 0, 0);
  const Family fam = choose_batched(*cfg, p);
  const MatrixCore *mc = matrix_core(fam);   // the row dispatch_batched uses
  return mc ? mc->name(p) : family_name(fam);
}

static const char *argreduce_name(const mm_config_t *cfg, unsigned n, unsigned k, unsigned m, unsigned batch, bool bt) {
  if (!valid_cfg(cfg)) return "invalid";
  mm::Problem p = batched_problem(cfg, nullptr, nullptr, nullptr, n, k, m, batch ? batch : 1, 0, 0, 0);
  p.b_transposed = bt;
  switch (argreduce_kernel_for(*cfg, p)) {   // the choice check_argreduce makes, before alignment
    case AR_TILE: return bt ? "argreduce_tile_nt" : "argreduce_tile";
    case AR_PLAIN: return bt ? "argreduce_nt" : "argreduce";
    default: return "unsupported";
  }
}

const char *mm_kernel_name_argreduce(const mm_config_t *cfg, unsigned n, unsigned k, unsigned m, unsigned batch) {
  return argreduce_name(cfg, n, k, m, batch, false);
}

const char *mm_kernel_name_argreduce_nt(const mm_config_t *cfg, unsigned n, unsigned k, unsigned m, unsigned batch) {
  return argreduce_name(cfg, n, k, m, batch, true);
}

// (the choice is the configuration's and the knob's, not the shape's)
static const char *logsumexp_name(const mm_config_t *cfg, bool bt) {
  if (!valid_cfg(cfg)) return "invalid";
  bool bad_knob;
  const LseKernel ker = lse_kernel_for(*cfg, &bad_knob);   // the choice check_lse makes
  if (ker == LSE_NONE || (bt && cfg->layout_a == MM_A_TRANSPOSED)) return "unsupported";
  if (bad_knob) return "invalid";
  if (bt) return ker == LSE_HYBRID ? "lse_hybrid_nt" : "lse_exact_nt";
  return ker == LSE_HYBRID ? "lse_hybrid" : "lse_exact";
}

const char *mm_kernel_name_logsumexp(const mm_config_t *cfg, unsigned n, unsigned k, unsigned m, unsigned batch) {
  (void)n, (void)k, (void)m, (void)batch;
  return logsumexp_name(cfg, false);
}

const char *mm_kernel_name_logsumexp_nt(const mm_config_t *cfg, unsigned n, unsigned k, unsigned m, unsigned batch) {
  (void)n, (void)k, (void)m, (void)batch;
  return logsumexp_name(cfg, true);
}

const char *mm_kernel_name_widen(const mm_config_t *cfg, unsigned n, unsigned k, unsigned m, unsigned batch) {
  if (!valid_cfg(cfg)) return "invalid";
  if (!widen_serves(*cfg)) return "unsupported";
  const mm::Problem p = batched_problem(cfg, nullptr, nullptr, nullptr, n, k, m, batch ? batch : 1, 0, 0, 0);
  const char *wide = widen_mfma_name(*cfg, p);   // the choice check_widen makes, before alignment
  return wide ? wide : "widen_ordered";
}

const char *mm_kernel_name_nt(const mm_config_t *cfg, unsigned n, unsigned k, unsigned m, unsigned batch) {
  if (!valid_cfg(cfg)) return "invalid";
  if (!nt_serves(*cfg)) return "unsupported";
  const mm::Problem p = batched_problem(cfg, nullptr, nullptr, nullptr, n, k, m, batch ? batch : 1, 0, 0, 0);
  switch (nt_kernel_for(*cfg, p)) {   // the choice check_nt makes, before alignment
    case NT_PREPASS: return "nt_prepass";
    case NT_VALU_TILE: return "valu_tile_nt";
    case NT_NONE: return "unsupported";
    default: return "ordered_nt";
  }
}

const char *mm_kernel_name_closure(const mm_config_t *cfg, unsigned n, unsigned batch, int with_witness) {
  (void)batch;   // the batch is chunked, never a different kernel
  if (!valid_cfg(cfg)) return "invalid";
  if ((cfg->reduce_op != MM_OP_MIN && cfg->reduce_op != MM_OP_MAX) || cfg->path == MM_PATH_SPLIT) return "unsupported";
  const unsigned b = closure_block(*cfg, with_witness != 0);   // the choice check_closure makes
  if (cfg->layout_a == MM_A_TRANSPOSED || b == 0) return "invalid";
  return n <= b ? "closure_onchip" : "closure_blocked";
}

const char *mm_kernel_name_bits_gemm(unsigned n, unsigned k, unsigned m, size_t lda, size_t ldb, size_t ldc, unsigned batch) {
  (void)n, (void)k, (void)lda, (void)batch;   // the batch is chunked, never a different kernel
  switch (bits_kernel_for(m, ldb, ldc)) {     // the choice bits_gemm_rules makes, before alignment
    case BITS_TILE: return "bits_tile";
    case BITS_INVALID: return "invalid";
    default: return "bits_plain";
  }
}

const char *mm_kernel_name_bits_gf2(unsigned n, unsigned k, unsigned m, size_t lda, size_t ldb, size_t ldc, unsigned batch) {
  (void)k, (void)lda, (void)batch;
  switch (bits_gf2_kernel_for(n, m, ldb, ldc)) {   // the choice bits_gf2_rules makes, before alignment
    case BITS_TILE: return "bits_gf2_tile";
    case BITS_INVALID: return "invalid";
    default: return "bits_gf2_plain";
  }
}

const char *mm_kernel_name_bits_count(unsigned n, unsigned k, unsigned m, size_t lda, size_t ldbt, size_t ldc, unsigned batch) {
  (void)k, (void)batch;   // the batch is chunked, never a different kernel
  switch (bits_count_kernel_for(n, m, lda, ldbt, ldc)) {   // the choice bits_count_rules makes, before alignment
    case BITS_TILE: return "bits_count_tile";
    case BITS_INVALID: return "invalid";
    default: return "bits_count_plain";
  }
}

const char *mm_kernel_name_bits_closure(unsigned n, unsigned batch) {
  (void)batch;
  return n <= kBitsClosureBlock ? "bits_closure_onchip" : "bits_closure_blocked";
}

int mm_kernel_info(const mm_config_t *cfg, unsigned n, unsigned k, unsigned m, mm_kernel_info_t *info) {
  if (!valid_cfg(cfg) || !info) return fail(MM_ERR_BAD_ARGUMENT, "invalid arguments to mm_kernel_info");
  mm::Problem p{nullptr, nullptr, nullptr, n, k, m, cfg->layout_a == MM_A_TRANSPOSED};
  kernel_info_for(cfg, p, info);
  return MM_OK;
}

}  // extern "C"

static void kernel_info_for(const mm_config_t *cfg, const mm::Problem &p, mm_kernel_info_t *info) {
  mm_kernel_info_t r = {};
  // the CURRENT device's compute units once the library is initialised (not device 0's); the MI355X's 256 before
  int cur = 0;
  if (g_init_status != MM_OK || hipGetDevice(&cur) != hipSuccess) { (void)hipGetLastError(); cur = 0; }
  r.compute_units = (unsigned)mm::device_compute_units(cur);
  r.max_clock_mhz = 2400.0;
  const mm::KernelRow *row = nullptr;
  switch (choose(*cfg, p)) {
    case FAM_MFMA_F32:
      mm::mfma_f32_geometry(f32_variant_for(p), &r.tile_n, &r.tile_m, &r.tile_k, &r.wavefronts);
      r.inst_n = 32; r.inst_m = 32; r.inst_k = 2; r.ops_per_clk_per_cu = 256.0;   // 64 FLOP/clk/SIMD
      r.measured_issue_efficiency = 0.967;  // 152.2 TF of 157.3 (profiles/r02z_f32_scalar_base_dma.log)
      break;
    // the other matrix-core families: the resolved kernel's row of the family's table
    case FAM_MFMA_F64: row = &mm::mfma_f64_row(p); r.ops_per_clk_per_cu = 128.0; break;
    case FAM_MFMA_F16: row = &mm::mfma_f16_row(p); r.ops_per_clk_per_cu = 4096.0; break;
    case FAM_MFMA_I8: row = &mm::mfma_i8_row(p); r.ops_per_clk_per_cu = 8192.0; break;
    case FAM_F32_SPLIT:
      {  // the 128 x 128 geometry runs only in the launcher's default branch (no schedule / product / flush bits set)
        const int sv = mm::tuning(mm::TUNE_SPLIT_VARIANT);
        const bool plain = sv <= 0 || (sv & (1 | 2 | 4 | 64 | 128)) == 0;
        r.tile_n = r.tile_m = plain ? (unsigned)mm::mfma_f32_split_tile(p, sv) : 256u;
      }
      r.tile_k = 16; r.wavefronts = r.tile_n == 256 ? 8 : 4;
      r.inst_n = 32; r.inst_m = 32; r.inst_k = 16;
      r.ops_per_clk_per_cu = 4096.0 / 6.0;  // six bf16 MFMAs per fp32 multiply-add block
      r.measured_issue_efficiency = 0.90;
      break;
    case FAM_ORDERED_TILE: {
      r.tile_n = 128; r.tile_m = 128; r.tile_k = (unsigned)(64 / mm_dtype_size(cfg->dtype)); r.wavefronts = mm_dtype_size(cfg->dtype) == 8 ? 8 : 4;
      r.inst_n = 1; r.inst_m = 64; r.inst_k = 1;
      // one instruction per operation (multiply and add are NOT fused here).  4-byte types: 2-cycle issue, 128 operations per
      // clock per CU; half: v_pk_mul_f16 / v_pk_add_f16 take two elements per lane but issue every 4 cycles (measured 4.30:
      // profiles/r06a_probe_valu_issue_rates_unfused_pairs.txt) -- the same 128; 8-byte types: 4-cycle issue, 64
      r.ops_per_clk_per_cu = mm_dtype_size(cfg->dtype) == 8 ? 64.0 : 128.0;
      r.measured_issue_efficiency = cfg->dtype == MM_DTYPE_F16 ? 0.94 : 0.74;   // half 74.4 / float 58.4 / double 28.9 TOp/s at 8192^3 (r06a)
      break;
    }
    case FAM_VALU_TILE: {
      r.tile_n = 128; r.tile_m = 128; r.tile_k = 16; r.wavefronts = 4;
      r.inst_n = 1; r.inst_m = 64; r.inst_k = 1;
      // 128 lane-instructions per clock per CU; a map+reduce step (2 ops) costs 2 instructions,
      // 1 when it fuses (float multiply-add), 1.5 for float min/max reductions (v_min3/v_max3)
      const bool fp = cfg->dtype == MM_DTYPE_F32 || cfg->dtype == MM_DTYPE_F16;
      const bool fma = cfg->map_op == MM_OP_MULTIPLY && cfg->reduce_op == MM_OP_ADD && (fp || cfg->dtype == MM_DTYPE_F64);
      const bool m3 = fp && (cfg->reduce_op == MM_OP_MIN || cfg->reduce_op == MM_OP_MAX);
      r.ops_per_clk_per_cu = fma ? 256.0 : (m3 ? 128.0 * 4.0 / 3.0 : 128.0);
      r.measured_issue_efficiency = 0.65;   // against 2-cycle issue; min/max instructions take 4.2 (profiles/r02_probe_valu_*)
      break;
    }
    default:
      r.tile_n = 64; r.tile_m = 64; r.tile_k = 16; r.wavefronts = 4;
      r.inst_n = 1; r.inst_m = 64; r.inst_k = 1; r.ops_per_clk_per_cu = 128.0;
      break;
  }
  if (row) {
    r.tile_n = row->tile_n; r.tile_m = row->tile_m; r.tile_k = row->tile_k; r.wavefronts = row->wavefronts;
    r.inst_n = row->inst_n; r.inst_m = row->inst_m; r.inst_k = row->inst_k;
    r.measured_issue_efficiency = row->measured_issue_efficiency;
  }
  *info = r;
}
