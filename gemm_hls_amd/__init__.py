"""gemm_hls_amd -- MI355X (gfx950) implementation of spcl/gemm_hls's hot path
C = A (map, reduce) B behind the reference's own boundary.

The product is the C-ABI shared library ``libmm_gemm_amd.so`` (``include/mm_gemm.h``) and the C++
host runner ``bin/RunHardware.exe``.  This module is the thin Python binding used by the tests
and ``bench.py``: ctypes onto the C ABI, with PyTorch only as plumbing for device memory, streams
and ``torch.distributed``.  There is no CPU fallback: importing works without a GPU (so the
symbol checks can run), every compute call raises ``MMError`` without one.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmm_gemm_amd.so")

# numerically identical to include/mm_gemm.h (asserted by tests/test_capi_symbols.py)
DTYPES = {"float": 0, "double": 1, "half": 2, "int8_t": 3, "uint8_t": 4, "int16_t": 5,
          "uint16_t": 6, "int": 7, "unsigned": 8, "long": 9, "unsigned long": 10}
OPS = {"Add": 0, "Multiply": 1, "And": 2, "Min": 3, "Max": 4}
PATH_AUTO, PATH_ORDERED, PATH_SPLIT = 0, 1, 2

EXPORTS = ["mm_init", "mm_alloc", "mm_free", "mm_copy_to_device", "mm_copy_to_host",
           "mm_fill_device", "mm_gemm_launch", "mm_gemm_enqueue", "mm_gemm_multi_device",
           "MatrixMultiplicationKernel", "mm_set_default_config", "mm_dtype_size",
           "mm_config_supported", "mm_kernel_name", "mm_kernel_info", "mm_last_error",
           "mm_gemm_host", "mm_tuning_set", "mm_tuning_get", "mm_release_workspace", "mm_device_pci_bus_id",
           "mm_row_slab", "mm_gemm_multi_device_timed", "mm_gemm_batched_enqueue", "mm_gemm_batched_launch",
           "mm_kernel_name_batched", "mm_gemm_accumulate_enqueue", "mm_gemm_accumulate_launch",
           "mm_gemm_batched_accumulate_enqueue", "mm_gemm_batched_accumulate_launch", "mm_gemm_argreduce_enqueue",
           "mm_gemm_argreduce_launch", "mm_kernel_name_argreduce", "mm_closure_enqueue", "mm_closure_launch",
           "mm_kernel_name_closure", "mm_gemm_logsumexp_enqueue", "mm_gemm_logsumexp_launch", "mm_kernel_name_logsumexp",
           "mm_gemm_widen_enqueue", "mm_gemm_widen_launch", "mm_kernel_name_widen", "mm_widen_dtype",
           "mm_gemm_nt_enqueue", "mm_gemm_nt_launch", "mm_kernel_name_nt", "mm_gemm_argreduce_nt_enqueue",
           "mm_gemm_argreduce_nt_launch", "mm_kernel_name_argreduce_nt", "mm_gemm_logsumexp_nt_enqueue",
           "mm_gemm_logsumexp_nt_launch", "mm_kernel_name_logsumexp_nt", "mm_bits_gemm_enqueue", "mm_bits_gemm_launch",
           "mm_kernel_name_bits_gemm", "mm_bits_closure_enqueue", "mm_bits_closure_launch", "mm_kernel_name_bits_closure",
           "mm_bits_pack_enqueue", "mm_bits_pack_launch", "mm_bits_unpack_enqueue", "mm_bits_unpack_launch",
           "mm_bits_count_enqueue", "mm_bits_count_launch", "mm_kernel_name_bits_count", "mm_bits_transpose_enqueue",
           "mm_bits_transpose_launch", "mm_device_max_grid_dim_y"]
# what include/mm_bits_gf2.h declares (included by mm_gemm.h; asserted by tests/test_bits_gf2_capi.py).  A list of its own:
# EXPORTS is pinned, symbol for symbol, against mm_gemm.h's own declarations and a literal prototype table
BITS_GF2_EXPORTS = ["mm_bits_gf2_enqueue", "mm_bits_gf2_launch", "mm_kernel_name_bits_gf2"]


class MMError(RuntimeError):
    pass


class Config(ctypes.Structure):
    _fields_ = [("dtype", ctypes.c_int), ("map_op", ctypes.c_int), ("reduce_op", ctypes.c_int),
                ("path", ctypes.c_int), ("layout_a", ctypes.c_int)]


class KernelInfo(ctypes.Structure):  # mm_kernel_info_t
    _fields_ = [("tile_n", ctypes.c_uint), ("tile_m", ctypes.c_uint), ("tile_k", ctypes.c_uint),
                ("wavefronts", ctypes.c_uint), ("inst_n", ctypes.c_uint), ("inst_m", ctypes.c_uint),
                ("inst_k", ctypes.c_uint), ("ops_per_clk_per_cu", ctypes.c_double),
                ("compute_units", ctypes.c_uint), ("max_clock_mhz", ctypes.c_double),
                ("measured_issue_efficiency", ctypes.c_double)]


_lib = None


def lib():
    """The loaded C-ABI library.  Raises (never falls back) if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise MMError(f"{LIB_PATH} is missing: run `python gemm_hls_amd/build.py` "
                          "(or __graft_entry__.build()); there is no fallback implementation")
        # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64 (same SONAME as
        # /opt/rocm's).  Whichever is loaded first serves both, but if THIS library came first and
        # torch then brought a second runtime, the second HSA initialisation finds no device
        # ("no ROCm-capable device is detected").  So torch -- the plumbing for device memory and
        # streams in this binding anyway -- is imported first whenever it is installed.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = ctypes.CDLL(LIB_PATH)
        vp, u, i, sz = ctypes.c_void_p, ctypes.c_uint, ctypes.c_int, ctypes.c_size_t
        cfgp, dp = ctypes.POINTER(Config), ctypes.POINTER(ctypes.c_double)
        L.mm_init.argtypes = [ctypes.POINTER(i)]
        L.mm_alloc.argtypes = [i, sz, ctypes.POINTER(vp)]
        L.mm_free.argtypes = [i, vp]
        L.mm_copy_to_device.argtypes = [i, vp, vp, sz]
        L.mm_copy_to_host.argtypes = [i, vp, vp, sz]
        L.mm_fill_device.argtypes = [i, i, vp, sz, ctypes.c_ulonglong]
        # Every <stem>_enqueue(stream, ...) has a blocking <stem>_launch(device, ..., double *elapsed_seconds): the arguments
        # between, once per pair
        gemm = [cfgp, vp, vp, vp, u, u, u]                  # a, b, c, n, k, m
        batched = gemm + [u, sz, sz, sz]                    # ..., batch, stride_a, stride_b, stride_c
        seeded = batched + [i]                              # ..., accumulate
        argreduce = [cfgp, vp, vp, vp, vp] + batched[4:] + [i, i]   # a, b, c, c_index, ..., index_base, accumulate
        convert = [vp, vp, u, u, sz, sz, u, sz, sz]
        pairs = {"mm_gemm": gemm, "mm_gemm_accumulate": gemm, "mm_gemm_batched": batched, "mm_gemm_batched_accumulate": batched,
                 "mm_gemm_argreduce": argreduce, "mm_gemm_argreduce_nt": argreduce, "mm_gemm_logsumexp": seeded,
                 "mm_gemm_logsumexp_nt": seeded, "mm_gemm_widen": seeded, "mm_gemm_nt": seeded,
                 "mm_closure": [cfgp, vp, vp, u, u, sz], "mm_bits_gemm": [vp, vp, vp, u, u, u, sz, sz, sz, u, sz, sz, sz, i],
                 "mm_bits_closure": [vp, u, sz, u, sz], "mm_bits_pack": convert, "mm_bits_unpack": convert,
                 "mm_bits_count": [i, vp, vp, vp, u, u, u, sz, sz, sz, u, sz, sz, sz, i], "mm_bits_transpose": convert}
        pairs["mm_bits_gf2"] = pairs["mm_bits_gemm"]
        for stem, between in pairs.items():
            getattr(L, stem + "_enqueue").argtypes = [vp] + between
            getattr(L, stem + "_launch").argtypes = [i] + between + [dp]
        # mm_kernel_name<suffix>(...): a string
        shape = [cfgp, u, u, u]
        names = {"": shape, "_closure": [cfgp, u, u, i], "_bits_gemm": [u, u, u, sz, sz, sz, u], "_bits_closure": [u, u],
                 "_bits_count": [u, u, u, sz, sz, sz, u], "_bits_gf2": [u, u, u, sz, sz, sz, u]}
        names.update((suffix, shape + [u]) for suffix in ("_batched", "_argreduce", "_logsumexp", "_widen", "_nt", "_argreduce_nt",
                                                          "_logsumexp_nt"))
        for suffix, args in names.items():
            fn = getattr(L, "mm_kernel_name" + suffix)
            fn.argtypes, fn.restype = args, ctypes.c_char_p
        L.mm_gemm_multi_device.argtypes = [i] + gemm + [dp]
        L.mm_gemm_multi_device_timed.argtypes = [i] + gemm + [dp, dp, dp]
        L.MatrixMultiplicationKernel.argtypes = [vp, vp, vp, u, u, u]
        L.MatrixMultiplicationKernel.restype = None
        L.mm_set_default_config.argtypes = [cfgp]
        L.mm_dtype_size.argtypes = [i]
        L.mm_dtype_size.restype = sz
        L.mm_config_supported.argtypes = [cfgp]
        L.mm_kernel_info.argtypes = shape + [ctypes.POINTER(KernelInfo)]
        L.mm_last_error.restype = ctypes.c_char_p
        L.mm_gemm_host.argtypes = gemm
        L.mm_tuning_set.argtypes = [ctypes.c_char_p, i]
        L.mm_tuning_get.argtypes = [ctypes.c_char_p, ctypes.POINTER(i)]
        L.mm_release_workspace.argtypes = [i]
        L.mm_device_pci_bus_id.argtypes = [i, ctypes.c_char_p, i]
        L.mm_device_max_grid_dim_y.argtypes = [i, ctypes.POINTER(i)]
        L.mm_row_slab.argtypes = shape + [i, i, ctypes.POINTER(u), ctypes.POINTER(u)]
        L.mm_widen_dtype.argtypes = [i]
        _lib = L
    return _lib


def _check(rc):
    if rc != 0:
        raise MMError(f"mm_gemm status {rc}: {lib().mm_last_error().decode()}")


def _enqueue(device, fn, *args):
    """fn(stream, *args) on torch's current stream of `device`, with `device` current: the C ABI's enqueue forms launch on
    the current device."""
    import torch
    with torch.cuda.device(device):
        _check(fn(ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream), *args))


def _output(x, name, shape, dtype, device):
    """The caller's output `x`, checked, or a new one: a contiguous `dtype` tensor of `shape` on `device`."""
    if x is None:
        import torch
        return torch.empty(shape, dtype=dtype, device=device)
    if tuple(x.shape) != shape or x.dtype != dtype or x.device != device or not x.is_contiguous():
        raise MMError(f"{name} must be a contiguous {dtype} tensor of shape {shape} on {device}; got "
                      f"{tuple(x.shape)}, {x.dtype}, {x.device}, contiguous={x.is_contiguous()}")
    return x


def make_config(dtype="float", map_op="Multiply", reduce_op="Add", path=PATH_AUTO, transposed_a=False):
    return Config(DTYPES[dtype], OPS[map_op], OPS[reduce_op], path, int(transposed_a))


def device_count():
    n = ctypes.c_int(0)
    _check(lib().mm_init(ctypes.byref(n)))
    return n.value


def device_max_grid_dim_y(device=0):
    """The largest gridDim.y HIP device `device` launches (mm_device_max_grid_dim_y)."""
    v = ctypes.c_int(0)
    _check(lib().mm_device_max_grid_dim_y(int(device), ctypes.byref(v)))
    return v.value


def _kernel_name(suffix, cfg, *args):
    return getattr(lib(), "mm_kernel_name" + suffix)(ctypes.byref(cfg), *args).decode()


def _batched_kernel_name(suffix):
    """kernel_name<suffix>(cfg, n, k, m, batch=1): the kernel the calls of that family run."""
    def name(cfg, n, k, m, batch=1):
        return _kernel_name(suffix, cfg, n, k, m, batch)
    name.__name__ = name.__qualname__ = "kernel_name" + suffix
    return name


def kernel_name(cfg, n, k, m):
    return _kernel_name("", cfg, n, k, m)


def kernel_name_batched(cfg, n, k, m, batch):
    return _kernel_name("_batched", cfg, n, k, m, batch)


def kernel_name_closure(cfg, n, batch=1, with_witness=False):
    return _kernel_name("_closure", cfg, n, batch, int(bool(with_witness)))


kernel_name_argreduce = _batched_kernel_name("_argreduce")
kernel_name_logsumexp = _batched_kernel_name("_logsumexp")
kernel_name_widen = _batched_kernel_name("_widen")
kernel_name_nt = _batched_kernel_name("_nt")
kernel_name_argreduce_nt = _batched_kernel_name("_argreduce_nt")
kernel_name_logsumexp_nt = _batched_kernel_name("_logsumexp_nt")


def widen_dtype(dtype):
    """Name of C's type in the widening calls for operands of `dtype`: "float" for "half", "int" for "int8_t"; None for every
    other type (mm_widen_dtype)."""
    code = lib().mm_widen_dtype(DTYPES[dtype])
    return next((name for name, value in DTYPES.items() if value == code), None)


def set_tuning(name, value):
    """Tuning knob of the library ("f32_variant", "f16_variant", "band_rows", ...; -1 = default)."""
    _check(lib().mm_tuning_set(name.encode(), int(value)))


def get_tuning(name):
    v = ctypes.c_int(0)
    _check(lib().mm_tuning_get(name.encode(), ctypes.byref(v)))
    return v.value


def kernel_info(cfg, n, k, m):
    info = KernelInfo()
    _check(lib().mm_kernel_info(ctypes.byref(cfg), n, k, m, ctypes.byref(info)))
    return info


_TORCH_DTYPES = None


def torch_dtype(dtype):
    global _TORCH_DTYPES
    import torch
    if _TORCH_DTYPES is None:
        _TORCH_DTYPES = {"float": torch.float32, "double": torch.float64, "half": torch.float16,
                         "int8_t": torch.int8, "uint8_t": torch.uint8, "int16_t": torch.int16,
                         "uint16_t": torch.uint16, "int": torch.int32, "unsigned": torch.uint32,
                         "long": torch.int64, "unsigned long": torch.uint64}
    return _TORCH_DTYPES[dtype]


def _device_operands(what, tdt, *xs):
    """The checks every torch entry point makes: device tensors of one device and of the configuration's dtype."""
    if not all(x.is_cuda for x in xs):
        raise MMError(f"{what} needs device tensors: there is no CPU path")
    if any(x.device != xs[0].device for x in xs):
        raise MMError(f"operands live on different devices: {', '.join(str(x.device) for x in xs)}")
    if any(x.dtype != tdt for x in xs):
        raise MMError(f"operand dtypes {', '.join(str(x.dtype) for x in xs)} do not match {tdt}")


def _inner_mismatch(a, b, transposed_a=False, nt=False):
    return MMError(f"inner dimensions differ: A {tuple(a.shape)}{' (K x N)' if transposed_a else ''}, B {tuple(b.shape)}"
                   f"{' (M, K)' if nt else ''}")


def _matrix_shapes(what, transposed_a, a, b, *c):
    """(n, k, m) of matmul's and addmm_'s operands, which the single-launch calls take 2-D and contiguous only."""
    if any(x.dim() != 2 for x in (a, b) + c):
        raise MMError(f"{what} takes 2-D operands")
    if not all(x.is_contiguous() for x in (a, b) + c):
        raise MMError(f"{what} needs contiguous (row-major) operands")
    k, m = b.shape
    n, ka = reversed(a.shape) if transposed_a else a.shape
    if ka != k:
        raise _inner_mismatch(a, b, transposed_a)
    return n, k, m


def matmul(a, b, dtype="float", map_op="Multiply", reduce_op="Add", path=PATH_AUTO, transposed_a=False,
           out=None):
    """C = A (map, reduce) B on the current CUDA(HIP) device and torch's current stream.
    a: (N, K) -- or (K, N) with transposed_a -- b: (K, M); contiguous device tensors whose torch
    dtype matches `dtype`.  Asynchronous, like any torch op."""
    tdt = torch_dtype(dtype)
    _device_operands("matmul", tdt, a, b)
    n, k, m = _matrix_shapes("matmul", transposed_a, a, b)
    out = _output(out, "out", (n, m), tdt, a.device)
    cfg = make_config(dtype, map_op, reduce_op, path, transposed_a)
    _enqueue(a.device, lib().mm_gemm_enqueue, ctypes.byref(cfg), a.data_ptr(), b.data_ptr(), out.data_ptr(), n, k, m)
    return out


def _batched_operand(x, name, rows, cols):
    """(batch or None, batch stride in elements) of a 2-D or 3-D operand whose matrices are dense row-major."""
    if x.dim() == 2:
        if tuple(x.shape) != (rows, cols):
            raise MMError(f"{name} has shape {tuple(x.shape)}, expected {(rows, cols)}")
        if not x.is_contiguous():
            raise MMError(f"{name} must be a dense row-major matrix")
        return None, 0
    if x.dim() != 3 or tuple(x.shape[1:]) != (rows, cols):
        raise MMError(f"{name} has shape {tuple(x.shape)}, expected (B, {rows}, {cols}) or {(rows, cols)}")
    if (rows > 1 and x.stride(1) != cols) or (cols > 1 and x.stride(2) != 1):
        raise MMError(f"each matrix of {name} must be dense row-major (strides {x.stride()})")
    if x.stride(0) < 0:
        raise MMError(f"{name} has a negative batch stride")
    return x.shape[0], (0 if x.shape[0] == 1 else x.stride(0))


def _shapes(what, a, b, transposed_a=False, nt=False):
    """(n, k, m, batch, stride_a, stride_b) of bmm-style operands: 2-D, 3-D, or expanded with batch stride 0.  a: (N, K), or
    (K, N) with transposed_a; b: (K, M), or (M, K) with nt (the A x B^T forms)."""
    if a.dim() not in (2, 3) or b.dim() not in (2, 3):
        raise MMError(f"{what} takes 2-D or 3-D operands")
    n, ka = reversed(a.shape[-2:]) if transposed_a else a.shape[-2:]
    m, k = reversed(b.shape[-2:]) if not nt else b.shape[-2:]
    if ka != k:
        raise _inner_mismatch(a, b, transposed_a, nt)
    ba, sa = _batched_operand(a, "a", *a.shape[-2:])
    bb, sb = _batched_operand(b, "b (M, K)" if nt else "b", *b.shape[-2:])
    batches = {x for x in (ba, bb) if x is not None and x != 1}
    if len(batches) > 1:
        raise MMError(f"batch sizes differ: {ba} and {bb}")
    return n, k, m, (batches.pop() if batches else 1), sa, sb


def _inplace_batch(c, n, m, batch):
    """(batch, stride_c) of an in-place C over bmm-style operands of `batch`: C's own batch, over which a one-matrix A and
    B broadcast."""
    bc, sc = _batched_operand(c, "c", n, m)
    if batch not in (1, bc or 1):
        raise MMError(f"c has shape {tuple(c.shape)}, expected ({batch}, {n}, {m})")
    batch = bc or 1
    if batch > 1 and sc == 0:
        raise MMError(f"c has batch stride 0: the {batch} outputs would overlap")
    return batch, sc


def _widen_types(what, dtype):
    wide = widen_dtype(dtype)
    if wide is None:
        raise MMError(f"{what} takes half or int8_t operands (got {dtype})")
    return torch_dtype(dtype), torch_dtype(wide)


def _product(what, symbol, a, b, dtype, map_op, reduce_op, path, transposed_a=False, *, nt=False, wide=False, indexed=False,
             index_base=0, c=None, c_index=None, out=None, out_index=None, flag=True, batched_out=False):
    """The skeleton of every batched product wrapper: check the operands, derive the shapes, check or allocate the outputs,
    enqueue lib().<symbol>.  A new wrapper is a call of this.

    dtype ... transposed_a: make_config's arguments.  nt: b is (M, K).  wide: C has the widened type of `dtype`.  indexed:
    an int32 index lies beside C, and index_base is passed on.  c (and c_index): the in-place form, which accumulates;
    otherwise the result is out (and out_index) or new, (N, M) when both operands are 2-D, else (B, N, M).  bmm and
    baddbmm_ alone set batched_out (a 3-D result always) or clear flag (their C calls do not end in the accumulate flag).
    Returns C, or (C, index)."""
    import torch
    tdt, cdt = _widen_types(what, dtype) if wide else (torch_dtype(dtype),) * 2
    in_place = c is not None
    if in_place and wide:
        _device_operands(what, tdt, a, b)
        _device_operands(what, cdt, c)
        if c.device != a.device:
            raise MMError(f"operands live on different devices: {c.device}, {a.device}")
    else:
        _device_operands(what, tdt, *((c, a, b) if in_place else (a, b)))
    if in_place:
        if indexed and (not c_index.is_cuda or c_index.device != c.device or c_index.dtype != torch.int32):
            raise MMError(f"c_index must be a torch.int32 tensor on {c.device}; got {c_index.dtype} on {c_index.device}")
        if c.dim() not in (2, 3):
            raise MMError(f"{what} takes 2-D or 3-D operands")
        if indexed and (tuple(c_index.shape) != tuple(c.shape) or c_index.stride() != c.stride()):
            raise MMError(f"c_index must have c's shape and strides: {tuple(c.shape)} {c.stride()}, got "
                          f"{tuple(c_index.shape)} {c_index.stride()}")
    n, k, m, batch, sa, sb = _shapes(what, a, b, transposed_a, nt)
    if in_place:
        batch, sc = _inplace_batch(c, n, m, batch)
        index = c_index
    else:
        shape = (n, m) if a.dim() == 2 and b.dim() == 2 and not batched_out else (batch, n, m)
        c, sc = _output(out, "out", shape, cdt, a.device), n * m
        index = _output(out_index, "out_index", shape, torch.int32, a.device) if indexed else None
    config = make_config(dtype, map_op, reduce_op, path, transposed_a)
    _enqueue(a.device, getattr(lib(), symbol), ctypes.byref(config), a.data_ptr(), b.data_ptr(), c.data_ptr(),
             *((index.data_ptr(),) if indexed else ()), n, k, m, batch, sa, sb, sc, *((int(index_base),) if indexed else ()),
             *((int(in_place),) if flag else ()))
    return (c, index) if indexed else c


def bmm(a, b, dtype="float", map_op="Multiply", reduce_op="Add", path=PATH_AUTO, transposed_a=False, out=None):
    """Strided-batched C[e] = A[e] (map, reduce) B[e] on torch's current stream (mm_gemm_batched_enqueue).
    a: (B, N, K) -- or (B, K, N) with transposed_a -- b: (B, K, M); either may be 2-D or expanded with batch stride 0
    (one operand shared by the batch).  Each matrix must be dense row-major; the batch stride may be anything the C ABI
    accepts.  out: (B, N, M) contiguous.  Asynchronous, like any torch op."""
    return _product("bmm", "mm_gemm_batched_enqueue", a, b, dtype, map_op, reduce_op, path, transposed_a, out=out, flag=False,
                    batched_out=True)


def addmm_(c, a, b, dtype="float", map_op="Multiply", reduce_op="Add", path=PATH_AUTO, transposed_a=False):
    """In place C <- C (+) (A (x) B) on torch's current stream (mm_gemm_accumulate_enqueue): each output's reduction starts
    at the value C holds instead of identity() -- torch.addmm_ for (Multiply, Add), D <- min(D, A + B) for (Add, Min).
    a: (N, K) -- or (K, N) with transposed_a -- b: (K, M), c: (N, M); contiguous device tensors of `dtype`, C not
    overlapping A or B.  Returns c.  Asynchronous, like any torch op."""
    _device_operands("addmm_", torch_dtype(dtype), c, a, b)
    n, k, m = _matrix_shapes("addmm_", transposed_a, a, b, c)
    if tuple(c.shape) != (n, m):
        raise MMError(f"c has shape {tuple(c.shape)}, expected {(n, m)}")
    cfg = make_config(dtype, map_op, reduce_op, path, transposed_a)
    _enqueue(a.device, lib().mm_gemm_accumulate_enqueue, ctypes.byref(cfg), a.data_ptr(), b.data_ptr(), c.data_ptr(), n, k, m)
    return c


def baddbmm_(c, a, b, dtype="float", map_op="Multiply", reduce_op="Add", path=PATH_AUTO, transposed_a=False):
    """Strided-batched in place C[e] <- C[e] (+) (A[e] (x) B[e]) on torch's current stream
    (mm_gemm_batched_accumulate_enqueue) -- torch.baddbmm_ for (Multiply, Add).  a and b as for bmm (2-D, 3-D, or expanded
    with batch stride 0); c: (B, N, M) with dense row-major matrices and a batch stride of at least N * M (2-D when B is 1),
    not overlapping A or B.  Returns c.  Asynchronous, like any torch op."""
    return _product("baddbmm_", "mm_gemm_batched_accumulate_enqueue", a, b, dtype, map_op, reduce_op, path, transposed_a, c=c,
                    flag=False)


def matmul_argreduce(a, b, dtype="float", map_op="Add", reduce_op="Min", path=PATH_AUTO, transposed_a=False, index_base=0,
                     out=None, out_index=None):
    """(values, indices) of a Min- or Max-reduced product on torch's current stream (mm_gemm_argreduce_enqueue): values is
    what matmul / bmm return with path=PATH_ORDERED, bit for bit; indices (torch.int32) holds, per output, index_base + the
    first k whose mapped value is the result, or -1 where no k improved on identity() -- torch.min(x, dim)'s pair.
    a and b as for bmm (2-D, 3-D, or expanded with batch stride 0); the outputs are (N, M) when both operands are 2-D,
    else (B, N, M).  out / out_index: contiguous tensors of that shape (values' dtype, torch.int32).  Asynchronous."""
    return _product("matmul_argreduce", "mm_gemm_argreduce_enqueue", a, b, dtype, map_op, reduce_op, path, transposed_a,
                    out=out, out_index=out_index, indexed=True, index_base=index_base)


def addmm_argreduce_(c, c_index, a, b, dtype="float", map_op="Add", reduce_op="Min", path=PATH_AUTO, transposed_a=False,
                     index_base=0):
    """In place (C, I) <- argreduce seeded with (C, I) on torch's current stream (mm_gemm_argreduce_enqueue, accumulate):
    each output's chain starts at the value C holds and the index I holds; a k that improves on it records index_base + k,
    an output whose seed survives keeps its index exactly.  D <- min(D, A + B) of min-plus relaxation with the predecessor
    alongside.  2-D operands as for addmm_, 3-D (and broadcast) as for baddbmm_; c_index: torch.int32 with c's shape and
    strides.  Returns (c, c_index).  Asynchronous, like any torch op."""
    return _product("addmm_argreduce_", "mm_gemm_argreduce_enqueue", a, b, dtype, map_op, reduce_op, path, transposed_a,
                    c=c, c_index=c_index, indexed=True, index_base=index_base)


def matmul_logsumexp(a, b, dtype="float", reduce_op="Max", path=PATH_AUTO, transposed_a=False, out=None):
    """Log-semiring product on torch's current stream (mm_gemm_logsumexp_enqueue): C = log sum_k exp(A[i,k] + B[k,j]) for
    reduce_op="Max" (the HMM forward step, the smooth max-plus product), -log sum_k exp(-(A[i,k] + B[k,j])) for "Min" (the
    soft-min).  dtype: "half", "float" or "double".  a and b as for bmm (2-D, 3-D, or expanded with batch stride 0); the
    output is (N, M) when both operands are 2-D, else (B, N, M); out: a contiguous tensor of that shape.  Asynchronous."""
    return _product("matmul_logsumexp", "mm_gemm_logsumexp_enqueue", a, b, dtype, "Add", reduce_op, path, transposed_a, out=out)


def addmm_logsumexp_(c, a, b, dtype="float", reduce_op="Max", path=PATH_AUTO, transposed_a=False):
    """In place C <- log(exp(C) + sum_k exp(A[i,k] + B[k,j])) (Min: the soft-min) on torch's current stream
    (mm_gemm_logsumexp_enqueue, accumulate): C's value is one more term, so two calls on the halves of K compose to one
    call on all of it.  2-D operands as for addmm_, 3-D (and broadcast) as for baddbmm_.  Returns c.  Asynchronous."""
    return _product("addmm_logsumexp_", "mm_gemm_logsumexp_enqueue", a, b, dtype, "Add", reduce_op, path, transposed_a, c=c)


def matmul_wide(a, b, dtype="half", path=PATH_AUTO, transposed_a=False, out=None):
    """Widening product on torch's current stream (mm_gemm_widen_enqueue): half operands to a torch.float32 C -- the f32 sums
    the matrix cores accumulate, not rounded to binary16 -- or int8_t operands to a torch.int32 C, the exact sums mod 2^32.
    a and b as for bmm (2-D, 3-D, or expanded with batch stride 0); the output is (N, M) when both operands are 2-D, else
    (B, N, M); out: a contiguous tensor of that shape and of the wide type.  Asynchronous."""
    return _product("matmul_wide", "mm_gemm_widen_enqueue", a, b, dtype, "Multiply", "Add", path, transposed_a, out=out,
                    wide=True)


def addmm_wide_(c, a, b, dtype="half", path=PATH_AUTO, transposed_a=False):
    """In place C <- C + A B in the wide type on torch's current stream (mm_gemm_widen_enqueue, accumulate): c is
    torch.float32 for half operands, torch.int32 for int8_t; a K-split accumulated through it never rounds to the operand
    type.  2-D operands as for addmm_, 3-D (and broadcast) as for baddbmm_.  Returns c.  Asynchronous."""
    return _product("addmm_wide_", "mm_gemm_widen_enqueue", a, b, dtype, "Multiply", "Add", path, transposed_a, c=c, wide=True)


def matmul_nt(a, b, dtype="float", map_op="Multiply", reduce_op="Add", path=PATH_AUTO, out=None):
    """C = A (map, reduce) B^T on torch's current stream (mm_gemm_nt_enqueue): C[i][j] = reduce_k map(a[i][k], b[j][k]), both
    operands stored with k contiguous -- pairwise products between two row-stored sets, without b.mT.contiguous().
    a: (N, K) or (B, N, K); b: (M, K) or (B, M, K); either may be expanded with batch stride 0, and a and b may be one
    buffer.  The output is (N, M) when both operands are 2-D, else (B, N, M); out: a contiguous tensor of that shape.
    Asynchronous, like any torch op."""
    return _product("matmul_nt", "mm_gemm_nt_enqueue", a, b, dtype, map_op, reduce_op, path, out=out, nt=True)


def addmm_nt_(c, a, b, dtype="float", map_op="Multiply", reduce_op="Add", path=PATH_AUTO):
    """In place C <- C (+) (A (x) B^T) on torch's current stream (mm_gemm_nt_enqueue, accumulate): each output's reduction
    starts at the value C holds, so two calls on the halves of K compose to one call on all of it.  a and b as for matmul_nt;
    c: (N, M), or (B, N, M) as for baddbmm_, not overlapping a or b.  Returns c.  Asynchronous."""
    return _product("addmm_nt_", "mm_gemm_nt_enqueue", a, b, dtype, map_op, reduce_op, path, c=c, nt=True)


def matmul_argreduce_nt(a, b, dtype="float", map_op="Add", reduce_op="Min", path=PATH_AUTO, index_base=0, out=None,
                        out_index=None):
    """(values, indices) of a Min- or Max-reduced A x B^T product on torch's current stream (mm_gemm_argreduce_nt_enqueue):
    matmul_argreduce on b.mT, bit for bit, without b.mT.contiguous() -- a Viterbi step and its backpointers from a to-state
    major transition matrix.  a and b as for matmul_nt: (N, K) or (B, N, K) and (M, K) or (B, M, K), either expanded with
    batch stride 0, possibly one buffer.  The outputs are (N, M) when both operands are 2-D, else (B, N, M).  out /
    out_index: contiguous tensors of that shape (values' dtype, torch.int32).  Asynchronous."""
    return _product("matmul_argreduce_nt", "mm_gemm_argreduce_nt_enqueue", a, b, dtype, map_op, reduce_op, path,
                    out=out, out_index=out_index, indexed=True, index_base=index_base, nt=True)


def addmm_argreduce_nt_(c, c_index, a, b, dtype="float", map_op="Add", reduce_op="Min", path=PATH_AUTO, index_base=0):
    """In place (C, I) <- the A x B^T argreduce seeded with (C, I) on torch's current stream (mm_gemm_argreduce_nt_enqueue,
    accumulate): addmm_argreduce_ on b.mT.  a and b as for matmul_nt; c: (N, M), or (B, N, M) as for baddbmm_; c_index:
    torch.int32 with c's shape and strides.  Returns (c, c_index).  Asynchronous, like any torch op."""
    return _product("addmm_argreduce_nt_", "mm_gemm_argreduce_nt_enqueue", a, b, dtype, map_op, reduce_op, path,
                    c=c, c_index=c_index, indexed=True, index_base=index_base, nt=True)


def matmul_logsumexp_nt(a, b, dtype="float", reduce_op="Max", path=PATH_AUTO, out=None):
    """Log-semiring A x B^T product on torch's current stream (mm_gemm_logsumexp_nt_enqueue): C = log sum_k exp(a[i,k] +
    b[j,k]) for reduce_op="Max" (Min: the soft-min) -- matmul_logsumexp on b.mT, the forward step over a to-state major
    transition matrix.  a and b as for matmul_nt; the output is (N, M) when both operands are 2-D, else (B, N, M); out: a
    contiguous tensor of that shape.  Asynchronous."""
    return _product("matmul_logsumexp_nt", "mm_gemm_logsumexp_nt_enqueue", a, b, dtype, "Add", reduce_op, path, out=out,
                    nt=True)


def addmm_logsumexp_nt_(c, a, b, dtype="float", reduce_op="Max", path=PATH_AUTO):
    """In place C <- log(exp(C) + sum_k exp(a[i,k] + b[j,k])) (Min: the soft-min) on torch's current stream
    (mm_gemm_logsumexp_nt_enqueue, accumulate): addmm_logsumexp_ on b.mT.  a and b as for matmul_nt; c: (N, M), or
    (B, N, M) as for baddbmm_.  Returns c.  Asynchronous."""
    return _product("addmm_logsumexp_nt_", "mm_gemm_logsumexp_nt_enqueue", a, b, dtype, "Add", reduce_op, path, c=c,
                    nt=True)


def closure_(d, d_witness=None, dtype="float", map_op="Add", reduce_op="Min", path=PATH_AUTO):
    """In place D <- the closure of D (mm_closure_enqueue) on torch's current stream: blocked Floyd-Warshall,
    D[i][j] <- D[i][j] (+) D[i][v] (x) D[v][j] over every v -- all-pairs shortest paths for (Add, Min), widest paths for
    (Min, Max), reachability for (And, Max).  No identity is added to the diagonal (paths of one or more edges).
    d: a contiguous (n, n) or (batch, n, n) device tensor of `dtype`; d_witness (optional): a contiguous torch.int32 tensor
    of d's shape, fully written with the intermediate vertex of each entry's last strict improvement, -1 where the entry
    kept its input value.  Returns d.  Asynchronous, like any torch op."""
    import torch
    tdt = torch_dtype(dtype)
    _device_operands("closure_", tdt, d)
    if d.dim() not in (2, 3) or d.shape[-1] != d.shape[-2]:
        raise MMError(f"closure_ takes an (n, n) or (batch, n, n) tensor; got shape {tuple(d.shape)}")
    if not d.is_contiguous():
        raise MMError("closure_ needs a contiguous (row-major) d")
    n, batch = d.shape[-1], (d.shape[0] if d.dim() == 3 else 1)
    w = 0
    if d_witness is not None:
        if (not d_witness.is_cuda or d_witness.device != d.device or d_witness.dtype != torch.int32
                or tuple(d_witness.shape) != tuple(d.shape) or not d_witness.is_contiguous()):
            raise MMError(f"d_witness must be a contiguous torch.int32 tensor of shape {tuple(d.shape)} on {d.device}; got "
                          f"{tuple(d_witness.shape)}, {d_witness.dtype}, {d_witness.device}, "
                          f"contiguous={d_witness.is_contiguous()}")
        w = d_witness.data_ptr()
    cfg = make_config(dtype, map_op, reduce_op, path)
    _enqueue(d.device, lib().mm_closure_enqueue, ctypes.byref(cfg), d.data_ptr(), w, n, batch, n * n)
    return d


# ---- bit-packed Boolean semiring (mm_bits_*): one bit per element, 32 columns per torch.int32 word, LSB first ---------------
def bits_words(cols):
    """Words of a packed row of `cols` columns."""
    return (cols + 31) // 32


def kernel_name_bits_gemm(n, k, m, lda=None, ldb=None, ldc=None, batch=1):
    """Name of the kernel bits_matmul / bits_addmm_ run; the row strides (words) default to the rows' own word counts."""
    lda, ldb, ldc = (bits_words(c) if ld is None else ld for ld, c in ((lda, k), (ldb, m), (ldc, m)))
    return lib().mm_kernel_name_bits_gemm(n, k, m, lda, ldb, ldc, batch).decode()


def kernel_name_bits_closure(n, batch=1):
    return lib().mm_kernel_name_bits_closure(n, batch).decode()


def _byte_rows(x, what):
    """(x or a dense copy, batch, batch stride, row stride) of a (..., rows, cols) tensor of one-byte elements."""
    if x.dim() < 2:
        raise MMError(f"{what} takes a (..., rows, cols) tensor; got shape {tuple(x.shape)}")
    rows, cols = x.shape[-2], x.shape[-1]
    dense = x.dim() <= 3 and (cols == 1 or x.stride(-1) == 1) and (rows == 1 or x.stride(-2) >= cols) and (
        x.dim() == 2 or x.shape[0] == 1 or x.stride(0) >= (rows - 1) * x.stride(-2) + cols)
    if not dense:
        x = x.contiguous()
    if x.dim() > 3:
        x = x.reshape(-1, rows, cols)
    batch = x.shape[0] if x.dim() == 3 else 1
    return x, batch, (x.stride(0) if batch > 1 else 0), (x.stride(-2) if rows > 1 else cols)


def pack_bits(x):
    """torch.bool or torch.uint8 (..., rows, cols) -> torch.int32 (..., rows, ceil(cols / 32)) on torch's current stream
    (mm_bits_pack_enqueue): column j is bit j & 31 of word j >> 5, a nonzero byte is 1, the padding bits are 0.  A 2-D or
    3-D x with unit column stride is read as it lies (row and batch strides), anything else through a dense copy."""
    import torch
    if not x.is_cuda:
        raise MMError("pack_bits needs a device tensor: there is no CPU path")
    if x.dtype not in (torch.bool, torch.uint8):
        raise MMError(f"pack_bits takes torch.bool or torch.uint8 (got {x.dtype})")
    shape = tuple(x.shape)
    x, batch, stride, ld = _byte_rows(x, "pack_bits")
    rows, cols = shape[-2], shape[-1]
    words = bits_words(cols)
    out = torch.empty(shape[:-1] + (words,), dtype=torch.int32, device=x.device)
    _enqueue(x.device, lib().mm_bits_pack_enqueue, x.data_ptr(), out.data_ptr(), rows, cols, ld, words, batch, stride,
             rows * words)
    return out


def _row_rule(x, name, rows, row, unit):
    """(batch or None, batch stride, row stride) of a 2-D or 3-D tensor of `rows` rows of `row` units ("words", "elements")
    each: unit stride along the row; the row stride is the tensor's own and at least `row`; the batch stride of one matrix
    is 0."""
    if x.shape[-1] > 1 and x.stride(-1) != 1:
        raise MMError(f"the {unit} of a row of {name} must be contiguous (strides {x.stride()})")
    ld = x.stride(-2) if rows > 1 else max(x.stride(-2), row)
    if ld < row:
        raise MMError(f"{name} has row stride {ld}, below its {row} {unit}")
    if x.dim() == 2:
        return None, 0, ld
    return x.shape[0], (0 if x.shape[0] == 1 else x.stride(0)), ld


def _packed_operand(x, name, rows, cols):
    """(batch or None, batch stride, row stride), in words, of a packed operand: torch.int32, (rows, W) or (B, rows, W) with
    W >= ceil(cols / 32) and unit stride along the words; the row stride is the tensor's own, so a slice of whole words of
    a wider packed matrix is an operand as it lies."""
    import torch
    words = bits_words(cols)
    if x.dtype != torch.int32:
        raise MMError(f"{name} must be a packed torch.int32 tensor (got {x.dtype})")
    if x.dim() not in (2, 3) or x.shape[-2] != rows or x.shape[-1] < words:
        raise MMError(f"{name} has shape {tuple(x.shape)}, expected ({rows}, W) or (B, {rows}, W) with W >= {words}")
    batch, stride, ld = _row_rule(x, name, rows, words, "words")
    if x.dim() == 3 and x.stride(0) < 0:
        raise MMError(f"{name} has a negative batch stride")
    return batch, stride, ld


def _count_output(c, name, n, m, batch, two_d, device):
    """(batch stride, row stride), in elements, of the int32 result `c`: (n, m), or (batch, n, m) unless two_d, with unit
    stride along a row and its own row and batch strides."""
    import torch
    if c.dtype != torch.int32:
        raise MMError(f"{name} must be a torch.int32 tensor (got {c.dtype})")
    if not c.is_cuda or c.device != device:
        raise MMError(f"{name} must live on {device} (got {c.device})")
    want = (n, m) if two_d else (batch, n, m)
    if tuple(c.shape) != want:
        raise MMError(f"{name} has shape {tuple(c.shape)}, expected {want}")
    return _row_rule(c, name, n, m, "elements")[1:]


def _flat_batch(what, p, cols):
    """(p, leading dimensions, rows, batch or None, batch stride, row stride) of a packed (..., rows, W) tensor with its
    leading dimensions as one batch: 2-D and 3-D as they lie, more dimensions through a dense copy."""
    if not p.is_cuda:
        raise MMError(f"{what} needs a device tensor: there is no CPU path")
    if p.dim() < 2:
        raise MMError(f"{what} takes a (..., rows, W) tensor; got shape {tuple(p.shape)}")
    lead = tuple(p.shape[:-2])
    if p.dim() > 3:
        p = p.contiguous().reshape(-1, *p.shape[-2:])
    rows = p.shape[-2]
    return (p, lead, rows) + _packed_operand(p, "p", rows, cols)


def unpack_bits(p, cols, dtype=None):
    """The inverse of pack_bits (mm_bits_unpack_enqueue): packed torch.int32 (..., rows, W), W >= ceil(cols / 32), to
    (..., rows, cols) of `dtype` -- torch.bool (the default) or torch.uint8 -- holding 0 / 1."""
    import torch
    dtype = torch.bool if dtype is None else dtype
    if dtype not in (torch.bool, torch.uint8):
        raise MMError(f"unpack_bits writes torch.bool or torch.uint8 (got {dtype})")
    p, lead, rows, batch, stride, ld = _flat_batch("unpack_bits", p, cols)
    out = torch.empty(lead + (rows, cols), dtype=dtype, device=p.device)
    _enqueue(p.device, lib().mm_bits_unpack_enqueue, p.data_ptr(), out.data_ptr(), rows, cols, ld, cols, batch or 1, stride,
             rows * cols)
    return out


def _packed_pair(what, a, b, b_name, b_rows, b_cols, k):
    """(n, b's rows, batch, stride_a, stride_b, lda, ldb) of a packed product's operands: a is (N, k) packed along k, b is
    (b_rows, b_cols) packed along b_cols -- its own row count when b_rows is None -- each 2-D, 3-D, or expanded with batch
    stride 0."""
    if not (a.is_cuda and b.is_cuda):
        raise MMError(f"{what} needs device tensors: there is no CPU path")
    if a.device != b.device:
        raise MMError(f"operands live on different devices: {a.device} and {b.device}")
    if a.dim() not in (2, 3) or b.dim() not in (2, 3):
        raise MMError(f"{what} takes 2-D or 3-D operands")
    n, b_rows = a.shape[-2], (b.shape[-2] if b_rows is None else b_rows)
    ba, sa, lda = _packed_operand(a, "a", n, k)
    bb, sb, ldb = _packed_operand(b, b_name, b_rows, b_cols)
    batches = {x for x in (ba, bb) if x is not None and x != 1}
    if len(batches) > 1:
        raise MMError(f"batch sizes differ: {ba} and {bb}")
    return n, b_rows, (batches.pop() if batches else 1), sa, sb, lda, ldb


def _packed_product(what, symbol, a, b, k, m=None, *, nt=False, counts=False, op=None, c=None, out=None):
    """The skeleton of every packed product wrapper, as _product is of the dense ones: check the operands, derive the shapes,
    check or allocate C, enqueue lib().<symbol>.

    nt: b is bt, (M, k) packed along k, and m is its row count; otherwise b is (k, m) packed along m.  counts: C holds int32
    elements, (N, M) with ldc and stride_c in elements; otherwise packed words, (N, W >= ceil(m / 32)).  op: the counting
    op's code, which leads the C call's arguments.  c: the in-place form, which accumulates and takes its batch from c, over
    which 2-D operands broadcast; otherwise the result is out or new, 2-D when both operands are.  Returns C."""
    import torch
    n, b_rows, batch, sa, sb, lda, ldb = _packed_pair(what, a, b, *(("bt", None, k) if nt else ("b", k, m)), k)
    m = b_rows if nt else m
    in_place, two_d = c is not None, a.dim() == 2 and b.dim() == 2
    if in_place and counts:
        two_d = c.dim() == 2
        if two_d and batch != 1:
            raise MMError(f"c has shape {tuple(c.shape)}, expected ({batch}, {n}, {m})")
        if not two_d and c.dim() == 3 and batch == 1:
            batch = c.shape[0]
        sc, ldc = _count_output(c, "c", n, m, batch, two_d, a.device)
    elif in_place:
        if not c.is_cuda or c.device != a.device:
            raise MMError(f"c must live on {a.device} (got {c.device})")
        bc, sc, ldc = _packed_operand(c, "c", n, m)
        if batch not in (1, bc or 1):
            raise MMError(f"c has shape {tuple(c.shape)}, expected ({batch}, {n}, W)")
        batch = bc or 1
    elif out is None:
        row = m if counts else bits_words(m)
        c = torch.empty((n, row) if two_d else (batch, n, row), dtype=torch.int32, device=a.device)
        sc, ldc = ((n * m if batch > 1 else 0), m) if counts else _packed_operand(c, "out", n, m)[1:]
    elif counts:
        c, (sc, ldc) = out, _count_output(out, "out", n, m, batch, two_d, a.device)
    else:
        if out.device != a.device or out.dim() != (2 if two_d else 3) or (not two_d and out.shape[0] != batch):
            raise MMError(f"out has shape {tuple(out.shape)} on {out.device}; expected {'(N, W)' if two_d else f'({batch}, N, W)'} on {a.device}")
        c, (bc, sc, ldc) = out, _packed_operand(out, "out", n, m)
    if (in_place or out is not None) and batch > 1 and sc <= 0:
        raise MMError(f"{'c' if in_place else 'out'} has batch stride {sc}: the {batch} outputs would overlap")
    _enqueue(a.device, getattr(lib(), symbol), *(() if op is None else (op,)), a.data_ptr(), b.data_ptr(), c.data_ptr(), n, k, m,
             lda, ldb, ldc, batch, sa, sb, sc, int(in_place))
    return c


def bits_matmul(a, b, k, m, out=None):
    """Packed Boolean product on torch's current stream (mm_bits_gemm_enqueue): C[i][j] = OR_k (A[i][k] AND B[k][j]).
    a: (N, Wk) packed along K, b: (K, Wm) packed along M, torch.int32; either may be 3-D, or expanded with batch stride 0.
    k and m are the logical bit counts (the word counts alone do not determine them); Wk >= ceil(k / 32), Wm >=
    ceil(m / 32), and row strides are taken from the tensors, so p[:, 1:3] of a wider packed matrix is a valid a without a
    copy.  Returns (N, ceil(m / 32)) when both operands are 2-D, else (B, N, ceil(m / 32)); out: a packed tensor of that
    shape (more words per row allowed; they are left alone).  Padding bits of the result are 0.  Asynchronous."""
    return _packed_product("bits_matmul", "mm_bits_gemm_enqueue", a, b, k, m, out=out)


def bits_addmm_(c, a, b, k, m):
    """In place C <- C | A B on torch's current stream (mm_bits_gemm_enqueue, accumulate); a and b as for bits_matmul, c:
    (N, Wm) or (B, N, Wm) packed torch.int32 with its own row stride, not overlapping a or b.  Two calls on the halves of K
    equal one call on all of it.  Returns c.  Asynchronous."""
    return _packed_product("bits_addmm_", "mm_bits_gemm_enqueue", a, b, k, m, c=c)


def kernel_name_bits_gf2(n, k, m, lda=None, ldb=None, ldc=None, batch=1):
    """Name of the kernel bits_matmul_gf2 / bits_addmm_gf2_ run; the row strides (words) default to the rows' own word counts."""
    lda, ldb, ldc = (bits_words(c) if ld is None else ld for ld, c in ((lda, k), (ldb, m), (ldc, m)))
    return lib().mm_kernel_name_bits_gf2(n, k, m, lda, ldb, ldc, batch).decode()


def bits_matmul_gf2(a, b, k, m, out=None):
    """Packed product over GF(2) on torch's current stream (mm_bits_gf2_enqueue): C[i][j] = XOR_k (A[i][k] AND B[k][j]).
    Operands, k, m, out and the result are those of bits_matmul; padding bits of a and b are ignored whatever they hold,
    those of the result are 0.  Asynchronous."""
    return _packed_product("bits_matmul_gf2", "mm_bits_gf2_enqueue", a, b, k, m, out=out)


def bits_addmm_gf2_(c, a, b, k, m):
    """In place C <- C ^ A B on torch's current stream (mm_bits_gf2_enqueue, accumulate); operands as for bits_addmm_.  Two
    calls on the halves of K equal one call on all of it; the same call twice restores c.  Returns c.  Asynchronous."""
    return _packed_product("bits_addmm_gf2_", "mm_bits_gf2_enqueue", a, b, k, m, c=c)


def bits_closure_(d, n=None):
    """In place D <- D+, the transitive closure of a packed adjacency matrix, on torch's current stream
    (mm_bits_closure_enqueue): (i, j) is set when a path of one or more edges leads from i to j; no identity is added to
    the diagonal.  d: packed torch.int32 (n, W) or (batch, n, W) with W >= ceil(n / 32) and its own row stride; n defaults
    to the number of rows.  Returns d.  Asynchronous."""
    if not d.is_cuda:
        raise MMError("bits_closure_ needs a device tensor: there is no CPU path")
    if d.dim() not in (2, 3):
        raise MMError(f"bits_closure_ takes an (n, W) or (batch, n, W) tensor; got shape {tuple(d.shape)}")
    n = d.shape[-2] if n is None else n
    batch, stride, ldd = _packed_operand(d, "d", n, n)
    if (batch or 1) > 1 and stride == 0:
        raise MMError(f"d has batch stride 0: the {batch} graphs would overlap")
    _enqueue(d.device, lib().mm_bits_closure_enqueue, d.data_ptr(), n, ldd, batch or 1, stride)
    return d


# ---- counting products on the packed format (mm_bits_count_*, A x B^T) and the packed transpose ---------------------------------
BITS_COUNT_OPS = {"And": 0, "Xor": 1}


def _count_op(what, op):
    if op not in BITS_COUNT_OPS:
        raise MMError(f"{what}: op must be one of {sorted(BITS_COUNT_OPS)} (got {op!r})")
    return BITS_COUNT_OPS[op]


def kernel_name_bits_count(n, k, m, lda=None, ldbt=None, ldc=None, batch=1):
    """Name of the kernel bits_matmul_count / bits_addmm_count_ run; lda and ldbt (words) default to ceil(k / 32), ldc
    (elements) to m."""
    lda, ldbt = (bits_words(k) if ld is None else ld for ld in (lda, ldbt))
    return lib().mm_kernel_name_bits_count(n, k, m, lda, ldbt, m if ldc is None else ldc, batch).decode()


def bits_matmul_count(a, bt, k, op="And", out=None):
    """Packed counting product on torch's current stream (mm_bits_count_enqueue): C[i][j] = sum_k (A[i][k] op Bt[j][k]), op
    "And" (common neighbours, intersections) or "Xor" (Hamming distances).  a: (N, W) and bt: (M, W), both packed along K,
    torch.int32, W >= ceil(k / 32); either may be 3-D, or expanded with batch stride 0.  Row strides are taken from the
    tensors, so a column slice of whole words is an operand without a copy; padding bits are ignored.  Returns torch.int32
    (N, M) when both operands are 2-D, else (B, N, M); out: an int32 tensor of that shape with its own row stride.
    Asynchronous."""
    return _packed_product("bits_matmul_count", "mm_bits_count_enqueue", a, bt, k, nt=True, counts=True,
                           op=_count_op("bits_matmul_count", op), out=out)


def bits_addmm_count_(c, a, bt, k, op="And"):
    """In place C += counts on torch's current stream (mm_bits_count_enqueue, accumulate), mod 2^32; a, bt and op as for
    bits_matmul_count, c: torch.int32 (N, M) or (B, N, M) with its own row stride, not overlapping a or bt.  Two calls on
    the halves of K equal one call on all of it.  Returns c.  Asynchronous."""
    return _packed_product("bits_addmm_count_", "mm_bits_count_enqueue", a, bt, k, nt=True, counts=True,
                           op=_count_op("bits_addmm_count_", op), c=c)


def transpose_bits(p, cols, out=None):
    """Packed transpose on torch's current stream (mm_bits_transpose_enqueue): packed torch.int32 (..., rows, W), W >=
    ceil(cols / 32), to packed (..., cols, ceil(rows / 32)) with out[..., j, i] = p[..., i, j] -- a K x M operand of
    bits_matmul as the M x K operand of bits_matmul_count.  Padding bits of p are ignored, those of the result are 0.  out: a
    packed tensor of the result's shape (more words per row allowed; they are left alone)."""
    import torch
    p, lead, rows, batch, stride, ld = _flat_batch("transpose_bits", p, cols)
    if out is None:
        out = torch.empty(lead + (cols, bits_words(rows)), dtype=torch.int32, device=p.device)
    elif out.device != p.device or tuple(out.shape[:-2]) != lead:
        raise MMError(f"out has shape {tuple(out.shape)} on {out.device}; expected {lead + (cols, 'W')} on {p.device}")
    o = out
    if out.dim() > 3:
        if not out.is_contiguous():
            raise MMError("out with more than one batch dimension must be contiguous")
        o = out.reshape(-1, *out.shape[-2:])
    bo, so, ldo = _packed_operand(o, "out", cols, rows)
    if (batch or 1) > 1 and so == 0:
        raise MMError(f"out has batch stride 0: the {batch} outputs would overlap")
    _enqueue(p.device, lib().mm_bits_transpose_enqueue, p.data_ptr(), o.data_ptr(), rows, cols, ld, ldo, batch or 1, stride, so)
    return out


def row_slab(cfg, n, k, m, world_size, rank):
    """(row0, rows) of `rank`'s slab of the N split, as mm_gemm_multi_device deals the rows out (mm_row_slab)."""
    row0, rows = ctypes.c_uint(0), ctypes.c_uint(0)
    _check(lib().mm_row_slab(ctypes.byref(cfg), n, k, m, world_size, rank, ctypes.byref(row0), ctypes.byref(rows)))
    return row0.value, rows.value


def matmul_host(a, b, dtype="float", map_op="Multiply", reduce_op="Add", path=PATH_AUTO, devices=1, transposed_a=False, timing=False):
    """numpy in, numpy out, through mm_gemm_multi_device (rows of C split over `devices` GPUs).
    a: (N, K), or (K, N) with transposed_a.  Returns (C, kernel_seconds); with timing=True (C, kernel_seconds, per-device
    kernel seconds, host-clock seconds) from mm_gemm_multi_device_timed."""
    import numpy as np
    a = np.ascontiguousarray(a)
    b = np.ascontiguousarray(b)
    k, m = b.shape
    n = a.shape[1] if transposed_a else a.shape[0]
    c = np.empty((n, m), dtype=a.dtype)
    cfg = make_config(dtype, map_op, reduce_op, path, transposed_a)
    t = ctypes.c_double(0)
    if timing:
        per_device = (ctypes.c_double * devices)()
        wall = ctypes.c_double(0)
        _check(lib().mm_gemm_multi_device_timed(devices, ctypes.byref(cfg), a.ctypes.data, b.ctypes.data, c.ctypes.data,
                                                n, k, m, ctypes.byref(t), per_device, ctypes.byref(wall)))
        return c, t.value, list(per_device), wall.value
    _check(lib().mm_gemm_multi_device(devices, ctypes.byref(cfg), a.ctypes.data, b.ctypes.data, c.ctypes.data,
                                      n, k, m, ctypes.byref(t)))
    return c, t.value


def matmul_capi(a, b, dtype="float", map_op="Multiply", reduce_op="Add", path=PATH_AUTO, transposed_a=False,
                device=0):
    """numpy in, numpy out, through the split-phase C ABI exactly as host/RunHardware.cpp drives the
    reference: mm_alloc x3, mm_copy_to_device x2, mm_gemm_launch (blocking, HIP-event timed),
    mm_copy_to_host.  Returns (C, kernel_seconds)."""
    import numpy as np
    L = lib()
    a = np.ascontiguousarray(a)
    b = np.ascontiguousarray(b)
    k, m = b.shape
    n = a.shape[1] if transposed_a else a.shape[0]
    c = np.empty((n, m), dtype=a.dtype)
    cfg = make_config(dtype, map_op, reduce_op, path, transposed_a)
    ptrs = [ctypes.c_void_p() for _ in range(3)]
    t = ctypes.c_double(0)
    try:
        for p, arr in zip(ptrs, (a, b, c)):
            _check(L.mm_alloc(device, arr.nbytes, ctypes.byref(p)))
        _check(L.mm_copy_to_device(device, ptrs[0], a.ctypes.data, a.nbytes))
        _check(L.mm_copy_to_device(device, ptrs[1], b.ctypes.data, b.nbytes))
        _check(L.mm_gemm_launch(device, ctypes.byref(cfg), ptrs[0], ptrs[1], ptrs[2], n, k, m, ctypes.byref(t)))
        _check(L.mm_copy_to_host(device, c.ctypes.data, ptrs[2], c.nbytes))
    finally:
        for p in ptrs:
            if p.value:
                L.mm_free(device, p)
    return c, t.value
