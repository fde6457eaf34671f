"""CPU tests of the torch binding's host-side rules: what every product wrapper hands to the C ABI, and what it refuses.

No device is needed: the operands are meta tensors that claim to live on a device and carry a fake address each, and
gemm_hls_amd._enqueue is replaced by a recorder.  For every wrapper the recorded call -- C symbol, mm_config_t fields, pointer
order, shapes, batch, strides, index_base, accumulate flag -- and every refusal's full message is compared with a literal.
The literals were recorded once from the binding as it stood before its wrappers were folded into one skeleton; they are
never computed from the code under test.  Two messages of matmul and bmm (devices that differ, a dtype that does not match)
are the exception: those two wrappers took the other wrappers' wording of the same facts with the skeleton.  The packed
counting wrappers' and the packed transpose's calls and refusals were recorded the same way, before their skeleton.  One more
table pins the ctypes prototype of every exported symbol."""
import collections
import ctypes

import pytest

import gemm_hls_amd as g

torch = pytest.importorskip("torch")

N, K, M, B = 8, 16, 12, 3
PTR = {"a": 0xA000000, "b": 0xB000000, "c": 0xC000000, "i": 0xD000000}   # c: C, out or D; i: the index or the witness
ORD = g.PATH_ORDERED


class Dev:
    """A meta tensor that claims to live on a device, with an address: the binding reads attributes only."""
    is_cuda = True

    def __init__(self, t, ptr):
        self.t, self.ptr = t, ptr

    def __getattr__(self, name):
        return getattr(self.t, name)

    def data_ptr(self):
        return self.ptr


class Make:
    """t.a(...), t.b(...), t.c(...), t.i(...): the operand of that role; remembers the last one made per role."""
    def __init__(self):
        self.made = {}

    def __getattr__(self, role):
        def make(*shape, strides=None, dtype=torch.float32, device="meta"):
            x = (torch.empty(shape, dtype=dtype, device=device) if strides is None else
                 torch.empty_strided(shape, strides, dtype=dtype, device=device))
            self.made[role] = Dev(x, PTR[role])
            return self.made[role]
        return make


@pytest.fixture
def recorded(monkeypatch):
    log = []

    def record(device, fn, *args):
        cfg = None
        if args and isinstance(getattr(args[0], "_obj", None), g.Config):
            c = args[0]._obj
            cfg, args = (c.dtype, c.map_op, c.reduce_op, c.path, c.layout_a), args[1:]
        log.append((str(device), fn.__name__, cfg, tuple(args)))

    monkeypatch.setattr(g, "_enqueue", record)
    return log


# wrapper: A x B^T, takes transposed_a, index output, widening, in place, shapes it takes
Spec = collections.namedtuple("Spec", "nt ta index wide inplace dims")
SPECS = {
    "matmul": Spec(False, True, False, False, False, (2,)),
    "bmm": Spec(False, True, False, False, False, (2, 3)),
    "addmm_": Spec(False, True, False, False, True, (2,)),
    "baddbmm_": Spec(False, True, False, False, True, (2, 3)),
    "matmul_argreduce": Spec(False, True, True, False, False, (2, 3)),
    "addmm_argreduce_": Spec(False, True, True, False, True, (2, 3)),
    "matmul_logsumexp": Spec(False, True, False, False, False, (2, 3)),
    "addmm_logsumexp_": Spec(False, True, False, False, True, (2, 3)),
    "matmul_wide": Spec(False, True, False, True, False, (2, 3)),
    "addmm_wide_": Spec(False, True, False, True, True, (2, 3)),
    "matmul_nt": Spec(True, False, False, False, False, (2, 3)),
    "addmm_nt_": Spec(True, False, False, False, True, (2, 3)),
    "matmul_argreduce_nt": Spec(True, False, True, False, False, (2, 3)),
    "addmm_argreduce_nt_": Spec(True, False, True, False, True, (2, 3)),
    "matmul_logsumexp_nt": Spec(True, False, False, False, False, (2, 3)),
    "addmm_logsumexp_nt_": Spec(True, False, False, False, True, (2, 3)),
}


def _config_kwargs(name):
    """A non-default configuration of the wrapper: (kwargs, operand dtype, C's dtype)."""
    if SPECS[name].wide:
        return {"dtype": "int8_t", "path": ORD}, torch.int8, torch.int32
    if "logsumexp" in name:
        return {"dtype": "double", "reduce_op": "Min", "path": ORD}, torch.float64, torch.float64
    if "argreduce" in name:
        return {"dtype": "int", "map_op": "Min", "reduce_op": "Max", "path": ORD}, torch.int32, torch.int32
    return {"dtype": "double", "map_op": "Add", "reduce_op": "Min", "path": ORD}, torch.float64, torch.float64


def _run(name, t, a, b, c=None, ci=None, **kw):
    s = SPECS[name]
    if s.inplace:
        return getattr(g, name)(*((c, ci, a, b) if s.index else (c, a, b)), **kw)
    return getattr(g, name)(a, b, **kw)


def _operands(name, t, batch_a=None, batch_b=None, batch_c=None, ta=False, dt=None, cdt=None, a_strides=None,
              b_strides=None, c_strides=None):
    """The wrapper's well-formed operands as keyword arguments of _run: c (and ci) only for the in-place forms."""
    s = SPECS[name]
    dt = dt or (torch.float16 if s.wide else torch.float32)
    cdt = cdt or (torch.float32 if s.wide else dt)
    lead = lambda batch: () if batch is None else (batch,)   # noqa: E731
    ops = {"a": t.a(*lead(batch_a), *((K, N) if ta else (N, K)), strides=a_strides, dtype=dt),
           "b": t.b(*lead(batch_b), *((M, K) if s.nt else (K, M)), strides=b_strides, dtype=dt)}
    if s.inplace:
        ops["c"] = t.c(*lead(batch_c), N, M, strides=c_strides, dtype=cdt)
        if s.index:
            ops["ci"] = t.i(*lead(batch_c), N, M, strides=c_strides, dtype=torch.int32)
    return ops


def _call_cases():
    cases = {}
    for name, s in SPECS.items():
        def add(case, fn, name=name):
            cases[f"{name}/{case}"] = (name, fn)
        bcols = K if s.nt else M
        add("2d", lambda t, n: _run(n, t, **_operands(n, t)))
        if s.ta:
            add("transposed_a", lambda t, n: _run(n, t, **_operands(n, t, ta=True), transposed_a=True))
        cfg_kw, dt, cdt = _config_kwargs(name)
        if s.index:
            cfg_kw = dict(cfg_kw, index_base=5)
        add("config", lambda t, n, kw=cfg_kw, dt=dt, cdt=cdt: _run(n, t, **_operands(n, t, dt=dt, cdt=cdt), **kw))
        if not s.inplace:
            out_shape = (1, N, M) if name == "bmm" else (N, M)
            add("out", lambda t, n, sh=out_shape, s=s: _run(
                n, t, **_operands(n, t), out=t.c(*sh, dtype=torch.float32),
                **({"out_index": t.i(*sh, dtype=torch.int32)} if s.index else {})))
        if 3 not in s.dims:
            continue
        add("3d", lambda t, n: _run(n, t, **_operands(n, t, B, B, B)))
        add("3d_a_2d_b", lambda t, n: _run(n, t, **_operands(n, t, B, None, B)))
        add("expanded_b", lambda t, n, bc=bcols: _run(n, t, **_operands(n, t, B, B, B, b_strides=(0, bc, 1))))
        add("batch_of_one_a", lambda t, n: _run(n, t, **_operands(n, t, 1, B, B, a_strides=(999, K, 1))))
        if s.ta:
            add("transposed_a_3d", lambda t, n: _run(n, t, **_operands(n, t, B, B, B, ta=True), transposed_a=True))
        if s.inplace:
            add("c_over_2d_operands", lambda t, n: _run(n, t, **_operands(n, t, None, None, B)))
            add("c_batch_stride", lambda t, n: _run(n, t, **_operands(n, t, B, B, B, c_strides=(200, M, 1))))
            add("c_one_matrix_3d", lambda t, n: _run(n, t, **_operands(n, t, None, None, 1)))
        else:
            add("out_3d", lambda t, n, s=s: _run(
                n, t, **_operands(n, t, B, None), out=t.c(B, N, M, dtype=torch.float32),
                **({"out_index": t.i(B, N, M, dtype=torch.int32), "index_base": 7} if s.index else {})))
    i32, u8 = torch.int32, torch.uint8
    other = {
        "closure_/2d": lambda t: g.closure_(t.c(9, 9)),
        "closure_/3d_witness": lambda t: g.closure_(t.c(B, 9, 9), t.i(B, 9, 9, dtype=i32)),
        "closure_/config": lambda t: g.closure_(t.c(9, 9, dtype=torch.float64), None, "double", "Min", "Max", ORD),
        "bits_matmul/2d": lambda t: g.bits_matmul(t.a(N, 2, dtype=i32), t.b(40, 3, dtype=i32), 40, 70),
        "bits_matmul/3d": lambda t: g.bits_matmul(t.a(B, N, 2, dtype=i32), t.b(B, 40, 3, dtype=i32), 40, 70),
        "bits_matmul/sliced_a_expanded_b": lambda t: g.bits_matmul(
            t.a(B, N, 2, strides=(64, 5, 1), dtype=i32), t.b(B, 40, 3, strides=(0, 3, 1), dtype=i32), 40, 70),
        "bits_matmul/wider_out": lambda t: g.bits_matmul(t.a(N, 2, dtype=i32), t.b(40, 3, dtype=i32), 40, 70,
                                                         out=t.c(N, 4, dtype=i32)),
        # no columns, and a batch of no rows: a fresh result's strides are what torch gives an empty tensor
        "bits_matmul/no_columns": lambda t: g.bits_matmul(t.a(N, 2, dtype=i32), t.b(40, 0, dtype=i32), 40, 0),
        "bits_matmul/3d_no_rows": lambda t: g.bits_matmul(t.a(B, 0, 2, dtype=i32), t.b(B, 40, 3, dtype=i32), 40, 70),
        "bits_addmm_/2d": lambda t: g.bits_addmm_(t.c(N, 3, dtype=i32), t.a(N, 2, dtype=i32), t.b(40, 3, dtype=i32), 40, 70),
        "bits_addmm_/c_over_2d_operands": lambda t: g.bits_addmm_(
            t.c(B, N, 3, strides=(100, 4, 1), dtype=i32), t.a(N, 2, dtype=i32), t.b(40, 3, dtype=i32), 40, 70),
        "bits_addmm_/3d": lambda t: g.bits_addmm_(t.c(B, N, 3, dtype=i32), t.a(B, N, 2, dtype=i32), t.b(40, 3, dtype=i32),
                                                 40, 70),
        "bits_closure_/2d": lambda t: g.bits_closure_(t.c(40, 2, dtype=i32)),
        "bits_closure_/3d_wider_rows": lambda t: g.bits_closure_(t.c(B, 40, 4, dtype=i32), 40),
        "pack_bits/2d": lambda t: g.pack_bits(t.a(N, 70, dtype=torch.bool)),
        "pack_bits/3d_row_stride": lambda t: g.pack_bits(t.a(B, N, 70, strides=(700, 80, 1), dtype=u8)),
        "unpack_bits/2d": lambda t: g.unpack_bits(t.a(N, 3, dtype=i32), 70),
        "unpack_bits/3d_wider_rows_uint8": lambda t: g.unpack_bits(t.a(B, N, 4, dtype=i32), 70, u8),
        "bits_matmul_count/2d": lambda t: g.bits_matmul_count(t.a(N, 2, dtype=i32), t.b(M, 2, dtype=i32), 40),
        # a column slice of whole words (row stride 5), a broadcast bt, a 3-D a, Xor, an out with its own row stride
        "bits_matmul_count/sliced_a_expanded_bt_xor_out": lambda t: g.bits_matmul_count(
            t.a(B, N, 2, strides=(40, 5, 1), dtype=i32), t.b(B, M, 2, strides=(0, 2, 1), dtype=i32), 64, op="Xor",
            out=t.c(B, N, M, strides=(200, 16, 1), dtype=i32)),
        "bits_matmul_count/3d_a_2d_bt": lambda t: g.bits_matmul_count(
            t.a(B, N, 2, strides=(40, 5, 1), dtype=i32), t.b(M, 2, dtype=i32), 64),
        "bits_addmm_count_/3d_a_2d_bt": lambda t: g.bits_addmm_count_(
            t.c(B, N, M, strides=(200, 16, 1), dtype=i32), t.a(B, N, 2, strides=(40, 5, 1), dtype=i32), t.b(M, 2, dtype=i32), 33),
        "transpose_bits/3d_row_stride": lambda t: g.transpose_bits(t.a(B, 70, 6, strides=(500, 7, 1), dtype=i32), 130),
        "transpose_bits/2d_wider_out": lambda t: g.transpose_bits(t.a(70, 5, dtype=i32), 130, out=t.c(130, 4, dtype=i32)),
        # more batch dimensions: one flat batch of a dense copy
        "transpose_bits/4d": lambda t: g.transpose_bits(t.a(2, B, 70, 5, dtype=i32), 130),
    }
    for key, fn in other.items():
        cases[key] = (None, fn)
    return cases


CALL_CASES = _call_cases()


def run_call_case(key, log):
    """The recorded call of one case, with the shapes of what the wrapper returned; the in-place forms and a supplied out /
    out_index come back as the very objects."""
    name, fn = CALL_CASES[key]
    t = Make()
    del log[:]
    res = fn(t, name) if name else fn(t)
    parts = res if isinstance(res, tuple) else (res,)
    for part, role in zip(parts, ("c", "i")):
        if role in t.made:
            assert part is t.made[role], (key, role)
    assert len(log) == 1, (key, log)
    return log[0] + (tuple((tuple(p.shape), str(p.dtype).replace("torch.", "")) for p in parts),)


A_, B_, C_, I_ = PTR["a"], PTR["b"], PTR["c"], PTR["i"]
# wrapper: (C symbol, (dtype, map, reduce, path) by default, the same and C's dtype in the "config" case)
SYMBOLS = {
    "matmul": ("mm_gemm_enqueue", (0, 1, 0, 0), (1, 0, 3, 1), "float64"),
    "bmm": ("mm_gemm_batched_enqueue", (0, 1, 0, 0), (1, 0, 3, 1), "float64"),
    "addmm_": ("mm_gemm_accumulate_enqueue", (0, 1, 0, 0), (1, 0, 3, 1), "float64"),
    "baddbmm_": ("mm_gemm_batched_accumulate_enqueue", (0, 1, 0, 0), (1, 0, 3, 1), "float64"),
    "matmul_argreduce": ("mm_gemm_argreduce_enqueue", (0, 0, 3, 0), (7, 3, 4, 1), "int32"),
    "addmm_argreduce_": ("mm_gemm_argreduce_enqueue", (0, 0, 3, 0), (7, 3, 4, 1), "int32"),
    "matmul_logsumexp": ("mm_gemm_logsumexp_enqueue", (0, 0, 4, 0), (1, 0, 3, 1), "float64"),
    "addmm_logsumexp_": ("mm_gemm_logsumexp_enqueue", (0, 0, 4, 0), (1, 0, 3, 1), "float64"),
    "matmul_wide": ("mm_gemm_widen_enqueue", (2, 1, 0, 0), (3, 1, 0, 1), "int32"),
    "addmm_wide_": ("mm_gemm_widen_enqueue", (2, 1, 0, 0), (3, 1, 0, 1), "int32"),
    "matmul_nt": ("mm_gemm_nt_enqueue", (0, 1, 0, 0), (1, 0, 3, 1), "float64"),
    "addmm_nt_": ("mm_gemm_nt_enqueue", (0, 1, 0, 0), (1, 0, 3, 1), "float64"),
    "matmul_argreduce_nt": ("mm_gemm_argreduce_nt_enqueue", (0, 0, 3, 0), (7, 3, 4, 1), "int32"),
    "addmm_argreduce_nt_": ("mm_gemm_argreduce_nt_enqueue", (0, 0, 3, 0), (7, 3, 4, 1), "int32"),
    "matmul_logsumexp_nt": ("mm_gemm_logsumexp_nt_enqueue", (0, 0, 4, 0), (1, 0, 3, 1), "float64"),
    "addmm_logsumexp_nt_": ("mm_gemm_logsumexp_nt_enqueue", (0, 0, 4, 0), (1, 0, 3, 1), "float64"),
}
# case: (batch, stride_a, stride_b, stride_c, the result's shape); the out-of-place forms pass N x M = 96 as stride_c where the
# in-place forms pass C's own batch stride -- 0 for one matrix
BATCH = {
    "2d": (1, 0, 0, (96, 0), (8, 12)),
    "transposed_a": (1, 0, 0, (96, 0), (8, 12)),
    "config": (1, 0, 0, (96, 0), (8, 12)),
    "out": (1, 0, 0, (96, 0), (8, 12)),
    "3d": (3, 128, 192, (96, 96), (3, 8, 12)),
    "3d_a_2d_b": (3, 128, 0, (96, 96), (3, 8, 12)),
    "expanded_b": (3, 128, 0, (96, 96), (3, 8, 12)),
    "batch_of_one_a": (3, 0, 192, (96, 96), (3, 8, 12)),
    "transposed_a_3d": (3, 128, 192, (96, 96), (3, 8, 12)),
    "out_3d": (3, 128, 0, (96, None), (3, 8, 12)),
    "c_over_2d_operands": (3, 0, 0, (None, 96), (3, 8, 12)),
    "c_batch_stride": (3, 128, 192, (None, 200), (3, 8, 12)),
    "c_one_matrix_3d": (1, 0, 0, (None, 0), (1, 8, 12)),
}
INDEX_BASE = {"config": 5, "out_3d": 7}
i32 = "int32"
OTHER_CALLS = {
    "closure_/2d": ("mm_closure_enqueue", (0, 0, 3, 0, 0), (C_, 0, 9, 1, 81), (((9, 9), "float32"),)),
    "closure_/3d_witness": ("mm_closure_enqueue", (0, 0, 3, 0, 0), (C_, I_, 9, 3, 81), (((3, 9, 9), "float32"),)),
    "closure_/config": ("mm_closure_enqueue", (1, 3, 4, 1, 0), (C_, 0, 9, 1, 81), (((9, 9), "float64"),)),
    "bits_matmul/2d": ("mm_bits_gemm_enqueue", None, (A_, B_, 0, 8, 40, 70, 2, 3, 3, 1, 0, 0, 0, 0), (((8, 3), i32),)),
    "bits_matmul/3d": ("mm_bits_gemm_enqueue", None, (A_, B_, 0, 8, 40, 70, 2, 3, 3, 3, 16, 120, 24, 0), (((3, 8, 3), i32),)),
    "bits_matmul/sliced_a_expanded_b": ("mm_bits_gemm_enqueue", None, (A_, B_, 0, 8, 40, 70, 5, 3, 3, 3, 64, 0, 24, 0),
                                        (((3, 8, 3), i32),)),
    "bits_matmul/wider_out": ("mm_bits_gemm_enqueue", None, (A_, B_, C_, 8, 40, 70, 2, 3, 4, 1, 0, 0, 0, 0), (((8, 4), i32),)),
    "bits_matmul/no_columns": ("mm_bits_gemm_enqueue", None, (A_, B_, 0, 8, 40, 0, 2, 1, 1, 1, 0, 0, 0, 0), (((8, 0), i32),)),
    "bits_matmul/3d_no_rows": ("mm_bits_gemm_enqueue", None, (A_, B_, 0, 0, 40, 70, 2, 3, 3, 3, 2, 120, 3, 0), (((3, 0, 3), i32),)),
    "bits_addmm_/2d": ("mm_bits_gemm_enqueue", None, (A_, B_, C_, 8, 40, 70, 2, 3, 3, 1, 0, 0, 0, 1), (((8, 3), i32),)),
    "bits_addmm_/c_over_2d_operands": ("mm_bits_gemm_enqueue", None, (A_, B_, C_, 8, 40, 70, 2, 3, 4, 3, 0, 0, 100, 1),
                                       (((3, 8, 3), i32),)),
    "bits_addmm_/3d": ("mm_bits_gemm_enqueue", None, (A_, B_, C_, 8, 40, 70, 2, 3, 3, 3, 16, 0, 24, 1), (((3, 8, 3), i32),)),
    "bits_closure_/2d": ("mm_bits_closure_enqueue", None, (C_, 40, 2, 1, 0), (((40, 2), i32),)),
    "bits_closure_/3d_wider_rows": ("mm_bits_closure_enqueue", None, (C_, 40, 4, 3, 160), (((3, 40, 4), i32),)),
    "pack_bits/2d": ("mm_bits_pack_enqueue", None, (A_, 0, 8, 70, 70, 3, 1, 0, 24), (((8, 3), i32),)),
    "pack_bits/3d_row_stride": ("mm_bits_pack_enqueue", None, (A_, 0, 8, 70, 80, 3, 3, 700, 24), (((3, 8, 3), i32),)),
    "unpack_bits/2d": ("mm_bits_unpack_enqueue", None, (A_, 0, 8, 70, 3, 70, 1, 0, 560), (((8, 70), "bool"),)),
    "unpack_bits/3d_wider_rows_uint8": ("mm_bits_unpack_enqueue", None, (A_, 0, 8, 70, 4, 70, 3, 32, 560), (((3, 8, 70), "uint8"),)),
    "bits_matmul_count/2d": ("mm_bits_count_enqueue", None, (0, A_, B_, 0, 8, 40, 12, 2, 2, 12, 1, 0, 0, 0, 0), (((8, 12), i32),)),
    "bits_matmul_count/sliced_a_expanded_bt_xor_out": ("mm_bits_count_enqueue", None,
                                                       (1, A_, B_, C_, 8, 64, 12, 5, 2, 16, 3, 40, 0, 200, 0), (((3, 8, 12), i32),)),
    "bits_matmul_count/3d_a_2d_bt": ("mm_bits_count_enqueue", None, (0, A_, B_, 0, 8, 64, 12, 5, 2, 12, 3, 40, 0, 96, 0),
                                     (((3, 8, 12), i32),)),
    "bits_addmm_count_/3d_a_2d_bt": ("mm_bits_count_enqueue", None, (0, A_, B_, C_, 8, 33, 12, 5, 2, 16, 3, 40, 0, 200, 1),
                                     (((3, 8, 12), i32),)),
    "transpose_bits/3d_row_stride": ("mm_bits_transpose_enqueue", None, (A_, 0, 70, 130, 7, 3, 3, 500, 390), (((3, 130, 3), i32),)),
    "transpose_bits/2d_wider_out": ("mm_bits_transpose_enqueue", None, (A_, C_, 70, 130, 5, 4, 1, 0, 0), (((130, 4), i32),)),
    # (the dense copy of a meta tensor has no address)
    "transpose_bits/4d": ("mm_bits_transpose_enqueue", None, (0, 0, 70, 130, 5, 3, 6, 350, 390), (((2, 3, 130, 3), i32),)),
}


def expected_call(key):
    """The literal tables above, put together: (device, symbol, config, arguments, (shape, dtype) of each result)."""
    if key in OTHER_CALLS:
        return ("meta",) + OTHER_CALLS[key]
    name, case = key.split("/")
    s = SPECS[name]
    symbol, cfg, other_cfg, other_dtype = SYMBOLS[name]
    cfg = (other_cfg if case == "config" else cfg) + (int(case.startswith("transposed_a")),)
    batch, stride_a, stride_b, stride_c, shape = BATCH[case]
    given = s.inplace or case.startswith("out")             # C (and the index) are the caller's: their addresses
    pointers = (A_, B_, C_ if given else 0) + ((I_ if given else 0,) if s.index else ())
    args = pointers + (8, 16, 12)
    if name not in ("matmul", "addmm_"):
        args += (batch, stride_a, stride_b, stride_c[s.inplace])
        args += ((INDEX_BASE.get(case, 0),) if s.index else ()) + ((int(s.inplace),) if name not in ("bmm", "baddbmm_") else ())
    if name == "bmm" and len(shape) == 2:
        shape = (1,) + shape                                  # bmm: always a 3-D result
    dtype = other_dtype if case == "config" else "float32"
    return ("meta", symbol, cfg, args, ((shape, dtype),) + (((shape, i32),) if s.index else ()))


EXPECTED_CALLS = {key: expected_call(key) for key in CALL_CASES}


def test_the_tables_cover_every_wrapper():
    assert set(SYMBOLS) == set(SPECS) and set(OTHER_CALLS) <= set(CALL_CASES)
    covered = {key.split("/")[0] for key in CALL_CASES}
    assert covered == set(SPECS) | {"closure_", "bits_matmul", "bits_addmm_", "bits_closure_", "pack_bits", "unpack_bits",
                                    "bits_matmul_count", "bits_addmm_count_", "transpose_bits"}
    assert {key.split("/")[0] for key in REFUSAL_CASES} == set(SPECS)
    assert {key.split("/")[0] for key in OTHER_REFUSALS} == {"bits_matmul_count", "bits_addmm_count_", "transpose_bits"}


@pytest.mark.parametrize("key", sorted(CALL_CASES))
def test_recorded_call(key, recorded):
    assert run_call_case(key, recorded) == EXPECTED_CALLS[key]


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def _refusal_cases():
    cases = {}
    f64 = torch.float64
    for name, s in SPECS.items():
        def add(case, fn, name=name):
            cases[f"{name}/{case}"] = (name, fn)

        def ops(t, n, **changes):
            """Well-formed 3-D (2-D for the 2-D-only wrappers) operands, `changes` replacing some."""
            batch = B if 3 in SPECS[n].dims else None
            o = _operands(n, t, batch, batch, batch)
            o.update(changes)
            return o
        lead = (B,) if 3 in s.dims else ()
        odt = torch.float16 if s.wide else torch.float32
        b2 = (M, K) if s.nt else (K, M)
        add("cpu_a", lambda t, n, lead=lead, odt=odt: _run(n, t, **ops(t, n, a=torch.zeros(*lead, N, K, dtype=odt))))
        add("other_device_b", lambda t, n, lead=lead, odt=odt, b2=b2: _run(
            n, t, **ops(t, n, b=t.b(*lead, *b2, dtype=odt, device="cpu"))))
        add("dtype_b", lambda t, n, lead=lead, b2=b2: _run(n, t, **ops(t, n, b=t.b(*lead, *b2, dtype=f64))))
        add("a_1d", lambda t, n, odt=odt: _run(n, t, **ops(t, n, a=t.a(K, dtype=odt))))
        add("inner", lambda t, n, lead=lead, odt=odt: _run(n, t, **ops(t, n, a=t.a(*lead, N, K + 1, dtype=odt))))
        add("not_dense_b_2d", lambda t, n, odt=odt, b2=b2: _run(
            n, t, **ops(t, n, b=t.b(*b2, strides=(2 * b2[1], 2), dtype=odt))))
        if 3 in s.dims:
            add("not_dense_b_3d", lambda t, n, odt=odt, b2=b2: _run(
                n, t, **ops(t, n, b=t.b(B, *b2, strides=(4 * b2[0] * b2[1], 2 * b2[1], 2), dtype=odt))))
            add("batch", lambda t, n, odt=odt: _run(n, t, **ops(t, n, a=t.a(2, N, K, dtype=odt))))
        if s.ta:
            add("inner_transposed_a", lambda t, n, lead=lead, odt=odt: _run(
                n, t, **ops(t, n, a=t.a(*lead, N, K, dtype=odt)), transposed_a=True))
        if s.wide:
            add("dtype_not_widened", lambda t, n: _run(n, t, **ops(t, n), dtype="float"))
        cdt = torch.float32
        if not s.inplace:
            full = (1, N, M) if name == "bmm" and not lead else (*lead, N, M)
            add("out_shape", lambda t, n, lead=lead: _run(n, t, **ops(t, n), out=t.c(*lead, M, N, dtype=cdt)))
            add("out_dtype", lambda t, n, full=full: _run(n, t, **ops(t, n), out=t.c(*full, dtype=f64)))
            add("out_not_contiguous", lambda t, n, full=full: _run(
                n, t, **ops(t, n), out=t.c(*full, strides=tuple(2 * x for x in torch.empty(full, device="meta").stride()),
                                           dtype=cdt)))
            if s.index:
                add("out_index_dtype", lambda t, n, full=full: _run(n, t, **ops(t, n), out_index=t.i(*full, dtype=cdt)))
                add("out_index_shape", lambda t, n, full=full: _run(
                    n, t, **ops(t, n), out_index=t.i(*full[:-1], M + 1, dtype=torch.int32)))
        else:
            add("c_shape", lambda t, n, lead=lead: _run(n, t, **ops(t, n, c=t.c(*lead, M, N, dtype=cdt),
                                                                    **({"ci": t.i(*lead, M, N, dtype=torch.int32)}
                                                                       if SPECS[n].index else {}))))
            add("c_1d", lambda t, n: _run(n, t, **ops(t, n, c=t.c(N * M, dtype=cdt),
                                                      **({"ci": t.i(N * M, dtype=torch.int32)} if SPECS[n].index else {}))))
            add("c_dtype", lambda t, n, lead=lead: _run(n, t, **ops(t, n, c=t.c(*lead, N, M, dtype=f64))))
            add("c_cpu", lambda t, n, lead=lead: _run(
                n, t, **ops(t, n, c=torch.zeros(*lead, N, M, dtype=torch.float32))))
            if 3 in s.dims:
                add("c_expanded", lambda t, n: _run(n, t, **ops(t, n, c=t.c(B, N, M, strides=(0, M, 1), dtype=cdt),
                                                                **({"ci": t.i(B, N, M, strides=(0, M, 1), dtype=torch.int32)}
                                                                   if SPECS[n].index else {}))))
                add("c_batch", lambda t, n: _run(n, t, **ops(t, n, c=t.c(2, N, M, dtype=cdt),
                                                             **({"ci": t.i(2, N, M, dtype=torch.int32)}
                                                                if SPECS[n].index else {}))))
                add("c_not_dense", lambda t, n: _run(n, t, **ops(t, n, c=t.c(B, N, M, strides=(400, 2 * M, 2), dtype=cdt),
                                                                 **({"ci": t.i(B, N, M, strides=(400, 2 * M, 2), dtype=torch.int32)}
                                                                    if SPECS[n].index else {}))))
            else:
                add("c_not_contiguous", lambda t, n: _run(n, t, **ops(t, n, c=t.c(N, M, strides=(2 * M, 2), dtype=cdt))))
            if s.index:
                add("c_index_dtype", lambda t, n, lead=lead: _run(n, t, **ops(t, n, ci=t.i(*lead, N, M, dtype=cdt))))
                add("c_index_cpu", lambda t, n, lead=lead: _run(
                    n, t, **ops(t, n, ci=torch.zeros(*lead, N, M, dtype=torch.int32))))
                add("c_index_strides", lambda t, n: _run(
                    n, t, **ops(t, n, ci=t.i(B, N, M, strides=(200, M, 1), dtype=torch.int32))))
                add("c_index_shape", lambda t, n: _run(n, t, **ops(t, n, ci=t.i(B, N, M + 1, dtype=torch.int32))))
    return cases


REFUSAL_CASES = _refusal_cases()


def run_refusal_case(key, log):
    name, fn = REFUSAL_CASES[key]
    del log[:]
    with pytest.raises(g.MMError) as info:
        fn(Make(), name)
    assert info.type is g.MMError and log == [], key
    return str(info.value)


OUT = "out must be a contiguous torch.float32 tensor of shape {shape} on meta; got "
OUT_INDEX = "out_index must be a contiguous torch.int32 tensor of shape (3, 8, 12) on meta; got "
# case: the message, or one per kind of wrapper.  {w}: the wrapper; {lead}: "(3, " for the wrappers that take a batch, else "(";
# {shape}: the output's; {b}: "b", or "b (M, K)" in the A x B^T forms; {dt}: the operands' dtype.
MESSAGES = {
    "cpu_a": "{w} needs device tensors: there is no CPU path",
    "c_cpu": "{w} needs device tensors: there is no CPU path",
    "other_device_b": {"in place": "operands live on different devices: meta, meta, cpu",
                       "else": "operands live on different devices: meta, cpu"},
    "dtype_b": {"in place": "operand dtypes torch.float32, torch.float32, torch.float64 do not match torch.float32",
                "else": "operand dtypes {dt}, torch.float64 do not match {dt}"},
    "a_1d": {"2-D only": "{w} takes 2-D operands", "else": "{w} takes 2-D or 3-D operands"},
    "c_1d": {"2-D only": "{w} takes 2-D operands", "else": "{w} takes 2-D or 3-D operands"},
    "inner": {"nt": "inner dimensions differ: A {lead}8, 17), B {lead}12, 16) (M, K)",
              "else": "inner dimensions differ: A {lead}8, 17), B {lead}16, 12)"},
    "inner_transposed_a": "inner dimensions differ: A {lead}8, 16) (K x N), B {lead}16, 12)",
    "not_dense_b_2d": {"2-D only": "{w} needs contiguous (row-major) operands", "else": "{b} must be a dense row-major matrix"},
    "not_dense_b_3d": {"nt": "each matrix of b (M, K) must be dense row-major (strides (768, 32, 2))",
                       "else": "each matrix of b must be dense row-major (strides (768, 24, 2))"},
    "batch": "batch sizes differ: 2 and 3",
    "dtype_not_widened": "{w} takes half or int8_t operands (got float)",
    "out_shape": {"2-D only": OUT + "(12, 8), torch.float32, meta, contiguous=True",
                  "else": OUT + "(3, 12, 8), torch.float32, meta, contiguous=True"},
    "out_dtype": OUT + "{shape}, torch.float64, meta, contiguous=True",
    "out_not_contiguous": OUT + "{shape}, torch.float32, meta, contiguous=False",
    "out_index_dtype": OUT_INDEX + "(3, 8, 12), torch.float32, meta, contiguous=True",
    "out_index_shape": OUT_INDEX + "(3, 8, 13), torch.int32, meta, contiguous=True",
    "c_shape": {"2-D only": "c has shape (12, 8), expected (8, 12)",
                "else": "c has shape (3, 12, 8), expected (B, 8, 12) or (8, 12)"},
    "c_dtype": {"wide": "operand dtypes torch.float64 do not match torch.float32",
                "else": "operand dtypes torch.float64, torch.float32, torch.float32 do not match torch.float32"},
    "c_expanded": "c has batch stride 0: the 3 outputs would overlap",
    "c_batch": "c has shape (2, 8, 12), expected (3, 8, 12)",
    "c_not_dense": "each matrix of c must be dense row-major (strides (400, 24, 2))",
    "c_not_contiguous": "{w} needs contiguous (row-major) operands",
    "c_index_dtype": "c_index must be a torch.int32 tensor on meta; got torch.float32 on meta",
    "c_index_cpu": "c_index must be a torch.int32 tensor on meta; got torch.int32 on cpu",
    "c_index_strides": "c_index must have c's shape and strides: (3, 8, 12) (96, 12, 1), got (3, 8, 12) (200, 12, 1)",
    "c_index_shape": "c_index must have c's shape and strides: (3, 8, 12) (96, 12, 1), got (3, 8, 13) (104, 13, 1)",
}

def expected_refusal(key):
    name, case = key.split("/")
    s = SPECS[name]
    kinds = [kind for kind, applies in (("2-D only", 3 not in s.dims), ("nt", s.nt), ("wide", s.wide),
                                        ("in place", s.inplace and not s.wide)) if applies] + ["else"]
    message = MESSAGES[case]
    if isinstance(message, dict):
        message = next(message[kind] for kind in kinds if kind in message)
    return message.format(w=name, lead="(3, " if 3 in s.dims else "(", shape=(3, 8, 12) if 3 in s.dims else (8, 12),
                          b="b (M, K)" if s.nt else "b", dt="torch.float16" if s.wide else "torch.float32")


EXPECTED_REFUSALS = {key: expected_refusal(key) for key in REFUSAL_CASES}


@pytest.mark.parametrize("key", sorted(REFUSAL_CASES))
def test_refusal_message(key, recorded):
    assert run_refusal_case(key, recorded) == EXPECTED_REFUSALS[key]


# ---- refusals of the packed counting wrappers and the packed transpose -----------------------------------------------------
def _claims(x, device):
    """x, claiming to live on `device`."""
    x.device = device
    return x


def _count_refusals():
    i32 = torch.int32
    cases = {}
    both = {"bits_matmul_count": lambda t, a, bt, k, **kw: g.bits_matmul_count(a, bt, k, **kw),
            "bits_addmm_count_": lambda t, a, bt, k, **kw: g.bits_addmm_count_(t.c(N, M, dtype=i32), a, bt, k, **kw)}
    for name, call in both.items():
        def add(case, fn, call=call, name=name):
            cases[f"{name}/{case}"] = lambda t: fn(t, call)
        a, bt = (lambda t: t.a(N, 2, dtype=i32)), (lambda t: t.b(M, 2, dtype=i32))
        add("dtype_a", lambda t, call: call(t, t.a(N, 2, dtype=torch.int64), bt(t), 40))
        add("dtype_bt", lambda t, call: call(t, a(t), t.b(M, 2, dtype=torch.uint8), 40))
        add("k_beyond_the_words", lambda t, call: call(t, a(t), bt(t), 65))
        add("bt_one_word", lambda t, call: call(t, a(t), t.b(M, 1, dtype=i32), 40))
        add("batch", lambda t, call: call(t, t.a(B, N, 2, dtype=i32), t.b(2, M, 2, dtype=i32), 40))
        add("other_device_bt", lambda t, call: call(t, a(t), _claims(t.b(M, 2, dtype=i32), torch.device("cuda", 1)), 40))
        add("op", lambda t, call: call(t, a(t), bt(t), 40, op="Or"))
        add("a_4d", lambda t, call: call(t, t.a(2, B, N, 2, dtype=i32), bt(t), 40))
        add("a_words_not_contiguous", lambda t, call: call(t, t.a(N, 2, strides=(4, 2), dtype=i32), bt(t), 40))
    a, bt = (lambda t: t.a(N, 2, dtype=i32)), (lambda t: t.b(M, 2, dtype=i32))
    cases.update({
        "bits_matmul_count/cpu": lambda t: g.bits_matmul_count(torch.zeros(4, 1, dtype=i32), torch.zeros(4, 1, dtype=i32), 4),
        "bits_matmul_count/out_dtype": lambda t: g.bits_matmul_count(a(t), bt(t), 40, out=t.c(N, M, dtype=torch.float32)),
        "bits_matmul_count/out_shape": lambda t: g.bits_matmul_count(a(t), bt(t), 40, out=t.c(N, M + 1, dtype=i32)),
        "bits_addmm_count_/batch_into_2d_c": lambda t: g.bits_addmm_count_(t.c(N, M, dtype=i32), t.a(B, N, 2, dtype=i32), bt(t), 40),
        "bits_addmm_count_/c_expanded": lambda t: g.bits_addmm_count_(t.c(B, N, M, strides=(0, M, 1), dtype=i32), a(t), bt(t), 40),
        "transpose_bits/cpu": lambda t: g.transpose_bits(torch.zeros(4, 1, dtype=i32), 4),
        "transpose_bits/dtype": lambda t: g.transpose_bits(t.a(70, 5, dtype=torch.int16), 130),
        "transpose_bits/cols_beyond_the_words": lambda t: g.transpose_bits(t.a(70, 4, dtype=i32), 130),
        "transpose_bits/out_rows_beyond_its_words": lambda t: g.transpose_bits(t.a(70, 5, dtype=i32), 130, out=t.c(130, 2, dtype=i32)),
    })
    return cases


OTHER_REFUSALS = _count_refusals()
# what both counting wrappers say of their operands; {w}: the wrapper
COUNT_OPERAND_MESSAGES = {
    "dtype_a": "a must be a packed torch.int32 tensor (got torch.int64)",
    "dtype_bt": "bt must be a packed torch.int32 tensor (got torch.uint8)",
    "k_beyond_the_words": "a has shape (8, 2), expected (8, W) or (B, 8, W) with W >= 3",
    "bt_one_word": "bt has shape (12, 1), expected (12, W) or (B, 12, W) with W >= 2",
    "batch": "batch sizes differ: 3 and 2",
    "other_device_bt": "operands live on different devices: meta and cuda:1",
    "op": "{w}: op must be one of ['And', 'Xor'] (got 'Or')",
    "a_4d": "{w} takes 2-D or 3-D operands",
    "a_words_not_contiguous": "the words of a row of a must be contiguous (strides (4, 2))",
}
EXPECTED_OTHER_REFUSALS = {
    "bits_matmul_count/cpu": "bits_matmul_count needs device tensors: there is no CPU path",
    "bits_matmul_count/out_dtype": "out must be a torch.int32 tensor (got torch.float32)",
    "bits_matmul_count/out_shape": "out has shape (8, 13), expected (8, 12)",
    "bits_addmm_count_/batch_into_2d_c": "c has shape (8, 12), expected (3, 8, 12)",
    "bits_addmm_count_/c_expanded": "c has batch stride 0: the 3 outputs would overlap",
    "transpose_bits/cpu": "transpose_bits needs a device tensor: there is no CPU path",
    "transpose_bits/dtype": "p must be a packed torch.int32 tensor (got torch.int16)",
    "transpose_bits/cols_beyond_the_words": "p has shape (70, 4), expected (70, W) or (B, 70, W) with W >= 5",
    "transpose_bits/out_rows_beyond_its_words": "out has shape (130, 2), expected (130, W) or (B, 130, W) with W >= 3",
}
EXPECTED_OTHER_REFUSALS.update((f"{w}/{case}", message.format(w=w)) for w in ("bits_matmul_count", "bits_addmm_count_")
                               for case, message in COUNT_OPERAND_MESSAGES.items())


@pytest.mark.parametrize("key", sorted(OTHER_REFUSALS))
def test_other_refusal_message(key, recorded):
    with pytest.raises(g.MMError) as info:
        OTHER_REFUSALS[key](Make())
    assert info.type is g.MMError and recorded == [], key
    assert str(info.value) == EXPECTED_OTHER_REFUSALS[key]


# ---- prototypes ----------------------------------------------------------------------------------------------------------------
def _type_name(tp):
    # (where unsigned long long has unsigned long's size, ctypes makes them one type: c_size_t's name wins here)
    names = {ctypes.c_void_p: "vp", ctypes.c_uint: "u", ctypes.c_int: "i", ctypes.c_ulonglong: "ull", ctypes.c_size_t: "sz",
             ctypes.c_char_p: "str", ctypes.POINTER(g.Config): "cfg*", ctypes.POINTER(g.KernelInfo): "info*",
             ctypes.POINTER(ctypes.c_double): "d*", ctypes.POINTER(ctypes.c_int): "i*", ctypes.POINTER(ctypes.c_uint): "u*",
             ctypes.POINTER(ctypes.c_void_p): "vp*", None: "void"}
    return names[tp]


def prototype(sym):
    fn = getattr(g.lib(), sym)
    args = "unset" if fn.argtypes is None else " ".join(_type_name(tp) for tp in fn.argtypes)
    return f"{_type_name(fn.restype)} <- {args}"


GEMM = "cfg* vp vp vp u u u"
BATCHED = GEMM + " u sz sz sz"
ARGREDUCE = "cfg* vp vp vp vp u u u u sz sz sz i i"
BITS_GEMM = "vp vp vp u u u sz sz sz u sz sz sz i"
BITS_CONVERT = "vp vp u u sz sz u sz sz"
NAME = "str <- cfg* u u u u"
EXPECTED_PROTOTYPES = {
    "mm_init": "i <- i*",
    "mm_alloc": "i <- i sz vp*",
    "mm_free": "i <- i vp",
    "mm_copy_to_device": "i <- i vp vp sz",
    "mm_copy_to_host": "i <- i vp vp sz",
    "mm_fill_device": "i <- i i vp sz sz",          # (the seed is an unsigned long long: ctypes' c_size_t here)
    "mm_gemm_launch": f"i <- i {GEMM} d*",
    "mm_gemm_enqueue": f"i <- vp {GEMM}",
    "mm_gemm_multi_device": f"i <- i {GEMM} d*",
    "MatrixMultiplicationKernel": "void <- vp vp vp u u u",
    "mm_set_default_config": "i <- cfg*",
    "mm_dtype_size": "sz <- i",
    "mm_config_supported": "i <- cfg*",
    "mm_kernel_name": "str <- cfg* u u u",
    "mm_kernel_info": "i <- cfg* u u u info*",
    "mm_last_error": "str <- unset",
    "mm_gemm_host": f"i <- {GEMM}",
    "mm_tuning_set": "i <- str i",
    "mm_tuning_get": "i <- str i*",
    "mm_release_workspace": "i <- i",
    "mm_device_pci_bus_id": "i <- i str i",
    "mm_device_max_grid_dim_y": "i <- i i*",
    "mm_row_slab": "i <- cfg* u u u i i u* u*",
    "mm_gemm_multi_device_timed": f"i <- i {GEMM} d* d* d*",
    "mm_gemm_batched_enqueue": f"i <- vp {BATCHED}",
    "mm_gemm_batched_launch": f"i <- i {BATCHED} d*",
    "mm_kernel_name_batched": NAME,
    "mm_gemm_accumulate_enqueue": f"i <- vp {GEMM}",
    "mm_gemm_accumulate_launch": f"i <- i {GEMM} d*",
    "mm_gemm_batched_accumulate_enqueue": f"i <- vp {BATCHED}",
    "mm_gemm_batched_accumulate_launch": f"i <- i {BATCHED} d*",
    "mm_gemm_argreduce_enqueue": f"i <- vp {ARGREDUCE}",
    "mm_gemm_argreduce_launch": f"i <- i {ARGREDUCE} d*",
    "mm_kernel_name_argreduce": NAME,
    "mm_closure_enqueue": "i <- vp cfg* vp vp u u sz",
    "mm_closure_launch": "i <- i cfg* vp vp u u sz d*",
    "mm_kernel_name_closure": "str <- cfg* u u i",
    "mm_gemm_logsumexp_enqueue": f"i <- vp {BATCHED} i",
    "mm_gemm_logsumexp_launch": f"i <- i {BATCHED} i d*",
    "mm_kernel_name_logsumexp": NAME,
    "mm_gemm_widen_enqueue": f"i <- vp {BATCHED} i",
    "mm_gemm_widen_launch": f"i <- i {BATCHED} i d*",
    "mm_kernel_name_widen": NAME,
    "mm_widen_dtype": "i <- i",
    "mm_gemm_nt_enqueue": f"i <- vp {BATCHED} i",
    "mm_gemm_nt_launch": f"i <- i {BATCHED} i d*",
    "mm_kernel_name_nt": NAME,
    "mm_gemm_argreduce_nt_enqueue": f"i <- vp {ARGREDUCE}",
    "mm_gemm_argreduce_nt_launch": f"i <- i {ARGREDUCE} d*",
    "mm_kernel_name_argreduce_nt": NAME,
    "mm_gemm_logsumexp_nt_enqueue": f"i <- vp {BATCHED} i",
    "mm_gemm_logsumexp_nt_launch": f"i <- i {BATCHED} i d*",
    "mm_kernel_name_logsumexp_nt": NAME,
    "mm_bits_gemm_enqueue": f"i <- vp {BITS_GEMM}",
    "mm_bits_gemm_launch": f"i <- i {BITS_GEMM} d*",
    "mm_kernel_name_bits_gemm": "str <- u u u sz sz sz u",
    "mm_bits_closure_enqueue": "i <- vp vp u sz u sz",
    "mm_bits_closure_launch": "i <- i vp u sz u sz d*",
    "mm_kernel_name_bits_closure": "str <- u u",
    "mm_bits_pack_enqueue": f"i <- vp {BITS_CONVERT}",
    "mm_bits_pack_launch": f"i <- i {BITS_CONVERT} d*",
    "mm_bits_unpack_enqueue": f"i <- vp {BITS_CONVERT}",
    "mm_bits_unpack_launch": f"i <- i {BITS_CONVERT} d*",
    "mm_bits_count_enqueue": f"i <- vp i {BITS_GEMM}",
    "mm_bits_count_launch": f"i <- i i {BITS_GEMM} d*",
    "mm_kernel_name_bits_count": "str <- u u u sz sz sz u",
    "mm_bits_transpose_enqueue": f"i <- vp {BITS_CONVERT}",
    "mm_bits_transpose_launch": f"i <- i {BITS_CONVERT} d*",
}


def test_prototype_of_every_exported_symbol():
    assert sorted(EXPECTED_PROTOTYPES) == sorted(g.EXPORTS)
    for sym in g.EXPORTS:
        assert prototype(sym) == EXPECTED_PROTOTYPES[sym], sym
