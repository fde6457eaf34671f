"""CPU tests of the A x B^T entry points (mm_gemm_nt_*, mm_kernel_name_nt): the header, the binding and EXPORTS agree; the
kernel's name follows the narrow batched call's family, row by row of the table in include/mm_gemm.h; every refusal comes
with its status and message before any device is touched; K = 0 accumulating and empty batches are no-ops; A and Bt may be
one buffer; the binding's shape errors name (M, K)."""
import ctypes
import os
import re

import pytest

import gemm_hls_amd as g

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "mm_gemm.h")).read()
SYMBOLS = ("mm_gemm_nt_enqueue", "mm_gemm_nt_launch", "mm_kernel_name_nt")
MM_OK, MM_ERR_NO_DEVICE, MM_ERR_BAD_ARGUMENT, MM_ERR_UNSUPPORTED = 0, 1, 2, 3

# Fake device addresses, never dereferenced: every call below is refused, or is a no-op, before a device is touched.
A0, B0, C0 = 1 << 22, 2 << 22, 3 << 22
E = 64 * 64


def _enq(cfg, a=A0, b=B0, c=C0, n=64, k=64, m=64, batch=4, sa=E, sb=E, sc=E, acc=0):
    return g.lib().mm_gemm_nt_enqueue(None, ctypes.byref(cfg), a, b, c, n, k, m, batch, sa, sb, sc, acc)


def _launch(cfg, a=A0, b=B0, c=C0, n=64, k=64, m=64, batch=4, sa=E, sb=E, sc=E, acc=0, device=0):
    t = ctypes.c_double(-1.0)
    return g.lib().mm_gemm_nt_launch(device, ctypes.byref(cfg), a, b, c, n, k, m, batch, sa, sb, sc, acc, ctypes.byref(t))


def _err():
    return g.lib().mm_last_error().decode()


def _cfg(dtype="float", map_op="Multiply", reduce_op="Add", path=g.PATH_AUTO, transposed_a=False):
    return g.make_config(dtype, map_op, reduce_op, path, transposed_a)


def test_nt_symbols_declared_exported_and_bound():
    for sym in SYMBOLS:
        assert re.search(rf"^(int|const char)\s*\*?\s*{sym}\(", HEADER, flags=re.M), sym
        assert sym in g.EXPORTS
        assert getattr(g.lib(), sym).argtypes is not None
    assert callable(g.matmul_nt) and callable(g.addmm_nt_) and callable(g.kernel_name_nt)


# ---- the name table, one block per row of the header's table -------------------------------------------------------------
PREPASS = [   # (dtype, (n, k, m), batch): a matrix-core family, the batched resolver names a kernel, K and M chunk multiples
    ("float", (130, 72, 136), 1), ("float", (1024, 1024, 1024), 3), ("double", (130, 72, 136), 1),
    ("half", (130, 80, 136), 1), ("half", (2048, 2048, 2048), 2), ("int8_t", (130, 96, 144), 1), ("uint8_t", (130, 96, 144), 3),
]


def test_nt_name_prepass_follows_the_narrow_batched_resolver():
    for dtype, (n, k, m), batch in PREPASS:
        cfg = _cfg(dtype)
        assert g.kernel_name_batched(cfg, n, k, m, batch).startswith("mfma_"), (dtype, n, k, m, batch)
        assert g.kernel_name_nt(cfg, n, k, m, batch) == "nt_prepass", (dtype, n, k, m, batch)
    assert g.kernel_name_nt(_cfg("float"), 512, 512, 512, 0) == g.kernel_name_nt(_cfg("float"), 512, 512, 512, 1) == "nt_prepass"


def test_nt_name_valu_tile_where_it_serves_else_ordered():
    # (Add, Min) and the integer algebras: the narrow call's valu_tile family -- and its K % 4 / M % 4 rule does not bind here
    for dtype, es in (("int8_t", 1), ("half", 2), ("uint16_t", 2), ("float", 4), ("int", 4), ("double", 8), ("long", 8)):
        bk, epc = 64 // es, 16 // es
        cfg = _cfg(dtype, "Add", "Min")
        for shape in ((1, bk, 1), (128, bk, 128), (130, 2 * bk + epc, 131), (257, 3 * bk, 129), (4096, 4096, 4096)):
            assert g.kernel_name_nt(cfg, *shape) == "valu_tile_nt", (dtype, shape)
            assert g.kernel_name_nt(cfg, *shape, 5) == "valu_tile_nt", (dtype, shape)
        assert g.kernel_name_nt(cfg, 64, bk - epc, 64) == "ordered_nt", dtype          # K < BK
        assert g.kernel_name_nt(cfg, 64, 2 * bk + 1, 64) == "ordered_nt", dtype        # K no multiple of the 16-byte chunk
    assert g.kernel_name_nt(_cfg("float", "Add", "Min"), 37, 19, 41) == "ordered_nt"
    # 128 rows of K reach 4 GiB: the 32-bit offsets of the DMA do not
    assert g.kernel_name_nt(_cfg("double", "Add", "Min"), 8, 1 << 22, 8) == "ordered_nt"
    assert g.kernel_name_nt(_cfg("double", "Add", "Min"), 8, (1 << 22) - 8, 8) == "valu_tile_nt"
    # operators the register tile does not hold
    assert g.kernel_name_nt(_cfg("int", "And", "Add"), 128, 128, 128) == "ordered_nt"
    assert g.kernel_name_nt(_cfg("int", "Add", "Multiply"), 128, 128, 128) == "ordered_nt"
    assert g.kernel_name_nt(_cfg("int", "Add", "And"), 128, 128, 128) == "ordered_nt"
    # a matrix-core configuration on a shape whose M is no chunk multiple (not half): the VALU kernel
    assert g.kernel_name_nt(_cfg("float"), 130, 72, 131) == "valu_tile_nt"
    assert g.kernel_name_nt(_cfg("int"), 130, 72, 131) == "valu_tile_nt"               # int (Multiply, Add): exact on the VALU
    assert g.kernel_name_nt(_cfg("float"), 130, 70, 136) == "ordered_nt"


def test_nt_name_k_ordered_contract():
    for dtype, mp, red in (("float", "Multiply", "Add"), ("float", "Add", "Min"), ("half", "Multiply", "Add"), ("int", "Multiply", "Add"),
                           ("uint8_t", "Multiply", "Add"), ("double", "Min", "Max")):
        for shape in ((130, 72, 136), (4096, 4096, 4096), (37, 19, 41)):
            assert g.kernel_name_nt(_cfg(dtype, mp, red, g.PATH_ORDERED), *shape) == "ordered_nt", (dtype, mp, red, shape)
    old = g.get_tuning("half_contract")
    try:
        g.set_tuning("half_contract", 1)
        assert g.kernel_name_nt(_cfg("half"), 2048, 2048, 2048) == "ordered_nt"
        assert g.kernel_name_nt(_cfg("half", "Add", "Min"), 2048, 2048, 2048) == "valu_tile_nt"   # the knob is (Multiply, Add)'s
    finally:
        g.set_tuning("half_contract", old)


def test_nt_name_half_multiply_add_keeps_the_f32_contract_off_the_matrix_cores():
    h = _cfg("half")
    assert g.kernel_name_batched(h, 130, 72, 136, 1) == "ordered_wide_f16"     # K % 16 != 0: no matrix-core kernel
    assert g.kernel_name_nt(h, 130, 72, 136) == "ordered_nt"                   # never valu_tile_nt (binary16 sums)
    assert g.kernel_name_nt(h, 130, 80, 132) == "ordered_nt"                   # M % 8 != 0
    assert g.kernel_name_nt(h, 130, 80, 136) == "nt_prepass"


def test_nt_name_unsupported_and_invalid():
    name = g.kernel_name_nt
    for dtype in ("float", "half", "int"):
        assert name(_cfg(dtype, path=g.PATH_SPLIT), 1024, 1024, 1024) == "unsupported"
        for path in (g.PATH_AUTO, g.PATH_ORDERED):
            assert name(_cfg(dtype, path=path, transposed_a=True), 1024, 1024, 1024) == "unsupported"
    assert name(g.Config(99, 1, 0, 0, 0), 1024, 1024, 1024) == "invalid"
    assert name(g.Config(0, 1, 0, 7, 0), 1024, 1024, 1024) == "invalid"


# ---- refusals --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("call", [_enq, _launch], ids=["enqueue", "launch"])
@pytest.mark.parametrize("acc", [0, 1], ids=["plain", "accumulate"])
def test_nt_refusals_without_a_device(call, acc):
    for dt in ("float", "half", "int8_t", "long"):
        assert call(_cfg(dt, path=g.PATH_SPLIT), acc=acc) == MM_ERR_UNSUPPORTED and "MM_PATH_AUTO or MM_PATH_ORDERED" in _err(), dt
        assert call(_cfg(dt, transposed_a=True), acc=acc) == MM_ERR_UNSUPPORTED and "row-major A" in _err(), dt
        assert call(g.Config(99, 1, 0, 0, 0), acc=acc) == MM_ERR_BAD_ARGUMENT and "invalid mm_config_t" in _err()
        assert call(g.Config(g.DTYPES[dt], 1, 0, 7, 0), acc=acc) == MM_ERR_BAD_ARGUMENT and "invalid mm_config_t" in _err()
        for kw in ("a", "b", "c"):
            assert call(_cfg(dt), acc=acc, **{kw: 0}) == MM_ERR_BAD_ARGUMENT and "null matrix pointer" in _err(), kw
        assert call(_cfg(dt), sc=E - 1, acc=acc) == MM_ERR_BAD_ARGUMENT and "stride_c" in _err() and "overlap" in _err()
    f, span = _cfg("float", "Add", "Min"), 4 * E * 4    # 4 elements of 64 x 64 floats
    for kw in ({"c": A0}, {"c": B0}, {"c": A0 + span - 64}, {"c": B0 + span - 64}, {"c": A0 - span + 64}, {"c": B0 - span + 64}):
        assert call(f, acc=acc, **kw) == MM_ERR_BAD_ARGUMENT and "c overlaps a or b" in _err(), kw
    assert call(f, b=C0 + 3 * E * 4, sb=0, acc=acc) == MM_ERR_BAD_ARGUMENT and "c overlaps a or b" in _err()   # a broadcast Bt inside C's span
    # Bt's extent is M * K elements: the last 16 bytes of a tall Bt (M = 256, K = 16) still count
    tall = dict(n=16, k=16, m=256, batch=1, sa=0, sb=0, sc=0)
    assert call(f, c=B0 + 256 * 16 * 4 - 16, acc=acc, **tall) == MM_ERR_BAD_ARGUMENT and "c overlaps a or b" in _err()


@pytest.mark.parametrize("call", [_enq, _launch], ids=["enqueue", "launch"])
def test_nt_k0_and_empty_calls(call):
    for cfg in (_cfg("float"), _cfg("half", path=g.PATH_ORDERED), _cfg("int", "Add", "Min"), _cfg("double")):
        assert call(cfg, k=0) == MM_ERR_BAD_ARGUMENT and "size_k must be positive" in _err()    # the plain form needs K
        assert call(cfg, k=0, acc=1) == MM_OK, _err()                                           # accumulating over no k: a no-op
        for acc in (0, 1):
            assert call(cfg, n=0, acc=acc) == MM_OK
            assert call(cfg, m=0, acc=acc) == MM_OK
            assert call(cfg, batch=0, acc=acc) == MM_OK
            assert call(cfg, batch=0, a=0, b=0, c=0, acc=acc) == MM_OK
    assert call(_cfg("float"), k=0, acc=1, c=0) == MM_ERR_BAD_ARGUMENT   # K = 0 accumulating still runs the argument checks
    assert call(_cfg("float", path=g.PATH_SPLIT), k=0, acc=1) == MM_ERR_UNSUPPORTED
    assert call(_cfg("float", transposed_a=True), n=0) == MM_ERR_UNSUPPORTED


def test_nt_launch_reports_zero_time_for_a_no_op():
    t = ctypes.c_double(-1.0)
    assert g.lib().mm_gemm_nt_launch(0, ctypes.byref(_cfg()), A0, B0, C0, 64, 0, 64, 4, E, E, E, 1, ctypes.byref(t)) == MM_OK
    assert t.value == 0.0


def test_nt_valid_call_needs_a_device_and_a_may_be_bt():
    # device -1 is refused only AFTER every argument check, so nothing is launched on any machine
    for cfg in (_cfg("float"), _cfg("float", "Add", "Min"), _cfg("half"), _cfg("int", path=g.PATH_ORDERED)):
        for acc in (0, 1):
            for kw in ({}, {"b": A0}, {"b": A0, "sb": 0}, {"b": A0 + 64}):       # A == Bt, and overlapping inputs, pass the checks
                rc = _launch(cfg, device=-1, acc=acc, **kw)
                assert rc in (MM_ERR_NO_DEVICE, MM_ERR_BAD_ARGUMENT), rc
                assert "overlap" not in _err() and "null" not in _err() and "A x B^T" not in _err(), _err()
    if g.lib().mm_init(None) != MM_ERR_NO_DEVICE:
        return   # a GPU is present: the fake addresses below must never reach a kernel
    for call in (_enq, _launch):
        for cfg in (_cfg("float"), _cfg("float", "Add", "Min"), _cfg("half"), _cfg("int8_t", path=g.PATH_ORDERED)):
            for acc in (0, 1):
                assert call(cfg, acc=acc) == MM_ERR_NO_DEVICE, (call.__name__, _err())
                assert call(cfg, b=A0, acc=acc) == MM_ERR_NO_DEVICE, (call.__name__, _err())
        assert call(_cfg("float", "Add", "Min"), c=C0 + 4, b=B0 + 4, sa=E + 1) == MM_ERR_NO_DEVICE, _err()   # element-aligned is enough


def test_nt_binding_refuses_bad_tensors():
    torch = pytest.importorskip("torch")
    a, b = torch.zeros((8, 16), dtype=torch.float32), torch.zeros((12, 16), dtype=torch.float32)
    with pytest.raises(g.MMError, match="device tensors"):
        g.matmul_nt(a, b)
    with pytest.raises(g.MMError, match="device tensors"):
        g.addmm_nt_(torch.zeros((8, 12)), a, b)

    class Dev:
        """A meta tensor that claims to live on a device: the checks under test read attributes only, and fail first."""
        is_cuda = True

        def __init__(self, t):
            self.t = t

        def __getattr__(self, name):
            return getattr(self.t, name)

    def dev(*shape, dtype=torch.float32):
        return Dev(torch.zeros(shape, dtype=dtype, device="meta"))

    with pytest.raises(g.MMError, match=r"inner dimensions differ.*\(M, K\)"):
        g.matmul_nt(dev(8, 16), dev(16, 12))                                   # a K x M b
    with pytest.raises(g.MMError, match="do not match torch.float32"):
        g.matmul_nt(dev(8, 16), dev(12, 16, dtype=torch.float16))
    with pytest.raises(g.MMError, match="do not match torch.float16"):
        g.matmul_nt(dev(8, 16), dev(12, 16), dtype="half")
    with pytest.raises(g.MMError, match=r"b \(M, K\) must be a dense row-major matrix"):
        g.matmul_nt(dev(8, 16), Dev(torch.zeros((16, 12), device="meta").t()))   # a transposed view is not M x K storage
    with pytest.raises(g.MMError, match=r"each matrix of b \(M, K\) must be dense"):
        g.matmul_nt(dev(8, 16), Dev(torch.zeros((3, 12, 32), device="meta")[:, :, ::2]))
    with pytest.raises(g.MMError, match="batch sizes differ"):
        g.matmul_nt(dev(2, 8, 16), dev(3, 12, 16))
    with pytest.raises(g.MMError, match=r"out must be a contiguous torch.float32 tensor of shape \(8, 12\)"):
        g.matmul_nt(dev(8, 16), dev(12, 16), out=dev(12, 8))
    with pytest.raises(g.MMError, match=r"c has shape \(12, 8\), expected \(8, 12\)"):
        g.addmm_nt_(dev(12, 8), dev(8, 16), dev(12, 16))
    with pytest.raises(g.MMError, match="2-D or 3-D"):
        g.addmm_nt_(dev(8), dev(8, 16), dev(12, 16))
