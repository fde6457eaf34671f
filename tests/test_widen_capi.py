"""CPU tests of the widening entry points (mm_gemm_widen_*, mm_kernel_name_widen, mm_widen_dtype): the header, the binding and
EXPORTS agree; the wide kernel is the narrow batched resolver's with "_wide" appended, widen_ordered where that resolver
names no matrix-core kernel and always under MM_PATH_ORDERED; every refusal comes with its status and message before any
device is touched; K = 0 accumulating and empty batches are no-ops; the binding checks operands against the narrow torch
dtype and c / out against the wide one."""
import ctypes
import os
import re

import pytest

import gemm_hls_amd as g

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "mm_gemm.h")).read()
SYMBOLS = ("mm_gemm_widen_enqueue", "mm_gemm_widen_launch", "mm_kernel_name_widen", "mm_widen_dtype")
MM_OK, MM_ERR_NO_DEVICE, MM_ERR_BAD_ARGUMENT, MM_ERR_UNSUPPORTED = 0, 1, 2, 3

# Fake device addresses, never dereferenced: every call below is refused, or is a no-op, before a device is touched.
A0, B0, C0 = 1 << 22, 2 << 22, 3 << 22
E = 64 * 64


def _enq(cfg, a=A0, b=B0, c=C0, n=64, k=64, m=64, batch=4, sa=E, sb=E, sc=E, acc=0):
    return g.lib().mm_gemm_widen_enqueue(None, ctypes.byref(cfg), a, b, c, n, k, m, batch, sa, sb, sc, acc)


def _launch(cfg, a=A0, b=B0, c=C0, n=64, k=64, m=64, batch=4, sa=E, sb=E, sc=E, acc=0, device=0):
    t = ctypes.c_double(-1.0)
    return g.lib().mm_gemm_widen_launch(device, ctypes.byref(cfg), a, b, c, n, k, m, batch, sa, sb, sc, acc, ctypes.byref(t))


def _err():
    return g.lib().mm_last_error().decode()


def _cfg(dtype="half", path=g.PATH_AUTO, map_op="Multiply", reduce_op="Add", transposed_a=False):
    return g.make_config(dtype, map_op, reduce_op, path, transposed_a)


def test_widen_symbols_declared_exported_and_bound():
    for sym in SYMBOLS:
        assert re.search(rf"^(int|const char)\s*\*?\s*{sym}\(", HEADER, flags=re.M), sym
        assert sym in g.EXPORTS
        assert getattr(g.lib(), sym).argtypes is not None
    assert callable(g.matmul_wide) and callable(g.addmm_wide_) and callable(g.kernel_name_widen) and callable(g.widen_dtype)


def test_widen_dtype_names_the_accumulator_type():
    assert g.lib().mm_widen_dtype(g.DTYPES["half"]) == g.DTYPES["float"]
    assert g.lib().mm_widen_dtype(g.DTYPES["int8_t"]) == g.DTYPES["int"]
    others = [d for d in g.DTYPES if d not in ("half", "int8_t")]
    assert len(others) == 9
    for d in others:
        assert g.lib().mm_widen_dtype(g.DTYPES[d]) == -1, d
        assert g.widen_dtype(d) is None
    assert g.lib().mm_widen_dtype(99) == -1
    assert g.widen_dtype("half") == "float" and g.widen_dtype("int8_t") == "int"


# (dtype, transposed_a, (n, k, m), batch)
NAME_SHAPES = [
    ("half", False, (16384, 16384, 16384), 1),     # pingpong_16x16x32
    ("half", False, (512, 4096, 512), 1),          # K % 64 == 0: the ping-pong default whatever the tile pick
    ("half", False, (2048, 160, 2048), 1),         # K % 32 == 0, not % 64: pingpong_k32
    ("half", False, (2048, 48, 2048), 1),          # K % 16 == 0 only: slab64
    ("half", False, (300, 48, 256), 3),            # slab64, the tile pick counts the batch
    ("half", True, (2048, 2048, 2048), 2),         # K x N A where it lies
    ("half", False, (100, 72, 64), 1),             # K % 16 != 0: no matrix-core kernel
    ("half", False, (100, 64, 100), 2),            # M % 8 != 0
    ("int8_t", False, (16384, 16384, 16384), 1),   # pingpong_16x16x64
    ("int8_t", False, (1000, 320, 512), 1),        # K % 64 == 0, not % 128: pingpong_k64
    ("int8_t", False, (1000, 96, 512), 2),         # K % 32 == 0 only: slab128
    ("int8_t", True, (1024, 1024, 1024), 1),       # K x N A
    ("int8_t", False, (256, 256, 40), 1),          # M % 16 != 0
    ("int8_t", False, (256, 48, 256), 4),          # K % 32 != 0
]


def test_kernel_name_widen_table():
    seen = set()
    for dtype, t, (n, k, m), batch in NAME_SHAPES:
        cfg = _cfg(dtype, transposed_a=t)
        narrow = g.kernel_name_batched(cfg, n, k, m, batch)
        want = narrow + "_wide" if narrow.startswith("mfma_") else "widen_ordered"
        assert g.kernel_name_widen(cfg, n, k, m, batch) == want, (dtype, t, n, k, m, batch, narrow)
        assert g.kernel_name_widen(_cfg(dtype, g.PATH_ORDERED, transposed_a=t), n, k, m, batch) == "widen_ordered"
        seen.add(want)
    assert g.kernel_name_widen(_cfg("half"), 100, 72, 64) == "widen_ordered"
    assert g.kernel_name_widen(_cfg("int8_t"), 256, 256, 40) == "widen_ordered"
    # the table reaches both families' ping-pong, K x N and slab kernels, and the fallback
    for part in ("mfma_f16_256x256_pingpong_16x16x32_wide", "mfma_f16_256x256_pingpong_k32_wide", "slab64_wide", "mfma_f16_256x256_pingpong_k32_KxN_wide",
                 "mfma_i8_256x256_pingpong_16x16x64_wide", "mfma_i8_256x256_pingpong_k64_wide", "slab128_wide", "mfma_i8_256x256_pingpong_k64_KxN_wide",
                 "widen_ordered"):
        assert any(part in s for s in seen), (part, sorted(seen))
    assert g.kernel_name_widen(_cfg("half"), 512, 512, 512, 0) == g.kernel_name_widen(_cfg("half"), 512, 512, 512, 1)


# A (knob value, K x N A, (n, k, m)) whose batched resolver picks each row of a family's kernel table
ROW_SHAPES = {
    "f16": ("f16_variant", {
        "mfma_f16_256x256_pingpong_16x16x32": (-1, False, (256, 256, 256)), "mfma_f16_256x256_pingpong_32x32x16": (100, False, (256, 256, 256)),
        "mfma_f16_256x256_pingpong_k32": (-1, False, (256, 128, 256)), "mfma_f16_256x256_pingpong_k32_KxN": (-1, True, (256, 256, 256)),
        "mfma_f16_256x256x64_slab64": (0, False, (256, 48, 256)), "mfma_f16_256x256x64_slab64_KxN": (0, True, (256, 48, 256)),
        "mfma_f16_128x256x64_slab64": (4, False, (256, 48, 256)), "mfma_f16_64x256x64_slab64": (5, False, (256, 48, 256))}),
    "i8": ("i8_variant", {
        "mfma_i8_256x256_pingpong_16x16x64": (-1, False, (512, 512, 512)), "mfma_i8_256x256_pingpong_32x32x32": (100, False, (512, 512, 512)),
        "mfma_i8_256x256_pingpong_k64": (-1, False, (256, 256, 256)), "mfma_i8_256x256_pingpong_k64_KxN": (-1, True, (256, 256, 256)),
        "mfma_i8_256x256x128_slab128": (0, False, (256, 96, 256)), "mfma_i8_256x256x128_slab128_KxN": (0, True, (256, 96, 256)),
        "mfma_i8_64x256x128_slab128": (5, False, (256, 96, 256))}),
}


@pytest.mark.parametrize("family", ["i8", "f16"])
def test_every_narrow_matrix_core_kernel_has_a_wide_instantiation(family):
    """A family's kernels are described in ONE table (mm_mfma_<family>_kernels.inc), which the narrow and the wide unit both
    include: each row names the kernel and its wide twin, and one launch_kind serves both C types.  No unit keeps a second
    name table or a second switch, and every row's shape resolves to that row's wide name."""
    csrc = os.path.join(ROOT, "gemm_hls_amd", "csrc")
    inc, narrow_unit, wide_unit = (open(os.path.join(csrc, f)).read() for f in
                                   (f"mm_mfma_{family}_kernels.inc", f"mm_mfma_{family}.hip", f"mm_mfma_{family}_wide.hip"))
    everything = inc + narrow_unit + wide_unit
    assert len(re.findall(r"\w+\[\] = \{\s*kernel_row<", everything)) == 1 and inc.count("kTable[] = {") == 1
    for gone in ("kNarrow", "kWide", "kNames", "launch_index"):
        assert gone not in everything, gone
    assert inc.count("switch (") == 1 and "switch (" not in wide_unit and "case K_" not in narrow_unit + wide_unit
    body = re.search(r"kTable\[\] = \{(.*?)\n\};", inc, flags=re.S).group(1)
    rows = re.findall(r'kernel_row<\w+>\("([^"]+)", (?:"([^"]+)"|nullptr)', body)
    assert len(rows) >= 8 and rows[-1] == ("unsupported", "")
    assert inc.count("case K_") == len(rows) - 1          # one launch per kernel
    knob, shapes = ROW_SHAPES[family]
    assert sorted(shapes) == sorted(name for name, _ in rows[:-1])
    dtype = {"i8": "int8_t", "f16": "half"}[family]
    old = g.get_tuning(knob)
    try:
        for name, wide in rows[:-1]:
            assert wide == name + "_wide"
            value, transposed, (n, k, m) = shapes[name]
            g.set_tuning(knob, value)
            cfg = _cfg(dtype, transposed_a=transposed)
            assert g.kernel_name_batched(cfg, n, k, m, 1) == name
            assert g.kernel_name_widen(cfg, n, k, m, 1) == wide
    finally:
        g.set_tuning(knob, old)


def test_kernel_name_widen_unsupported_and_invalid():
    name = g.kernel_name_widen
    for path in (g.PATH_AUTO, g.PATH_ORDERED):
        assert name(_cfg("uint8_t", path), 1024, 1024, 1024) == "unsupported"
        assert name(_cfg("float", path), 1024, 1024, 1024) == "unsupported"
        assert name(_cfg("half", path, "Add", "Min"), 1024, 1024, 1024) == "unsupported"
    assert name(_cfg("half", g.PATH_SPLIT), 1024, 1024, 1024) == "unsupported"
    assert name(_cfg("int8_t", g.PATH_SPLIT), 1024, 1024, 1024) == "unsupported"
    assert name(g.Config(99, 1, 0, 0, 0), 1024, 1024, 1024) == "invalid"


def test_the_half_contract_knob_does_not_apply():
    old = g.get_tuning("half_contract")
    try:
        g.set_tuning("half_contract", 1)
        assert g.kernel_name_widen(_cfg("half"), 2048, 2048, 2048) == "mfma_f16_256x256_pingpong_16x16x32_wide"
    finally:
        g.set_tuning("half_contract", old)


@pytest.mark.parametrize("call", [_enq, _launch], ids=["enqueue", "launch"])
@pytest.mark.parametrize("acc", [0, 1], ids=["plain", "accumulate"])
def test_widen_refusals_without_a_device(call, acc):
    for dt in ("float", "double", "uint8_t", "int16_t", "uint16_t", "int", "unsigned", "long", "unsigned long"):
        assert call(_cfg(dt), acc=acc) == MM_ERR_UNSUPPORTED and "widening serves half and int8_t" in _err(), dt
    for mp, red in (("Add", "Min"), ("Add", "Add"), ("Multiply", "Max"), ("And", "Add"), ("Min", "Max")):
        for dt in ("half", "int8_t"):
            assert call(_cfg(dt, map_op=mp, reduce_op=red), acc=acc) == MM_ERR_UNSUPPORTED and "(Multiply, Add)" in _err()
    for dt in ("half", "int8_t"):
        assert call(_cfg(dt, g.PATH_SPLIT), acc=acc) == MM_ERR_UNSUPPORTED and "MM_PATH_AUTO or MM_PATH_ORDERED" in _err()
        assert call(g.Config(99, 1, 0, 0, 0), acc=acc) == MM_ERR_BAD_ARGUMENT and "invalid mm_config_t" in _err()
        assert call(g.Config(g.DTYPES[dt], 1, 0, 7, 0), acc=acc) == MM_ERR_BAD_ARGUMENT and "invalid mm_config_t" in _err()
        for kw in ("a", "b", "c"):
            assert call(_cfg(dt), acc=acc, **{kw: 0}) == MM_ERR_BAD_ARGUMENT and "null matrix pointer" in _err(), kw
        assert call(_cfg(dt), sc=E - 1, acc=acc) == MM_ERR_BAD_ARGUMENT and "stride_c" in _err() and "overlap" in _err()
    # C's span counts 4-byte elements, A's and B's their own: half, 4 elements of 64 x 64
    h, c_bytes, a_bytes = _cfg("half"), 4 * E * 4, 4 * E * 2
    for kw in ({"c": A0}, {"c": B0}, {"c": B0 + a_bytes - 64}, {"c": A0 - c_bytes + 64}):
        assert call(h, acc=acc, **kw) == MM_ERR_BAD_ARGUMENT and "c overlaps a or b" in _err(), kw
    assert call(h, b=C0 + 3 * E * 4, sb=0, acc=acc) == MM_ERR_BAD_ARGUMENT and "c overlaps a or b" in _err()   # a broadcast B inside C's span
    assert call(_cfg("int8_t"), c=A0 + 4 * E - 16, acc=acc) == MM_ERR_BAD_ARGUMENT and "c overlaps a or b" in _err()


@pytest.mark.parametrize("call", [_enq, _launch], ids=["enqueue", "launch"])
def test_widen_k0_and_empty_calls(call):
    for cfg in (_cfg("half"), _cfg("int8_t", g.PATH_ORDERED), _cfg("half", transposed_a=True), _cfg("int8_t")):
        assert call(cfg, k=0) == MM_ERR_BAD_ARGUMENT and "size_k must be positive" in _err()    # the plain form needs K
        assert call(cfg, k=0, acc=1) == MM_OK, _err()                                           # accumulating over no k: a no-op
        for acc in (0, 1):
            assert call(cfg, n=0, acc=acc) == MM_OK
            assert call(cfg, m=0, acc=acc) == MM_OK
            assert call(cfg, batch=0, acc=acc) == MM_OK
            assert call(cfg, batch=0, a=0, b=0, c=0, acc=acc) == MM_OK
    assert call(_cfg("half"), k=0, acc=1, c=0) == MM_ERR_BAD_ARGUMENT   # K = 0 accumulating still runs the argument checks
    assert call(_cfg("uint8_t"), k=0, acc=1) == MM_ERR_UNSUPPORTED


def test_widen_launch_reports_zero_time_for_a_no_op():
    t = ctypes.c_double(-1.0)
    assert g.lib().mm_gemm_widen_launch(0, ctypes.byref(_cfg()), A0, B0, C0, 64, 0, 64, 4, E, E, E, 1, ctypes.byref(t)) == MM_OK
    assert t.value == 0.0


def test_widen_valid_call_needs_a_device():
    # device -1 is refused only AFTER every argument check, so nothing is launched on any machine
    for dt in ("half", "int8_t"):
        for acc in (0, 1):
            rc = _launch(_cfg(dt), device=-1, acc=acc)
            assert rc in (MM_ERR_NO_DEVICE, MM_ERR_BAD_ARGUMENT), rc
            assert "overlap" not in _err() and "widening" not in _err(), _err()
    if g.lib().mm_init(None) != MM_ERR_NO_DEVICE:
        return   # a GPU is present: the fake addresses below must never reach a kernel
    for call in (_enq, _launch):
        for cfg in (_cfg("half"), _cfg("int8_t"), _cfg("half", g.PATH_ORDERED), _cfg("int8_t", transposed_a=True)):
            for acc in (0, 1):
                assert call(cfg, acc=acc) == MM_ERR_NO_DEVICE, (call.__name__, _err())
        assert call(_cfg("half"), c=C0 + 4, a=A0 + 2, sa=E + 1) == MM_ERR_NO_DEVICE, _err()   # element-aligned is enough


def test_binding_refuses_bad_tensors():
    torch = pytest.importorskip("torch")
    a, b = torch.zeros((8, 16), dtype=torch.float16), torch.zeros((16, 8), dtype=torch.float16)
    with pytest.raises(g.MMError, match="device tensors"):
        g.matmul_wide(a, b)
    with pytest.raises(g.MMError, match="device tensors"):
        g.addmm_wide_(torch.zeros((8, 8), dtype=torch.float32), a, b)
    with pytest.raises(g.MMError, match="half or int8_t"):
        g.matmul_wide(a.float(), b.float(), dtype="float")
    with pytest.raises(g.MMError, match="half or int8_t"):
        g.addmm_wide_(torch.zeros((8, 8), dtype=torch.int32), a, b, dtype="uint8_t")
    class Dev:
        """A meta tensor that claims to live on a device: the checks under test read attributes only, and fail first."""
        is_cuda = True

        def __init__(self, t):
            self.t = t

        def __getattr__(self, name):
            return getattr(self.t, name)

    da, db = Dev(a.to("meta")), Dev(b.to("meta"))
    with pytest.raises(g.MMError, match="do not match torch.int8"):       # a wrong operand dtype
        g.matmul_wide(da, db, dtype="int8_t")
    with pytest.raises(g.MMError, match="do not match torch.float32"):    # a half c
        g.addmm_wide_(Dev(torch.zeros((8, 8), dtype=torch.float16, device="meta")), da, db)
    with pytest.raises(g.MMError, match="out must be a contiguous torch.float32 tensor of shape \\(8, 8\\)"):   # a mis-shaped out
        g.matmul_wide(da, db, out=Dev(torch.zeros((8, 4), dtype=torch.float32, device="meta")))
    with pytest.raises(g.MMError, match="out must be a contiguous torch.float32"):                              # a half out
        g.matmul_wide(da, db, out=Dev(torch.zeros((8, 8), dtype=torch.float16, device="meta")))
