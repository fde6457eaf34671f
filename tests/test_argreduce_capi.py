"""CPU tests of the argmin / argmax entry points (mm_gemm_argreduce_*, mm_kernel_name_argreduce): the header, the binding and
EXPORTS agree; bad arguments are refused before any device is touched; K = 0 accumulating and empty batches are no-ops; a
valid call without a GPU fails with MM_ERR_NO_DEVICE; the kernel names follow shape, layout, map and path; and no argreduce
kernel uses scratch (hipcc cross-compiles the three units here)."""
import concurrent.futures
import ctypes
import os
import re
import subprocess

import pytest

import gemm_hls_amd as g

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "mm_gemm.h")).read()
SYMBOLS = ("mm_gemm_argreduce_enqueue", "mm_gemm_argreduce_launch", "mm_kernel_name_argreduce")
MM_OK, MM_ERR_NO_DEVICE, MM_ERR_BAD_ARGUMENT, MM_ERR_UNSUPPORTED = 0, 1, 2, 3
INT32_MAX = 2 ** 31 - 1

# Fake device addresses, never dereferenced: every call below is refused, or is a no-op, before a device is touched.
# 4 MiB apart, so that a 4 x 64 x 64 batch of any element size keeps A, B, C and I disjoint.
A0, B0, C0, I0 = 1 << 22, 2 << 22, 3 << 22, 4 << 22
E = 64 * 64


def _enq(cfg, a=A0, b=B0, c=C0, i=I0, n=64, k=64, m=64, batch=4, sa=E, sb=E, sc=E, base=0, acc=0):
    return g.lib().mm_gemm_argreduce_enqueue(None, ctypes.byref(cfg), a, b, c, i, n, k, m, batch, sa, sb, sc, base, acc)


def _launch(cfg, a=A0, b=B0, c=C0, i=I0, n=64, k=64, m=64, batch=4, sa=E, sb=E, sc=E, base=0, acc=0, device=0):
    t = ctypes.c_double(-1.0)
    return g.lib().mm_gemm_argreduce_launch(device, ctypes.byref(cfg), a, b, c, i, n, k, m, batch, sa, sb, sc, base, acc,
                                            ctypes.byref(t))


def _err():
    return g.lib().mm_last_error().decode()


def _minplus(path=g.PATH_AUTO, dtype="float", reduce_op="Min", map_op="Add"):
    return g.make_config(dtype, map_op, reduce_op, path)


def test_argreduce_symbols_declared_exported_and_bound():
    for sym in SYMBOLS:
        assert re.search(rf"^(int|const char)\s*\*?\s*{sym}\(", HEADER, flags=re.M), sym
        assert sym in g.EXPORTS
        assert getattr(g.lib(), sym).argtypes is not None
    assert callable(g.matmul_argreduce) and callable(g.addmm_argreduce_)


@pytest.mark.parametrize("call", [_enq, _launch], ids=["enqueue", "launch"])
@pytest.mark.parametrize("acc", [0, 1], ids=["plain", "accumulate"])
def test_argreduce_refusals_without_a_device(call, acc):
    f32 = _minplus()
    # reductions other than Min / Max, and MM_PATH_SPLIT
    for red in ("Add", "Multiply", "And"):
        assert call(_minplus(reduce_op=red), acc=acc) == MM_ERR_UNSUPPORTED, red
    assert call(g.make_config("float", "Add", "Min", g.PATH_SPLIT), acc=acc) == MM_ERR_UNSUPPORTED
    assert call(g.Config(99, 0, 3, 0, 0), acc=acc) == MM_ERR_BAD_ARGUMENT          # unknown enums
    # null pointers, the index matrix among them
    for kw in ("a", "b", "c", "i"):
        assert call(f32, acc=acc, **{kw: 0}) == MM_ERR_BAD_ARGUMENT, kw
    assert call(f32, i=0, acc=acc) == MM_ERR_BAD_ARGUMENT and "index" in _err()
    # outputs of the batch overlapping
    assert call(f32, sc=E - 1, acc=acc) == MM_ERR_BAD_ARGUMENT and "overlap" in _err()
    # index_base: negative, or index_base + K - 1 beyond INT32_MAX; the largest admissible one is accepted by the checks
    assert call(f32, base=-1, acc=acc) == MM_ERR_BAD_ARGUMENT and "index_base" in _err()
    assert call(f32, base=INT32_MAX - 62, acc=acc) == MM_ERR_BAD_ARGUMENT and "int32" in _err()
    assert call(f32, base=INT32_MAX, acc=acc) == MM_ERR_BAD_ARGUMENT
    assert call(f32, base=INT32_MAX - 63, n=0, acc=acc) == MM_OK
    # C or I overlapping A, B, or each other (the accumulating calls' span test)
    for kw in ({"c": A0}, {"c": B0}, {"i": A0}, {"i": B0}, {"i": C0}, {"c": I0}, {"i": C0 + 4 * E * 4 - 64},
               {"c": B0 + 4 * E * 4 - 64}, {"i": A0 - 4 * E * 4 + 64}):
        assert call(f32, acc=acc, **kw) == MM_ERR_BAD_ARGUMENT and "overlap" in _err(), kw
    # a broadcast B whose single matrix lies inside I's span
    assert call(f32, b=I0 + 2 * 4 * E, sb=0, acc=acc) == MM_ERR_BAD_ARGUMENT and "overlap" in _err()


@pytest.mark.parametrize("call", [_enq, _launch], ids=["enqueue", "launch"])
def test_argreduce_k0_and_empty_calls(call):
    for cfg in (_minplus(), _minplus(g.PATH_ORDERED, "int", "Max"), _minplus(dtype="half")):
        assert call(cfg, k=0) == MM_ERR_BAD_ARGUMENT and "size_k" in _err()    # the plain form needs K
        assert call(cfg, k=0, acc=1) == MM_OK, _err()                             # accumulating over no k: a no-op
        for acc in (0, 1):
            assert call(cfg, n=0, acc=acc) == MM_OK
            assert call(cfg, m=0, acc=acc) == MM_OK
            assert call(cfg, batch=0, acc=acc) == MM_OK
            assert call(cfg, batch=0, a=0, b=0, c=0, i=0, acc=acc) == MM_OK
    # K = 0 accumulating still runs the argument checks
    assert call(_minplus(), k=0, acc=1, i=0) == MM_ERR_BAD_ARGUMENT
    assert call(_minplus(), k=0, acc=1, c=I0) == MM_ERR_BAD_ARGUMENT   # (A and B span nothing when K = 0)
    assert call(_minplus(reduce_op="Add"), k=0, acc=1) == MM_ERR_UNSUPPORTED


def test_argreduce_launch_reports_zero_time_for_a_no_op():
    t = ctypes.c_double(-1.0)
    assert g.lib().mm_gemm_argreduce_launch(0, ctypes.byref(_minplus()), A0, B0, C0, I0, 64, 0, 64, 4, E, E, E, 0, 1,
                                            ctypes.byref(t)) == MM_OK
    assert t.value == 0.0


def test_argreduce_valid_call_needs_a_device():
    # device -1 is refused only AFTER every argument check, so nothing is launched on any machine
    for acc in (0, 1):
        rc = _launch(_minplus(), device=-1, acc=acc)
        assert rc in (MM_ERR_NO_DEVICE, MM_ERR_BAD_ARGUMENT), rc
        assert "overlap" not in _err() and "index" not in _err(), _err()
    if g.lib().mm_init(None) != MM_ERR_NO_DEVICE:
        return   # a GPU is present: the fake addresses below must never reach a kernel
    for call in (_enq, _launch):
        for cfg in (_minplus(), _minplus(g.PATH_ORDERED), _minplus(dtype="double", reduce_op="Max"),
                    _minplus(dtype="uint8_t", map_op="And")):
            for acc in (0, 1):
                assert call(cfg, acc=acc) == MM_ERR_NO_DEVICE, (call.__name__, _err())
        # a misaligned pointer is not refused: it runs the predicated kernel
        assert call(_minplus(), c=C0 + 4) == MM_ERR_NO_DEVICE, _err()


def test_kernel_name_argreduce_by_shape_layout_map_and_path():
    name = g.kernel_name_argreduce
    f32 = _minplus()
    assert name(f32, 200, 68, 132) == "argreduce_tile"                    # K % 4, M % 4: the tile, ragged N included
    assert name(f32, 8192, 8192, 8192) == "argreduce_tile"
    assert name(f32, 128, 128, 128, 4096) == "argreduce_tile"
    assert name(f32, 67, 37, 61) == "argreduce"                           # K % 4 != 0
    assert name(f32, 64, 64, 62) == "argreduce"                           # M % 4 != 0
    kxn = g.make_config("float", "Add", "Min", g.PATH_AUTO, transposed_a=True)
    assert name(kxn, 200, 68, 132) == "argreduce_tile"
    assert name(kxn, 202, 68, 132) == "argreduce"                         # K x N A needs N % 4 == 0
    assert name(_minplus(map_op="And", dtype="int"), 256, 256, 256) == "argreduce"
    for dt in ("half", "int8_t", "uint16_t", "unsigned"):
        assert name(_minplus(dtype=dt, reduce_op="Max"), 256, 256, 256) == "argreduce_tile", dt
    for dt in ("double", "long", "unsigned long"):                      # the tile is for elements of at most 4 bytes
        assert name(_minplus(dtype=dt, reduce_op="Max"), 256, 256, 256) == "argreduce", dt
    assert name(_minplus(g.PATH_ORDERED), 8192, 8192, 8192) == "argreduce"
    assert name(_minplus(reduce_op="Add"), 256, 256, 256) == "unsupported"
    assert name(g.make_config("float", "Add", "Min", g.PATH_SPLIT), 256, 256, 256) == "unsupported"
    assert name(g.Config(99, 0, 3, 0, 0), 256, 256, 256) == "invalid"


def test_python_entry_points_refuse_host_tensors():
    torch = pytest.importorskip("torch")
    a, b = torch.zeros(4, 4), torch.zeros(4, 4)
    with pytest.raises(g.MMError, match="device tensors"):
        g.matmul_argreduce(a, b)
    with pytest.raises(g.MMError, match="device tensors"):
        g.addmm_argreduce_(torch.zeros(4, 4), torch.zeros(4, 4, dtype=torch.int32), a, b)


ARGREDUCE_UNITS = ("mm_argreduce_fp.hip", "mm_argreduce_int_narrow.hip", "mm_argreduce_int_wide.hip")


def _device_asm(unit):
    from gemm_hls_amd import build
    flags = [f for f in build.COMMON if f != "--offload-compress"]          # the flags the shipped objects are built with
    src = os.path.join(ROOT, "gemm_hls_amd", "csrc", unit)
    r = subprocess.run([build.HIPCC, *flags, *build.EXTRA.get(unit, []), "-S", "--cuda-device-only", src, "-o", "-"],
                       capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


def test_no_argreduce_kernel_spills():
    """Every kernel of the three argreduce units: no scratch_ instruction, a zero private segment, and no AGPR (the compiler's
    spill space once the 256 VGPRs are full: no v_accvgpr_* instruction, NumAgprs 0).  The units ask for contraction off
    themselves (#pragma), so they get no per-file flag."""
    from gemm_hls_amd import build
    assert not any(u in build.EXTRA for u in ARGREDUCE_UNITS)
    with concurrent.futures.ThreadPoolExecutor(max_workers=3) as ex:
        outputs = dict(zip(ARGREDUCE_UNITS, ex.map(_device_asm, ARGREDUCE_UNITS)))
    plain = tile = 0
    for unit, asm in outputs.items():
        assert "#pragma clang fp contract(off)" in open(os.path.join(ROOT, "gemm_hls_amd", "csrc", unit)).read(), unit
        names = re.findall(r"^(_Z\w*argreduce\w*):", asm, flags=re.M)
        assert names, unit
        tile += sum("argreduce_tile_kernel" in nm for nm in names)
        plain += sum("argreduce_kernel" in nm for nm in names)
        ops = {ln.split()[0] for ln in asm.split("\n") if ln.startswith("\t")}
        spill = sorted(op for op in ops if op.startswith(("scratch_", "v_accvgpr")))
        assert spill == [], (unit, spill)
        sizes = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", asm)
        assert sizes and all(s == "0" for s in sizes), (unit, sizes)
        agprs = re.findall(r"; NumAgprs:\s*(\d+)", asm)
        assert len(agprs) >= len(names) and all(a == "0" for a in agprs), (unit, sorted(set(agprs)))
    # {Min, Max} x {N x K, K x N A}: the plain kernel for 11 types x 5 maps, the tile for the 8 types of at most 4 bytes
    # and every map but And
    assert (plain, tile) == (11 * 5 * 4, 8 * 4 * 4), (plain, tile)
