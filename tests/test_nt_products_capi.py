"""CPU tests of the A x B^T forms of argmin / argmax and of the log semiring (mm_gemm_argreduce_nt_*, mm_gemm_logsumexp_nt_*
and their resolvers): the header, the binding and EXPORTS agree; everything the row-major call of each product refuses is
refused here too, and MM_A_TRANSPOSED as in mm_gemm_nt_*, before any device is touched; K = 0 accumulating and empty batches
are no-ops; the kernel names follow configuration, shape, path and knob; and no kernel of the new units uses scratch or
AGPRs (hipcc cross-compiles the four units here)."""
import concurrent.futures
import ctypes
import os
import re
import subprocess

import pytest

import gemm_hls_amd as g

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "mm_gemm.h")).read()
SYMBOLS = ("mm_gemm_argreduce_nt_enqueue", "mm_gemm_argreduce_nt_launch", "mm_kernel_name_argreduce_nt",
           "mm_gemm_logsumexp_nt_enqueue", "mm_gemm_logsumexp_nt_launch", "mm_kernel_name_logsumexp_nt")
MM_OK, MM_ERR_NO_DEVICE, MM_ERR_BAD_ARGUMENT, MM_ERR_UNSUPPORTED = 0, 1, 2, 3
INT32_MAX = 2 ** 31 - 1

# Fake device addresses, never dereferenced: every call below is refused, or is a no-op, before a device is touched.
# 4 MiB apart, so that a 4 x 64 x 64 batch of any element size keeps A, Bt, C and I disjoint.
A0, B0, C0, I0 = 1 << 22, 2 << 22, 3 << 22, 4 << 22
E = 64 * 64


def _ar_enq(cfg, a=A0, b=B0, c=C0, i=I0, n=64, k=64, m=64, batch=4, sa=E, sb=E, sc=E, base=0, acc=0):
    return g.lib().mm_gemm_argreduce_nt_enqueue(None, ctypes.byref(cfg), a, b, c, i, n, k, m, batch, sa, sb, sc, base, acc)


def _ar_launch(cfg, a=A0, b=B0, c=C0, i=I0, n=64, k=64, m=64, batch=4, sa=E, sb=E, sc=E, base=0, acc=0, device=0):
    t = ctypes.c_double(-1.0)
    return g.lib().mm_gemm_argreduce_nt_launch(device, ctypes.byref(cfg), a, b, c, i, n, k, m, batch, sa, sb, sc, base, acc,
                                               ctypes.byref(t))


def _lse_enq(cfg, a=A0, b=B0, c=C0, n=64, k=64, m=64, batch=4, sa=E, sb=E, sc=E, acc=0):
    return g.lib().mm_gemm_logsumexp_nt_enqueue(None, ctypes.byref(cfg), a, b, c, n, k, m, batch, sa, sb, sc, acc)


def _lse_launch(cfg, a=A0, b=B0, c=C0, n=64, k=64, m=64, batch=4, sa=E, sb=E, sc=E, acc=0, device=0):
    t = ctypes.c_double(-1.0)
    return g.lib().mm_gemm_logsumexp_nt_launch(device, ctypes.byref(cfg), a, b, c, n, k, m, batch, sa, sb, sc, acc,
                                               ctypes.byref(t))


def _refused(rc, status, word=None):
    """rc is `status`, and mm_last_error() says why (and mentions `word`)."""
    err = g.lib().mm_last_error().decode()
    return rc == status and err != "" and (word is None or word in err)


def _minplus(path=g.PATH_AUTO, dtype="float", reduce_op="Min", map_op="Add", transposed_a=False):
    return g.make_config(dtype, map_op, reduce_op, path, transposed_a)


def _lse(dtype="float", reduce_op="Max", path=g.PATH_AUTO, map_op="Add", transposed_a=False):
    return g.make_config(dtype, map_op, reduce_op, path, transposed_a)


@pytest.fixture
def lse_variant():
    """Sets the lse_variant knob for one test and restores the previous value."""
    old = g.get_tuning("lse_variant")
    yield lambda v: g.set_tuning("lse_variant", v)
    g.set_tuning("lse_variant", old)


def test_nt_product_symbols_declared_exported_and_bound():
    for sym in SYMBOLS:
        assert re.search(rf"^(int|const char)\s*\*?\s*{sym}\(", HEADER, flags=re.M), sym
        assert sym in g.EXPORTS
        assert getattr(g.lib(), sym).argtypes is not None
    for fn in ("matmul_argreduce_nt", "addmm_argreduce_nt_", "matmul_logsumexp_nt", "addmm_logsumexp_nt_",
               "kernel_name_argreduce_nt", "kernel_name_logsumexp_nt"):
        assert callable(getattr(g, fn)), fn
    assert g.kernel_name_argreduce_nt(_minplus(), 200, 68, 132) == "argreduce_tile_nt"
    assert g.kernel_name_logsumexp_nt(_lse(), 64, 64, 64) == "lse_hybrid_nt"


@pytest.mark.parametrize("call", [_ar_enq, _ar_launch], ids=["enqueue", "launch"])
@pytest.mark.parametrize("acc", [0, 1], ids=["plain", "accumulate"])
def test_argreduce_nt_refusals_without_a_device(call, acc):
    f32 = _minplus()
    for path in (g.PATH_AUTO, g.PATH_ORDERED):                                     # A^T B^T is not served
        assert _refused(call(_minplus(path, transposed_a=True), acc=acc), MM_ERR_UNSUPPORTED, "row-major A")
    for red in ("Add", "Multiply", "And"):
        assert _refused(call(_minplus(reduce_op=red), acc=acc), MM_ERR_UNSUPPORTED), red
    assert _refused(call(g.make_config("float", "Add", "Min", g.PATH_SPLIT), acc=acc), MM_ERR_UNSUPPORTED)
    assert _refused(call(g.Config(99, 0, 3, 0, 0), acc=acc), MM_ERR_BAD_ARGUMENT)          # unknown enums
    for kw in ("a", "b", "c", "i"):                                                  # null pointers, the index among them
        assert _refused(call(f32, acc=acc, **{kw: 0}), MM_ERR_BAD_ARGUMENT, "null"), kw
    assert _refused(call(f32, sc=E - 1, acc=acc), MM_ERR_BAD_ARGUMENT, "overlap")     # outputs of the batch overlapping
    assert _refused(call(f32, base=-1, acc=acc), MM_ERR_BAD_ARGUMENT, "index_base")
    assert _refused(call(f32, base=INT32_MAX - 62, acc=acc), MM_ERR_BAD_ARGUMENT, "int32")
    assert call(f32, base=INT32_MAX - 63, n=0, acc=acc) == MM_OK
    # C or I overlapping A, Bt, or each other
    for kw in ({"c": A0}, {"c": B0}, {"i": A0}, {"i": B0}, {"i": C0}, {"c": I0}, {"i": C0 + 4 * E * 4 - 64},
               {"c": B0 + 4 * E * 4 - 64}, {"i": A0 - 4 * E * 4 + 64}):
        assert _refused(call(f32, acc=acc, **kw), MM_ERR_BAD_ARGUMENT, "overlap"), kw
    assert _refused(call(f32, b=I0 + 2 * 4 * E, sb=0, acc=acc), MM_ERR_BAD_ARGUMENT, "overlap")   # a broadcast Bt inside I's span
    # Bt's extent is M x K whatever M and K are: 64 x 16 elements of Bt end where C begins, one more row overlaps it
    rc = _ar_launch(f32, b=C0 - 64 * 16 * 4, k=16, batch=1, device=-1, acc=acc)   # (device -1: refused after every check)
    assert rc in (MM_ERR_NO_DEVICE, MM_ERR_BAD_ARGUMENT) and "overlap" not in g.lib().mm_last_error().decode()
    assert _refused(call(f32, b=C0 - 63 * 16 * 4, k=16, batch=1, acc=acc), MM_ERR_BAD_ARGUMENT, "overlap")


@pytest.mark.parametrize("call", [_lse_enq, _lse_launch], ids=["enqueue", "launch"])
@pytest.mark.parametrize("acc", [0, 1], ids=["plain", "accumulate"])
def test_logsumexp_nt_refusals_without_a_device(call, acc, lse_variant):
    for path in (g.PATH_AUTO, g.PATH_ORDERED):
        assert _refused(call(_lse(path=path, transposed_a=True), acc=acc), MM_ERR_UNSUPPORTED, "row-major A")
    for dt in ("int8_t", "uint8_t", "int16_t", "uint16_t", "int", "unsigned", "long", "unsigned long"):
        assert _refused(call(_lse(dt), acc=acc), MM_ERR_UNSUPPORTED), dt
    for mp in ("Multiply", "And", "Min", "Max"):
        assert _refused(call(_lse(map_op=mp), acc=acc), MM_ERR_UNSUPPORTED), mp
    for red in ("Add", "Multiply", "And"):
        assert _refused(call(_lse(reduce_op=red), acc=acc), MM_ERR_UNSUPPORTED), red
    assert _refused(call(_lse(path=g.PATH_SPLIT), acc=acc), MM_ERR_UNSUPPORTED)
    assert _refused(call(g.Config(99, 0, 4, 0, 0), acc=acc), MM_ERR_BAD_ARGUMENT)
    for kw in ("a", "b", "c"):
        assert _refused(call(_lse(), acc=acc, **{kw: 0}), MM_ERR_BAD_ARGUMENT, "null"), kw
    assert _refused(call(_lse(), sc=E - 1, acc=acc), MM_ERR_BAD_ARGUMENT, "overlap")
    for kw in ({"c": A0}, {"c": B0}, {"c": B0 + 4 * E * 4 - 64}, {"c": A0 - 4 * E * 4 + 64}):
        assert _refused(call(_lse(), acc=acc, **kw), MM_ERR_BAD_ARGUMENT, "overlap"), kw
    assert _refused(call(_lse(), b=C0 + 2 * 4 * E, sb=0, acc=acc), MM_ERR_BAD_ARGUMENT, "overlap")
    for v in (-2, 3):
        lse_variant(v)
        assert _refused(call(_lse(), acc=acc), MM_ERR_BAD_ARGUMENT, "lse_variant"), v
        assert _refused(call(_lse(path=g.PATH_ORDERED), acc=acc), MM_ERR_BAD_ARGUMENT, "lse_variant"), v
        assert _refused(call(_lse(reduce_op="Add"), acc=acc), MM_ERR_UNSUPPORTED), v   # an unsupported configuration says so first


@pytest.mark.parametrize("call,cfgs", [
    (_ar_enq, (_minplus(), _minplus(g.PATH_ORDERED, "int", "Max"), _minplus(dtype="half"))),
    (_ar_launch, (_minplus(), _minplus(g.PATH_ORDERED, "int", "Max"), _minplus(dtype="half"))),
    (_lse_enq, (_lse(), _lse("double", "Min", g.PATH_ORDERED), _lse("half"))),
    (_lse_launch, (_lse(), _lse("double", "Min", g.PATH_ORDERED), _lse("half")))],
    ids=["argreduce-enqueue", "argreduce-launch", "logsumexp-enqueue", "logsumexp-launch"])
def test_nt_products_k0_and_empty_calls(call, cfgs):
    for cfg in cfgs:
        assert _refused(call(cfg, k=0), MM_ERR_BAD_ARGUMENT, "size_k")                  # the plain form needs K
        assert call(cfg, k=0, acc=1) == MM_OK, g.lib().mm_last_error().decode()        # accumulating over no k: a no-op
        for acc in (0, 1):
            assert call(cfg, n=0, acc=acc) == MM_OK
            assert call(cfg, m=0, acc=acc) == MM_OK
            assert call(cfg, batch=0, acc=acc) == MM_OK
    assert _refused(call(cfgs[0], k=0, acc=1, c=0), MM_ERR_BAD_ARGUMENT)   # K = 0 accumulating still runs the argument checks


def test_nt_products_accept_one_buffer_for_a_and_bt_and_need_a_device():
    """A and Bt may be the same buffer: the checks pass, and only the device is missing (device -1 is refused after every
    argument check, so nothing is launched on any machine)."""
    for call, cfg in ((_ar_launch, _minplus()), (_lse_launch, _lse())):
        for acc in (0, 1):
            rc = call(cfg, b=A0, device=-1, acc=acc)
            assert rc in (MM_ERR_NO_DEVICE, MM_ERR_BAD_ARGUMENT), rc
            assert "overlap" not in g.lib().mm_last_error().decode()
    t = ctypes.c_double(-1.0)   # a no-op reports zero time
    assert g.lib().mm_gemm_argreduce_nt_launch(0, ctypes.byref(_minplus()), A0, B0, C0, I0, 64, 0, 64, 4, E, E, E, 0, 1,
                                               ctypes.byref(t)) == MM_OK and t.value == 0.0
    if g.lib().mm_init(None) != MM_ERR_NO_DEVICE:
        return   # a GPU is present: the fake addresses below must never reach a kernel
    for call, cfgs in (((_ar_enq, _ar_launch), (_minplus(), _minplus(g.PATH_ORDERED), _minplus(dtype="double", reduce_op="Max"),
                                                _minplus(dtype="uint8_t", map_op="And"))),
                       ((_lse_enq, _lse_launch), (_lse(), _lse(path=g.PATH_ORDERED), _lse("double", "Min"), _lse("half")))):
        for fn in call:
            for cfg in cfgs:
                for acc in (0, 1):
                    assert fn(cfg, acc=acc) == MM_ERR_NO_DEVICE, (fn.__name__, g.lib().mm_last_error().decode())
            assert fn(cfgs[0], c=C0 + 4) == MM_ERR_NO_DEVICE   # a misaligned pointer is not refused


def test_kernel_name_argreduce_nt_pins():
    name = g.kernel_name_argreduce_nt
    f32 = _minplus()
    assert name(f32, 200, 68, 132) == "argreduce_tile_nt"
    assert name(f32, 200, 68, 132, 5) == "argreduce_tile_nt"
    assert name(f32, 67, 37, 61) == "argreduce_nt"
    assert name(f32, 130, 72, 134) == "argreduce_nt"                          # M % 4 != 0
    assert name(f32, 130, 70, 132) == "argreduce_nt"                          # K % 4 != 0
    assert name(f32, 202, 68, 132) == "argreduce_tile_nt"                     # nothing is asked of N
    assert name(_minplus(dtype="double"), 200, 68, 132) == "argreduce_nt"     # the tile is for elements of at most 4 bytes
    assert name(_minplus(dtype="int", map_op="And", reduce_op="Max"), 200, 68, 132) == "argreduce_nt"
    for dt in ("half", "int8_t", "uint16_t", "unsigned", "int"):
        for mp in ("Add", "Multiply", "Min", "Max"):
            assert name(_minplus(dtype=dt, map_op=mp, reduce_op="Max"), 256, 256, 256) == "argreduce_tile_nt", (dt, mp)
    for dt in ("long", "unsigned long"):
        assert name(_minplus(dtype=dt), 256, 256, 256) == "argreduce_nt", dt
    for dt in g.DTYPES:                                                        # every MM_PATH_ORDERED configuration
        for mp in g.OPS:
            for rd in ("Min", "Max"):
                assert name(g.make_config(dt, mp, rd, g.PATH_ORDERED), 200, 68, 132) == "argreduce_nt", (dt, mp, rd)
    assert name(_minplus(reduce_op="Add"), 200, 68, 132) == "unsupported"
    assert name(g.make_config("float", "Add", "Min", g.PATH_SPLIT), 200, 68, 132) == "unsupported"
    assert name(_minplus(transposed_a=True), 200, 68, 132) == "unsupported"
    assert name(g.Config(99, 0, 3, 0, 0), 200, 68, 132) == "invalid"
    # the row-major resolver is what it was
    assert g.kernel_name_argreduce(f32, 200, 68, 132) == "argreduce_tile"
    assert g.kernel_name_argreduce(f32, 67, 37, 61) == "argreduce"


def test_kernel_name_logsumexp_nt_follows_the_row_major_rule(lse_variant):
    for v in (-1, 0, 1, 2):
        lse_variant(v)
        for dt in ("half", "float", "double"):
            for red in ("Min", "Max"):
                for path in (g.PATH_AUTO, g.PATH_ORDERED):
                    cfg = _lse(dt, red, path)
                    row_major = g.kernel_name_logsumexp(cfg, 300, 64, 272)
                    assert row_major in ("lse_hybrid", "lse_exact")
                    assert g.kernel_name_logsumexp_nt(cfg, 300, 64, 272) == row_major + "_nt", (v, dt, red, path)
    lse_variant(3)
    assert g.kernel_name_logsumexp_nt(_lse(), 64, 64, 64) == "invalid"
    assert g.kernel_name_logsumexp_nt(_lse("int"), 64, 64, 64) == "unsupported"
    lse_variant(-1)
    for cfg in (_lse("int"), _lse(map_op="Multiply"), _lse(reduce_op="Add"), _lse(path=g.PATH_SPLIT), _lse(transposed_a=True)):
        assert g.kernel_name_logsumexp_nt(cfg, 64, 64, 64) == "unsupported"
    assert g.kernel_name_logsumexp_nt(g.Config(99, 0, 4, 0, 0), 64, 64, 64) == "invalid"


def test_python_entry_points_refuse_host_tensors_and_bad_shapes():
    torch = pytest.importorskip("torch")
    a, b = torch.zeros(4, 6), torch.zeros(5, 6)
    with pytest.raises(g.MMError, match="device tensors"):
        g.matmul_argreduce_nt(a, b)
    with pytest.raises(g.MMError, match="device tensors"):
        g.addmm_argreduce_nt_(torch.zeros(4, 5), torch.zeros(4, 5, dtype=torch.int32), a, b)
    with pytest.raises(g.MMError, match="device tensors"):
        g.matmul_logsumexp_nt(a, b)
    with pytest.raises(g.MMError, match="device tensors"):
        g.addmm_logsumexp_nt_(torch.zeros(4, 5), a, b)


NT_UNITS = ("mm_argreduce_nt_fp.hip", "mm_argreduce_nt_int_narrow.hip", "mm_argreduce_nt_int_wide.hip", "mm_lse_nt_fp.hip")


def _device_asm(unit):
    from gemm_hls_amd import build
    flags = [f for f in build.COMMON if f != "--offload-compress"]          # the flags the shipped objects are built with
    src = os.path.join(ROOT, "gemm_hls_amd", "csrc", unit)
    r = subprocess.run([build.HIPCC, *flags, *build.EXTRA.get(unit, []), "-S", "--cuda-device-only", src, "-o", "-"],
                       capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


def test_no_nt_product_kernel_spills():
    """Every kernel of the four new units: no scratch_ instruction and a zero private segment; the argreduce and exact
    kernels use no AGPR either (the compiler's spill space once the 256 VGPRs are full: no v_accvgpr_* instruction,
    NumAgprs 0) -- and neither does the expansion.  The units ask for contraction off themselves (#pragma)."""
    from gemm_hls_amd import build
    assert not any(u in build.EXTRA for u in NT_UNITS)
    with concurrent.futures.ThreadPoolExecutor(max_workers=4) as ex:
        outputs = dict(zip(NT_UNITS, ex.map(_device_asm, NT_UNITS)))
    counts = {"argreduce_tile_kernel": 0, "argreduce_kernel": 0, "lse_exact_kernel": 0, "lse_expand_kernel": 0}
    for unit, asm in outputs.items():
        assert "#pragma clang fp contract(off)" in open(os.path.join(ROOT, "gemm_hls_amd", "csrc", unit)).read(), unit
        names = re.findall(r"^(_Z\w+kernel\w*):", asm, flags=re.M)
        assert names, unit
        for nm in names:
            key = next((k for k in counts if k in nm), None)
            assert key, (unit, nm)     # a unit holds the M x K B kernels and nothing else
            counts[key] += 1
        ops = {ln.split()[0] for ln in asm.split("\n") if ln.startswith("\t")}
        spill = sorted(op for op in ops if op.startswith(("scratch_", "v_accvgpr")))
        assert spill == [], (unit, spill)
        sizes = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", asm)
        assert len(sizes) == len(names) and all(s == "0" for s in sizes), (unit, sizes)
        agprs = re.findall(r"; NumAgprs:\s*(\d+)", asm)
        assert len(agprs) >= len(names) and all(a == "0" for a in agprs), (unit, sorted(set(agprs)))
    # {Min, Max}: the plain kernel for 11 types x 5 maps, the tile for the 8 types of at most 4 bytes and every map but And;
    # the exact kernel and the expansion for half, float and double
    assert counts == {"argreduce_kernel": 11 * 5 * 2, "argreduce_tile_kernel": 8 * 4 * 2, "lse_exact_kernel": 6,
                      "lse_expand_kernel": 6}, counts
