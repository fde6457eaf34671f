"""CPU tests of the semiring closure (mm_closure_enqueue / _launch, mm_kernel_name_closure, closure_): the header, the binding
and EXPORTS agree; bad arguments are refused before any device is touched, with their status codes; n = 0 and batch = 0 are
no-ops; a valid call without a GPU fails with MM_ERR_NO_DEVICE; the kernel names follow n, the form and the block knob; no
closure kernel uses scratch, AGPRs or a private segment; the numpy restatement of the blocked algorithm that the GPU tests
use as their oracle equals plain Floyd-Warshall on absorptive inputs; and the graphs those tests draw have a closure that a
constant, or the input itself, could not pass for."""
import concurrent.futures
import ctypes
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

import _closure_ref as cr
import _semiring_ref as sr
import gemm_hls_amd as g

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "mm_gemm.h")).read()
SYMBOLS = ("mm_closure_enqueue", "mm_closure_launch", "mm_kernel_name_closure")
MM_OK, MM_ERR_NO_DEVICE, MM_ERR_BAD_ARGUMENT, MM_ERR_UNSUPPORTED = 0, 1, 2, 3

# Fake device addresses, never dereferenced: every call below is refused, or is a no-op, before a device is touched.
D0, W0 = 1 << 24, 2 << 24
N = 64
E = N * N


def _enq(cfg, d=D0, w=W0, n=N, batch=4, sd=E):
    return g.lib().mm_closure_enqueue(None, ctypes.byref(cfg), d, w, n, batch, sd)


def _launch(cfg, d=D0, w=W0, n=N, batch=4, sd=E, device=0):
    t = ctypes.c_double(-1.0)
    rc = g.lib().mm_closure_launch(device, ctypes.byref(cfg), d, w, n, batch, sd, ctypes.byref(t))
    _launch.elapsed = t.value
    return rc


def _err():
    return g.lib().mm_last_error().decode()


def _cfg(dtype="float", map_op="Add", reduce_op="Min", path=g.PATH_AUTO, transposed_a=False):
    return g.make_config(dtype, map_op, reduce_op, path, transposed_a)


class _Block:
    """closure_block set for the duration of a with-block."""
    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.old = g.get_tuning("closure_block")
        g.set_tuning("closure_block", self.value)

    def __exit__(self, *exc):
        g.set_tuning("closure_block", self.old)


def test_closure_symbols_declared_exported_and_bound():
    for sym in SYMBOLS:
        assert re.search(rf"^(int|const char)\s*\*?\s*{sym}\(", HEADER, flags=re.M), sym
        assert sym in g.EXPORTS
        assert getattr(g.lib(), sym).argtypes is not None
    assert callable(g.closure_) and callable(g.kernel_name_closure)
    assert "closure_block" in HEADER and "MM_CLOSURE_BLOCK" in open(
        os.path.join(ROOT, "gemm_hls_amd", "csrc", "mm_common.h")).read()


@pytest.mark.parametrize("call", [_enq, _launch], ids=["enqueue", "launch"])
@pytest.mark.parametrize("w", [W0, 0], ids=["witness", "values"])
def test_closure_refusals_without_a_device(call, w):
    f32 = _cfg()
    for red in ("Add", "Multiply", "And"):                       # not idempotent: no closure
        assert call(_cfg(reduce_op=red), w=w) == MM_ERR_UNSUPPORTED, red
        assert "idempotent" in _err()
    assert call(_cfg(path=g.PATH_SPLIT), w=w) == MM_ERR_UNSUPPORTED
    assert call(_cfg(transposed_a=True), w=w) == MM_ERR_BAD_ARGUMENT and "transpose" in _err()
    assert call(g.Config(99, 0, 3, 0, 0), w=w) == MM_ERR_BAD_ARGUMENT        # unknown enums
    assert call(f32, d=0, w=w) == MM_ERR_BAD_ARGUMENT and "null" in _err()
    assert call(f32, sd=E - 1, w=w) == MM_ERR_BAD_ARGUMENT and "overlap" in _err()
    if w:
        for wk in (D0, D0 + 4 * E * 4 - 4, D0 - 4 * E * 4 + 4, D0 + 2 * E * 4):
            assert call(f32, w=wk) == MM_ERR_BAD_ARGUMENT and "overlap" in _err(), hex(wk)


@pytest.mark.parametrize("call", [_enq, _launch], ids=["enqueue", "launch"])
def test_closure_block_knob_is_validated_at_call_time(call):
    for bad in (0, 32, 100, 512):
        with _Block(bad):
            assert g.get_tuning("closure_block") == bad   # the knob takes it; the call refuses it
            assert call(_cfg()) == MM_ERR_BAD_ARGUMENT and "closure_block" in _err(), bad
            assert g.kernel_name_closure(_cfg(), 300) == "invalid"
    with _Block(256):   # 256: value-only, elements of at most 4 bytes
        assert call(_cfg(), w=W0) == MM_ERR_BAD_ARGUMENT and "closure_block" in _err()
        assert call(_cfg("double"), w=0) == MM_ERR_BAD_ARGUMENT
        assert call(_cfg("long"), w=0) == MM_ERR_BAD_ARGUMENT
        assert call(_cfg(), d=0, w=0) == MM_ERR_BAD_ARGUMENT and "null" in _err()   # accepted, then the next check


@pytest.mark.parametrize("call", [_enq, _launch], ids=["enqueue", "launch"])
def test_closure_n0_and_batch0_are_no_ops(call):
    for cfg in (_cfg(), _cfg("int", "Min", "Max", g.PATH_ORDERED), _cfg("half")):
        for w in (W0, 0):
            assert call(cfg, n=0, w=w) == MM_OK, _err()
            assert call(cfg, batch=0, w=w) == MM_OK, _err()
            assert call(cfg, n=0, d=0, w=w) == MM_OK
            assert call(cfg, batch=0, d=0, sd=0, w=w) == MM_OK
            if call is _launch:
                assert _launch.elapsed == 0.0
    # the configuration checks still run
    assert call(_cfg(reduce_op="Add"), n=0) == MM_ERR_UNSUPPORTED
    assert call(_cfg(transposed_a=True), batch=0) == MM_ERR_BAD_ARGUMENT


def test_closure_valid_call_needs_a_device():
    # device -1 is refused only AFTER every argument check, so nothing is launched on any machine
    for w in (W0, 0):
        rc = _launch(_cfg(), device=-1, w=w)
        assert rc in (MM_ERR_NO_DEVICE, MM_ERR_BAD_ARGUMENT), rc
        assert "overlap" not in _err() and "null" not in _err(), _err()
    if g.lib().mm_init(None) != MM_ERR_NO_DEVICE:
        return   # a GPU is present: the fake addresses below must never reach a kernel
    for call in (_enq, _launch):
        for cfg in (_cfg(), _cfg(path=g.PATH_ORDERED), _cfg("double", "Multiply", "Max"), _cfg("uint8_t", "And", "Max")):
            for w in (W0, 0):
                for n in (N, 1000):
                    assert call(cfg, w=w, n=n, batch=4 if n == N else 1) == MM_ERR_NO_DEVICE, (call.__name__, _err())


def test_kernel_name_closure_by_n_form_and_knob():
    name = g.kernel_name_closure
    f32 = _cfg()
    assert name(f32, 1) == name(f32, 256) == name(f32, 64, 4096) == "closure_onchip"     # value-only float: B = 256
    assert name(f32, 257) == name(f32, 8192) == "closure_blocked"
    assert name(f32, 128, 1, True) == "closure_onchip" and name(f32, 129, 1, True) == "closure_blocked"   # witness: 128
    for dt in ("double", "long", "unsigned long"):                                          # 8-byte elements: 128
        assert name(_cfg(dt), 128) == "closure_onchip" and name(_cfg(dt), 129) == "closure_blocked", dt
    for dt in ("half", "int8_t", "uint16_t", "int", "unsigned"):
        assert name(_cfg(dt, "Max", "Min"), 256) == "closure_onchip", dt
    assert name(_cfg(path=g.PATH_ORDERED), 256) == "closure_onchip"
    with _Block(64):
        assert name(f32, 64) == "closure_onchip" and name(f32, 65) == "closure_blocked"
        assert name(_cfg("double"), 65, 1, True) == "closure_blocked"
    with _Block(-1):
        assert name(f32, 256) == "closure_onchip"
    for red in ("Add", "Multiply", "And"):
        assert name(_cfg(reduce_op=red), 64) == "unsupported"
    assert name(_cfg(path=g.PATH_SPLIT), 64) == "unsupported"
    assert name(_cfg(transposed_a=True), 64) == "invalid"
    assert name(g.Config(99, 0, 3, 0, 0), 64) == "invalid"


def test_closure_python_entry_point_refusals_on_the_host():
    torch = pytest.importorskip("torch")
    with pytest.raises(g.MMError, match="device tensors"):
        g.closure_(torch.zeros(4, 4))


CLOSURE_UNITS = ("mm_closure_fp.hip", "mm_closure_int_narrow.hip", "mm_closure_int_wide.hip")


def _device_asm(unit):
    from gemm_hls_amd import build
    flags = [f for f in build.COMMON if f != "--offload-compress"]          # the flags the shipped objects are built with
    src = os.path.join(ROOT, "gemm_hls_amd", "csrc", unit)
    r = subprocess.run([build.HIPCC, *flags, *build.EXTRA.get(unit, []), "-S", "--cuda-device-only", src, "-o", "-"],
                       capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


def test_no_closure_kernel_spills():
    """Every kernel of the three closure units: no scratch_ instruction, a zero private segment, no AGPR.  The units ask for
    contraction off themselves (#pragma)."""
    from gemm_hls_amd import build
    assert not any(u in build.EXTRA for u in CLOSURE_UNITS)
    with concurrent.futures.ThreadPoolExecutor(max_workers=3) as ex:
        outputs = dict(zip(CLOSURE_UNITS, ex.map(_device_asm, CLOSURE_UNITS)))
    diag = panel = 0
    for unit, asm in outputs.items():
        assert "#pragma clang fp contract(off)" in open(os.path.join(ROOT, "gemm_hls_amd", "csrc", unit)).read(), unit
        names = re.findall(r"^(_Z\w*closure\w*):", asm, flags=re.M)
        assert names, unit
        diag += sum("closure_diag_kernel" in nm for nm in names)
        panel += sum("closure_panel_kernel" in nm for nm in names)
        ops = {ln.split()[0] for ln in asm.split("\n") if ln.startswith("\t")}
        spill = sorted(op for op in ops if op.startswith(("scratch_", "v_accvgpr")))
        assert spill == [], (unit, spill)
        sizes = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", asm)
        assert sizes and all(s == "0" for s in sizes), (unit, sizes)
        agprs = re.findall(r"; NumAgprs:\s*(\d+)", asm)
        assert len(agprs) >= len(names) and all(a == "0" for a in agprs), (unit, sorted(set(agprs)))
    # 110 configurations x {values, witnesses}: diagonal blocks of 64 and 128 for every one, 256 for the value-only form of
    # the 8 types of at most 4 bytes; panels of 128 for every one, 256 for those
    assert (diag, panel) == (220 * 2 + 80, 220 + 80), (diag, panel)


def _absorptive(dtype, mp, rd, n, rng):
    """Inputs on which (dtype, mp, rd) is absorptive: the closure is well defined and blocking cannot change it."""
    t = sr.NP_DTYPES[dtype]
    if (mp, rd) == ("Add", "Min"):             # non-negative weights, "no edge" = max() / 2 for integers
        hi = 64 if dtype in ("int8_t", "uint8_t") else 1000
        d = rng.integers(0, hi, size=(n, n)).astype(t)
        if not sr.is_float(dtype):
            d[rng.random((n, n)) < 0.7] = sr.limits(dtype)[1] // 2 if hi > 64 else 60   # sums of two stay in range
        return d
    if (mp, rd) == ("Add", "Max"):             # a DAG: edges i -> j only for i < j, "no edge" = lowest() / 2
        d = rng.integers(0, 10, size=(n, n)).astype(t)
        lo = sr.limits(dtype)[0]
        d[np.tril_indices(n)] = -np.inf if sr.is_float(dtype) else lo // 2
        return d
    if (mp, rd) == ("And", "Max"):
        return (rng.random((n, n)) < 0.02).astype(t)
    return rng.integers(0, 100, size=(n, n)).astype(t)   # (Min, Max), (Max, Min): always absorptive


@pytest.mark.parametrize("dtype,mp,rd", [("float", "Add", "Min"), ("int", "Add", "Min"), ("double", "Add", "Max"),
                                         ("long", "Add", "Max"), ("half", "Min", "Max"), ("uint8_t", "Max", "Min"),
                                         ("uint8_t", "And", "Max"), ("int16_t", "Min", "Max")])
@pytest.mark.parametrize("n,block", [(40, 64), (64, 64), (165, 64), (200, 16), (97, 32)])
def test_blocked_restatement_equals_floyd_warshall_on_absorptive_inputs(dtype, mp, rd, n, block):
    rng = np.random.default_rng(n * 131 + block)
    d = _absorptive(dtype, mp, rd, n, rng)
    got, gw = cr.blocked(dtype, mp, rd, d, block, witness=True)
    want, _ = cr.floyd_warshall(dtype, mp, rd, d)
    assert sr.same_bits(got, want)
    # witnesses: every improved entry is the composition through its witness, every other kept its input
    t = sr.NP_DTYPES[dtype]
    i, j = np.nonzero(gw >= 0)
    v = gw[i, j]
    with np.errstate(all="ignore"):
        assert sr.same_bits(sr._apply(mp, got[i, v], got[v, j], t, False), got[i, j])
    assert sr.same_bits(got[gw < 0], d[gw < 0])
    # and the value-only form is the same
    assert sr.same_bits(cr.blocked(dtype, mp, rd, d, block)[0], want)


@pytest.mark.parametrize("dtype,mp,rd", cr.CONFIGS)
def test_closure_graphs_have_an_informative_closure(dtype, mp, rd):
    """The criterion of _closure_ref.assert_informative on the restatement alone, for every configuration, at a size that
    takes every step of the blocked algorithm (n = 293 = 2 * 128 + 37)."""
    rng = np.random.default_rng(zlib.crc32(f"{dtype},{mp},{rd}".encode()))
    d = cr.graphs(dtype, mp, rd, 293, rng)[0]
    want, _ = cr.blocked(dtype, mp, rd, d, 128)
    cr.assert_informative(dtype, mp, rd, d, want)


@pytest.mark.parametrize("dtype,mp,rd", [("float", "Min", "Max"), ("half", "Max", "Min"), ("float", "Multiply", "Min"),
                                         ("double", "Add", "Min"), ("uint8_t", "Add", "Min"), ("double", "Max", "Min")])
def test_the_criterion_refuses_the_closure_of_a_dense_graph(dtype, mp, rd):
    """What the criterion is for: dense random graphs close to (nearly) one value."""
    d = cr.full_range(dtype, 293, np.random.default_rng(3))[0]
    want, _ = cr.blocked(dtype, mp, rd, d, 128)
    with pytest.raises(AssertionError):
        cr.assert_informative(dtype, mp, rd, d, want)


@pytest.mark.parametrize("dtype,mp,rd,full", [("float", "Multiply", "Min", False), ("float", "Multiply", "Max", False),
                                              ("half", "Add", "Min", False), ("half", "Add", "Max", False),
                                              ("int", "Add", "Min", True), ("uint8_t", "Multiply", "Max", True)])
def test_rounded_and_wrapping_closures_depend_on_the_block_size(dtype, mp, rd, full):
    """Why the GPU tests run every shipped block size: on rounded floating products and sums, and on wrapping integers
    (the full-range set), the blocked algorithm at B = 256 and at B = 64 differ in bits."""
    rng = np.random.default_rng(4)
    d = (cr.full_range(dtype, 293, rng) if full else cr.graphs(dtype, mp, rd, 293, rng))[0]
    assert not sr.same_bits(cr.blocked(dtype, mp, rd, d, 256)[0], cr.blocked(dtype, mp, rd, d, 64)[0])
