"""CPU tests of the bit-packed Boolean calls (mm_bits_gemm_*, mm_bits_closure_*, mm_bits_pack_*, mm_bits_unpack_*): the
header, the binding and EXPORTS agree; every refusal returns its status, with a message, before any device is touched; zero
extents are no-ops; the kernel names follow the serving rule on both sides of each threshold; no kernel of the new units uses
scratch, a private segment or AGPRs; and the numpy restatement of the storage format that the GPU tests use puts every bit
where include/mm_gemm.h says."""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import _bits_ref as br
import _bits_rig
import gemm_hls_amd as g
from _bits_rig import LAUNCH, _err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "mm_gemm.h")).read()
SYMBOLS = ("mm_bits_gemm_enqueue", "mm_bits_gemm_launch", "mm_kernel_name_bits_gemm", "mm_bits_closure_enqueue",
           "mm_bits_closure_launch", "mm_kernel_name_bits_closure", "mm_bits_pack_enqueue", "mm_bits_pack_launch",
           "mm_bits_unpack_enqueue", "mm_bits_unpack_launch")
MM_OK, MM_ERR_NO_DEVICE, MM_ERR_BAD_ARGUMENT = 0, 1, 2

# Fake device addresses, never dereferenced: every call below is refused, or is a no-op, before a device is touched.
A0, B0, C0 = 1 << 24, 2 << 24, 3 << 24
N, K, M = 70, 100, 130          # 4 words of K, 5 words of M
KW, MW = 4, 5


def _gemm(launch, a=A0, b=B0, c=C0, n=N, k=K, m=M, lda=KW, ldb=MW, ldc=MW, batch=1, sa=0, sb=0, sc=0, acc=0, device=0):
    if not launch:
        return g.lib().mm_bits_gemm_enqueue(None, a, b, c, n, k, m, lda, ldb, ldc, batch, sa, sb, sc, acc)
    t = ctypes.c_double(-1.0)
    rc = g.lib().mm_bits_gemm_launch(device, a, b, c, n, k, m, lda, ldb, ldc, batch, sa, sb, sc, acc, ctypes.byref(t))
    _gemm.elapsed = t.value
    return rc


def _closure(launch, d=C0, n=N, ldd=3, batch=1, sd=0, device=0):
    if not launch:
        return g.lib().mm_bits_closure_enqueue(None, d, n, ldd, batch, sd)
    t = ctypes.c_double(-1.0)
    rc = g.lib().mm_bits_closure_launch(device, d, n, ldd, batch, sd, ctypes.byref(t))
    _closure.elapsed = t.value
    return rc


def _convert(launch, to_bits, src=A0, dst=C0, rows=N, cols=M, ld_src=None, ld_dst=None, batch=1, ss=0, sd=0, device=0):
    ld_src = (cols if to_bits else br.words(cols)) if ld_src is None else ld_src
    ld_dst = (br.words(cols) if to_bits else cols) if ld_dst is None else ld_dst
    name = "mm_bits_pack" if to_bits else "mm_bits_unpack"
    if not launch:
        return getattr(g.lib(), name + "_enqueue")(None, src, dst, rows, cols, ld_src, ld_dst, batch, ss, sd)
    t = ctypes.c_double(-1.0)
    rc = getattr(g.lib(), name + "_launch")(device, src, dst, rows, cols, ld_src, ld_dst, batch, ss, sd, ctypes.byref(t))
    _convert.elapsed = t.value
    return rc


_Variant = functools.partial(_bits_rig._Variant, "bits_variant")


def test_bits_symbols_declared_exported_and_bound():
    for sym in SYMBOLS:
        assert re.search(rf"^(int|const char)\s*\*?\s*{sym}\(", HEADER, flags=re.M), sym
        assert sym in g.EXPORTS
        assert getattr(g.lib(), sym).argtypes is not None
    for fn in ("pack_bits", "unpack_bits", "bits_matmul", "bits_addmm_", "bits_closure_", "kernel_name_bits_gemm",
               "kernel_name_bits_closure"):
        assert callable(getattr(g, fn)), fn
    assert "bits_variant" in HEADER and "MM_BITS_VARIANT" in open(os.path.join(ROOT, "gemm_hls_amd", "csrc", "mm_common.h")).read()
    # the existing vocabularies are untouched: the packed calls take no mm_config_t
    assert len(g.DTYPES) == 11 and len(g.OPS) == 5


@LAUNCH
def test_bits_gemm_refusals_without_a_device(launch):
    for acc in (0, 1):
        for null in ("a", "b", "c"):
            assert _gemm(launch, acc=acc, **{null: 0}) == MM_ERR_BAD_ARGUMENT and "null" in _err(), null
        for ld in ({"lda": KW - 1}, {"ldb": MW - 1}, {"ldc": MW - 1}):
            assert _gemm(launch, acc=acc, **ld) == MM_ERR_BAD_ARGUMENT and "row stride" in _err(), ld
        # a strided C whose elements overlap: one matrix spans (N - 1) ldc + ceil(M / 32) words
        span = (N - 1) * 7 + MW
        assert _gemm(launch, acc=acc, ldc=7, batch=3, sc=span - 1) == MM_ERR_BAD_ARGUMENT and "overlap" in _err()
        assert _gemm(True, acc=acc, ldc=7, batch=3, sc=span, device=-1) != MM_OK and "overlap" not in _err()   # (device -1: never runs)
        # C's span against A's and B's, from either side and inside
        a_bytes, b_bytes, c_bytes = 4 * ((N - 1) * KW + KW), 4 * ((K - 1) * MW + MW), 4 * ((N - 1) * MW + MW)
        for kw in ({"a": C0}, {"b": C0}, {"a": C0 + c_bytes - 4}, {"b": C0 + c_bytes - 4}, {"a": C0 - a_bytes + 4},
                   {"b": C0 - b_bytes + 4}):
            assert _gemm(launch, acc=acc, **kw) == MM_ERR_BAD_ARGUMENT and "overlaps" in _err(), kw
        for kw in ({"a": C0 + c_bytes}, {"b": C0 - b_bytes}):      # adjacent is fine: refused only for the device
            assert _gemm(True, acc=acc, device=-1, **kw) != MM_OK and "overlaps" not in _err(), kw
        # a batch widens the spans: A broadcast stays one matrix, C grows by its stride
        assert _gemm(launch, acc=acc, batch=4, sc=1 << 10, sb=1 << 10, a=C0 + 3 * (4 << 10)) == MM_ERR_BAD_ARGUMENT
    with _Variant(2):
        assert _gemm(launch) == MM_ERR_BAD_ARGUMENT and "bits_variant" in _err()


@LAUNCH
def test_bits_closure_and_convert_refusals_without_a_device(launch):
    assert _closure(launch, d=0) == MM_ERR_BAD_ARGUMENT and "null" in _err()
    assert _closure(launch, ldd=2) == MM_ERR_BAD_ARGUMENT and "ldd" in _err()
    span = (N - 1) * 3 + 3
    assert _closure(launch, batch=2, sd=span - 1) == MM_ERR_BAD_ARGUMENT and "overlap" in _err()
    assert _closure(True, batch=2, sd=span, device=-1) != MM_OK and "overlap" not in _err()   # (device -1: never runs)
    for to_bits in (True, False):
        assert _convert(launch, to_bits, src=0) == MM_ERR_BAD_ARGUMENT and "null" in _err()
        assert _convert(launch, to_bits, dst=0) == MM_ERR_BAD_ARGUMENT and "null" in _err()
        row_src, row_dst = (M, MW) if to_bits else (MW, M)
        assert _convert(launch, to_bits, ld_src=row_src - 1) == MM_ERR_BAD_ARGUMENT and "row stride" in _err()
        assert _convert(launch, to_bits, ld_dst=row_dst - 1) == MM_ERR_BAD_ARGUMENT and "row stride" in _err()
        assert _convert(launch, to_bits, batch=2, ss=1 << 16, sd=N * row_dst - 1) == MM_ERR_BAD_ARGUMENT and "overlap" in _err()
        assert _convert(launch, to_bits, src=C0 + 8) == MM_ERR_BAD_ARGUMENT and "overlaps" in _err()


@LAUNCH
def test_bits_zero_extents_are_no_ops(launch):
    for acc in (0, 1):
        for kw in ({"n": 0}, {"m": 0}, {"batch": 0}, {"n": 0, "a": 0, "b": 0, "c": 0}, {"batch": 0, "c": 0}):
            assert _gemm(launch, acc=acc, **kw) == MM_OK, (kw, _err())
            assert not launch or _gemm.elapsed == 0.0
    assert _gemm(launch, acc=1, k=0) == MM_OK and _gemm(launch, acc=1, k=0, a=0, b=0, lda=0, ldb=0) == MM_OK   # C keeps its value
    assert not launch or _gemm.elapsed == 0.0
    for kw in ({"n": 0}, {"batch": 0}, {"n": 0, "d": 0}):
        assert _closure(launch, **kw) == MM_OK, (kw, _err())
        assert not launch or _closure.elapsed == 0.0
    for to_bits in (True, False):
        for kw in ({"rows": 0}, {"cols": 0}, {"batch": 0}, {"rows": 0, "src": 0, "dst": 0}):
            assert _convert(launch, to_bits, **kw) == MM_OK, (kw, _err())
            assert not launch or _convert.elapsed == 0.0


def test_bits_valid_calls_need_a_device():
    # device -1 is refused only AFTER every argument check, so nothing is launched on any machine
    for rc in (_gemm(True, device=-1), _gemm(True, device=-1, acc=1), _gemm(True, device=-1, k=0, a=0, b=0),
               _closure(True, device=-1), _closure(True, n=40, ldd=2, batch=5, sd=80, device=-1),
               _convert(True, True, device=-1), _convert(True, False, device=-1)):
        assert rc in (MM_ERR_NO_DEVICE, MM_ERR_BAD_ARGUMENT), rc
        assert "null" not in _err() and "overlap" not in _err() and "stride" not in _err(), _err()
    if g.lib().mm_init(None) != MM_ERR_NO_DEVICE:
        return   # a GPU is present: the fake addresses must never reach a kernel
    for launch in (False, True):
        assert _gemm(launch) == MM_ERR_NO_DEVICE and _closure(launch) == MM_ERR_NO_DEVICE
        assert _convert(launch, True) == MM_ERR_NO_DEVICE and _convert(launch, False) == MM_ERR_NO_DEVICE


def test_kernel_name_bits_gemm_on_both_sides_of_the_serving_rule():
    name = g.kernel_name_bits_gemm
    # the default rule: M > 2048 (more than 64 words), ldb % 4 == 0, ldc % 2 == 0
    assert name(64, 64, 2049, ldb=68, ldc=66) == "bits_tile"
    assert name(64, 64, 2048, ldb=68, ldc=66) == "bits_plain"
    assert name(64, 64, 2049) == "bits_plain"                       # ld = 65 words
    assert name(64, 64, 2049, ldb=68, ldc=65) == "bits_plain"
    assert name(64, 64, 2049, ldb=66, ldc=66) == "bits_plain"
    assert name(64, 64, 2049, ldb=68, ldc=68, lda=3, batch=7) == "bits_tile"   # lda and the batch never matter
    assert name(1, 1, 4096) == name(16384, 16384, 16384) == "bits_tile"
    with _Variant(0):
        assert name(16384, 16384, 16384) == "bits_plain"
    with _Variant(1):                                                # the tile wherever its ld rule holds, whatever M
        assert name(65, 95, 129, ldb=8, ldc=6) == "bits_tile"
        assert name(65, 95, 129, ldb=7, ldc=6) == name(65, 95, 129, ldb=8, ldc=5) == "bits_plain"
    for bad in (-2, 2, 7):
        with _Variant(bad):
            assert name(64, 64, 64) == "invalid"
    assert name(64, 64, 2049, ldb=68, ldc=66) == "bits_tile"        # the knob is restored


def test_kernel_name_bits_closure_by_n():
    name = g.kernel_name_bits_closure
    assert name(1) == name(64) == name(40, 1 << 20) == "bits_closure_onchip"
    assert name(65) == name(65536) == name(200, 5) == "bits_closure_blocked"


def test_python_entry_point_refusals_on_the_host():
    torch = pytest.importorskip("torch")
    with pytest.raises(g.MMError, match="device tensor"):
        g.pack_bits(torch.zeros(4, 4, dtype=torch.bool))
    with pytest.raises(g.MMError, match="device tensor"):
        g.unpack_bits(torch.zeros(4, 1, dtype=torch.int32), 4)
    with pytest.raises(g.MMError, match="device tensors"):
        g.bits_matmul(torch.zeros(4, 1, dtype=torch.int32), torch.zeros(4, 1, dtype=torch.int32), 4, 4)
    with pytest.raises(g.MMError, match="device tensor"):
        g.bits_closure_(torch.zeros(4, 1, dtype=torch.int32))


BITS_UNITS = ("mm_bits.hip", "mm_bits_closure.hip")


@pytest.mark.parametrize("unit", BITS_UNITS)
def test_no_bits_kernel_uses_private_memory_or_agprs(unit):
    """The compiler's own resource lines of every kernel of the unit, cross-compiled for gfx950 with the flags the shipped
    objects are built with."""
    from gemm_hls_amd import build
    flags = [f for f in build.COMMON if f != "--offload-compress"]
    src = os.path.join(ROOT, "gemm_hls_amd", "csrc", unit)
    r = subprocess.run([build.HIPCC, *flags, *build.EXTRA.get(unit, []), "-S", "--cuda-device-only", src, "-o", "-"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    asm = r.stdout
    kernels = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, flags=re.M)
    assert len(kernels) == (4 if unit == "mm_bits.hip" else 1), kernels     # tile, plain, pack, unpack; the wavefront closure
    for line, want in ((r"\.private_segment_fixed_size:\s*(\d+)", "0"), (r"; ScratchSize:\s*(\d+)", "0"), (r"; NumAgprs:\s*(\d+)", "0")):
        got = re.findall(line, asm)
        assert len(got) == len(kernels) and all(v == want for v in got), (unit, line, got)


def test_pack_reference_round_trip_and_bit_positions():
    rng = np.random.default_rng(5)
    for cols in (1, 31, 32, 33, 64, 1000):
        x = rng.random((7, cols)) < 0.4
        p = br.pack(x)
        assert p.dtype == np.uint32 and p.shape == (7, br.words(cols))
        assert np.array_equal(br.unpack(p, cols), x)
        # the same words through the documented recipe: packbits, little bit order, padded to 4 bytes, viewed as uint32
        by = np.packbits(x, axis=-1, bitorder="little")
        by = np.pad(by, ((0, 0), (0, 4 * br.words(cols) - by.shape[1])))
        assert np.array_equal(p, by.view("<u4"))
        if cols % 32:
            assert not (p[:, -1] >> (cols % 32)).any()                # padding bits are 0
    cols = 70
    for j in (0, 31, 32, cols - 1):
        x = np.zeros((1, cols), bool)
        x[0, j] = True
        want = np.zeros(3, np.uint32)
        want[j >> 5] = np.uint32(1) << np.uint32(j & 31)
        assert np.array_equal(br.pack(x)[0], want), j
    # a wider ld keeps the gap words' fill; nonzero bytes other than 1 are 1; unpack ignores padding and gap words
    x = (rng.integers(0, 4, size=(3, 40)) * 85).astype(np.uint8)
    p = br.pack(x, ld=4, fill=0xDEADBEEF)
    assert np.array_equal(p[:, :2], br.pack(x != 0)) and (p[:, 2:] == 0xDEADBEEF).all()
    p[:, 1] |= np.uint32(0xFFFFFF00)
    assert np.array_equal(br.unpack(p, 40), x != 0)


def test_bits_reference_product_and_closure():
    rng = np.random.default_rng(6)
    a, b = rng.random((9, 50)) < br.density(50), rng.random((50, 11)) < br.density(50)
    want = np.array([[any(a[i, k] and b[k, j] for k in range(50)) for j in range(11)] for i in range(9)])
    assert np.array_equal(br.matmul(a, b), want)
    d = br.graph(33, 2)
    c = br.closure(d)
    power, reach = d.copy(), d.copy()
    for _ in range(33):
        power = br.matmul(power, d)
        reach |= power
    assert np.array_equal(c, reach) and (c != d).any()
