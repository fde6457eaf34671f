"""CPU tests of the packed counting calls (mm_bits_count_*, mm_kernel_name_bits_count, mm_bits_transpose_*): include/mm_gemm.h,
the binding's EXPORTS and the library agree; every refusal returns its status, with a message, before any device is touched;
zero extents are no-ops; the kernel names follow the serving rule on both sides of its thresholds; no kernel of the unit uses
scratch; and the numpy oracle of the GPU tests counts what a loop counts.  (What the torch wrappers hand to the C ABI and
what they refuse: tests/test_binding_calls.py.)"""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import _bits_count_ref as cr
import _bits_rig
import gemm_hls_amd as g
from _bits_rig import LAUNCH, _err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "mm_gemm.h")).read()
SYMBOLS = ("mm_bits_count_enqueue", "mm_bits_count_launch", "mm_kernel_name_bits_count", "mm_bits_transpose_enqueue",
           "mm_bits_transpose_launch")
MM_OK, MM_ERR_NO_DEVICE, MM_ERR_BAD_ARGUMENT = 0, 1, 2

# Fake device addresses, never dereferenced: every call below is refused, or is a no-op, before a device is touched.
A0, B0, C0 = 1 << 24, 2 << 24, 3 << 24
N, K, M = 70, 100, 130          # 4 words of K
KW = 4


def _count(launch, op=0, a=A0, b=B0, c=C0, n=N, k=K, m=M, lda=KW, ldbt=KW, ldc=M, batch=1, sa=0, sb=0, sc=0, acc=0, device=0):
    if not launch:
        return g.lib().mm_bits_count_enqueue(None, op, a, b, c, n, k, m, lda, ldbt, ldc, batch, sa, sb, sc, acc)
    t = ctypes.c_double(-1.0)
    rc = g.lib().mm_bits_count_launch(device, op, a, b, c, n, k, m, lda, ldbt, ldc, batch, sa, sb, sc, acc, ctypes.byref(t))
    _count.elapsed = t.value
    return rc


def _transpose(launch, src=A0, dst=C0, rows=N, cols=M, ld_src=5, ld_dst=3, batch=1, ss=0, sd=0, device=0):
    if not launch:
        return g.lib().mm_bits_transpose_enqueue(None, src, dst, rows, cols, ld_src, ld_dst, batch, ss, sd)
    t = ctypes.c_double(-1.0)
    rc = g.lib().mm_bits_transpose_launch(device, src, dst, rows, cols, ld_src, ld_dst, batch, ss, sd, ctypes.byref(t))
    _transpose.elapsed = t.value
    return rc


_Variant = functools.partial(_bits_rig._Variant, "bits_count_variant")


def test_bits_count_symbols_declared_exported_and_bound():
    for sym in SYMBOLS:
        assert re.search(rf"^(int|const char)\s*\*?\s*{sym}\(", HEADER, flags=re.M), sym
        assert sym in g.EXPORTS
        assert getattr(g.lib(), sym).argtypes is not None
    assert g.lib().mm_kernel_name_bits_count.restype is ctypes.c_char_p
    for fn in ("bits_matmul_count", "bits_addmm_count_", "transpose_bits", "kernel_name_bits_count"):
        assert callable(getattr(g, fn)), fn
    ops = {k: int(v) for k, v in re.findall(r"MM_BITS_COUNT_(\w+)\s*=\s*(\d+)", HEADER)}
    assert ops == {"AND": 0, "XOR": 1} == {k.upper(): v for k, v in g.BITS_COUNT_OPS.items()}
    assert HEADER.count("bits_count_variant") >= 2     # where the calls are declared, and in the list of knobs
    assert "MM_BITS_COUNT_VARIANT" in open(os.path.join(ROOT, "gemm_hls_amd", "csrc", "mm_common.h")).read()
    assert g.get_tuning("bits_count_variant") == -1
    # the existing vocabularies are untouched: the packed calls take no mm_config_t
    assert len(g.DTYPES) == 11 and len(g.OPS) == 5


@LAUNCH
def test_bits_count_refusals_without_a_device(launch):
    for bad_op in (-1, 2, 7):
        assert _count(launch, op=bad_op) == MM_ERR_BAD_ARGUMENT and "op" in _err(), bad_op
    for op in (0, 1):
        for acc in (0, 1):
            for null in ("a", "b", "c"):
                assert _count(launch, op, acc=acc, **{null: 0}) == MM_ERR_BAD_ARGUMENT and "null" in _err(), null
            for ld in ({"lda": KW - 1}, {"ldbt": KW - 1}, {"ldc": M - 1}):
                assert _count(launch, op, acc=acc, **ld) == MM_ERR_BAD_ARGUMENT and "row stride" in _err(), ld
            # a strided C whose elements overlap: one matrix spans (N - 1) ldc + M elements
            span = (N - 1) * 140 + M
            assert _count(launch, op, acc=acc, ldc=140, batch=3, sc=span - 1) == MM_ERR_BAD_ARGUMENT and "overlap" in _err()
            assert _count(True, op, acc=acc, ldc=140, batch=3, sc=span, device=-1) != MM_OK and "overlap" not in _err()   # (device -1: never runs)
            # C's span in bytes against A's and Bt's, from either side and inside
            a_bytes, b_bytes, c_bytes = 4 * N * KW, 4 * M * KW, 4 * N * M
            for kw in ({"a": C0}, {"b": C0}, {"a": C0 + c_bytes - 4}, {"b": C0 + c_bytes - 4}, {"a": C0 - a_bytes + 4},
                       {"b": C0 - b_bytes + 4}):
                assert _count(launch, op, acc=acc, **kw) == MM_ERR_BAD_ARGUMENT and "overlaps" in _err(), kw
            for kw in ({"a": C0 + c_bytes}, {"b": C0 - b_bytes}):      # adjacent is fine: refused only for the device
                assert _count(True, op, acc=acc, device=-1, **kw) != MM_OK and "overlaps" not in _err(), kw
            # a batch widens the spans: A broadcast stays one matrix, C grows by its stride (in elements)
            assert _count(launch, op, acc=acc, batch=4, sc=1 << 14, sb=1 << 10, a=C0 + 3 * (4 << 14)) == MM_ERR_BAD_ARGUMENT
            assert "overlaps" in _err()
    for bad in (-2, 2):
        with _Variant(bad):
            assert _count(launch) == MM_ERR_BAD_ARGUMENT and "bits_count_variant" in _err()


@LAUNCH
def test_bits_transpose_refusals_without_a_device(launch):
    assert _transpose(launch, src=0) == MM_ERR_BAD_ARGUMENT and "null" in _err()
    assert _transpose(launch, dst=0) == MM_ERR_BAD_ARGUMENT and "null" in _err()
    assert _transpose(launch, ld_src=4) == MM_ERR_BAD_ARGUMENT and "row stride" in _err()      # 130 columns: 5 words
    assert _transpose(launch, ld_dst=2) == MM_ERR_BAD_ARGUMENT and "row stride" in _err()      # 70 rows: 3 words
    span = (M - 1) * 3 + 3                                                                       # the destination: M rows of 3 words
    assert _transpose(launch, batch=2, ss=1 << 16, sd=span - 1) == MM_ERR_BAD_ARGUMENT and "overlap" in _err()
    assert _transpose(True, batch=2, ss=1 << 16, sd=span, device=-1) != MM_OK and "overlap" not in _err()
    assert _transpose(launch, src=C0) == MM_ERR_BAD_ARGUMENT and "overlaps" in _err()            # no in-place form
    assert _transpose(launch, src=C0 + 4 * span - 4) == MM_ERR_BAD_ARGUMENT and "overlaps" in _err()
    assert _transpose(True, src=C0 + 4 * span, device=-1) != MM_OK and "overlaps" not in _err()


@LAUNCH
def test_bits_count_zero_extents_are_no_ops(launch):
    for op in (0, 1):
        for acc in (0, 1):
            for kw in ({"n": 0}, {"m": 0}, {"batch": 0}, {"n": 0, "a": 0, "b": 0, "c": 0}, {"batch": 0, "c": 0}):
                assert _count(launch, op, acc=acc, **kw) == MM_OK, (kw, _err())
                assert not launch or _count.elapsed == 0.0
        # accumulating over no k: C keeps its value, a and bt are not read
        assert _count(launch, op, acc=1, k=0) == MM_OK and _count(launch, op, acc=1, k=0, a=0, b=0, lda=0, ldbt=0) == MM_OK
        assert not launch or _count.elapsed == 0.0
    for kw in ({"rows": 0}, {"cols": 0}, {"batch": 0}, {"rows": 0, "src": 0, "dst": 0}):
        assert _transpose(launch, **kw) == MM_OK, (kw, _err())
        assert not launch or _transpose.elapsed == 0.0


def test_bits_count_valid_calls_need_a_device():
    # device -1 is refused only AFTER every argument check, so nothing is launched on any machine
    for rc in (_count(True, device=-1), _count(True, 1, device=-1, acc=1), _count(True, device=-1, k=0, a=0, b=0),
               _count(True, 1, device=-1, batch=3, sc=N * M), _transpose(True, device=-1),
               _transpose(True, batch=3, ss=0, sd=M * 3, device=-1)):
        assert rc in (MM_ERR_NO_DEVICE, MM_ERR_BAD_ARGUMENT), rc
        assert "null" not in _err() and "overlap" not in _err() and "stride" not in _err(), _err()
    if g.lib().mm_init(None) != MM_ERR_NO_DEVICE:
        return   # a GPU is present: the fake addresses must never reach a kernel
    for launch in (False, True):
        assert _count(launch) == MM_ERR_NO_DEVICE and _count(launch, 1, k=0, a=0, b=0) == MM_ERR_NO_DEVICE
        assert _transpose(launch) == MM_ERR_NO_DEVICE


def test_kernel_name_bits_count_on_both_sides_of_the_serving_rule():
    name = g.kernel_name_bits_count
    assert name(8, 40, 12) == "bits_count_plain"                        # ld defaulted: ceil(K / 32) words, M elements
    # the default rule: ceil(N / 128) ceil(M / 128) >= 256 tiles, lda % 4 == ldbt % 4 == ldc % 4 == 0
    assert name(2048, 128, 2048) == "bits_count_tile"                  # 16 x 16 tiles, ld = 4, 4, 2048
    assert name(1921, 128, 1921, ldc=1924) == "bits_count_tile"        # ... counted in started tiles
    assert name(1920, 128, 2048) == "bits_count_plain"                 # 15 x 16
    assert name(2048, 128, 1920) == "bits_count_plain"
    assert name(128, 128, 32768) == name(32768, 128, 128) == "bits_count_tile"
    assert name(16384, 16384, 16384) == name(16384, 64, 16384, lda=4, ldbt=4) == "bits_count_tile"
    assert name(16384, 64, 16384) == "bits_count_plain"                # ld = 2 words
    for ld in ({"lda": 5}, {"lda": 3}, {"ldbt": 5}, {"ldbt": 3}, {"ldc": 2049}, {"ldc": 2051}):   # one off a multiple of 4
        assert name(2048, 128, 2048, **{"lda": 4, "ldbt": 4, "ldc": 2048, **ld}) == "bits_count_plain", ld
    assert name(2048, 128, 2048, lda=8, ldbt=12, ldc=2052, batch=7) == "bits_count_tile"   # the batch never matters
    assert name(2048, 0, 2048, lda=0, ldbt=0) == "bits_count_tile"     # nor does K
    with _Variant(0):
        assert name(16384, 16384, 16384) == "bits_count_plain"
    with _Variant(1):                                                   # the tile wherever its ld rule holds, whatever the shape
        assert name(1, 128, 1, ldc=4) == name(65, 95, 129, lda=4, ldbt=4, ldc=132) == "bits_count_tile"
        assert name(65, 95, 129) == name(65, 95, 129, lda=4, ldbt=4) == name(65, 95, 129, lda=4, ldbt=5, ldc=132) == "bits_count_plain"
    for bad in (-2, 2, 7):
        with _Variant(bad):
            assert name(64, 64, 64) == "invalid"
    assert name(2048, 128, 2048) == "bits_count_tile"                  # the knob is restored


def test_no_bits_count_kernel_uses_private_memory_or_agprs():
    """The compiler's own resource lines of every kernel of the unit, cross-compiled for gfx950 with the flags the shipped
    objects are built with; the 128 x 128 kernels stay far below the 474 registers of a fully unrolled slab."""
    from gemm_hls_amd import build
    flags = [f for f in build.COMMON if f != "--offload-compress"]
    src = os.path.join(ROOT, "gemm_hls_amd", "csrc", "mm_bits_count.hip")
    r = subprocess.run([build.HIPCC, *flags, *build.EXTRA.get("mm_bits_count.hip", []), "-S", "--cuda-device-only", src, "-o", "-"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    asm = r.stdout
    kernels = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, flags=re.M)
    assert len(kernels) == 5, kernels     # tile and plain, each AND and XOR; the transpose
    for line, want in ((r"\.private_segment_fixed_size:\s*(\d+)", "0"), (r"; ScratchSize:\s*(\d+)", "0"), (r"; NumAgprs:\s*(\d+)", "0")):
        got = re.findall(line, asm)
        assert len(got) == len(kernels) and all(v == want for v in got), (line, got)
    vgprs = [int(v) for v in re.findall(r"; NumVgprs:\s*(\d+)", asm)]
    assert len(vgprs) == 5 and max(vgprs) <= 128, vgprs
    assert asm.count("v_bcnt_u32_b32") >= 2 * 64 + 2 * 16            # one per accumulator and instantiation, at least


def test_count_reference_against_loops():
    rng = np.random.default_rng(7)
    a, bt = rng.random((9, 50)) < 0.5, rng.random((11, 50)) < 0.5
    want_and = np.array([[sum(int(a[i, k] and bt[j, k]) for k in range(50)) for j in range(11)] for i in range(9)])
    want_xor = np.array([[sum(int(a[i, k] != bt[j, k]) for k in range(50)) for j in range(11)] for i in range(9)])
    assert np.array_equal(cr.count(a, bt, "And"), want_and) and cr.count(a, bt).dtype == np.int32
    assert np.array_equal(cr.count(a, bt, "Xor"), want_xor)
    seed = np.full((9, 11), 0x7FFFFFFF, np.int32)
    assert np.array_equal(cr.count(a, bt, "And", seed).view(np.uint32), (want_and + 0x7FFFFFFF).astype(np.uint32))   # wraps
    assert (cr.count(a, bt, "And", seed) < 0).any()
    x = rng.random((2, 5, 70)) < 0.5
    assert np.array_equal(cr.transpose(x)[1, 69, 3], x[1, 3, 69]) and cr.transpose(x).shape == (2, 70, 5)
    assert np.array_equal(cr.unpack(cr.pack(cr.transpose(x)), 5), cr.transpose(x))
