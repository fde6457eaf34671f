"""CPU tests of the bit-packed product over GF(2) (mm_bits_gf2_*): the header, the binding and EXPORTS agree; every refusal of
mm_bits_gemm_* is this call's too, with its status and text, before any device is touched; zero extents are no-ops; the
kernel names follow the serving rule on both sides of each clause; the unit has exactly the two kernels the header names,
without scratch or AGPRs, and the table kernel's LDS is the figure DESIGN.md states; and the numpy restatement of the table
scheme that documents the kernel's index arithmetic agrees with the definition."""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import _bits_gf2_ref as gr
import _bits_rig
import gemm_hls_amd as g
from _bits_rig import LAUNCH, _err, _poison_padding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN_HEADER = open(os.path.join(ROOT, "include", "mm_gemm.h")).read()
HEADER = open(os.path.join(ROOT, "include", "mm_bits_gf2.h")).read()   # the call's own header, which mm_gemm.h includes
SYMBOLS = ("mm_bits_gf2_enqueue", "mm_bits_gf2_launch", "mm_kernel_name_bits_gf2")
MM_OK, MM_ERR_NO_DEVICE, MM_ERR_BAD_ARGUMENT = 0, 1, 2

# Fake device addresses, never dereferenced: every call below is refused, or is a no-op, before a device is touched.
A0, B0, C0 = 1 << 24, 2 << 24, 3 << 24
N, K, M = 70, 100, 130          # 4 words of K, 5 words of M
KW, MW = 4, 5


def _gf2(launch, a=A0, b=B0, c=C0, n=N, k=K, m=M, lda=KW, ldb=MW, ldc=MW, batch=1, sa=0, sb=0, sc=0, acc=0, device=0):
    if not launch:
        return g.lib().mm_bits_gf2_enqueue(None, a, b, c, n, k, m, lda, ldb, ldc, batch, sa, sb, sc, acc)
    t = ctypes.c_double(-1.0)
    rc = g.lib().mm_bits_gf2_launch(device, a, b, c, n, k, m, lda, ldb, ldc, batch, sa, sb, sc, acc, ctypes.byref(t))
    _gf2.elapsed = t.value
    return rc


_Variant = functools.partial(_bits_rig._Variant, "bits_gf2_variant")


def test_bits_gf2_symbols_declared_exported_and_bound():
    for sym in SYMBOLS:
        assert re.search(rf"^(int|const char)\s*\*?\s*{sym}\(", HEADER, flags=re.M), sym
        assert sym in g.BITS_GF2_EXPORTS and sym not in g.EXPORTS   # (EXPORTS: mm_gemm.h's own declarations, pinned elsewhere)
        assert getattr(g.lib(), sym).argtypes is not None
    assert g.lib().mm_bits_gf2_enqueue.argtypes == g.lib().mm_bits_gemm_enqueue.argtypes
    assert g.lib().mm_bits_gf2_launch.argtypes == g.lib().mm_bits_gemm_launch.argtypes
    for fn in ("bits_matmul_gf2", "bits_addmm_gf2_", "kernel_name_bits_gf2"):
        assert callable(getattr(g, fn)), fn
    assert sorted(re.findall(r"^(?:int|const char)\s*\*?\s*(mm_\w+)\(", HEADER, flags=re.M)) == sorted(g.BITS_GF2_EXPORTS)
    assert '#include "mm_bits_gf2.h"' in MAIN_HEADER and "mm_bits_gf2_" in MAIN_HEADER
    assert "bits_gf2_variant" in HEADER and "MM_BITS_GF2_VARIANT" in HEADER   # where the calls are declared ...
    assert "bits_gf2_variant" in MAIN_HEADER                                   # ... and in the list of knobs
    assert "MM_BITS_GF2_VARIANT" in open(os.path.join(ROOT, "gemm_hls_amd", "csrc", "mm_common.h")).read()
    assert g.get_tuning("bits_gf2_variant") == -1
    # the existing vocabularies are untouched: the call takes no mm_config_t
    assert len(g.DTYPES) == 11 and len(g.OPS) == 5


@LAUNCH
def test_bits_gf2_refusals_without_a_device(launch):
    for acc in (0, 1):
        for null in ("a", "b", "c"):
            assert _gf2(launch, acc=acc, **{null: 0}) == MM_ERR_BAD_ARGUMENT and _err() == "null matrix pointer", null
        for ld in ({"lda": KW - 1}, {"ldb": MW - 1}, {"ldc": MW - 1}):
            assert _gf2(launch, acc=acc, **ld) == MM_ERR_BAD_ARGUMENT and "a row stride is below its row's words" in _err(), ld
        # a strided C whose elements overlap: one matrix spans (N - 1) ldc + ceil(M / 32) words
        span = (N - 1) * 7 + MW
        assert _gf2(launch, acc=acc, ldc=7, batch=3, sc=span - 1) == MM_ERR_BAD_ARGUMENT
        assert "the outputs of the batch would overlap" in _err() and "ceil(M / 32)" in _err()
        assert _gf2(True, acc=acc, ldc=7, batch=3, sc=span, device=-1) != MM_OK and "overlap" not in _err()   # (device -1: never runs)
        # C's span against A's and B's, from either side and inside
        a_bytes, b_bytes, c_bytes = 4 * ((N - 1) * KW + KW), 4 * ((K - 1) * MW + MW), 4 * ((N - 1) * MW + MW)
        for kw in ({"a": C0}, {"b": C0}, {"a": C0 + c_bytes - 4}, {"b": C0 + c_bytes - 4}, {"a": C0 - a_bytes + 4},
                   {"b": C0 - b_bytes + 4}):
            assert _gf2(launch, acc=acc, **kw) == MM_ERR_BAD_ARGUMENT and "c overlaps a or b" in _err(), kw
        for kw in ({"a": C0 + c_bytes}, {"b": C0 - b_bytes}):      # adjacent is fine: refused only for the device
            assert _gf2(True, acc=acc, device=-1, **kw) != MM_OK and "overlaps" not in _err(), kw
        # a batch widens the spans: A broadcast stays one matrix, C grows by its stride
        assert _gf2(launch, acc=acc, batch=4, sc=1 << 10, sb=1 << 10, a=C0 + 3 * (4 << 10)) == MM_ERR_BAD_ARGUMENT
    for bad in (2, -2):
        with _Variant(bad):
            assert _gf2(launch) == MM_ERR_BAD_ARGUMENT and _err() == f"bits_gf2_variant {bad} is not one of -1, 0, 1"
    assert g.get_tuning("bits_gf2_variant") == -1


@LAUNCH
def test_bits_gf2_zero_extents_are_no_ops(launch):
    for acc in (0, 1):
        for kw in ({"n": 0}, {"m": 0}, {"batch": 0}, {"n": 0, "a": 0, "b": 0, "c": 0}, {"batch": 0, "c": 0}):
            assert _gf2(launch, acc=acc, **kw) == MM_OK, (kw, _err())
            assert not launch or _gf2.elapsed == 0.0
    assert _gf2(launch, acc=1, k=0) == MM_OK and _gf2(launch, acc=1, k=0, a=0, b=0, lda=0, ldb=0) == MM_OK   # C keeps its value
    assert not launch or _gf2.elapsed == 0.0


def test_bits_gf2_valid_calls_need_a_device():
    # device -1 is refused only AFTER every argument check, so nothing is launched on any machine
    for rc in (_gf2(True, device=-1), _gf2(True, device=-1, acc=1), _gf2(True, device=-1, k=0, a=0, b=0)):
        assert rc in (MM_ERR_NO_DEVICE, MM_ERR_BAD_ARGUMENT), rc
        assert "null" not in _err() and "overlap" not in _err() and "stride" not in _err(), _err()
    if g.lib().mm_init(None) != MM_ERR_NO_DEVICE:
        return   # a GPU is present: the fake addresses must never reach a kernel
    for launch in (False, True):
        assert _gf2(launch) == MM_ERR_NO_DEVICE


def test_kernel_name_bits_gf2_on_both_sides_of_the_serving_rule():
    name = g.kernel_name_bits_gf2
    # the default rule: N >= 128 and M >= 128 (profiles/bits_gf2_sweep_mi355x.txt), ldb % 2 == 0, ldc % 2 == 0
    assert name(128, 64, 128) == "bits_gf2_tile"                     # 4 words per row
    assert name(127, 64, 128) == "bits_gf2_plain"
    assert name(128, 64, 127) == "bits_gf2_plain"
    assert name(128, 64, 257, ldb=10, ldc=10) == "bits_gf2_tile"
    assert name(128, 64, 257) == "bits_gf2_plain"                    # ld = 9 words
    assert name(128, 64, 257, ldb=10, ldc=9) == "bits_gf2_plain"
    assert name(128, 64, 257, ldb=9, ldc=10) == "bits_gf2_plain"
    assert name(128, 1, 257, ldb=12, ldc=10, lda=3, batch=7) == "bits_gf2_tile"   # K, lda and the batch never matter
    assert name(16384, 16384, 16384) == name(65536, 64, 128) == "bits_gf2_tile"
    assert name(1, 4096, 16384) == name(16384, 4096, 32) == "bits_gf2_plain"
    with _Variant(0):
        assert name(16384, 16384, 16384) == "bits_gf2_plain"
    with _Variant(1):                                                # the tile wherever its ld rule holds, whatever the shape
        assert name(65, 95, 129, ldb=8, ldc=6) == name(1, 1, 1, ldb=2, ldc=2) == "bits_gf2_tile"
        assert name(65, 95, 129, ldb=7, ldc=6) == name(65, 95, 129, ldb=8, ldc=5) == "bits_gf2_plain"
    for bad in (-2, 2, 7):
        with _Variant(bad):
            assert name(64, 64, 64) == name(16384, 16384, 16384) == "invalid"
    assert name(128, 64, 128) == "bits_gf2_tile"                     # the knob is restored


def test_bits_gf2_unit_has_the_two_kernels_without_private_memory_or_agprs():
    """The compiler's own resource lines of every kernel of the unit, cross-compiled for gfx950 with the flags the shipped
    objects are built with."""
    from gemm_hls_amd import build
    unit = "mm_bits_gf2.hip"
    flags = [f for f in build.COMMON if f != "--offload-compress"]
    src = os.path.join(ROOT, "gemm_hls_amd", "csrc", unit)
    r = subprocess.run([build.HIPCC, *flags, *build.EXTRA.get(unit, []), "-S", "--cuda-device-only", src, "-o", "-"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    asm = r.stdout
    kernels = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, flags=re.M)
    assert len(kernels) == 2, kernels                                # "bits_gf2_tile" and "bits_gf2_plain", as the header names them
    tile = [k for k in kernels if "bits_gf2_tile_kernel" in k]
    plain = [k for k in kernels if "bits_gemm_kernelILi1ELb0ELb1E" in k]   # the shared mask loop: W = 1, word accesses, XOR
    assert len(tile) == 1 and len(plain) == 1, kernels
    for line, want in ((r"\.private_segment_fixed_size:\s*(\d+)", "0"), (r"; ScratchSize:\s*(\d+)", "0"), (r"; NumAgprs:\s*(\d+)", "0")):
        got = re.findall(line, asm)
        assert len(got) == 2 and all(v == want for v in got), (line, got)
    lds = dict(zip(kernels, map(int, re.findall(r"\.amdhsa_group_segment_fixed_size\s+(\d+)", asm))))
    assert lds[tile[0]] <= 163840
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    stated = re.search(r"`bits_gf2_tile`: (\d+) VGPRs, no AGPRs, no scratch, (\d+) B of LDS", design)
    assert stated, "DESIGN.md states the table kernel's resource line"
    assert int(stated.group(2)) == lds[tile[0]]
    vgprs = dict(zip(kernels, map(int, re.findall(r"; NumVgprs:\s*(\d+)", asm))))
    assert int(stated.group(1)) == vgprs[tile[0]]
    assert f'#include "mm_bits_product.inc"' in open(src).read()     # the mask loop is the Boolean product's, not a copy
    assert '#include "mm_bits_product.inc"' in open(os.path.join(ROOT, "gemm_hls_amd", "csrc", "mm_bits.hip")).read()


class _OnDevice:
    """A meta tensor that claims to live on a device, with an address: the binding reads attributes only."""
    is_cuda = True

    def __init__(self, t, ptr):
        self.t, self.ptr = t, ptr

    def __getattr__(self, name):
        return getattr(self.t, name)

    def data_ptr(self):
        return self.ptr


def test_python_entry_points_refuse_on_the_host_and_enqueue_the_new_symbol(monkeypatch):
    torch = pytest.importorskip("torch")
    cpu = torch.zeros(4, 1, dtype=torch.int32)
    with pytest.raises(g.MMError, match="bits_matmul_gf2 needs device tensors"):
        g.bits_matmul_gf2(cpu, cpu, 4, 4)
    with pytest.raises(g.MMError, match="bits_addmm_gf2_ needs device tensors"):
        g.bits_addmm_gf2_(cpu, cpu, cpu, 4, 4)
    log = []
    monkeypatch.setattr(g, "_enqueue", lambda device, fn, *args: log.append((fn.__name__, args)))

    def dev(*shape, dtype=torch.int32, ptr=A0):
        return _OnDevice(torch.empty(shape, dtype=dtype, device="meta"), ptr)
    with pytest.raises(g.MMError, match="a must be a packed torch.int32 tensor"):
        g.bits_matmul_gf2(dev(8, 2, dtype=torch.int64), dev(40, 3, ptr=B0), 40, 70)
    with pytest.raises(g.MMError, match="b must be a packed torch.int32 tensor"):
        g.bits_matmul_gf2(dev(8, 2), dev(40, 3, dtype=torch.uint8, ptr=B0), 40, 70)
    with pytest.raises(g.MMError, match="batch sizes differ: 3 and 2"):
        g.bits_matmul_gf2(dev(3, 8, 2), dev(2, 40, 3, ptr=B0), 40, 70)
    with pytest.raises(g.MMError, match=r"c has shape \(2, 8, 3\), expected \(3, 8, W\)"):
        g.bits_addmm_gf2_(dev(2, 8, 3, ptr=C0), dev(3, 8, 2), dev(40, 3, ptr=B0), 40, 70)
    assert log == []
    c = dev(3, 8, 4, ptr=C0)
    assert g.bits_addmm_gf2_(c, dev(8, 2), dev(40, 3, ptr=B0), 40, 70) is c     # a 3-D c over 2-D operands
    assert log == [("mm_bits_gf2_enqueue", (A0, B0, C0, 8, 40, 70, 2, 3, 4, 3, 0, 0, 32, 1))]


@pytest.mark.parametrize("k", [1, 3, 31, 32, 33, 95, 513])
def test_table_scheme_restated_in_numpy_agrees_with_the_definition(k):
    """The index arithmetic of bits_gf2_tile without a GPU: Gray-code build from 4 rows, entry selection by A's nibble, a
    nibble group that straddles K, the K tail of A's last word under poisoned padding, rows of B at k >= K as zero."""
    rng = np.random.default_rng(k)
    n, m = 9, 70
    a, b = rng.random((n, k)) < 0.5, rng.random((k, m)) < 0.5
    want = gr.matmul(a, b)
    assert np.array_equal(want, np.array([[sum(int(a[i, x] and b[x, j]) for x in range(k)) % 2 for j in range(m)] for i in range(n)], bool))
    pa = _poison_padding(gr.pack(a), k)
    pb = np.concatenate([_poison_padding(gr.pack(b), m), np.full((5, gr.words(m)), 0xFFFFFFFF, np.uint32)])   # rows >= K: never used
    got = gr.table_product(pa, pb, k, m)
    assert got.dtype == np.uint32 and np.array_equal(got, gr.pack(want))
    if k % 32:                                                       # the masking is what makes the poison harmless
        live = gr.pack(a)
        live[0, -1] |= np.uint32(1 << (k % 32))
        unmasked = gr.table_product(live, np.concatenate([gr.pack(b), np.full((32, gr.words(m)), 0xFFFFFFFF, np.uint32)]), gr.words(k) * 32, m)
        assert not np.array_equal(unmasked, gr.pack(want))


def test_gray_code_tables_hold_every_combination():
    rng = np.random.default_rng(3)
    pb = rng.integers(0, 1 << 32, size=(70, 3), dtype=np.uint64).astype(np.uint32)
    for s, k_total in ((0, 70), (2, 70), (2, 66)):
        t = gr.tables(pb, k_total, s)
        for grp in range(8):
            for v in range(16):
                want = np.zeros(3, np.uint32)
                for bit in range(4):
                    k = 32 * s + 4 * grp + bit
                    if (v >> bit) & 1 and k < k_total:
                        want ^= pb[k]
                assert np.array_equal(t[grp][v], want), (s, grp, v)
