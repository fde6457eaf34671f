"""CPU tests of the accumulating entry points (mm_gemm_accumulate_* / mm_gemm_batched_accumulate_*, C <- C (+) A (x) B): the
header, the binding and EXPORTS agree, bad arguments -- C overlapping A or B among them -- are refused before any device is
touched, K = 0 and empty batches are no-ops, and a valid call without a GPU fails with MM_ERR_NO_DEVICE."""
import ctypes
import os
import re

import pytest

import gemm_hls_amd as g

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "mm_gemm.h")).read()
ACCUMULATE = ("mm_gemm_accumulate_enqueue", "mm_gemm_accumulate_launch", "mm_gemm_batched_accumulate_enqueue",
              "mm_gemm_batched_accumulate_launch")
MM_OK, MM_ERR_NO_DEVICE, MM_ERR_BAD_ARGUMENT, MM_ERR_UNSUPPORTED = 0, 1, 2, 3

# Fake device addresses, never dereferenced: every call below is refused, or is a no-op, before a device is touched.
# 4 MiB apart, so that a 4 x 64 x 64 batch of any element size keeps A, B and C disjoint.
A0, B0, C0 = 1 << 22, 2 << 22, 3 << 22
E = 64 * 64


def _benq(cfg, a=A0, b=B0, c=C0, n=64, k=64, m=64, batch=4, sa=E, sb=E, sc=E):
    return g.lib().mm_gemm_batched_accumulate_enqueue(None, ctypes.byref(cfg), a, b, c, n, k, m, batch, sa, sb, sc)


def _blaunch(cfg, a=A0, b=B0, c=C0, n=64, k=64, m=64, batch=4, sa=E, sb=E, sc=E, device=0):
    t = ctypes.c_double(-1.0)
    rc = g.lib().mm_gemm_batched_accumulate_launch(device, ctypes.byref(cfg), a, b, c, n, k, m, batch, sa, sb, sc,
                                                   ctypes.byref(t))
    return rc


def _enq(cfg, a=A0, b=B0, c=C0, n=64, k=64, m=64, **_):
    return g.lib().mm_gemm_accumulate_enqueue(None, ctypes.byref(cfg), a, b, c, n, k, m)


def _launch(cfg, a=A0, b=B0, c=C0, n=64, k=64, m=64, device=0, **_):
    return g.lib().mm_gemm_accumulate_launch(device, ctypes.byref(cfg), a, b, c, n, k, m, None)


def _err():
    return g.lib().mm_last_error().decode()


def test_accumulate_symbols_declared_exported_and_bound():
    for sym in ACCUMULATE:
        assert re.search(rf"^int\s*{sym}\(", HEADER, flags=re.M), sym
        assert sym in g.EXPORTS
        assert getattr(g.lib(), sym).argtypes is not None
    assert callable(g.addmm_) and callable(g.baddbmm_)


@pytest.mark.parametrize("call", [_benq, _blaunch, _enq, _launch], ids=["batched_enqueue", "batched_launch", "enqueue", "launch"])
def test_accumulate_bad_arguments_refused_without_a_device(call):
    f32 = g.make_config("float")
    assert call(f32, c=0) == MM_ERR_BAD_ARGUMENT                     # null c
    assert call(f32, a=0) == MM_ERR_BAD_ARGUMENT
    assert call(g.Config(99, 1, 0, 0, 0)) == MM_ERR_BAD_ARGUMENT      # unknown enums
    assert call(g.Config(0, 1, 0, 7, 0)) == MM_ERR_BAD_ARGUMENT
    # C overlapping A or B: the same base, and C starting inside the last element of the operand
    assert call(f32, c=A0) == MM_ERR_BAD_ARGUMENT and "overlap" in _err()
    assert call(f32, c=B0) == MM_ERR_BAD_ARGUMENT and "overlap" in _err()
    assert call(f32, c=B0 + 4 * E - 64) == MM_ERR_BAD_ARGUMENT and "overlap" in _err()
    assert call(f32, c=A0 - 4 * E + 64) == MM_ERR_BAD_ARGUMENT and "overlap" in _err()   # C's span reaches into A
    # a misaligned pointer on the fast path (float (Multiply, Add) under AUTO: 16 B)
    assert call(f32, c=C0 + 4) == MM_ERR_BAD_ARGUMENT and "16-byte" in _err()
    assert call(f32, a=A0 + 8) == MM_ERR_BAD_ARGUMENT and "16-byte" in _err()
    # MM_PATH_SPLIT has no accumulating form
    assert call(g.make_config("float", path=g.PATH_SPLIT)) == MM_ERR_UNSUPPORTED


@pytest.mark.parametrize("call", [_benq, _blaunch], ids=["enqueue", "launch"])
def test_batched_accumulate_stride_checks(call):
    f32 = g.make_config("float")
    assert call(f32, sc=E - 1) == MM_ERR_BAD_ARGUMENT and "overlap" in _err()        # outputs of the batch overlap
    assert call(f32, sa=E + 1) == MM_ERR_BAD_ARGUMENT and "16-byte" in _err()        # misaligned element strides
    assert call(f32, sc=E + 2) == MM_ERR_BAD_ARGUMENT and "16-byte" in _err()
    # a broadcast B whose single matrix lies inside C's span
    assert call(f32, b=C0 + 2 * 4 * E, sb=0) == MM_ERR_BAD_ARGUMENT and "overlap" in _err()


@pytest.mark.parametrize("call", [_benq, _blaunch, _enq, _launch], ids=["batched_enqueue", "batched_launch", "enqueue", "launch"])
def test_accumulate_k0_and_empty_calls_are_no_ops_without_a_device(call):
    for cfg in (g.make_config("float"), g.make_config("int", "Add", "Min", g.PATH_ORDERED), g.make_config("half")):
        assert call(cfg, k=0) == MM_OK, _err()
        assert call(cfg, n=0) == MM_OK
        assert call(cfg, m=0) == MM_OK
    if call in (_benq, _blaunch):
        assert call(g.make_config("float"), batch=0) == MM_OK
        assert call(g.make_config("float"), batch=0, a=0, b=0, c=0) == MM_OK
    # K = 0 still runs the argument checks
    assert call(g.make_config("float"), k=0, c=0) == MM_ERR_BAD_ARGUMENT
    assert call(g.make_config("float", path=g.PATH_SPLIT), k=0) == MM_ERR_UNSUPPORTED


def test_batched_accumulate_launch_reports_zero_time_for_a_no_op():
    t = ctypes.c_double(-1.0)
    assert g.lib().mm_gemm_batched_accumulate_launch(0, ctypes.byref(g.make_config("float")), A0, B0, C0, 64, 0, 64, 4,
                                                     E, E, E, ctypes.byref(t)) == MM_OK
    assert t.value == 0.0


def test_accumulate_valid_call_needs_a_device():
    # device -1 is refused only AFTER every argument check, so nothing is launched on any machine
    for call in (_blaunch, _launch):
        rc = call(g.make_config("float"), device=-1)
        assert rc in (MM_ERR_NO_DEVICE, MM_ERR_BAD_ARGUMENT), rc
        assert "overlap" not in _err() and "aligned" not in _err(), _err()
    if g.lib().mm_init(None) != MM_ERR_NO_DEVICE:
        return   # a GPU is present: the fake addresses below must never reach a kernel
    for call in (_benq, _blaunch, _enq, _launch):
        for cfg in (g.make_config("float"), g.make_config("float", "Add", "Min", g.PATH_ORDERED),
                    g.make_config("uint8_t"), g.make_config("double")):
            assert call(cfg) == MM_ERR_NO_DEVICE, (call.__name__, _err())


def test_python_entry_points_refuse_host_tensors():
    torch = pytest.importorskip("torch")
    c, a, b = torch.zeros(4, 4), torch.zeros(4, 4), torch.zeros(4, 4)
    with pytest.raises(g.MMError, match="device tensors"):
        g.addmm_(c, a, b)
    with pytest.raises(g.MMError, match="device tensors"):
        g.baddbmm_(c[None], a[None], b[None])
