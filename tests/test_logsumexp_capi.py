"""CPU tests of the log-semiring entry points (mm_gemm_logsumexp_*, mm_kernel_name_logsumexp): the header, the binding and
EXPORTS agree; bad arguments and knob values are refused before any device is touched; K = 0 accumulating and empty
batches are no-ops; a valid call without a GPU fails with MM_ERR_NO_DEVICE; kernel names follow path and knob; the new unit
uses no scratch, AGPRs or atomics; and the numpy reference agrees with a brute-force loop, special values included."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

import _lse_ref
import gemm_hls_amd as g

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "mm_gemm.h")).read()
SYMBOLS = ("mm_gemm_logsumexp_enqueue", "mm_gemm_logsumexp_launch", "mm_kernel_name_logsumexp")
MM_OK, MM_ERR_NO_DEVICE, MM_ERR_BAD_ARGUMENT, MM_ERR_UNSUPPORTED = 0, 1, 2, 3

# Fake device addresses, never dereferenced: every call below is refused, or is a no-op, before a device is touched.
A0, B0, C0 = 1 << 22, 2 << 22, 3 << 22
E = 64 * 64


def _enq(cfg, a=A0, b=B0, c=C0, n=64, k=64, m=64, batch=4, sa=E, sb=E, sc=E, acc=0):
    return g.lib().mm_gemm_logsumexp_enqueue(None, ctypes.byref(cfg), a, b, c, n, k, m, batch, sa, sb, sc, acc)


def _launch(cfg, a=A0, b=B0, c=C0, n=64, k=64, m=64, batch=4, sa=E, sb=E, sc=E, acc=0, device=0):
    t = ctypes.c_double(-1.0)
    return g.lib().mm_gemm_logsumexp_launch(device, ctypes.byref(cfg), a, b, c, n, k, m, batch, sa, sb, sc, acc,
                                            ctypes.byref(t))


def _err():
    return g.lib().mm_last_error().decode()


def _cfg(dtype="float", reduce_op="Max", path=g.PATH_AUTO, map_op="Add", transposed_a=False):
    return g.make_config(dtype, map_op, reduce_op, path, transposed_a)


@pytest.fixture
def lse_variant():
    """Sets the lse_variant knob for one test and restores the previous value."""
    old = g.get_tuning("lse_variant")
    yield lambda v: g.set_tuning("lse_variant", v)
    g.set_tuning("lse_variant", old)


def test_logsumexp_symbols_declared_exported_and_bound():
    for sym in SYMBOLS:
        assert re.search(rf"^(int|const char)\s*\*?\s*{sym}\(", HEADER, flags=re.M), sym
        assert sym in g.EXPORTS
        assert getattr(g.lib(), sym).argtypes is not None
    assert callable(g.matmul_logsumexp) and callable(g.addmm_logsumexp_) and callable(g.kernel_name_logsumexp)
    assert "lse_variant" in HEADER and "MM_LSE_VARIANT" in open(
        os.path.join(ROOT, "gemm_hls_amd", "csrc", "mm_capi.hip")).read()
    assert "Add" in g.OPS and len(g.OPS) == 5   # the semiring is named by the entry point, not by a new operator


@pytest.mark.parametrize("call", [_enq, _launch], ids=["enqueue", "launch"])
@pytest.mark.parametrize("acc", [0, 1], ids=["plain", "accumulate"])
def test_logsumexp_refusals_without_a_device(call, acc):
    for dt in ("int8_t", "uint8_t", "int16_t", "uint16_t", "int", "unsigned", "long", "unsigned long"):
        assert call(_cfg(dt), acc=acc) == MM_ERR_UNSUPPORTED, dt
    for mp in ("Multiply", "And", "Min", "Max"):
        assert call(_cfg(map_op=mp), acc=acc) == MM_ERR_UNSUPPORTED, mp
    for red in ("Add", "Multiply", "And"):
        assert call(_cfg(reduce_op=red), acc=acc) == MM_ERR_UNSUPPORTED, red
    assert call(_cfg(path=g.PATH_SPLIT), acc=acc) == MM_ERR_UNSUPPORTED
    assert call(g.Config(99, 0, 4, 0, 0), acc=acc) == MM_ERR_BAD_ARGUMENT           # unknown enums
    assert call(g.Config(0, 0, 4, 7, 0), acc=acc) == MM_ERR_BAD_ARGUMENT
    for kw in ("a", "b", "c"):
        assert call(_cfg(), acc=acc, **{kw: 0}) == MM_ERR_BAD_ARGUMENT and "null" in _err(), kw
    assert call(_cfg(), sc=E - 1, acc=acc) == MM_ERR_BAD_ARGUMENT and "overlap" in _err()
    for kw in ({"c": A0}, {"c": B0}, {"c": B0 + 4 * E * 4 - 64}, {"c": A0 - 4 * E * 4 + 64}):
        assert call(_cfg(), acc=acc, **kw) == MM_ERR_BAD_ARGUMENT and "overlap" in _err(), kw
    assert call(_cfg(), b=C0 + 2 * 4 * E, sb=0, acc=acc) == MM_ERR_BAD_ARGUMENT   # a broadcast B inside C's span


@pytest.mark.parametrize("call", [_enq, _launch], ids=["enqueue", "launch"])
def test_logsumexp_k0_and_empty_calls(call):
    for cfg in (_cfg(), _cfg("double", "Min", g.PATH_ORDERED), _cfg("half", transposed_a=True)):
        assert call(cfg, k=0) == MM_ERR_BAD_ARGUMENT and "size_k" in _err()     # the plain form needs K
        assert call(cfg, k=0, acc=1) == MM_OK, _err()                              # accumulating over no k: a no-op
        for acc in (0, 1):
            assert call(cfg, n=0, acc=acc) == MM_OK
            assert call(cfg, m=0, acc=acc) == MM_OK
            assert call(cfg, batch=0, acc=acc) == MM_OK
            assert call(cfg, batch=0, a=0, b=0, c=0, acc=acc) == MM_OK
    assert call(_cfg(), k=0, acc=1, c=0) == MM_ERR_BAD_ARGUMENT   # K = 0 accumulating still runs the argument checks
    assert call(_cfg(reduce_op="Add"), k=0, acc=1) == MM_ERR_UNSUPPORTED


def test_logsumexp_launch_reports_zero_time_for_a_no_op():
    t = ctypes.c_double(-1.0)
    assert g.lib().mm_gemm_logsumexp_launch(0, ctypes.byref(_cfg()), A0, B0, C0, 64, 0, 64, 4, E, E, E, 1,
                                            ctypes.byref(t)) == MM_OK
    assert t.value == 0.0


@pytest.mark.parametrize("call", [_enq, _launch], ids=["enqueue", "launch"])
def test_logsumexp_invalid_knob_is_refused(call, lse_variant):
    for v in (-2, 3, 7):
        lse_variant(v)
        assert call(_cfg()) == MM_ERR_BAD_ARGUMENT and "lse_variant" in _err(), v
        assert call(_cfg(path=g.PATH_ORDERED), acc=1) == MM_ERR_BAD_ARGUMENT, v
        assert g.kernel_name_logsumexp(_cfg(), 64, 64, 64) == "invalid"
        assert call(_cfg(reduce_op="Add")) == MM_ERR_UNSUPPORTED   # an unsupported configuration says so first


def test_logsumexp_valid_call_needs_a_device(lse_variant):
    # device -1 is refused only AFTER every argument check, so nothing is launched on any machine
    for acc in (0, 1):
        rc = _launch(_cfg(), device=-1, acc=acc)
        assert rc in (MM_ERR_NO_DEVICE, MM_ERR_BAD_ARGUMENT), rc
        assert "overlap" not in _err() and "lse_variant" not in _err(), _err()
    if g.lib().mm_init(None) != MM_ERR_NO_DEVICE:
        return   # a GPU is present: the fake addresses below must never reach a kernel
    for v in (-1, 0, 1, 2):
        lse_variant(v)
        for call in (_enq, _launch):
            for cfg in (_cfg(), _cfg(path=g.PATH_ORDERED), _cfg("double", "Min"), _cfg("half", transposed_a=True)):
                for acc in (0, 1):
                    assert call(cfg, acc=acc) == MM_ERR_NO_DEVICE, (v, call.__name__, _err())
            assert call(_cfg(), c=C0 + 4, a=A0 + 2, sa=E + 1) == MM_ERR_NO_DEVICE, _err()   # element-aligned is enough


def test_kernel_name_logsumexp_by_path_knob_and_config(lse_variant):
    name = g.kernel_name_logsumexp
    for dt in ("half", "float", "double"):
        for red in ("Min", "Max"):
            for t in (False, True):
                assert name(_cfg(dt, red, transposed_a=t), 37, 70001, 5) == "lse_hybrid"
                assert name(_cfg(dt, red, g.PATH_ORDERED, transposed_a=t), 8192, 8192, 8192, 4) == "lse_exact"
    for v, want in ((-1, "lse_hybrid"), (0, "lse_exact"), (1, "lse_hybrid"), (2, "lse_hybrid")):
        lse_variant(v)
        assert name(_cfg(), 300, 64, 272) == want, v
        assert name(_cfg(path=g.PATH_ORDERED), 300, 64, 272) == "lse_exact", v
    lse_variant(-1)
    assert name(_cfg("int"), 64, 64, 64) == "unsupported"
    assert name(_cfg(map_op="Multiply"), 64, 64, 64) == "unsupported"
    assert name(_cfg(reduce_op="Add"), 64, 64, 64) == "unsupported"
    assert name(_cfg(path=g.PATH_SPLIT), 64, 64, 64) == "unsupported"
    assert name(g.Config(99, 0, 4, 0, 0), 64, 64, 64) == "invalid"


def test_python_entry_points_refuse_host_tensors():
    torch = pytest.importorskip("torch")
    a, b = torch.zeros(4, 4), torch.zeros(4, 4)
    with pytest.raises(g.MMError, match="device tensors"):
        g.matmul_logsumexp(a, b)
    with pytest.raises(g.MMError, match="device tensors"):
        g.addmm_logsumexp_(torch.zeros(4, 4), a, b)


LSE_UNITS = ("mm_lse_fp.hip",)


def test_no_logsumexp_kernel_spills_or_uses_atomics():
    """Every kernel of the new unit: no scratch_ or v_accvgpr instruction, a zero private segment, NumAgprs 0, no atomic, and
    every store a vector-memory or LDS store."""
    from gemm_hls_amd import build
    for unit in LSE_UNITS:
        src = os.path.join(ROOT, "gemm_hls_amd", "csrc", unit)
        flags = [f for f in build.COMMON if f != "--offload-compress"]
        r = subprocess.run([build.HIPCC, *flags, *build.EXTRA.get(unit, []), "-S", "--cuda-device-only", src, "-o", "-"],
                           capture_output=True, text=True, timeout=1800)
        assert r.returncode == 0, r.stderr[-3000:]
        asm = r.stdout
        names = re.findall(r"^(_Z\w*lse_\w*kernel\w*):", asm, flags=re.M)
        # exact: 3 types x {Min, Max} x 2 layouts; epilogue, rowmax, colmax: 6 each; expand: 6 x 3 forms
        assert len(names) == 12 + 6 * 3 + 18, len(names)
        ops = {ln.split()[0] for ln in asm.split("\n") if ln.startswith("\t")}
        bad = sorted(op for op in ops if op.startswith(("scratch_", "v_accvgpr")) or "atomic" in op or
                     ("store" in op and not op.startswith(("global_store", "buffer_store", "ds_"))))
        assert bad == [], bad
        sizes = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", asm)
        assert sizes and all(s == "0" for s in sizes), sizes
        agprs = re.findall(r"; NumAgprs:\s*(\d+)", asm)
        assert len(agprs) >= len(names) and all(a == "0" for a in agprs), sorted(set(agprs))
        assert any(op.startswith("v_exp_f32") for op in ops) and any(op.startswith("v_max3_f32") for op in ops)


def _brute(a, b, reduce_op, seed=None):
    """One output at a time, math.fsum over the exponentials, the special values spelled out."""
    n, k = a.shape
    m = b.shape[1]
    sg = -1.0 if reduce_op == "Min" else 1.0
    out = np.empty((n, m))
    for i in range(n):
        for j in range(m):
            ts = [sg * float(np.float32(a[i, q]) + np.float32(b[q, j])) for q in range(k)]
            if seed is not None:
                ts.append(sg * float(seed[i, j]))
            if any(math.isnan(t) for t in ts):
                r = math.nan
            elif any(t == math.inf for t in ts):
                r = math.inf
            elif all(t == -math.inf for t in ts):
                r = -math.inf
            else:
                mx = max(ts)
                r = mx + math.log(math.fsum(math.exp(t - mx) for t in ts))
            out[i, j] = sg * r
    return out


@pytest.mark.parametrize("reduce_op", ["Max", "Min"])
def test_reference_matches_a_brute_force_loop(reduce_op):
    rng = np.random.default_rng(7)
    a = rng.uniform(-30, 30, size=(9, 13)).astype(np.float32)
    b = rng.uniform(-30, 30, size=(13, 11)).astype(np.float32)
    a[1, 3] = np.nan
    a[2, :] = -np.inf
    a[3, 5] = np.inf
    b[4, 6] = -np.inf          # with a[3, 5]: no pair, since k differs; a[3, 4] + b[4, 6] = -inf only
    b[5, 7] = -np.inf          # a[3, 5] + b[5, 7] = inf + -inf: NaN
    a[4, :] = -1e4
    a[4, 0] = 0                # one dominant term per output of row 4
    b[:, 2] = np.inf
    b[6, 2] = np.nan
    seed = rng.uniform(-5, 5, size=(9, 11))
    seed[0, 0], seed[1, 1], seed[2, 2] = -np.inf, np.inf, np.nan
    for s in (None, seed):
        ref = _lse_ref.logsumexp_ref(a, b, "float", reduce_op, s)
        want = _brute(a, b, reduce_op, s)
        assert np.array_equal(np.isnan(ref), np.isnan(want))
        fin = np.isfinite(want)
        assert np.array_equal(ref[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)])
        assert np.allclose(ref[fin], want[fin], rtol=0, atol=1e-9)
    # the K x N layout is the transpose, the bound is positive and grows with K and the magnitudes
    assert np.array_equal(_lse_ref.logsumexp_ref(a.T.copy(), b, "float", reduce_op, transposed_a=True),
                          _lse_ref.logsumexp_ref(a, b, "float", reduce_op), equal_nan=True)
    bnd = _lse_ref.bound(np.zeros((2, 4)), np.zeros((4, 3)), np.zeros((2, 3)))
    assert np.allclose(bnd, 2.0 ** -24 * (2 * 4 + 512))
    assert (_lse_ref.bound(np.full((2, 4), 100.0), np.zeros((4, 3)), np.zeros((2, 3)), "half") > bnd).all()
