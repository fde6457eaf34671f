"""Randomised shape fuzz on the GPU: every fast family against an independent result, over shapes
that straddle tile edges, partial k-slabs, flush boundaries (fp32 flushes its accumulators every
4096 k) and the minimum sizes each family accepts.  Seeded, so failures reproduce.

The second half is the differential shape fuzz over every product call in every form -- single and batched, plain and seeded,
N x K and K x N A, aligned and demoted -- on the case lists of tests/_fuzz_cases.py (whose coverage tests/test_fuzz_cases.py
checks on the CPU), against the numpy references the feature tests use.  What the cases reach, how long each test takes
next to the older ones, and which tests go red when a reference is perturbed: profiles/fuzz_coverage_mi355x.txt."""
import ctypes
import os
import zlib

import numpy as np
import pytest

import _bounds
import _closure_ref as cr
import _fuzz_cases as fc
import _lse_ref
import _oracle
import _product_ref as pr
import _semiring_ref as sr
import gemm_hls_amd as g

pytestmark = pytest.mark.gpu
SCALE = int(os.environ.get("MM_FUZZ_SCALE", "1"))  # MM_FUZZ_SCALE=10 for a long soak

#            dtype      k-multiple m-multiple  tolerance (None = bit-exact vs oracle Naive)
FAMILIES = {
    "float": (8, 4, 1e-5),
    "double": (8, 2, 1e-12),
    "half": (16, 8, 2.0 ** -10),
    "uint8_t": (32, 16, None),
    "int8_t": (32, 16, None),
}


def _shapes(rng, kmul, mmul, count):
    out = []
    for i in range(count):
        n = int(rng.choice([1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 511, 513, 700]))
        m = int(rng.choice([1, 2, 3, 7, 8, 15, 16, 17, 31, 32, 33, 40, 64, 65])) * mmul
        if i % 7 == 0:
            k = int(rng.choice([4096, 4096 + kmul, 8192 - kmul, 8192 + 2 * kmul]))  # around flush boundaries
            n, m = min(n, 300), min(m, 40 * mmul)
        else:
            k = int(rng.integers(1, 40)) * kmul
        out.append((n, k, m))
    return out


@pytest.mark.parametrize("dtype", list(FAMILIES))
def test_fuzz_fast_family_shapes(dtype):
    kmul, mmul, tol = FAMILIES[dtype]
    rng = np.random.default_rng(zlib.crc32(dtype.encode()))
    npdt = _oracle.NP_DTYPES[dtype]
    for (n, k, m) in _shapes(rng, kmul, mmul, 40 * SCALE):
        name = g.kernel_name(g.make_config(dtype), n, k, m)
        assert name.startswith("mfma_"), (dtype, n, k, m, name)
        if tol is None:
            a = rng.integers(0, 256, size=(n, k), dtype=np.uint8).view(npdt)
            b = rng.integers(0, 256, size=(k, m), dtype=np.uint8).view(npdt)
            want = _oracle.naive(dtype, "Multiply", "Add", a, b)
            c, _ = g.matmul_capi(a, b, dtype)
            assert np.array_equal(c, want), (dtype, n, k, m)
        else:
            lo, hi = (0.5, 2.0) if dtype == "half" else (1.0, 10.0)  # keep half sums finite at K = 8192
            a = rng.uniform(lo, hi, size=(n, k)).astype(npdt)
            b = rng.uniform(lo, hi, size=(k, m)).astype(npdt)
            exact = a.astype(np.float64) @ b.astype(np.float64)
            c, _ = g.matmul_capi(a, b, dtype)
            rel = np.abs(c.astype(np.float64) - exact) / exact
            assert rel.max() <= tol, (dtype, n, k, m, float(rel.max()))


@pytest.mark.parametrize("dtype,ops", [("float", ("Add", "Min")), ("int", ("Multiply", "Add")), ("double", ("Add", "Max")),
                                        ("long", ("Min", "Max")), ("int16_t", ("Multiply", "Add"))])
def test_fuzz_valu_tile_vs_ordered_and_oracle(dtype, ops):
    rng = np.random.default_rng(11)
    for (n, k, m) in _shapes(rng, 4, 4, 25 * SCALE):
        k = min(k, 600)
        a, b = _oracle.fill(dtype, n, k, m)
        c_fast, _ = g.matmul_capi(a, b, dtype, *ops)
        c_ord, _ = g.matmul_capi(a, b, dtype, *ops, path=g.PATH_ORDERED)
        assert np.array_equal(c_fast.view(np.uint8), c_ord.view(np.uint8)), (dtype, ops, n, k, m)
        assert np.array_equal(c_ord, _oracle.naive(dtype, ops[0], ops[1], a, b))


def test_fuzz_unaligned_shapes_take_the_predicated_path_and_stay_exact():
    rng = np.random.default_rng(5)
    for _ in range(20 * SCALE):
        n, k, m = (int(x) for x in rng.integers(1, 200, size=3))
        for dtype, ops in (("float", ("Multiply", "Add")), ("int", ("Multiply", "Add")), ("float", ("Add", "Min"))):
            a, b = _oracle.fill(dtype, n, k, m)
            c, _ = g.matmul_capi(a, b, dtype, *ops)
            want = _oracle.naive(dtype, ops[0], ops[1], a, b)
            if dtype == "float" and ops == ("Multiply", "Add"):
                assert _oracle.compare("float", c, want, 1e-5)[0] == 0, (n, k, m)
            else:
                assert np.array_equal(c, want), (dtype, ops, n, k, m)


def test_fuzz_split_path_any_shape_mixed_sign():
    """MM_PATH_SPLIT takes any N, K, M (the pack step pads): odd sizes straddling fragment (32), tile (128 / 256), slab
    (16) and flush (8256 k) boundaries, mixed-sign operands, both layouts of A, both tiles -- normwise against fp64 and
    bitwise between the two tile sizes."""
    rng = np.random.default_rng(2024)
    sizes = [1, 2, 31, 32, 33, 63, 65, 127, 129, 255, 256, 257, 300, 383, 511, 513, 700]
    for i in range(40 * SCALE):
        n, m = int(rng.choice(sizes)), int(rng.choice(sizes))
        k = int(rng.choice([8256, 8257, 8272, 16511])) if i % 8 == 0 else int(rng.integers(1, 700))
        if i % 8 == 0:
            n, m = min(n, 257), min(m, 257)
        a = rng.uniform(-3, 3, size=(n, k)).astype(np.float32)
        b = rng.uniform(-3, 3, size=(k, m)).astype(np.float32)
        exact = a.astype(np.float64) @ b.astype(np.float64)
        den = np.abs(a).astype(np.float64) @ np.abs(b).astype(np.float64)
        out = []
        for variant in (256, 512):                       # pinned 256 x 256 / 128 x 128 tile
            g.set_tuning("split_variant", variant)
            c, _ = g.matmul_capi(a, b, path=g.PATH_SPLIT)
            out.append(c)
        g.set_tuning("split_variant", -1)
        assert np.array_equal(out[0], out[1]), (n, k, m)
        assert float(np.max(np.abs(out[0] - exact) / np.maximum(den, 1e-300))) < 2.0 ** -19, (n, k, m)
        if i % 4 == 0:
            ct, _ = g.matmul_capi(np.ascontiguousarray(a.T), b, path=g.PATH_SPLIT, transposed_a=True)
            assert np.array_equal(ct, out[0]), (n, k, m)


@pytest.mark.parametrize("dtype", ["half", "float", "double"])
def test_fuzz_k_ordered_tile_kernel_is_naive_bit_for_bit(dtype):
    """MM_PATH_ORDERED (Multiply, Add) on the floating types -- the unfused, k-ascending contract of the reference's kernel
    (kernel/Compute.cpp:129-133), binary16 accumulating in binary16 for half -- through the register-tile kernel
    (mm_valu_tile_fp_exact.hip), on shapes with ragged N, one-chunk M, K below / not a multiple of the slab depth (synchronous
    staging, the shifted last slab) and K x N A: the bits of the CPU oracle's Naive and of the 64 x 64 anchor kernel."""
    rng = np.random.default_rng(zlib.crc32(("ordered" + dtype).encode()))
    for i, (n, k, m) in enumerate(_shapes(rng, 4, 4, 30 * SCALE)):
        k = min(k, 700)
        ta = i % 3 == 2
        if ta:
            n = (n + 3) // 4 * 4                              # a K x N A is served by the tile kernel when N % 4 == 0
        a, b = _oracle.fill(dtype, n, k, m)
        if dtype == "half":                                   # keep most binary16 sums finite so that the bits say something
            a, b = (a * np.float16(0.125)).astype(np.float16), (b * np.float16(0.25)).astype(np.float16)
        want = _oracle.naive(dtype, "Multiply", "Add", a, b)
        a_dev = np.ascontiguousarray(a.T) if ta else a
        assert g.kernel_name(g.make_config(dtype, path=g.PATH_ORDERED, transposed_a=ta), n, k, m) == "ordered_tile"
        c_tile, _ = g.matmul_capi(a_dev, b, dtype, path=g.PATH_ORDERED, transposed_a=ta)
        assert np.array_equal(c_tile.view(np.uint8), want.view(np.uint8)), (dtype, n, k, m, ta)
        if i % 5 == 0:
            g.set_tuning("ordered_variant", 0)
            try:
                c_anchor, _ = g.matmul_capi(a_dev, b, dtype, path=g.PATH_ORDERED, transposed_a=ta)
            finally:
                g.set_tuning("ordered_variant", -1)
            assert np.array_equal(c_anchor.view(np.uint8), want.view(np.uint8)), (dtype, n, k, m, ta)


# ======================================================================================================================
# The differential shape fuzz over every product call (tests/_fuzz_cases.py draws the cases; tests/test_fuzz_cases.py
# checks on the CPU that they reach every kernel name in every form).  C, the argreduce index I and the closure's D and W
# live between guard elements that are checked after the call; the gaps of a padded stride must keep their fill.
# ======================================================================================================================
GUARD = 64      # guard elements on each side of an output (64 elements keep a 16-byte aligned base for every type)
FILL = 7        # what a plain call's C (and I) hold before the call: every element of them must be overwritten
MA = fc.MA


def _group_ids(call):
    return [pytest.param(call, dtype, id=f"{call}-{dtype}") for dtype in fc.CONFIGS[call]]


def _fuzz(call, dtype, check):
    """check(case, rng, what) over the planned cases of (call, dtype); a failure names the case, the seed and the kernel."""
    seed, cases = fc.planned(call, dtype, SCALE)
    for case in cases:
        assert case.name not in ("unsupported", "invalid"), case
        what = f"{case} (seed {seed}, kernel {case.name})"
        try:
            check(case, fc.case_rng(seed, case), what)
        except AssertionError as e:
            raise AssertionError(f"{what}: {e}") from e


def _pattern(t, count):
    return (np.arange(count * np.dtype(t).itemsize) % 251 + 1).astype(np.uint8).view(t)


def _upload(host, off=0):
    """`host` on the device behind `off` elements of its type (an allocation is 256-byte aligned); (owner, address)."""
    import torch
    flat = np.ascontiguousarray(host).reshape(-1)
    raw = np.concatenate([np.zeros(off, dtype=flat.dtype), flat]).view(np.uint8)
    buf = torch.from_numpy(raw.copy()).to("cuda:0")
    return buf, buf.data_ptr() + off * flat.dtype.itemsize


class _Guarded:
    """A (batch, count) output at `stride` elements per element of the batch, its base moved by `off` elements, between two
    guards; the gaps of a padded stride hold a pattern."""

    def __init__(self, init, stride, off):
        self.batch, self.count = init.shape
        self.stride, self.lead, t = stride, GUARD + off, init.dtype
        body = np.empty((self.batch, stride), dtype=t)
        body[:, :self.count] = init
        body[:, self.count:] = _pattern(t, stride - self.count)
        self.host = np.concatenate([_pattern(t, self.lead), body.reshape(-1), _pattern(t, GUARD)])
        self.dev, base = _upload(self.host)
        self.ptr = base + self.lead * t.itemsize

    def read(self, name):
        out = self.dev.cpu().numpy().view(self.host.dtype)
        assert out[:self.lead].tobytes() == self.host[:self.lead].tobytes(), f"the guard in front of {name} was overwritten"
        assert out[-GUARD:].tobytes() == self.host[-GUARD:].tobytes(), f"the guard behind {name} was overwritten"
        body = out[self.lead:-GUARD].reshape(self.batch, self.stride)
        want = self.host[self.lead:-GUARD].reshape(self.batch, self.stride)
        assert body[:, self.count:].tobytes() == want[:, self.count:].tobytes(), f"a gap of {name}'s padded stride was overwritten"
        return body[:, :self.count].copy()


def _launch(case, a, b, c_init, i_init=None, index_base=0):
    """The blocking launch of case.call on host operands: a (1 or batch, rows, cols) and b likewise -- one matrix when the
    case broadcasts it -- c_init (batch, n, m): the seed, or the fill a plain call must overwrite.  Returns C (batch, n, m),
    and I with it for the argreduce calls."""
    n, k, m, batch = case.n, case.k, case.m, case.batch
    sa, sb, sc = fc.strides(case)
    assert a.shape[0] == (batch if sa else 1) and b.shape[0] == (batch if sb else 1)
    (ka, pa), (kb, pb) = _upload(a, int(case.misalign == "a")), _upload(b, int(case.misalign == "b"))
    c = _Guarded(c_init.reshape(batch, n * m), sc, int(case.misalign == "c"))
    cfg = ctypes.byref(g.make_config(case.dtype, case.mp, case.rd, case.path, case.ta))
    L, acc = g.lib(), int(case.seeded)
    if case.call == "batched":
        if case.seeded and batch == 1 and case.draw % 2 == 0:
            rc = L.mm_gemm_accumulate_launch(0, cfg, pa, pb, c.ptr, n, k, m, None)
        else:
            fn = L.mm_gemm_batched_accumulate_launch if case.seeded else L.mm_gemm_batched_launch
            rc = fn(0, cfg, pa, pb, c.ptr, n, k, m, batch, sa, sb, sc, None)
    elif case.call in ("argreduce", "argreduce_nt"):
        i = _Guarded(i_init.reshape(batch, n * m), sc, int(case.misalign == "i"))
        fn = L.mm_gemm_argreduce_launch if case.call == "argreduce" else L.mm_gemm_argreduce_nt_launch
        rc = fn(0, cfg, pa, pb, c.ptr, i.ptr, n, k, m, batch, sa, sb, sc, index_base, acc, None)
    else:
        fn = {"logsumexp": L.mm_gemm_logsumexp_launch, "logsumexp_nt": L.mm_gemm_logsumexp_nt_launch,
              "widen": L.mm_gemm_widen_launch, "nt": L.mm_gemm_nt_launch}[case.call]
        rc = fn(0, cfg, pa, pb, c.ptr, n, k, m, batch, sa, sb, sc, acc, None)
    assert rc == 0, (rc, L.mm_last_error().decode())
    out = c.read("C").reshape(batch, n, m)
    return (out, i.read("I").reshape(batch, n, m)) if case.call in ("argreduce", "argreduce_nt") else out


def _counts(case):
    """(matrices of A, matrices of B) the case's batch holds."""
    return 1 if case.stride == "a_bcast" else case.batch, 1 if case.stride == "b_bcast" else case.batch


def _a_shape(case):
    return (case.k, case.n) if case.ta else (case.n, case.k)


def _semiring_operands(case, rng, non_finite):
    """_semiring_ref's edge-valued operand sets, one draw per matrix: a (na, N x K or K x N), b (nb, K, M)."""
    na, nb = _counts(case)
    pairs = []
    for _ in range(max(na, nb)):
        if sr.is_float(case.dtype):   # (the all-inf row needs a row 3)
            pairs.append(sr.float_operands(case.dtype, case.mp, case.rd, _a_shape(case), (case.k, case.m), rng,
                                           non_finite and case.n > sr.INF_ROW, a_row_axis=1 if case.ta else 0))
        else:
            pairs.append(sr.int_operands(case.dtype, case.mp, case.rd, _a_shape(case), (case.k, case.m), rng,
                                         a_row_axis=1 if case.ta else 0))
    return np.stack([p[0] for p in pairs[:na]]), np.stack([p[1] for p in pairs[:nb]])


def _uniform_operands(case, rng, lo, hi):
    na, nb = _counts(case)
    t = sr.NP_DTYPES[case.dtype]
    return rng.uniform(lo, hi, size=(na,) + _a_shape(case)).astype(t), rng.uniform(lo, hi, size=(nb, case.k, case.m)).astype(t)


def _transposed(b):
    """(nb, K, M) as the M x K storage of the A x B^T calls, and back."""
    return np.ascontiguousarray(b.transpose(0, 2, 1))


def _fill(case, t):
    return np.full((case.batch, case.n, case.m), FILL, dtype=t)


def _element(x, e):
    return x[0 if x.shape[0] == 1 else e]


def _reversed_batch(case, a, b, *outs):
    """The same batch in the opposite order (a broadcast matrix stays where it is)."""
    flip = lambda x: x if x.shape[0] == 1 else np.ascontiguousarray(x[::-1])   # noqa: E731
    return (flip(a), flip(b)) + tuple(np.ascontiguousarray(x[::-1]) for x in outs)


# ---- batched and accumulating ----------------------------------------------------------------------------------------------
def _check_batched(case, rng, what):
    from test_gpu_accumulate import seeds
    dtype, mp, rd, ta, k = case.dtype, case.mp, case.rd, case.ta, case.k
    t = sr.NP_DTYPES[dtype]
    shape = (case.batch, case.n, case.m)
    auto = case.path == g.PATH_AUTO
    bounded = sr.is_float(dtype) and (mp, rd) == MA and auto         # floating (Multiply, Add) on the fast path: a bound
    minmax_float = sr.is_float(dtype) and rd in ("Min", "Max") and auto
    if sr.is_float(dtype) and (mp, rd) == MA:
        a, b = _uniform_operands(case, rng, -2, 2)
        c0 = rng.uniform(-8, 8, size=shape).astype(t)
    else:
        a, b = _semiring_operands(case, rng, non_finite=not minmax_float)
        c0 = seeds(dtype, shape, rng, nan=not minmax_float)
    got = _launch(case, a, b, c0 if case.seeded else _fill(case, t))
    for e in range(case.batch):
        ae, be = _element(a, e), _element(b, e)
        if bounded:
            ok, err = pr.within_bound(dtype, got[e], ae, be, c0[e] if case.seeded else np.zeros(shape[1:], t), ta)
            assert ok, (e, err, pr.MUL_ADD_TOL[dtype])
            if dtype == "float":
                assert err < _bounds.f32_chain_guard(k), (e, err, _bounds.f32_chain_guard(k))
            continue
        tile = minmax_float and case.name.startswith("valu_tile")        # minNum / maxNum: which zero a tie returns is open
        want = (pr.seeded_reference(dtype, mp, rd, ae, be, c0[e], ta, auto_minmax=tile) if case.seeded else
                sr.reference(dtype, mp, rd, ae, be, ta, auto_minmax=tile))
        same = sr.same_values if minmax_float else sr.same_bits
        assert same(got[e], want), (e, sr.first_difference(got[e], want, by_value=minmax_float))
    if case.batch > 1:   # an element's bits do not depend on its position in the batch
        ar, br, c0r = _reversed_batch(case, a, b, c0)
        again = _launch(case, ar, br, c0r if case.seeded else _fill(case, t))
        assert sr.same_bits(again[::-1], got), ("batch reversed", sr.first_difference(again[::-1], got))
    cfg = g.make_config(dtype, mp, rd, case.path, ta)
    if not case.seeded and g.kernel_name(cfg, case.n, k, case.m) == g.kernel_name_batched(cfg, case.n, k, case.m, 1) == case.name:
        single, _ = g.matmul_capi(a[0], b[0], dtype, mp, rd, case.path, ta)
        assert sr.same_bits(got[0], single), ("the single launch", sr.first_difference(got[0], single))


@pytest.mark.parametrize("call,dtype", _group_ids("batched"))
def test_fuzz_batched_and_accumulating(call, dtype):
    """mm_gemm_batched_launch, mm_gemm_batched_accumulate_launch and, for a seeded batch of one, mm_gemm_accumulate_launch:
    exact configurations the bits of _semiring_ref.reference / seeded_reference, floating Min / Max on valu_tile by value
    against minNum / maxNum, floating (Multiply, Add) under MM_PATH_AUTO within MUL_ADD_TOL (float: and the chain guard of
    tests/_bounds.py); the batch in reverse order gives the same bits per element, and element 0 the single launch's bits
    wherever mm_kernel_name names the kernel the batched resolver names."""
    _fuzz(call, dtype, _check_batched)


# ---- argmin / argmax, row-major B and B^T --------------------------------------------------------------------------------------
def _check_argreduce(case, rng, what):
    from test_gpu_argreduce import seeds
    dtype, mp, rd = case.dtype, case.mp, case.rd
    t = sr.NP_DTYPES[dtype]
    shape = (case.batch, case.n, case.m)
    a, b = _semiring_operands(case, rng, non_finite=True)
    c0, i0 = seeds(dtype, shape, rng), rng.integers(-1, 1000, size=shape).astype(np.int32)
    base = 5 if case.seeded else 0
    b_dev = _transposed(b) if case.call == "argreduce_nt" else b
    got_c, got_i = _launch(case, a, b_dev, c0 if case.seeded else _fill(case, t),
                           i0 if case.seeded else _fill(case, np.int32), base)
    for e in range(case.batch):
        want_c, want_i = pr.oracle(dtype, mp, rd, _element(a, e), _element(b, e), c0[e] if case.seeded else None,
                                   i0[e] if case.seeded else None, case.ta, base)
        assert sr.same_bits(got_c[e], want_c), (e, "values", sr.first_difference(got_c[e], want_c))
        assert np.array_equal(got_i[e], want_i), (e, "indices", sr.first_difference(got_i[e], want_i))


@pytest.mark.parametrize("call,dtype", _group_ids("argreduce") + _group_ids("argreduce_nt"))
def test_fuzz_argreduce(call, dtype):
    """mm_gemm_argreduce_launch / mm_gemm_argreduce_nt_launch on both paths, plain and seeded with index_base = 5: values and
    indices exactly the contract's loop (_product_ref.oracle; for the B^T form on the transposed operand)."""
    _fuzz(call, dtype, _check_argreduce)


# ---- log-sum-exp, row-major B and B^T ------------------------------------------------------------------------------------------
def _check_logsumexp(case, rng, what):
    dtype, rd = case.dtype, case.rd
    t = sr.NP_DTYPES[dtype]
    a, b = _uniform_operands(case, rng, -8, 8)
    seed = rng.uniform(-8, 8, size=(case.batch, case.n, case.m)).astype(t)
    got = _launch(case, a, _transposed(b) if case.call == "logsumexp_nt" else b, seed if case.seeded else _fill(case, t))
    for e in range(case.batch):
        ae, be = _element(a, e), _element(b, e)
        ref = _lse_ref.logsumexp_ref(ae, be, dtype, rd, seed[e] if case.seeded else None, case.ta)
        _lse_ref.check(got[e], ref, ae, be, dtype, rd, case.ta, f"element {e}")


@pytest.mark.parametrize("call,dtype", _group_ids("logsumexp") + _group_ids("logsumexp_nt"))
def test_fuzz_logsumexp(call, dtype):
    """mm_gemm_logsumexp_launch / mm_gemm_logsumexp_nt_launch, both reductions and both paths, plain and seeded (the
    row-major form with a K x N A as well): _lse_ref.check against _lse_ref.logsumexp_ref."""
    _fuzz(call, dtype, _check_logsumexp)


# ---- widening ------------------------------------------------------------------------------------------------------------------
def _half(x):
    with np.errstate(over="ignore"):
        return x.astype(np.float16)


def _check_widen(case, rng, what):
    dtype, k = case.dtype, case.k
    na, nb = _counts(case)
    shape = (case.batch, case.n, case.m)
    if dtype == "int8_t":
        a = rng.integers(-128, 128, (na,) + _a_shape(case), dtype=np.int8)
        b = rng.integers(-128, 128, (nb, k, case.m), dtype=np.int8)
        seed = rng.integers(-2 ** 31, 2 ** 31, shape, dtype=np.int64).astype(np.int32)
    elif case.draw % 2:     # bmm's own range: one rounding of the wide C stays finite
        a, b = _uniform_operands(case, rng, -2, 2)
        seed = rng.uniform(-8, 8, size=shape).astype(np.float32)
    else:                   # mixed signs, magnitudes log-uniform over binary16's normal range (tests/test_gpu_widen.py)
        wide = lambda s: (np.minimum(2.0 ** rng.uniform(-14.0, 16.0, s), 65504.0) * rng.choice([-1.0, 1.0], s)).astype(np.float16)  # noqa: E731
        a, b = wide((na,) + _a_shape(case)), wide((nb, k, case.m))
        seed = (rng.standard_normal(shape) * np.abs(a.astype(np.float64)).mean() * np.abs(b.astype(np.float64)).mean() * k
                ).astype(np.float32)
    ct = np.int32 if dtype == "int8_t" else np.float32
    got = _launch(case, a, b, seed if case.seeded else _fill(case, ct))
    assert got.dtype == ct
    for e in range(case.batch):
        ae = _element(a, e).T if case.ta else _element(a, e)
        be, se = _element(b, e), seed[e] if case.seeded else None
        if dtype == "int8_t":
            assert np.array_equal(got[e], pr._int_ref(ae, be, se)), (e, sr.first_difference(got[e], pr._int_ref(ae, be, se)))
        elif case.path == g.PATH_ORDERED:
            want = pr._f32_loop(ae, be, se)
            assert sr.same_bits(got[e], want), (e, sr.first_difference(got[e], want))
        else:
            pr._check_bound(f"element {e}", got[e], ae, be, se)
    aligned = case.misalign is None and case.stride != "c_pad1"       # (a demoted launch sums in blocks of k: other bits)
    if dtype == "half" and case.path == g.PATH_AUTO and not case.seeded and aligned:
        narrow = _launch(case._replace(call="batched"), a, b, _fill(case, np.float16))
        assert sr.same_bits(_half(got), narrow), ("one rounding of the wide C is not the narrow batched launch's C",
                                                  sr.first_difference(_half(got), narrow))


@pytest.mark.parametrize("call,dtype", _group_ids("widen"))
def test_fuzz_widen(call, dtype):
    """mm_gemm_widen_launch: int8_t exactly _int_ref on both paths; half under MM_PATH_ORDERED the bits of _f32_loop, under
    MM_PATH_AUTO within the header's 1e-6 (_check_bound), and one rounding of a plain, aligned result to binary16 the bits
    of mm_gemm_batched_launch on the same operands.  (Measured: at most 0.57 of that bound.  The k-ascending fallback for a
    shape the matrix cores do not take is bounded by (K - 1) 2^-24, says the header; the planned cases draw it at K <= 96,
    a float32 loop on the host reaches 1.07 of 1e-6 at K = 697 on these operands: a finding a long soak may repeat.)"""
    _fuzz(call, dtype, _check_widen)


# ---- A x B^T -------------------------------------------------------------------------------------------------------------------
def _check_nt(case, rng, what):
    from test_gpu_accumulate import seeds
    dtype, mp, rd, k = case.dtype, case.mp, case.rd, case.k
    t = sr.NP_DTYPES[dtype]
    shape = (case.batch, case.n, case.m)
    auto = case.path == g.PATH_AUTO
    float_ma = sr.is_float(dtype) and (mp, rd) == MA
    minmax_float = sr.is_float(dtype) and rd in ("Min", "Max") and auto
    # what the launch runs: a moved A or Bt demotes valu_tile_nt, and a moved or oddly strided C demotes nt_prepass as well
    demoted = (case.name == "valu_tile_nt" and case.misalign in ("a", "b")) or (
        case.name == "nt_prepass" and (case.misalign is not None or case.stride == "c_pad1"))
    running = "ordered_nt" if demoted else case.name
    if float_ma and auto and dtype != "half" and running == "valu_tile_nt":   # the operands of tests/test_gpu_nt.py's bound
        na, nb = _counts(case)
        pairs = [sr.float_operands(dtype, mp, rd, (case.n, k), (k, case.m), rng, non_finite=False, largest=False)
                 for _ in range(max(na, nb))]
        a, b = np.stack([p[0] for p in pairs[:na]]), np.stack([p[1] for p in pairs[:nb]])
        c0 = rng.uniform(-8, 8, size=shape).astype(t)
    elif float_ma:
        a, b = _uniform_operands(case, rng, -2, 2)
        c0 = rng.uniform(-8, 8, size=shape).astype(t)
    else:
        a, b = _semiring_operands(case, rng, non_finite=not minmax_float)
        c0 = seeds(dtype, shape, rng, nan=not minmax_float)
    bt = _transposed(b)
    init = c0 if case.seeded else _fill(case, t)
    got = _launch(case, a, bt, init)
    for e in range(case.batch):
        ae, be, ce = _element(a, e), _element(b, e), c0[e] if case.seeded else None
        if float_ma and auto and dtype == "half":
            if running != "nt_prepass":   # exact products, f32 sums k ascending, one rounding (test_nt_misaligned_bt_keeps_halfs_f32_contract)
                want = _half(pr._f32_loop(ae, be, ce))
                assert sr.same_bits(got[e], want), (e, running, sr.first_difference(got[e], want))
            ok, err = pr.within_bound(dtype, got[e], ae, be, ce if case.seeded else np.zeros(shape[1:], t))
            assert ok, (e, err)
        elif float_ma and auto:           # the bound of test_nt_valu_tile_float_multiply_add_within_the_bound
            exact, scale = sr.exact_and_scale(dtype, ae, be)
            assert exact is not None and sr.wide_type(dtype) is not None, "no type wide enough for the exact product"
            tiny = np.finfo(t).smallest_subnormal.astype(exact.dtype)
            if case.seeded:
                exact, scale = exact + ce.astype(exact.dtype), scale + np.abs(ce.astype(exact.dtype))
            assert np.all(np.isfinite(got[e]))
            err = _bounds.normwise(got[e].astype(exact.dtype), exact, scale + k * tiny)
            if dtype == "float":
                _bounds.north_star(err, f"{running} float, element {e}")
                _bounds.guard(err, _bounds.f32_chain_guard(k), f"{running} float, element {e}")
            else:
                assert err < 1e-12, (e, err)
        else:                             # exact: Naive on the transposed operand
            tile = minmax_float and running == "valu_tile_nt"
            want = (pr.seeded_reference(dtype, mp, rd, ae, be, ce, auto_minmax=tile) if case.seeded else
                    sr.reference(dtype, mp, rd, ae, be, auto_minmax=tile))
            same = sr.same_values if minmax_float else sr.same_bits
            assert same(got[e], want), (e, running, sr.first_difference(got[e], want, by_value=minmax_float))
    if running == "nt_prepass":   # bit for bit the batched call on a materialised transpose
        want = _launch(case._replace(call="batched"), a, b, init)
        assert sr.same_bits(got, want), ("the batched call on a materialised transpose", sr.first_difference(got, want))


@pytest.mark.parametrize("call,dtype", _group_ids("nt"))
def test_fuzz_nt(call, dtype):
    """mm_gemm_nt_launch: exact semirings the bits of the reference on the transposed operand (floating Min / Max on
    valu_tile_nt by value), nt_prepass the bits of the batched call on a materialised transpose, float and double (Multiply,
    Add) within the bound of tests/test_gpu_nt.py, half (Multiply, Add) off the matrix cores the f32-sum contract."""
    _fuzz(call, dtype, _check_nt)


# ---- closure -------------------------------------------------------------------------------------------------------------------
def _check_closure(case, rng, what):
    dtype, mp, rd, n, batch = case.dtype, case.mp, case.rd, case.n, case.batch
    t = np.dtype(sr.NP_DTYPES[dtype])
    block = fc.closure_block(case)
    assert (case.name == "closure_onchip") == (n <= block), (case.name, block)
    seed = fc.PLAN[case.call, dtype][0]
    d = fc.closure_graphs(seed, case)
    stride = n * n + {"c_pad64": 64, "c_pad1": 1}.get(case.stride, 0)
    off = int(case.misalign is not None)
    dd = _Guarded(d.reshape(batch, n * n), stride, off)
    dw = _Guarded(np.full((batch, n * n), 12345, dtype=np.int32), stride, off) if case.witness else None
    cfg = g.make_config(dtype, mp, rd, case.path)
    rc = g.lib().mm_closure_launch(0, ctypes.byref(cfg), dd.ptr, dw.ptr if dw else None, n, batch, stride, None)
    assert rc == 0, (rc, g.lib().mm_last_error().decode())
    got_d = dd.read("D").reshape(batch, n, n)
    got_w = dw.read("W").reshape(batch, n, n) if dw else None
    auto = case.path == g.PATH_AUTO and not case.witness        # step 3 on valu_tile: minNum / maxNum (tests/test_gpu_closure.py)
    for e in range(batch):
        want_d, want_w = cr.blocked(dtype, mp, rd, d[e], block, witness=case.witness, auto=auto)
        if n >= fc.CLOSURE_INFORMATIVE_MIN_N:
            cr.assert_informative(dtype, mp, rd, d[e], want_d, f"graph {e}")
        if auto and sr.is_float(dtype):
            assert sr.same_values(got_d[e], want_d), (e, sr.first_difference(got_d[e], want_d, by_value=True))
        else:
            assert sr.same_bits(got_d[e], want_d), (e, sr.first_difference(got_d[e], want_d))
        if case.witness:
            assert np.array_equal(got_w[e], want_w), (e, "witness", np.argwhere(got_w[e] != want_w)[:3])


@pytest.mark.parametrize("call,dtype", _group_ids("closure"))
def test_fuzz_closure(call, dtype):
    """mm_closure_launch at the default block size, n on both sides of it, with and without witnesses, batches at dense and
    padded strides, D 16-byte aligned or moved by one element: values and witnesses exactly as tests/test_gpu_closure.py
    compares them with _closure_ref.blocked, on graphs of _closure_ref.graphs whose closure is informative."""
    _fuzz(call, dtype, _check_closure)
