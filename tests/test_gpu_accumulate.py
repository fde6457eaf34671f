"""GPU tests of the accumulating entry points (mm_gemm_accumulate_* / mm_gemm_batched_accumulate_*, addmm_ / baddbmm_):
C <- C (+) (A (x) B), each output's reduction starting at the value C holds.  The reference is Naive's loop with acc = C,
written here on top of _semiring_ref's operators."""
import ctypes
import zlib

import numpy as np
import pytest

import _semiring_ref as sr
import gemm_hls_amd as g
from _product_ref import MUL_ADD_TOL, seeded_reference, within_bound

pytestmark = pytest.mark.gpu

GUARD = 64   # elements of guard pattern on each side of C


def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x).reshape(-1).view(np.uint8).copy()).to("cuda:0")


def accumulate(cfg, a_flat, b_flat, c_flat, n, k, m, batch=1, sa=0, sb=0, sc=0, single=False):
    """Runs the accumulating launch on host arrays (C inside a guarded buffer); checks the guards; returns C flat."""
    t = c_flat.dtype
    pattern = (np.arange(GUARD * t.itemsize) % 251 + 1).astype(np.uint8).view(t)
    buf = np.concatenate([pattern, c_flat, pattern])
    da, db, dc = _dev(a_flat), _dev(b_flat), _dev(buf)
    cp = dc.data_ptr() + GUARD * t.itemsize
    if single:
        rc = g.lib().mm_gemm_accumulate_launch(0, ctypes.byref(cfg), da.data_ptr(), db.data_ptr(), cp, n, k, m, None)
    else:
        rc = g.lib().mm_gemm_batched_accumulate_launch(0, ctypes.byref(cfg), da.data_ptr(), db.data_ptr(), cp, n, k, m,
                                                       batch, sa, sb, sc, None)
    assert rc == 0, (rc, g.lib().mm_last_error().decode())
    out = dc.cpu().numpy().view(t)
    assert out[:GUARD].tobytes() == pattern.tobytes() and out[-GUARD:].tobytes() == pattern.tobytes(), "guard overwritten"
    return out[GUARD:-GUARD]


def plain(cfg, a_flat, b_flat, n, k, m, batch=1, sa=0, sb=0, sc=0, c_init=None):
    c = np.zeros((batch - 1) * sc + n * m, dtype=a_flat.dtype) if c_init is None else c_init.copy()
    da, db, dc = _dev(a_flat), _dev(b_flat), _dev(c)
    rc = g.lib().mm_gemm_batched_launch(0, ctypes.byref(cfg), da.data_ptr(), db.data_ptr(), dc.data_ptr(), n, k, m, batch,
                                        sa, sb, sc, None)
    assert rc == 0, (rc, g.lib().mm_last_error().decode())
    return dc.cpu().numpy().view(a_flat.dtype)


def operands(dtype, mp, rd, n, k, m, rng, ta=False, non_finite=True):
    a_shape = (k, n) if ta else (n, k)
    if sr.is_float(dtype):
        return sr.float_operands(dtype, mp, rd, a_shape, (k, m), rng, non_finite, a_row_axis=1 if ta else 0)
    return sr.int_operands(dtype, mp, rd, a_shape, (k, m), rng, a_row_axis=1 if ta else 0)


def seeds(dtype, shape, rng, nan=True):
    """Full-range seeds with the type's min, max, 0 (and +-inf, NaN for floating types) planted."""
    t = sr.NP_DTYPES[dtype]
    if sr.is_float(dtype):
        c = (rng.uniform(-4, 4, size=shape)).astype(t)
        lo, hi = sr.limits(dtype)
        special = [t(0), t(-0.0), lo, hi, t(np.inf), t(-np.inf)] + ([t(np.nan)] if nan else [])
    else:
        info = np.iinfo(t)
        u = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[np.dtype(t).itemsize]
        c = rng.integers(0, np.iinfo(u).max, size=shape, dtype=u, endpoint=True).view(t)
        special = [t(0), t(info.min), t(info.max), t(1)]
    flat = c.reshape(-1)
    idx = rng.choice(flat.size, size=min(flat.size, 4 * len(special)), replace=False)
    flat[idx] = np.resize(np.array(special, dtype=t), idx.size)
    return c


# ---- 1. MM_PATH_ORDERED: all 275 configurations, seeded Naive's bits, single and batched -------------------------------
@pytest.mark.parametrize("dtype,mp,rd", sr.CONFIGS, ids=lambda x: str(x))
def test_ordered_every_config_is_seeded_naive(dtype, mp, rd):
    n, k, m, batch = 33, 17, 29, 2
    rng = np.random.default_rng(zlib.crc32(f"acc/{dtype}/{mp}/{rd}".encode()))
    a, b = operands(dtype, mp, rd, n, k, m, rng)
    c0 = seeds(dtype, (batch, n, m), rng)
    cfg = g.make_config(dtype, mp, rd, g.PATH_ORDERED)
    got = accumulate(cfg, a, b, c0.ravel(), n, k, m, batch, 0, 0, n * m).reshape(batch, n, m)   # A and B broadcast
    single = accumulate(cfg, a, b, c0[0].ravel(), n, k, m, single=True).reshape(n, m)
    for e in range(batch):
        want = seeded_reference(dtype, mp, rd, a, b, c0[e])
        assert sr.same_bits(got[e], want), (e, sr.first_difference(got[e], want))
    assert sr.same_bits(single, seeded_reference(dtype, mp, rd, a, b, c0[0]))


def test_ordered_min_seed_inf_stays_inf():
    # a Min chain seeded with +inf whose mapped values are all +inf returns +inf, not max()
    a = np.full((4, 8), np.inf, dtype=np.float32)
    b = np.ones((8, 4), dtype=np.float32)
    c0 = np.full((4, 4), np.inf, dtype=np.float32)
    for path in (g.PATH_ORDERED, g.PATH_AUTO):
        got = accumulate(g.make_config("float", "Add", "Min", path), a, b, c0.ravel(), 4, 8, 4, single=True)
        assert np.all(np.isposinf(got)), got


# ---- 2. MM_PATH_AUTO: all 275 ------------------------------------------------------------------------------------------
def _auto_family(dtype, mp, rd):
    if (mp, rd) == ("Multiply", "Add"):
        return {"float": "mfma_f32", "double": "mfma_f64", "half": "mfma_f16", "int8_t": "mfma_i8", "uint8_t": "mfma_i8"}.get(
            dtype, "valu_tile")
    return "valu_tile" if mp != "And" and rd in ("Add", "Min", "Max") else "ordered"


@pytest.mark.parametrize("dtype,mp,rd", sr.CONFIGS, ids=lambda x: str(x))
def test_auto_every_config(dtype, mp, rd):
    n, k, m, batch = 250, 128, 256, 2
    rng = np.random.default_rng(zlib.crc32(f"auto/{dtype}/{mp}/{rd}".encode()))
    mul_add_float = (mp, rd) == ("Multiply", "Add") and sr.is_float(dtype)
    minmax_float = sr.is_float(dtype) and rd in ("Min", "Max")
    if mul_add_float:
        a = rng.uniform(-2, 2, size=(n, k)).astype(sr.NP_DTYPES[dtype])
        b = rng.uniform(-2, 2, size=(k, m)).astype(sr.NP_DTYPES[dtype])
        c0 = rng.uniform(-8, 8, size=(batch, n, m)).astype(sr.NP_DTYPES[dtype])
    else:
        a, b = operands(dtype, mp, rd, n, k, m, rng, non_finite=not minmax_float)
        c0 = seeds(dtype, (batch, n, m), rng, nan=not minmax_float)
    cfg = g.make_config(dtype, mp, rd)
    name = g.kernel_name_batched(cfg, n, k, m, batch)
    assert name.startswith(_auto_family(dtype, mp, rd)), name
    got = accumulate(cfg, a, b, c0.ravel(), n, k, m, batch, 0, 0, n * m).reshape(batch, n, m)
    for e in range(batch):
        if mul_add_float:
            ok, err = within_bound(dtype, got[e], a, b, c0[e])
            assert ok, (name, err)
        elif sr.is_float(dtype) and "Min" in (mp, rd) or sr.is_float(dtype) and "Max" in (mp, rd):
            # valu_tile: minNum / maxNum, the same value as std::min / max for numbers; which zero a tie returns is unspecified
            want = seeded_reference(dtype, mp, rd, a, b, c0[e], auto_minmax=name.startswith("valu_tile"))
            assert sr.same_values(got[e], want), (name, sr.first_difference(got[e], want, by_value=True))
        else:
            want = seeded_reference(dtype, mp, rd, a, b, c0[e])
            assert sr.same_bits(got[e], want), (name, sr.first_difference(got[e], want))


# ---- 3. every batched family by name, ragged N (and M where the family allows it), guarded C ---------------------------
FAMILIES = [  # (dtype, map, reduce, path, (n, k, m), transposed_a, knob, value, expected name prefix)
    ("float", "Add", "Min", g.PATH_ORDERED, (33, 17, 29), False, None, None, "ordered"),
    # two tiles each way, a one-line last tile, a one-k last slab: both stagings of the 64 x 64 kernel's seeded form
    ("float", "Add", "Min", g.PATH_ORDERED, (65, 17, 67), False, None, None, "ordered"),
    ("int", "Multiply", "Add", g.PATH_ORDERED, (65, 17, 67), True, None, None, "ordered"),
    ("float", "Add", "Min", g.PATH_ORDERED, (130, 128, 136), False, None, None, "ordered_tile"),
    ("half", "Multiply", "Add", g.PATH_AUTO, (130, 128, 132), False, None, None, "ordered_wide_f16"),
    ("int", "Add", "Min", g.PATH_AUTO, (130, 128, 136), False, None, None, "valu_tile"),              # DMA-staged
    ("int", "Add", "Min", g.PATH_AUTO, (132, 64, 136), True, None, None, "valu_tile"),                # synchronous
    ("long", "Multiply", "Max", g.PATH_AUTO, (130, 128, 136), False, None, None, "valu_tile"),        # 8-byte DMA form
    ("int", "Add", "Min", g.PATH_AUTO, (130, 128, 136), False, "valu_variant", 0, "valu_tile"),       # synchronous, row-major
    ("float", "Multiply", "Add", g.PATH_AUTO, (300, 264, 260), False, "f32_variant", 33, "mfma_f32_128x256"),
    ("float", "Multiply", "Add", g.PATH_AUTO, (300, 264, 260), False, "f32_variant", 8, "mfma_f32_256x256"),
    ("float", "Multiply", "Add", g.PATH_AUTO, (300, 264, 260), False, "f32_variant", 35, "mfma_f32_128x128"),
    ("float", "Multiply", "Add", g.PATH_AUTO, (300, 264, 260), True, None, None, "mfma_f32_256x256"),
    ("float", "Multiply", "Add", g.PATH_AUTO, (300, 4200, 260), False, "f32_variant", 35, "mfma_f32_128x128"),  # mid flush
] + [("double", "Multiply", "Add", g.PATH_AUTO, (250, 256, 264), ta, "f64_variant", v, "mfma_f64")
     for v in range(5) for ta in (False, True)] + [
    ("half", "Multiply", "Add", g.PATH_AUTO, (250, 512, 512), False, "f16_variant", v, name) for v, name in
    [(-1, "mfma_f16_256x256_pingpong_16x16x32"), (100, "mfma_f16_256x256_pingpong_32x32x16"),
     (0, "mfma_f16_256x256x64_slab64"), (4, "mfma_f16_128x256x64_slab64"), (5, "mfma_f16_64x256x64_slab64")]] + [
    ("half", "Multiply", "Add", g.PATH_AUTO, (256, 512, 512), True, "f16_variant", v, name) for v, name in
    [(-1, "mfma_f16_256x256_pingpong_k32_KxN"), (0, "mfma_f16_256x256x64_slab64_KxN")]] + [
    ("uint8_t", "Multiply", "Add", g.PATH_AUTO, (250, 512, 512), False, "i8_variant", 10, "mfma_i8_256x256_pingpong_k64"),
] + [("int8_t" if v % 2 else "uint8_t", "Multiply", "Add", g.PATH_AUTO, (250, 512, 512), False, "i8_variant", v, name)
     for v, name in [(-1, "mfma_i8_256x256_pingpong_16x16x64"), (100, "mfma_i8_256x256_pingpong_32x32x32"),
                     (0, "mfma_i8_256x256x128_slab128"), (5, "mfma_i8_64x256x128_slab128")]] + [
    ("int8_t", "Multiply", "Add", g.PATH_AUTO, (256, 512, 512), True, "i8_variant", v, name) for v, name in
    [(-1, "mfma_i8_256x256_pingpong_k64_KxN"), (0, "mfma_i8_256x256x128_slab128_KxN")]]


@pytest.mark.parametrize("case", FAMILIES, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}-{c[3]}-{c[4]}-{'KxN' if c[5] else 'NxK'}-{c[6]}={c[7]}")
def test_every_batched_family(case):
    dtype, mp, rd, path, (n, k, m), ta, knob, value, prefix = case
    rng = np.random.default_rng(zlib.crc32(repr(case).encode()))
    batch = 2
    t = sr.NP_DTYPES[dtype]
    if sr.is_float(dtype):
        a = rng.uniform(-2, 2, size=(k, n) if ta else (n, k)).astype(t)
        b = rng.uniform(-2, 2, size=(k, m)).astype(t)
        c0 = rng.uniform(-8, 8, size=(batch, n, m)).astype(t)
    else:
        a, b = operands(dtype, mp, rd, n, k, m, rng, ta)
        c0 = seeds(dtype, (batch, n, m), rng)
    cfg = g.make_config(dtype, mp, rd, path, ta)
    old = g.get_tuning(knob) if knob else None
    try:
        if knob:
            g.set_tuning(knob, value)
        name = g.kernel_name_batched(cfg, n, k, m, batch)
        assert name.startswith(prefix), name
        got = accumulate(cfg, a, b, c0.ravel(), n, k, m, batch, 0, 0, n * m).reshape(batch, n, m)
    finally:
        if knob:
            g.set_tuning(knob, old)
    for e in range(batch):
        if (mp, rd) == ("Multiply", "Add") and sr.is_float(dtype) and path == g.PATH_AUTO:
            ok, err = within_bound(dtype, got[e], a, b, c0[e], ta)
            assert ok, (name, err)
        else:
            want = seeded_reference(dtype, mp, rd, a, b, c0[e], ta)
            assert sr.same_bits(got[e], want), (name, sr.first_difference(got[e], want))


# ---- 4. seed = identity gives the plain batched launch --------------------------------------------------------------
@pytest.mark.parametrize("dtype,mp,rd,shape", [
    ("float", "Add", "Min", (130, 128, 136)), ("int", "Multiply", "Add", (130, 128, 136)), ("uint8_t", "Multiply", "Add", (250, 512, 512)),
    ("float", "Multiply", "Add", (300, 264, 260)), ("double", "Multiply", "Add", (250, 256, 264)),
    ("half", "Multiply", "Add", (250, 512, 512)), ("half", "Multiply", "Add", (130, 128, 132)), ("long", "Multiply", "Multiply", (33, 17, 29))],
    ids=lambda x: str(x))
def test_identity_seed_equals_plain_launch(dtype, mp, rd, shape):
    n, k, m = shape
    batch = 2
    rng = np.random.default_rng(n * k + m)
    a, b = operands(dtype, mp, rd, n, k, m, rng, non_finite=False)
    if sr.is_float(dtype) and (mp, rd) == ("Multiply", "Add"):
        a = rng.uniform(-2, 2, size=(n, k)).astype(a.dtype)
        b = rng.uniform(-2, 2, size=(k, m)).astype(a.dtype)
    cfg = g.make_config(dtype, mp, rd)
    c0 = np.full(batch * n * m, sr.identity(dtype, rd), dtype=a.dtype)
    got = accumulate(cfg, a, b, c0, n, k, m, batch, 0, 0, n * m)
    want = plain(cfg, a, b, n, k, m, batch, 0, 0, n * m)
    if sr.is_float(dtype) and (mp, rd) == ("Multiply", "Add"):
        assert sr.same_values(got, want)   # -0 + 0 == +0
    else:
        assert sr.same_bits(got, want)


# ---- 5. K split: plain over K1, then accumulate over K2 == the whole K ------------------------------------------------
@pytest.mark.parametrize("dtype,mp,rd,shape,k1", [
    ("int", "Multiply", "Add", (130, 256, 136), 128), ("float", "Add", "Min", (130, 256, 136), 64), ("uint16_t", "Min", "And", (33, 40, 29), 16),
    ("uint8_t", "Multiply", "Add", (250, 1024, 512), 512), ("float", "Multiply", "Add", (300, 528, 260), 264),
    ("double", "Multiply", "Add", (250, 512, 264), 256), ("half", "Multiply", "Add", (250, 1024, 512), 512)], ids=lambda x: str(x))
def test_k_split_composes(dtype, mp, rd, shape, k1):
    n, k, m = shape
    rng = np.random.default_rng(k1 + n)
    a, b = operands(dtype, mp, rd, n, k, m, rng, non_finite=False)
    if sr.is_float(dtype) and (mp, rd) == ("Multiply", "Add"):
        a = rng.uniform(-2, 2, size=(n, k)).astype(a.dtype)
        b = rng.uniform(-2, 2, size=(k, m)).astype(a.dtype)
    cfg = g.make_config(dtype, mp, rd)
    whole = plain(cfg, a, b, n, k, m)[:n * m]
    a1, a2 = np.ascontiguousarray(a[:, :k1]), np.ascontiguousarray(a[:, k1:])
    part = plain(cfg, a1, b[:k1], n, k1, m)[:n * m]
    got = accumulate(cfg, a2, np.ascontiguousarray(b[k1:]), part, n, k - k1, m, single=True)
    if sr.is_float(dtype) and (mp, rd) == ("Multiply", "Add"):
        ok, err = within_bound(dtype, got.reshape(n, m), a, b, np.zeros((n, m), a.dtype))
        assert ok, err
    elif sr.is_float(dtype):   # Min / Max: the same values (a tie of zeros may return either)
        assert sr.same_values(got, whole)
    else:
        assert sr.same_bits(got, whole)
    # the same with B broadcast over a batch of 3 and a padded stride_c: the gaps stay untouched
    batch, pad = 3, 64   # (a pad of 64 elements keeps every element 16-byte aligned)
    sc = n * m + pad
    a_b = np.stack([a2] * batch)
    c_pad = np.full((batch - 1) * sc + n * m, sr.NP_DTYPES[dtype](7), dtype=a.dtype)
    for e in range(batch):
        c_pad[e * sc:e * sc + n * m] = part
    got_b = accumulate(cfg, a_b.ravel(), np.ascontiguousarray(b[k1:]), c_pad, n, k - k1, m, batch, n * (k - k1), 0, sc)
    for e in range(batch):
        assert sr.same_bits(got_b[e * sc:e * sc + n * m], got)
        if e + 1 < batch:
            assert np.all(got_b[e * sc + n * m:(e + 1) * sc] == sr.NP_DTYPES[dtype](7))


# ---- 6. application: min-plus closure of a weighted digraph ------------------------------------------------------------
def test_min_plus_closure_matches_floyd_warshall():
    import torch
    n = 1024
    rng = np.random.default_rng(1024)
    d = np.full((n, n), np.inf, dtype=np.float32)
    edges = rng.random((n, n)) < 4.0 / n
    d[edges] = rng.integers(1, 100, size=int(edges.sum())).astype(np.float32)
    unreachable = rng.choice(n, size=16, replace=False)
    d[:, unreachable] = np.inf                      # no edges into these nodes
    np.fill_diagonal(d, 0.0)
    want = d.copy()
    for kk in range(n):                             # Floyd-Warshall
        np.minimum(want, want[:, kk:kk + 1] + want[kk:kk + 1, :], out=want)
    cfg = g.make_config("float", "Add", "Min")
    assert g.kernel_name_batched(cfg, n, n, n, 1) == "valu_tile"
    D = torch.from_numpy(d).to("cuda:0")
    for _ in range(12):
        prev = D.clone()                            # C must not alias A or B: square a copy
        g.addmm_(D, prev, prev, "float", "Add", "Min")
        torch.cuda.synchronize()
        if torch.equal(D, prev):
            break
    got = D.cpu().numpy()
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    assert np.isinf(got[0, unreachable[unreachable != 0][0]])


# ---- 7. Python: addmm_ / baddbmm_ against torch --------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float", "double", "half"])
def test_addmm_and_baddbmm_against_torch(dtype):
    import torch
    tdt = g.torch_dtype(dtype)
    torch.manual_seed(0)
    n, k, m, batch = 136, 256, 264, 3
    a = torch.rand(n, k, device="cuda:0", dtype=tdt) - 0.5
    b = torch.rand(k, m, device="cuda:0", dtype=tdt) - 0.5
    c = torch.rand(n, m, device="cuda:0", dtype=tdt) - 0.5
    want = torch.addmm(c.double(), a.double(), b.double())
    got = c.clone()
    assert g.addmm_(got, a, b, dtype) is got
    scale = torch.addmm(c.double().abs(), a.double().abs(), b.double().abs())
    tol = MUL_ADD_TOL[dtype]
    assert float(((got.double() - want).abs() / scale).max()) < tol
    A = torch.rand(batch, n, k, device="cuda:0", dtype=tdt) - 0.5
    Bx = b.expand(batch, k, m)                                     # batch stride 0
    C = torch.rand(batch, n, m, device="cuda:0", dtype=tdt) - 0.5
    want = torch.baddbmm(C.double(), A.double(), Bx.double())
    scale = torch.baddbmm(C.double().abs(), A.double().abs(), Bx.double().abs())
    got = C.clone()
    assert g.baddbmm_(got, A, Bx, dtype) is got
    assert float(((got.double() - want).abs() / scale).max()) < tol


def test_python_raise_cases():
    import torch
    a = torch.ones(64, 64, device="cuda:0")
    c = torch.ones(64, 64, device="cuda:0")
    with pytest.raises(g.MMError, match="overlap"):
        g.addmm_(a, a, c)                                          # C is A
    with pytest.raises(g.MMError, match="shape"):
        g.addmm_(torch.ones(64, 32, device="cuda:0"), a, c)
    with pytest.raises(g.MMError, match="dtype"):
        g.addmm_(c.double(), a, c)
    with pytest.raises(g.MMError, match="contiguous"):
        g.addmm_(c, a.t().contiguous().t(), c.clone())
    with pytest.raises(g.MMError):
        g.baddbmm_(c.expand(2, 64, 64), a, a.clone())              # C with batch stride 0


# ---- 8. determinism ------------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bits():
    rng = np.random.default_rng(8)
    for dtype, shape in (("float", (300, 528, 260)), ("half", (250, 512, 512)), ("double", (250, 256, 264))):
        n, k, m = shape
        a = rng.uniform(-1, 1, size=(n, k)).astype(sr.NP_DTYPES[dtype])
        b = rng.uniform(-1, 1, size=(k, m)).astype(sr.NP_DTYPES[dtype])
        c0 = rng.uniform(-1, 1, size=n * m).astype(sr.NP_DTYPES[dtype])
        cfg = g.make_config(dtype)
        assert sr.same_bits(accumulate(cfg, a, b, c0, n, k, m, single=True), accumulate(cfg, a, b, c0, n, k, m, single=True))
