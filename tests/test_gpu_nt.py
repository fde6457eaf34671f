"""GPU tests of the A x B^T entry points (mm_gemm_nt_*, matmul_nt / addmm_nt_): C[i][j] = reduce_k map(A[i][k], Bt[j][k]) with
Bt stored M x K.  The reference is _semiring_ref.reference() on bt.T -- Naive on the transposed operand -- and, for the
matrix-core route, the row-major batched call on a materialised transpose."""
import ctypes
import time
import zlib

import numpy as np
import pytest

import _bounds
import _semiring_ref as sr
import gemm_hls_amd as g
from test_gpu_accumulate import seeded_reference, seeds

pytestmark = pytest.mark.gpu

GUARD = 64   # elements of guard pattern on each side of C


def _dev(x, offset=0):
    """The bytes of x on the device, `offset` bytes into a 256-byte aligned allocation; (owner, address)."""
    import torch
    raw = np.ascontiguousarray(x).reshape(-1).view(np.uint8)
    buf = torch.zeros(offset + raw.size, dtype=torch.uint8, device="cuda:0")
    buf[offset:] = torch.from_numpy(raw.copy()).to("cuda:0")
    return buf, buf.data_ptr() + offset


def run_nt(cfg, a, bt, n, k, m, batch=1, sa=0, sb=0, sc=0, c0=None, b_offset=0):
    """mm_gemm_nt_launch on host arrays, C inside a guarded buffer (seeded with c0 when given); returns C flat."""
    t = np.dtype(a.dtype)
    c_flat = np.zeros((batch - 1) * sc + n * m, dtype=t) if c0 is None else np.ascontiguousarray(c0).reshape(-1)
    pattern = (np.arange(GUARD * t.itemsize) % 251 + 1).astype(np.uint8).view(t)
    (ka, pa), (kb, pb), (kc, pc) = _dev(a), _dev(bt, b_offset), _dev(np.concatenate([pattern, c_flat, pattern]))
    rc = g.lib().mm_gemm_nt_launch(0, ctypes.byref(cfg), pa, pb, pc + GUARD * t.itemsize, n, k, m, batch, sa, sb, sc,
                                   int(c0 is not None), None)
    assert rc == 0, (rc, g.lib().mm_last_error().decode())
    out = kc.cpu().numpy().view(t)
    assert out[:GUARD].tobytes() == pattern.tobytes() and out[-GUARD:].tobytes() == pattern.tobytes(), "guard overwritten"
    return out[GUARD:-GUARD]


def operands(dtype, mp, rd, n, k, m, rng, non_finite=True):
    """(a, bt): a N x K, bt M x K (the transposed storage of _semiring_ref's K x M operand)."""
    if sr.is_float(dtype):
        a, b = sr.float_operands(dtype, mp, rd, (n, k), (k, m), rng, non_finite)
    else:
        a, b = sr.int_operands(dtype, mp, rd, (n, k), (k, m), rng)
    return a, np.ascontiguousarray(b.T)


def _rng(*key):
    return np.random.default_rng(zlib.crc32("/".join(str(x) for x in ("nt",) + key).encode()))


# ---- 1. ordered_nt: all 275 configurations, Naive's bits on the transposed operand, plain and seeded -----------------------
@pytest.mark.parametrize("dtype,mp,rd", sr.CONFIGS, ids=lambda x: str(x))
def test_nt_ordered_every_config_is_naive_on_the_transposed_operand(dtype, mp, rd):
    rng = _rng(dtype, mp, rd)
    # one ragged tile; then two tiles each way with a one-line last tile and a one-k last slab
    for n, k, m in [(37, 19, 41), (65, 17, 67)]:
        a, bt = operands(dtype, mp, rd, n, k, m, rng)
        cfg = g.make_config(dtype, mp, rd, g.PATH_ORDERED)
        assert g.kernel_name_nt(cfg, n, k, m) == "ordered_nt"
        want = sr.reference(dtype, mp, rd, a, bt.T)
        sr.assert_not_degenerate(want, mp, rd, f"{dtype} ({mp}, {rd})")
        got = run_nt(cfg, a, bt, n, k, m).reshape(n, m)
        assert sr.same_bits(got, want), sr.first_difference(got, want)
        c0 = seeds(dtype, (n, m), rng)
        want = seeded_reference(dtype, mp, rd, a, bt.T, c0)
        # (a seeded chain starts at an arbitrary value, so assert_not_degenerate's {0, 1} does not apply: the reference must take
        # several values -- two where an And leaves only 0 and 1 to an unsigned Min -- and must not be the seed itself)
        values = np.unique(want[~np.isnan(want)] if sr.is_float(dtype) else want).size
        assert values >= (2 if sr.binary_result(mp, rd) else 3) and not sr.same_bits(want, c0), f"degenerate seeded reference for {dtype} ({mp}, {rd})"
        got = run_nt(cfg, a, bt, n, k, m, c0=c0).reshape(n, m)
        assert sr.same_bits(got, want), sr.first_difference(got, want)


# ---- 2. valu_tile_nt: one type per element size and two more, ragged tiles, the shifted last slab -----------------------------
VT_TYPES = {"int8_t": 1, "half": 2, "uint16_t": 2, "float": 4, "double": 8, "long": 8}
VT_PAIRS = [("Add", "Min"), ("Add", "Max"), ("Min", "Max"), ("Multiply", "Add")]


def _vt_shapes(es):
    bk, epc = 64 // es, 16 // es
    return [(1, bk, 1), (128, bk, 128), (130, 2 * bk + epc, 131), (257, 3 * bk, 129)]


@pytest.mark.parametrize("dtype,shape", [(d, s) for d, es in VT_TYPES.items() for s in _vt_shapes(es)],
                         ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_nt_valu_tile_bits_and_values(dtype, shape):
    n, k, m = shape
    for mp, rd in VT_PAIRS:
        if (mp, rd) == ("Multiply", "Add") and sr.is_float(dtype):
            continue    # a tolerance family (half: another kernel): test_nt_valu_tile_float_multiply_add_within_the_bound
        cfg = g.make_config(dtype, mp, rd)
        # (int8_t (Multiply, Add) is the matrix cores' wherever K and M allow: of these shapes, at 128 x 64 x 128 -- exact mod 2^8 too)
        on_mfma = (dtype, mp, rd, shape) == ("int8_t", "Multiply", "Add", (128, 64, 128))
        assert g.kernel_name_nt(cfg, n, k, m) == ("nt_prepass" if on_mfma else "valu_tile_nt"), (mp, rd)
        rng = _rng("vt", dtype, mp, rd, shape)
        minmax_float = sr.is_float(dtype)
        a, bt = operands(dtype, mp, rd, n, k, m, rng, non_finite=n > sr.INF_ROW)    # (the all-inf row needs a row 3)
        want = sr.reference(dtype, mp, rd, a, bt.T, auto_minmax=minmax_float)
        if n * m >= 3:
            sr.assert_not_degenerate(want, mp, rd, f"{dtype} ({mp}, {rd}) {shape}")
        got = run_nt(cfg, a, bt, n, k, m).reshape(n, m)
        same = sr.same_values if minmax_float else sr.same_bits
        assert same(got, want), (mp, rd, sr.first_difference(got, want, by_value=minmax_float))
        # seeded: the chains start from C (no NaN seed for minNum / maxNum, as in the row-major calls' tests)
        c0 = seeds(dtype, (n, m), rng, nan=not minmax_float)
        want = seeded_reference(dtype, mp, rd, a, bt.T, c0, auto_minmax=minmax_float)
        got = run_nt(cfg, a, bt, n, k, m, c0=c0).reshape(n, m)
        assert same(got, want), ("seeded", mp, rd, sr.first_difference(got, want, by_value=minmax_float))


@pytest.mark.parametrize("dtype", ["float", "double"])
def test_nt_valu_tile_float_multiply_add_within_the_bound(dtype):
    """(Multiply, Add) may fuse: bounded like valu_tile's -- the normwise 1e-5 bar and the chain guard of tests/_bounds.py that
    tests/test_gpu_parity.py applies to fp32 for this K, 1e-12 (test_gpu_parity.py's double tolerance) for double."""
    es = VT_TYPES[dtype]
    n, k, m = _vt_shapes(es)[2]
    cfg = g.make_config(dtype)
    assert g.kernel_name_nt(cfg, n, k, m) == "valu_tile_nt"
    rng = _rng("vt-muladd", dtype)
    a, b = sr.float_operands(dtype, "Multiply", "Add", (n, k), (k, m), rng, non_finite=False, largest=False)
    bt = np.ascontiguousarray(b.T)
    exact, scale = sr.exact_and_scale(dtype, a, b)
    if exact is None or sr.wide_type(dtype) is None:
        pytest.fail("no type wide enough for the exact product on this platform")
    sr.assert_not_degenerate(exact, "Multiply", "Add", dtype)
    got = run_nt(cfg, a, bt, n, k, m).reshape(n, m)
    assert np.all(np.isfinite(got))
    tiny = np.finfo(sr.NP_DTYPES[dtype]).smallest_subnormal.astype(exact.dtype)
    err = _bounds.normwise(got.astype(exact.dtype), exact, scale + k * tiny)
    print(f"valu_tile_nt {dtype} (Multiply, Add) {n}x{k}x{m}: normwise error {err:.3e}")
    if dtype == "float":
        _bounds.north_star(err, "valu_tile_nt float")
        _bounds.guard(err, _bounds.f32_chain_guard(k), "valu_tile_nt float")
    else:
        assert err < 1e-12, err


# ---- 3. nt_prepass: the matrix-core kernels on the library's own transposed copy ------------------------------------------------
PREPASS = [("float", (130, 72, 136)), ("double", (130, 72, 136)), ("half", (130, 80, 136)), ("uint8_t", (130, 96, 144))]


def _muladd_operands(dtype, shape, rng):
    import torch
    t = sr.NP_DTYPES[dtype]
    if sr.is_float(dtype):
        return torch.from_numpy(rng.uniform(-2, 2, size=shape).astype(t)).cuda()
    return torch.from_numpy(rng.integers(0, 255, size=shape, endpoint=True).astype(t)).cuda()


@pytest.mark.parametrize("dtype,shape", PREPASS, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_nt_prepass_equals_the_batched_call_on_a_materialised_transpose(dtype, shape):
    n, k, m = shape
    cfg = g.make_config(dtype)
    rng = _rng("prepass", dtype)
    for batch in (1, 3):
        assert g.kernel_name_batched(cfg, n, k, m, batch).startswith("mfma_")
        assert g.kernel_name_nt(cfg, n, k, m, batch) == "nt_prepass"
    a1, bt1 = _muladd_operands(dtype, (n, k), rng), _muladd_operands(dtype, (m, k), rng)
    a3, bt3 = _muladd_operands(dtype, (3, n, k), rng), _muladd_operands(dtype, (3, m, k), rng)
    for a, bt in ((a1, bt1), (a3, bt3)):
        b = bt.mT.contiguous()
        want = g.bmm(a, b, dtype).cpu().numpy()
        assert np.unique(want).size >= 3
        got = g.matmul_nt(a, bt, dtype).cpu().numpy()
        assert got.shape == (want.shape[1:] if a.dim() == 2 else want.shape)
        assert sr.same_bits(got.reshape(want.shape), want), sr.first_difference(got.reshape(want.shape), want)
        c0 = _muladd_operands(dtype, tuple(got.shape), rng)
        want = g.baddbmm_(c0.clone(), a, b, dtype).cpu().numpy()
        got = g.addmm_nt_(c0.clone(), a, bt, dtype).cpu().numpy()
        assert not np.array_equal(got, c0.cpu().numpy())
        assert sr.same_bits(got, want), ("seeded", sr.first_difference(got, want))


# ---- 4. batches: broadcast operands, a padded stride, chunked launches -------------------------------------------------------
BATCH_CASES = [   # (kernel, dtype, map, reduce, path, shape)
    ("ordered_nt", "float", "Add", "Min", g.PATH_ORDERED, (37, 19, 41)),
    ("valu_tile_nt", "float", "Add", "Min", g.PATH_AUTO, (130, 36, 131)),
    ("nt_prepass", "uint8_t", "Multiply", "Add", g.PATH_AUTO, (130, 96, 144)),
    ("nt_prepass", "float", "Multiply", "Add", g.PATH_AUTO, (130, 72, 136)),
]


@pytest.mark.parametrize("kernel,dtype,mp,rd,path,shape", BATCH_CASES, ids=lambda v: str(v) if not isinstance(v, tuple) else "x".join(map(str, v)))
def test_nt_batches_broadcast_padded_and_chunked(kernel, dtype, mp, rd, path, shape):
    n, k, m = shape
    batch, pad = 5, 16
    cfg = g.make_config(dtype, mp, rd, path)
    assert g.kernel_name_nt(cfg, n, k, m, batch) == kernel
    rng = _rng("batch", kernel, dtype)
    t = sr.NP_DTYPES[dtype]
    if sr.is_float(dtype):
        a = rng.uniform(-2, 2, size=(batch, n, k)).astype(t)
        bt = rng.uniform(-2, 2, size=(batch, m * k + pad)).astype(t)      # a padded stride_b
    else:
        a = rng.integers(0, 255, size=(batch, n, k), endpoint=True).astype(t)
        bt = rng.integers(0, 255, size=(batch, m * k + pad), endpoint=True).astype(t)
    sb = m * k + pad
    exact = not (sr.is_float(dtype) and (mp, rd) == ("Multiply", "Add"))
    g.set_tuning("batch_chunk", 2)
    try:
        full = run_nt(cfg, a, bt, n, k, m, batch, n * k, sb, n * m).reshape(batch, n, m)
        b_shared = run_nt(cfg, a, bt[0], n, k, m, batch, n * k, 0, n * m).reshape(batch, n, m)
        a_shared = run_nt(cfg, a[0], bt, n, k, m, batch, 0, sb, n * m).reshape(batch, n, m)
    finally:
        g.set_tuning("batch_chunk", -1)
    assert np.unique(full).size >= 3
    for e in range(batch):
        be = bt[e, :m * k]
        if exact:   # each element's bits are its own single call's, and Naive's
            assert sr.same_bits(full[e], run_nt(cfg, a[e], be, n, k, m).reshape(n, m)), e
            assert sr.same_bits(b_shared[e], run_nt(cfg, a[e], bt[0, :m * k], n, k, m).reshape(n, m)), e
            assert sr.same_bits(a_shared[e], run_nt(cfg, a[0], be, n, k, m).reshape(n, m)), e
            assert sr.same_bits(full[e], sr.reference(dtype, mp, rd, a[e], be.reshape(m, k).T)), e
    if not exact:   # fp32 on the matrix cores: the kernel is resolved on the whole batch, so the yardstick is the row-major
        import torch    # batched call of the same batch on materialised transposes, chunked differently
        ta = torch.from_numpy(a).cuda()
        tb = torch.from_numpy(np.ascontiguousarray(bt[:, :m * k].reshape(batch, m, k).transpose(0, 2, 1))).cuda()
        assert sr.same_bits(full, g.bmm(ta, tb, dtype).cpu().numpy())
        assert sr.same_bits(b_shared, g.bmm(ta, tb[0], dtype).cpu().numpy())
        assert sr.same_bits(a_shared, g.bmm(ta[0], tb, dtype).cpu().numpy())


# (the pre-pass's OWN loop over the batch -- a second transposition into the reused workspace, batch_slice at e0 > 0, the
# stride_b of the second chunk's product -- is bounded by the workspace alone: batch_chunk does not reach it)
@pytest.mark.parametrize("dtype,k", [("uint8_t", 1024), ("float", 512)])
def test_nt_prepass_second_workspace_chunk(dtype, k):
    """K = M = 1024 of uint8_t, or 512 of float: a transposed copy is K * M * es = 2^20 bytes, the 256 MiB of workspace hold
    2^28 / 2^20 = 256 of them, and a batch of 261 runs as 256 + 5.  The batch is base[e % 7] -- no chunk boundary falls on
    a period -- gathered on the device, Bt with a padded batch stride (M * K + 16; the pads hold 255 / NaN).  uint8_t, plain
    and seeded: every element is numpy's sums mod 2^8 of its base.  float: the whole batch is, bit for bit, bmm / baddbmm_ on
    the materialised transposes of the same 261 elements, and the first 7 are within the north_star bar and the chain guard
    of the float64 products."""
    import torch
    n, m, batch, period, pad = 64, k, 261, 7, 16
    t = sr.NP_DTYPES[dtype]
    assert ((256 << 20) // (k * m * t().itemsize)) == 256 < batch
    assert g.kernel_name_nt(g.make_config(dtype), n, k, m, batch) == "nt_prepass"
    rng = _rng("second-chunk", dtype)
    if dtype == "float":
        a, bt, c0 = (rng.uniform(-2, 2, size=shape).astype(t) for shape in ((period, n, k), (period, m * k), (period, n, m)))
    else:
        a, bt, c0 = (rng.integers(0, 255, size=shape, endpoint=True).astype(t) for shape in ((period, n, k), (period, m * k), (period, n, m)))
    index = torch.arange(batch, device="cuda:0") % period
    ta, tc0 = torch.from_numpy(a).cuda()[index], torch.from_numpy(c0).cuda()[index]
    buf = torch.full((batch, m * k + pad), float("nan") if dtype == "float" else 255, dtype=ta.dtype, device="cuda:0")
    buf[:, :m * k] = torch.from_numpy(bt).cuda()[index]
    tbt = torch.as_strided(buf, (batch, m, k), (m * k + pad, k, 1))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = g.matmul_nt(ta, tbt, dtype)
    got_seeded = g.addmm_nt_(tc0.clone(), ta, tbt, dtype)
    torch.cuda.synchronize()
    print(f"nt_prepass {dtype}, {batch} x {n}x{k}x{m} in two workspace chunks, plain + seeded: {time.perf_counter() - t0:.3f} s")
    if dtype == "uint8_t":   # exact, and independent of any kernel
        prod = np.stack([a[e].astype(np.int64) @ bt[e].reshape(m, k).T.astype(np.int64) for e in range(period)])
        want, want_seeded = (prod % 256).astype(t), ((prod + c0) % 256).astype(t)
        assert np.unique(want).size >= 3 and not np.array_equal(want, want_seeded)
        assert torch.equal(got, torch.from_numpy(want).cuda()[index])
        assert torch.equal(got_seeded, torch.from_numpy(want_seeded).cuda()[index])
        return
    tb = tbt.mT.contiguous()
    want, want_seeded = g.bmm(ta, tb, dtype), g.baddbmm_(tc0.clone(), ta, tb, dtype)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert torch.equal(got_seeded.view(torch.int32), want_seeded.view(torch.int32)) and not torch.equal(got_seeded, got)
    first = got[:period].cpu().numpy()
    tiny = np.finfo(t).smallest_subnormal
    for e in range(period):
        exact, scale = sr.exact_and_scale(dtype, a[e], bt[e].reshape(m, k).T)
        sr.assert_not_degenerate(exact, "Multiply", "Add", f"base {e}")
        err = _bounds.normwise(first[e].astype(exact.dtype), exact, scale + k * tiny.astype(exact.dtype))
        _bounds.north_star(err, f"nt_prepass float, base {e}")
        _bounds.guard(err, _bounds.f32_chain_guard(k), f"nt_prepass float, base {e}")


# ---- 5. composition and symmetry ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,mp,rd", [("float", "Add", "Min"), ("int", "Multiply", "Add")], ids=lambda x: str(x))
def test_nt_two_halves_of_k_compose(dtype, mp, rd):
    import torch
    n, k, m = 130, 72, 131
    a, bt = operands(dtype, mp, rd, n, k, m, _rng("halves", dtype), non_finite=False)
    assert g.kernel_name_nt(g.make_config(dtype, mp, rd), n, k // 2, m) == "valu_tile_nt"
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(bt).cuda()
    whole = g.matmul_nt(ta, tb, dtype, mp, rd)
    halves = g.matmul_nt(ta[:, :k // 2].contiguous(), tb[:, :k // 2].contiguous(), dtype, mp, rd)
    assert not torch.equal(halves, whole)
    g.addmm_nt_(halves, ta[:, k // 2:].contiguous(), tb[:, k // 2:].contiguous(), dtype, mp, rd)
    want = sr.reference(dtype, mp, rd, a, bt.T)
    sr.assert_not_degenerate(want, mp, rd, dtype)
    assert sr.same_bits(whole.cpu().numpy(), want) and sr.same_bits(halves.cpu().numpy(), want)


def test_nt_a_with_itself_is_symmetric():
    import torch
    n, k = 130, 36
    a, _ = operands("float", "Add", "Min", n, k, n, _rng("self"), non_finite=False)
    ta = torch.from_numpy(a).cuda()
    for path, kernel in ((g.PATH_AUTO, "valu_tile_nt"), (g.PATH_ORDERED, "ordered_nt")):
        assert g.kernel_name_nt(g.make_config("float", "Add", "Min", path), n, k, n) == kernel
        c = g.matmul_nt(ta, ta, "float", "Add", "Min", path).cpu().numpy()     # one buffer for both operands
        sr.assert_not_degenerate(c, "Add", "Min", "A (x) A^T")
        assert sr.same_bits(c, np.ascontiguousarray(c.T))
        assert sr.same_bits(c, sr.reference("float", "Add", "Min", a, a.T))


# ---- 6. demotion: a Bt that is only element-aligned -------------------------------------------------------------------------
def test_nt_misaligned_bt_runs_ordered_nt_float_minplus():
    n, k, m = 130, 36, 131
    a, bt = operands("float", "Add", "Min", n, k, m, _rng("demote"))
    cfg = g.make_config("float", "Add", "Min")
    assert g.kernel_name_nt(cfg, n, k, m) == "valu_tile_nt"      # the name is the shape's; the launch is demoted
    got = run_nt(cfg, a, bt, n, k, m, b_offset=4).reshape(n, m)
    want = sr.reference("float", "Add", "Min", a, bt.T)          # std::min to the letter, NaN and zero ties included
    sr.assert_not_degenerate(want, "Add", "Min", "demoted")
    assert sr.same_bits(got, want), sr.first_difference(got, want)
    ordered = run_nt(g.make_config("float", "Add", "Min", g.PATH_ORDERED), a, bt, n, k, m).reshape(n, m)
    assert sr.same_bits(got, ordered)


def test_nt_misaligned_bt_keeps_halfs_f32_contract():
    n, k, m = 130, 80, 136
    rng = _rng("demote-half")
    a = rng.uniform(-2, 2, size=(n, k)).astype(np.float16)
    bt = rng.uniform(-2, 2, size=(m, k)).astype(np.float16)
    cfg = g.make_config("half")
    assert g.kernel_name_nt(cfg, n, k, m) == "nt_prepass"
    got = run_nt(cfg, a, bt, n, k, m, b_offset=2).reshape(n, m)
    acc = np.zeros((n, m), dtype=np.float32)    # exact products, f32 sums k ascending, ONE rounding
    a32, b32 = a.astype(np.float32), bt.T.astype(np.float32)
    for kk in range(k):
        acc = acc + a32[:, kk:kk + 1] * b32[kk:kk + 1, :]
    want = acc.astype(np.float16)
    sr.assert_not_degenerate(want, "Multiply", "Add", "half demoted")
    assert sr.same_bits(got, want), sr.first_difference(got, want)
    naive = sr.reference("half", "Multiply", "Add", a, bt.T)     # binary16 sums are another result
    assert not sr.same_bits(got, naive)


# ---- 7. torch-side errors --------------------------------------------------------------------------------------------------------
def test_nt_binding_errors_on_device_tensors():
    import torch
    a = torch.zeros((8, 16), device="cuda")
    bt = torch.zeros((12, 16), device="cuda")
    with pytest.raises(g.MMError, match=r"inner dimensions differ.*\(M, K\)"):
        g.matmul_nt(a, torch.zeros((16, 12), device="cuda"))
    with pytest.raises(g.MMError, match="do not match"):
        g.matmul_nt(a, bt.half())
    with pytest.raises(g.MMError, match="device tensors"):
        g.matmul_nt(a, bt.cpu())
    with pytest.raises(g.MMError, match=r"b \(M, K\) must be a dense row-major matrix"):
        g.matmul_nt(a, torch.zeros((16, 12), device="cuda").t())
    with pytest.raises(g.MMError, match="must be dense row-major"):
        g.matmul_nt(torch.zeros((2, 8, 32), device="cuda")[:, :, ::2], bt)
    with pytest.raises(g.MMError, match="c has shape"):
        g.addmm_nt_(torch.zeros((12, 8), device="cuda"), a, bt)
    with pytest.raises(g.MMError, match="c overlaps a or b"):
        g.addmm_nt_(a.view(-1)[:96].view(8, 12), a, bt)
    out = g.matmul_nt(a.expand(3, 8, 16), bt)                       # a broadcast A: (B, N, M)
    assert tuple(out.shape) == (3, 8, 12)
