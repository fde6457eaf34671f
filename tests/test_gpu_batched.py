"""GPU tests of the strided-batched entry points (mm_gemm_batched_launch / _enqueue, gemm_hls_amd.bmm): per element the
single launch's contract -- Naive's bits under MM_PATH_ORDERED, the single launch's bits for the exact configurations
under MM_PATH_AUTO, its error bound for floating (Multiply, Add) -- for every stride form, independent of the element's
position, its neighbours and how the batch is chunked into launches."""
import ctypes
import os
import warnings
import zlib

import numpy as np
import pytest

import _oracle
import _semiring_ref as sr
import gemm_hls_amd as g
from _bounds import NORTH_STAR_F32, normwise

pytestmark = pytest.mark.gpu

ALL_TYPES = list(g.DTYPES)
ALL_OPS = list(g.OPS)


def _dev_buffer(np_flat):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(np_flat).view(np.uint8).copy()).to("cuda:0")
    return t


def batched_launch(cfg, a_flat, b_flat, n, k, m, batch, sa, sb, sc, c_init=None, expect=0):
    """Runs mm_gemm_batched_launch on host arrays laid out flat with the given element strides; returns C flat."""
    c_len = (batch - 1) * sc + n * m if batch else 0
    c_host = np.zeros(max(c_len, 1), dtype=a_flat.dtype) if c_init is None else c_init.copy()
    da, db, dc = _dev_buffer(a_flat), _dev_buffer(b_flat), _dev_buffer(c_host)
    rc = g.lib().mm_gemm_batched_launch(0, ctypes.byref(cfg), da.data_ptr(), db.data_ptr(), dc.data_ptr(), n, k, m, batch,
                                        sa, sb, sc, None)
    assert rc == expect, (rc, g.lib().mm_last_error().decode())
    return dc.cpu().numpy().view(a_flat.dtype)[:c_host.size]


def random_operands(dtype, shape, rng):
    t = _oracle.NP_DTYPES[dtype]
    if np.issubdtype(t, np.integer):
        info = np.iinfo(t)
        return rng.integers(info.min, info.max, size=shape, endpoint=True, dtype=t)
    return rng.uniform(-2.0, 2.0, size=shape).astype(t)


def stack(dtype, batch, rows, cols, rng):
    return random_operands(dtype, (batch, rows, cols), rng)


def element(flat, e, stride, rows, cols):
    return flat[e * stride:e * stride + rows * cols].reshape(rows, cols)


# ---- MM_PATH_ORDERED: all 275 configurations, every element Naive's bits ---------------------------------------------
@pytest.mark.parametrize("dtype", ALL_TYPES)
@pytest.mark.parametrize("mp", ALL_OPS)
@pytest.mark.parametrize("rd", ALL_OPS)
def test_batched_ordered_every_config_matches_naive(dtype, mp, rd):
    rng = np.random.default_rng(zlib.crc32(f"{dtype}/{mp}/{rd}".encode()))
    # a row-major A on one ragged tile; a K x N A on two tiles each way with a one-line last tile and a one-k last slab
    for n, k, m, batch, ta in [(33, 17, 29, 3, False), (65, 17, 67, 2, True)]:
        a, b = stack(dtype, batch, k if ta else n, n if ta else k, rng), stack(dtype, batch, k, m, rng)
        cfg = g.make_config(dtype, mp, rd, g.PATH_ORDERED, ta)
        assert g.kernel_name_batched(cfg, n, k, m, batch) == "ordered"
        c = batched_launch(cfg, a.ravel(), b.ravel(), n, k, m, batch, n * k, k * m, n * m)
        for e in range(batch):
            want = _oracle.naive(dtype, mp, rd, a[e], b[e], transposed_a=ta)
            got = element(c, e, n * m, n, m)
            assert sr.same_bits(got, want), (e, ta, sr.first_difference(got, want))


# ---- MM_PATH_AUTO, exact configurations: every element the single launch's bits ---------------------------------------
EXACT = [("float", "Add", "Min"), ("float", "Min", "Max"), ("int", "Multiply", "Add"), ("unsigned", "Add", "Max"),
         ("uint8_t", "Multiply", "Add"), ("int8_t", "Multiply", "Add"), ("double", "Add", "Max"), ("half", "Max", "Min"),
         ("long", "Multiply", "Min"), ("int16_t", "Add", "Min"), ("int", "Multiply", "And"), ("uint16_t", "Multiply", "Multiply")]


@pytest.mark.parametrize("dtype,mp,rd", EXACT, ids=lambda x: str(x))
@pytest.mark.parametrize("shape,ta", [((130, 128, 136), False),    # valu_tile, DMA-staged
                                      ((132, 64, 136), True),      # valu_tile, synchronous (K x N A)
                                      ((33, 17, 29), False),       # ordered
                                      ((256, 256, 256), False),    # mfma_i8 for the 8-bit products when single
                                      ((256, 192, 128), True)],    # ... and its K x N pre-pass
                         ids=["dma", "sync_kxn", "ordered", "i8", "i8_kxn"])
def test_batched_auto_exact_configs_equal_the_single_launch(dtype, mp, rd, shape, ta):
    n, k, m = shape
    batch = 3
    rng = np.random.default_rng(n + k + m)
    ar, ac = (k, n) if ta else (n, k)
    a, b = stack(dtype, batch, ar, ac, rng), stack(dtype, batch, k, m, rng)
    cfg = g.make_config(dtype, mp, rd, transposed_a=ta)
    c = batched_launch(cfg, a.ravel(), b.ravel(), n, k, m, batch, n * k, k * m, n * m)
    for e in range(batch):
        single, _ = g.matmul_capi(a[e], b[e], dtype, mp, rd, transposed_a=ta)
        got = element(c, e, n * m, n, m)
        assert sr.same_bits(got, single), (e, g.kernel_name(cfg, n, k, m), g.kernel_name_batched(cfg, n, k, m, batch))


def test_batched_synchronous_row_major_tile_kernel_ragged_below_a_slab():
    """valu_variant 0 with a row-major A: the Batched form of the synchronous register-tile kernel, which the cases above (DMA-staged,
    or synchronous with a K x N A) do not launch.  130 x 132 is two tiles each way with a last tile of 2 rows and 4 columns, K = 4
    is less than a slab, and the element strides are padded by 16 elements (the tile kernels want 16-byte aligned elements).
    Integer (Add, Min): every element Naive's bits, C's pads untouched."""
    n, k, m, batch, pad = 130, 4, 132, 3, 16
    sa, sb, sc = n * k + pad, k * m + pad, n * m + pad
    rng = np.random.default_rng(n + k + m)
    a, b = random_operands("int", (batch, sa), rng), random_operands("int", (batch, sb), rng)
    c_init = np.full((batch - 1) * sc + n * m, -7, dtype=np.int32)
    cfg = g.make_config("int", "Add", "Min")
    g.set_tuning("valu_variant", 0)
    try:
        assert g.kernel_name_batched(cfg, n, k, m, batch) == "valu_tile"
        c = batched_launch(cfg, a.ravel(), b.ravel(), n, k, m, batch, sa, sb, sc, c_init=c_init)
    finally:
        g.set_tuning("valu_variant", -1)
    for e in range(batch):
        want = _oracle.naive("int", "Add", "Min", a[e, :n * k].reshape(n, k), b[e, :k * m].reshape(k, m))
        assert sr.same_bits(element(c, e, sc, n, m), want), (e, sr.first_difference(element(c, e, sc, n, m), want))
        assert np.all(c[e * sc + n * m:(e + 1) * sc] == -7), e


# ---- floating (Multiply, Add) --------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [-1, 33, 8, 35])
@pytest.mark.parametrize("ta", [False, True], ids=["rowmajorA", "KxN_A"])
def test_batched_f32_each_geometry_within_the_bound(variant, ta):
    n, k, m, batch = 300, 264, 260, 3
    rng = np.random.default_rng(variant + 7)
    a = rng.uniform(-1, 1, size=(batch, k, n) if ta else (batch, n, k)).astype(np.float32)
    b = rng.uniform(-1, 1, size=(batch, k, m)).astype(np.float32)
    g.set_tuning("f32_variant", variant)
    try:
        cfg = g.make_config("float", transposed_a=ta)
        name = g.kernel_name_batched(cfg, n, k, m, batch)
        assert name.startswith("mfma_f32_") and "split" not in name and "stream" not in name, name
        c = batched_launch(cfg, a.ravel(), b.ravel(), n, k, m, batch, n * k, k * m, n * m)
    finally:
        g.set_tuning("f32_variant", -1)
    for e in range(batch):
        ae = a[e].T if ta else a[e]
        exact = ae.astype(np.float64) @ b[e].astype(np.float64)
        scale = np.abs(ae.astype(np.float64)) @ np.abs(b[e].astype(np.float64))
        assert normwise(element(c, e, n * m, n, m), exact, scale) < NORTH_STAR_F32


def test_batched_f32_large_elements_sampled_rows():
    n = k = m = 2048
    batch = 2
    rng = np.random.default_rng(11)
    a = rng.uniform(1, 10, size=(batch, n, k)).astype(np.float32)
    b = rng.uniform(1, 10, size=(batch, k, m)).astype(np.float32)
    c = batched_launch(g.make_config("float"), a.ravel(), b.ravel(), n, k, m, batch, n * k, k * m, n * m)
    rows = rng.choice(n, size=16, replace=False)
    for e in range(batch):
        exact = a[e][rows].astype(np.float64) @ b[e].astype(np.float64)
        rel = np.max(np.abs(element(c, e, n * m, n, m)[rows] - exact) / exact)
        assert rel < NORTH_STAR_F32, (e, rel)


def test_batched_f64_within_the_bound():
    n, k, m, batch = 130, 256, 136, 3
    rng = np.random.default_rng(5)
    a, b = rng.uniform(-1, 1, size=(batch, n, k)), rng.uniform(-1, 1, size=(batch, k, m))
    c = batched_launch(g.make_config("double"), a.ravel(), b.ravel(), n, k, m, batch, n * k, k * m, n * m)
    for e in range(batch):
        exact = a[e] @ b[e]
        scale = np.abs(a[e]) @ np.abs(b[e])
        assert normwise(element(c, e, n * m, n, m), exact, scale) < 1e-13


@pytest.mark.parametrize("ta", [False, True], ids=["rowmajorA", "KxN_A"])
def test_batched_half_wide_contract_and_reference_contract(ta):
    n, k, m, batch = 132, 256, 136, 3   # (a K x N A takes the register tiles with N % 4 == 0)
    rng = np.random.default_rng(3)
    a = rng.uniform(0.5, 2.0, size=(batch, k, n) if ta else (batch, n, k)).astype(np.float16)
    b = rng.uniform(0.5, 2.0, size=(batch, k, m)).astype(np.float16)
    cfg = g.make_config("half", transposed_a=ta)
    c = batched_launch(cfg, a.ravel(), b.ravel(), n, k, m, batch, n * k, k * m, n * m)
    for e in range(batch):
        wide = _oracle.naive("half", "Multiply", "Add", a[e], b[e], transposed_a=ta, wide_half=True)
        got = element(c, e, n * m, n, m)
        assert np.abs(got.view(np.int16).astype(np.int32) - wide.view(np.int16).astype(np.int32)).max() <= 1
    g.set_tuning("half_contract", 1)
    try:
        assert g.kernel_name_batched(cfg, n, k, m, batch) == "ordered_tile"
        c = batched_launch(cfg, a.ravel(), b.ravel(), n, k, m, batch, n * k, k * m, n * m)
    finally:
        g.set_tuning("half_contract", -1)
    for e in range(batch):
        want = _oracle.naive("half", "Multiply", "Add", a[e], b[e], transposed_a=ta)
        assert sr.same_bits(element(c, e, n * m, n, m), want), e


# pp32: the Batched form of the 32x32x16 kernel (f16_variant 100).  300 x 320 x 264 is two tiles each way, both ragged, and ten
# 32-deep slabs: two trips of the 4-slab loop and its even-pair tail.
@pytest.mark.parametrize("shape,ta,batch,family,pin", [((256, 256, 256), False, 6, "mfma_f16_256x256_pingpong_16x16x32", None),
                                                      ((130, 160, 264), False, 3, "mfma_f16_256x256_pingpong_k32", None),
                                                      ((128, 48, 256), False, 3, "mfma_f16_64x256x64_slab64", None),
                                                      ((264, 160, 256), True, 3, "mfma_f16_256x256_pingpong_k32_KxN", None),
                                                      ((264, 48, 256), True, 3, "mfma_f16_256x256x64_slab64_KxN", None),
                                                      ((300, 320, 264), False, 2, "mfma_f16_256x256_pingpong_32x32x16", ("f16_variant", 100))],
                         ids=["pp16", "ppk32", "slab64_64", "ppk32_kxn", "slab64_kxn", "pp32"])
def test_batched_half_matrix_core_kernels_keep_the_wide_contract(shape, ta, batch, family, pin):
    n, k, m = shape
    rng = np.random.default_rng(n + 3 * k + m)
    a = rng.uniform(0.5, 2.0, size=(batch, k, n) if ta else (batch, n, k)).astype(np.float16)
    b = rng.uniform(0.5, 2.0, size=(batch, k, m)).astype(np.float16)
    cfg = g.make_config("half", transposed_a=ta)
    old = g.get_tuning(pin[0]) if pin else None
    try:
        if pin:
            g.set_tuning(*pin)
        assert g.kernel_name_batched(cfg, n, k, m, batch) == family
        c = batched_launch(cfg, a.ravel(), b.ravel(), n, k, m, batch, n * k, k * m, n * m)
    finally:
        if pin:
            g.set_tuning(pin[0], old)
    for e in range(batch):
        wide = _oracle.naive("half", "Multiply", "Add", a[e], b[e], transposed_a=ta, wide_half=True)
        got = element(c, e, n * m, n, m)
        assert np.abs(got.view(np.int16).astype(np.int32) - wide.view(np.int16).astype(np.int32)).max() <= 1, e


# ---- strides ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,mp,rd", [("float", "Multiply", "Add"), ("float", "Add", "Max"), ("int", "Multiply", "Add"),
                                         ("half", "Multiply", "Add")], ids=lambda x: str(x))
@pytest.mark.parametrize("which", ["A", "B"])
def test_batched_broadcast_operand_equals_per_element_launches(dtype, mp, rd, which):
    n, k, m, batch = 64, 128, 128, 5
    rng = np.random.default_rng(17)
    a = stack(dtype, 1 if which == "A" else batch, n, k, rng)
    b = stack(dtype, 1 if which == "B" else batch, k, m, rng)
    cfg = g.make_config(dtype, mp, rd)
    sa, sb = (0, k * m) if which == "A" else (n * k, 0)
    c = batched_launch(cfg, a.ravel(), b.ravel(), n, k, m, batch, sa, sb, n * m)
    full = batched_launch(cfg, np.broadcast_to(a, (batch, n, k)).ravel(), np.broadcast_to(b, (batch, k, m)).ravel(), n, k, m,
                          batch, n * k, k * m, n * m)
    assert sr.same_bits(c, full)   # an element's bits do not depend on the strides
    if dtype != "half" and not (dtype == "float" and rd == "Add"):
        for e in range(batch):
            single, _ = g.matmul_capi(a[0 if which == "A" else e], b[0 if which == "B" else e], dtype, mp, rd)
            assert sr.same_bits(element(c, e, n * m, n, m), single), e


# (dtype, map, reduce, path, (n, k, m), batch, (knob, value) or None, the kernel the batch must run on or None).  The last case:
# the Batched form of the int8 32x32x32 kernel (i8_variant 100) on two ragged tiles each way and ten 64-deep slabs -- two trips
# of its 4-slab loop and the even-pair tail.
PADDED = [("float", "Multiply", "Add", g.PATH_AUTO, (40, 64, 48), 4, None, None),
          ("float", "Add", "Min", g.PATH_AUTO, (40, 64, 48), 4, None, None),
          ("uint8_t", "Max", "Min", g.PATH_AUTO, (40, 64, 48), 4, None, None),
          ("double", "Multiply", "Max", g.PATH_ORDERED, (40, 64, 48), 4, None, None),
          ("int8_t", "Multiply", "Add", g.PATH_AUTO, (300, 640, 272), 2, ("i8_variant", 100), "mfma_i8_256x256_pingpong_32x32x32")]


@pytest.mark.parametrize("dtype,mp,rd,path,shape,batch,pin,family", PADDED,
                         ids=["-".join(str(x) for x in c[:4]) + ("-" + c[7] if c[7] else "") for c in PADDED])
def test_batched_padded_strides_leave_the_gaps_untouched(dtype, mp, rd, path, shape, batch, pin, family, request):
    n, k, m = shape
    if pin:
        old = g.get_tuning(pin[0])
        request.addfinalizer(lambda: g.set_tuning(pin[0], old))
        g.set_tuning(*pin)
    es = np.dtype(_oracle.NP_DTYPES[dtype]).itemsize
    pad = 64 // es   # keeps every element 16-byte aligned
    sa, sb, sc = n * k + pad, k * m + 2 * pad, n * m + 3 * pad
    rng = np.random.default_rng(23)
    a = random_operands(dtype, ((batch - 1) * sa + n * k,), rng)
    b = random_operands(dtype, ((batch - 1) * sb + k * m,), rng)
    sentinel = np.full((batch - 1) * sc + n * m, 77, dtype=a.dtype)
    cfg = g.make_config(dtype, mp, rd, path)
    if family:
        assert g.kernel_name_batched(cfg, n, k, m, batch) == family
    c = batched_launch(cfg, a, b, n, k, m, batch, sa, sb, sc, c_init=sentinel)
    for e in range(batch):
        ae, be, ce = element(a, e, sa, n, k), element(b, e, sb, k, m), element(c, e, sc, n, m)
        if family:   # the 8-bit product: the low 8 bits of the exact sums
            assert np.array_equal(ce, (ae.astype(np.int32) @ be.astype(np.int32)).astype(np.int8)), e
        if (dtype, mp, rd, path) == ("float", "Multiply", "Add", g.PATH_AUTO):   # the bound, not the single launch's order
            exact = ae.astype(np.float64) @ be.astype(np.float64)
            assert normwise(ce, exact, np.abs(ae.astype(np.float64)) @ np.abs(be.astype(np.float64))) < NORTH_STAR_F32, e
        else:
            single, _ = g.matmul_capi(ae, be, dtype, mp, rd, path)
            assert sr.same_bits(ce, single), e
        if e < batch - 1:
            assert np.all(c[e * sc + n * m:(e + 1) * sc] == 77), e


def test_batched_element_misaligned_strides_refused_on_auto_correct_on_ordered():
    n, k, m, batch = 36, 20, 28, 3
    sa, sb, sc = n * k + 1, k * m + 3, n * m + 1    # float elements: 4-byte, not 16-byte aligned
    rng = np.random.default_rng(29)
    a = random_operands("float", ((batch - 1) * sa + n * k,), rng)
    b = random_operands("float", ((batch - 1) * sb + k * m,), rng)
    batched_launch(g.make_config("float", "Add", "Min"), a, b, n, k, m, batch, sa, sb, sc, expect=2)
    c = batched_launch(g.make_config("float", "Add", "Min", g.PATH_ORDERED), a, b, n, k, m, batch, sa, sb, sc)
    for e in range(batch):
        want = _oracle.naive("float", "Add", "Min", element(a, e, sa, n, k), element(b, e, sb, k, m))
        assert sr.same_bits(element(c, e, sc, n, m), want), e


# ---- determinism -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,mp,rd,shape", [("float", "Multiply", "Add", (96, 128, 132)), ("half", "Multiply", "Add", (96, 128, 132)),
                                               ("half", "Multiply", "Add", (96, 256, 128)), ("half", "Multiply", "Add", (128, 48, 256)),
                                               ("float", "Add", "Min", (96, 128, 132)), ("double", "Multiply", "Add", (96, 128, 132)),
                                               ("double", "Multiply", "Add", (512, 64, 512)), ("uint8_t", "Multiply", "Add", (96, 256, 128))],
                         ids=lambda x: str(x))
def test_batched_bits_do_not_depend_on_chunking_or_position(dtype, mp, rd, shape):
    (n, k, m), batch = shape, 10
    rng = np.random.default_rng(31)
    a, b = stack(dtype, batch, n, k, rng), stack(dtype, batch, k, m, rng)
    cfg = g.make_config(dtype, mp, rd)
    whole = batched_launch(cfg, a.ravel(), b.ravel(), n, k, m, batch, n * k, k * m, n * m)
    g.set_tuning("batch_chunk", 3)
    try:
        chunked = batched_launch(cfg, a.ravel(), b.ravel(), n, k, m, batch, n * k, k * m, n * m)
    finally:
        g.set_tuning("batch_chunk", -1)
    assert sr.same_bits(whole, chunked)
    # element 0 of this batch, placed last in a batch of 4 others
    other = stack(dtype, 4, n, k, rng), stack(dtype, 4, k, m, rng)
    a2 = np.concatenate([other[0], a[:1]]); b2 = np.concatenate([other[1], b[:1]])
    c2 = batched_launch(cfg, a2.ravel(), b2.ravel(), n, k, m, 5, n * k, k * m, n * m)
    assert sr.same_bits(element(c2, 4, n * m, n, m), element(whole, 0, n * m, n, m))


# ---- the torch binding -----------------------------------------------------------------------------------------------
def test_bmm_on_torch_tensors_with_expanded_operands():
    import torch
    dev = torch.device("cuda:0")
    gen = torch.Generator(device="cpu").manual_seed(1)
    a = torch.rand(6, 64, 96, generator=gen).to(dev)
    b = torch.rand(96, 80, generator=gen).to(dev)
    c = g.bmm(a, b)
    torch.cuda.synchronize()
    assert c.shape == (6, 64, 80)
    ref = torch.matmul(a.double(), b.double())
    assert (c.double() - ref).abs().max().item() < 1e-4
    c2 = g.bmm(a, b.expand(6, 96, 80))   # batch stride 0
    assert torch.equal(c, c2)
    c3 = g.bmm(a[:1].expand(6, 64, 96), b.expand(6, 96, 80), map_op="Add", reduce_op="Min")
    want = (a[0][:, :, None] + b[None, :, :]).min(dim=1).values
    assert torch.equal(c3[5], want) and torch.equal(c3[0], want)
    at = a.transpose(1, 2).contiguous()
    c4 = g.bmm(at, b, transposed_a=True)
    assert (c4.double() - ref).abs().max().item() < 1e-4
    out = torch.empty(6, 64, 80, device=dev)
    assert g.bmm(a, b, out=out) is out


def test_bmm_raises_on_wrong_shape_dtype_or_layout():
    import torch
    dev = torch.device("cuda:0")
    a = torch.rand(4, 32, 48, device=dev)
    b = torch.rand(4, 48, 16, device=dev)
    with pytest.raises(g.MMError):
        g.bmm(a, torch.rand(4, 40, 16, device=dev))           # inner dimensions
    with pytest.raises(g.MMError):
        g.bmm(a, torch.rand(3, 48, 16, device=dev))           # batch sizes
    with pytest.raises(g.MMError):
        g.bmm(a, b.double())                                  # dtype
    with pytest.raises(g.MMError):
        g.bmm(a, b.transpose(1, 2).contiguous().transpose(1, 2))   # not row-major
    with pytest.raises(g.MMError):
        g.bmm(a.cpu(), b.cpu())                               # no CPU path
    with pytest.raises(g.MMError):
        g.bmm(a, b, out=torch.empty(4, 32, 17, device=dev))


# ---- throughput floors (collected last; fail only with MM_PERF_FLOORS=1) ---------------------------------------------
def _ratio(dtype, mp, rd, batch, n, k, m):
    import importlib.util
    spec = importlib.util.spec_from_file_location("batched_sweep", os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "tools", "batched_sweep.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    tb, tl = mod.measure(dtype, mp, rd, batch, n, k, m, False, reps=5)
    return tl / tb


# Floors: about 15 % below the MI355X run of tools/batched_sweep.py (profiles/batched_sweep_mi355x.txt: 465x, 27.7x,
# 1.01x the per-element loop).
@pytest.mark.parametrize("dtype,mp,rd,batch,n,k,m,family,floor", [
    ("float", "Add", "Min", 4096, 128, 128, 128, "valu_tile", 380.0),
    ("float", "Multiply", "Add", 1024, 256, 256, 256, "mfma_f32_", 23.0),
    ("float", "Multiply", "Add", 8, 4096, 4096, 4096, "mfma_f32_", 0.86),
], ids=["minplus_4096x128", "f32_1024x256", "f32_8x4096"])
def test_throughput_floor_batched_vs_loop(dtype, mp, rd, batch, n, k, m, family, floor):
    assert g.kernel_name_batched(g.make_config(dtype, mp, rd), n, k, m, batch).startswith(family)
    ratio = _ratio(dtype, mp, rd, batch, n, k, m)
    msg = f"batched {dtype} ({mp}, {rd}) {batch} x {n}x{k}x{m}: {ratio:.2f}x the per-element loop, floor {floor}x"
    if os.environ.get("MM_PERF_FLOORS") == "1":
        assert ratio >= floor, msg
    elif ratio < floor:
        warnings.warn(msg)
