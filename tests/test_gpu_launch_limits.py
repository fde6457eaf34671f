"""GPU tests that run every launch at the grid limit its host code caps, splits or ignores ("Launch limits"):
the second launch of a chunked batch, the grid-stride part of a conversion, a gridDim.y that does not fit, a 1-D grid of
more than 65536 rows of tiles.  The cases, their shapes and the limits are tests/_limit_cases.py's, checked on the CPU by
tests/test_limit_cases.py.

Every test follows the same rules.  Operands are drawn on the device from a seeded generator and differ from element to
element, so a launch that starts one element off shows.  They hold small integers (or wrap, where the type does), so every
comparison is exact: no tolerance appears here.  The reference is broadcast or float64 torch on the device, never this
library, formed and compared in pieces of the batch so that it fits the memory budget; its first piece must hold at least 16
distinct values.  Every output is a view into an allocation pre-filled with a sentinel the reference cannot produce, with 64
guard elements on each side; guards and stride gaps must keep the fill.  The whole output is compared, never a sample."""
import pytest
import torch

import _closure_ref as cr
import _limit_cases as lc
import gemm_hls_amd as g

pytestmark = pytest.mark.gpu

GUARD = 64
PIECES = 16
PATHS = {"auto": g.PATH_AUTO, "ordered": g.PATH_ORDERED, "split": g.PATH_SPLIT}
# values no reference below produces: sums and minima of small integers, counts, 0 / 1, vertices, and -- for the types that
# wrap -- even numbers only (A holds even values)
SENTINEL = {torch.float32: -2.0**100, torch.float64: -2.0**100, torch.float16: -32768.0, torch.int32: 0x5A5A5A5B,
            torch.int8: 0x5B, torch.uint8: 0x5A}
PEAK = {}   # test id -> peak bytes of torch's allocator, printed for profiles/launch_limits_mi355x.txt


@pytest.fixture(autouse=True)
def _device_memory(request):
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    failed = request.session.testsfailed
    yield
    torch.cuda.synchronize()
    name = request.node.name
    PEAK[name] = torch.cuda.max_memory_allocated()
    print(f"\npeak device memory {name}: {PEAK[name] / 2**20:.0f} MiB")
    torch.cuda.empty_cache()
    case = lc.BY_ID[max((cid for cid in lc.BY_ID if cid in name), key=len)]   # every test carries its case's id
    if request.session.testsfailed == failed:   # (a failing comparison allocates to say where it failed)
        assert PEAK[name] <= lc.device_bytes(case), "the case's memory estimate (tests/_limit_cases.py) is below what it took"


def _dev():
    return torch.device("cuda:0")


def _gen(seed):
    return torch.Generator(device=_dev()).manual_seed(seed)


def _ints(gen, shape, lo, hi, dtype):
    """Integers lo .. hi - 1 as `dtype`, drawn on the device."""
    return torch.randint(lo, hi, shape, generator=gen, device=_dev(), dtype=dtype)


def _random_bytes(gen, shape, dtype):
    """`dtype` (an integer type) over its whole range: random bytes, viewed."""
    count = dtype.itemsize
    for s in shape:
        count *= s
    return torch.randint(0, 256, (count,), generator=gen, device=_dev(), dtype=torch.uint8).view(dtype).view(shape)


def _random_words(gen, shape):
    """int32 words of 32 random bits each."""
    return _random_bytes(gen, shape, torch.int32)


class Guarded:
    """`extent` elements of `dtype` between two guards of GUARD elements, all pre-filled with the type's sentinel."""

    def __init__(self, dtype, extent, sentinel=None):
        self.sentinel = SENTINEL[dtype] if sentinel is None else sentinel
        self.buf = torch.full((GUARD + extent + GUARD,), self.sentinel, dtype=dtype, device=_dev())
        self.flat = self.buf[GUARD:GUARD + extent]

    def dense(self, *shape):
        return self.flat.view(*shape)

    def assert_guards(self):
        assert bool((self.buf[:GUARD] == self.sentinel).all()) and bool((self.buf[-GUARD:] == self.sentinel).all()), "a guard element was written"

    def assert_fill(self, view, what):
        assert bool((view == self.sentinel).all()), f"{what} lost its fill"


def _pieces(count, pieces=PIECES):
    step = -(-count // pieces)
    return [slice(lo, min(count, lo + step)) for lo in range(0, count, step)]


def _distinct(ref):
    flat = ref.reshape(-1)
    return torch.unique(flat[::max(1, flat.numel() >> 20)]).numel()


def _assert_equal(got, ref, first_row, what, sentinel, check_distinct):
    """got == ref exactly; on a mismatch names the first differing row (batch element, or matrix row)."""
    assert got.shape == ref.shape and got.dtype == ref.dtype, (got.shape, ref.shape, got.dtype, ref.dtype)
    if check_distinct:
        assert _distinct(ref) >= 16, f"{what}: a degenerate reference ({_distinct(ref)} distinct values)"
    assert not bool((ref == sentinel).any()), f"{what}: the reference produces the sentinel"
    if torch.equal(got, ref):
        return
    bad = (got != ref).reshape(got.shape[0], -1).any(1).nonzero().flatten()
    r = int(bad[0])
    raise AssertionError(f"{what}: {bad.numel()} of {got.shape[0]} rows of this piece differ, first row {first_row + r} "
                         f"(piece starts at {first_row}): got {got[r].flatten()[:8].tolist()}, want {ref[r].flatten()[:8].tolist()}")


# ---- references -----------------------------------------------------------------------------------------------------------
def _wrap(x, dtype):
    """int64 -> `dtype` the way the element type wraps."""
    bits = torch.iinfo(dtype).bits
    half = 1 << (bits - 1)
    return (((x + half) % (1 << bits)) - half).to(dtype)


def _product_ref(c, a, b, out_dtype):
    """a (..., n, k) (map, reduce) b (..., k, m) of one piece, in `out_dtype`; with the first winning k for argreduce."""
    if c.reduce_op == "Add":
        if c.dtype == "int":                               # full-range operands: int32 products and sums, which wrap
            return (a.unsqueeze(-1) * b.unsqueeze(-3)).sum(-2, dtype=torch.int32)
        exact = torch.matmul(a.double(), b.double())       # small integers: float64 holds every sum exactly
        return exact.to(out_dtype) if out_dtype.is_floating_point else _wrap(exact.to(torch.int64), out_dtype)
    assert c.map_op == "Add"
    t = a.unsqueeze(-1) + b.unsqueeze(-3)
    v = t.amin(-2) if c.reduce_op == "Min" else t.amax(-2)
    if c.call != "matmul_argreduce":
        return v
    index = torch.full(v.shape, c.k - 1, dtype=torch.int32, device=v.device)
    for k in range(c.k - 2, -1, -1):                      # the first k whose mapped value is the result
        index = torch.where(t.select(-2, k) == v, k, index)
    return v, index + c.extra["index_base"]


# ---- dense products: L1, L2, L5, L6 ------------------------------------------------------------------------------------------
RANGE = {"float": (-20, 21), "double": (-20, 21), "half": (-4, 5)}


def _operand(c, gen, shape, even=False):
    tdt = g.torch_dtype(c.dtype)
    if c.dtype in RANGE:
        return _ints(gen, shape, *RANGE[c.dtype], tdt)
    if c.dtype == "int8_t" and c.call == "matmul_wide":
        return _ints(gen, shape, -128, 128, tdt)
    # the types whose results wrap: the whole range; A even, so that every result is even and the sentinel, odd, is not one
    x = _random_bytes(gen, shape, tdt)
    return x & ~1 if even else x


def _dense_case(c, n=None, seed=1):
    """Runs the case's call on fresh operands and compares the whole output, piece by piece."""
    n = c.n if n is None else n
    name = lc.kernel_name(c, n)
    assert name.startswith(c.kernel), name
    gen = _gen(seed)
    batch, nt = c.batch, c.call == "matmul_nt"
    lead = () if batch == 1 else (batch,)
    a = _operand(c, gen, (() if "a" in c.shared else lead) + (n, c.k), even=True)
    b = _operand(c, gen, (() if "b" in c.shared else lead) + ((c.m, c.k) if nt else (c.k, c.m)))
    cdt = g.torch_dtype(g.widen_dtype(c.dtype)) if c.call == "matmul_wide" else g.torch_dtype(c.dtype)
    nm = n * c.m
    stride_c = c.extra.get("stride_c", nm)
    out = Guarded(cdt, batch * stride_c)
    index = Guarded(torch.int32, batch * stride_c, -77) if c.call == "matmul_argreduce" else None
    shape = lead + (n, c.m)
    cfg = dict(dtype=c.dtype, path=PATHS[c.path])
    ops = dict(map_op=c.map_op, reduce_op=c.reduce_op)
    seed_c = None
    with lc.pinned(c):
        if c.call == "baddbmm_":
            cv = torch.as_strided(out.flat, shape, (stride_c, c.m, 1))
            seed_c = _ints(gen, shape, 0, 50, cdt)
            cv.copy_(seed_c)
            g.baddbmm_(cv, a, b, **cfg, **ops)
        elif c.call == "bmm":
            g.bmm(a, b, **cfg, **ops, out=out.dense(*shape))
        elif c.call == "matmul":
            g.matmul(a, b, **cfg, **ops, out=out.dense(*shape))
        elif c.call == "matmul_nt":
            g.matmul_nt(a, b, **cfg, **ops, out=out.dense(*shape))
        elif c.call == "matmul_wide":
            g.matmul_wide(a, b, **cfg, out=out.dense(*shape))
        else:
            g.matmul_argreduce(a, b, **cfg, **ops, index_base=c.extra["index_base"], out=out.dense(*shape),
                               out_index=index.dense(*shape))
    torch.cuda.synchronize()
    got = torch.as_strided(out.flat, shape, ((stride_c,) if lead else ()) + (c.m, 1))
    bt = b.mT if nt else b
    wide = batch == 1 and c.m > n                                # a wide single launch goes in pieces of its columns
    rows = c.m if wide else (batch if lead else n)
    for i, sl in enumerate(_pieces(rows)):
        if wide:
            a_p, b_p, take = a, bt[..., sl], (lambda x: x[..., sl].mT)   # (compared with the columns leading)
        else:
            a_p, b_p, take = (a if "a" in c.shared else a[sl]), (bt if "b" in c.shared or not lead else bt[sl]), (lambda x: x[sl])
        ref = _product_ref(c, a_p, b_p, cdt)
        ref_index = None
        if index is not None:
            ref, ref_index = ref
        if seed_c is not None:
            ref = torch.maximum(ref, seed_c[sl]) if c.reduce_op == "Max" else torch.minimum(ref, seed_c[sl])
        ref = ref.mT if wide else ref
        _assert_equal(take(got), ref, sl.start, c.id, out.sentinel, i == 0)
        if index is not None:
            ref_index = ref_index.mT if wide else ref_index
            _assert_equal(take(index.dense(*shape)), ref_index, sl.start, c.id + " (index)", index.sentinel, False)
    out.assert_guards()
    if stride_c > nm:
        out.assert_fill(out.flat.view(batch, stride_c)[:, nm:], "the gap between two elements of C")
    if index is not None:
        index.assert_guards()


L1_DENSE = [c for c in lc.CASES if c.limit == "L1" and c.dtype != "bits"]
L2 = [c for c in lc.CASES if c.limit == "L2"]
L6 = [c for c in lc.CASES if c.limit == "L6"]


@pytest.mark.parametrize("c", L1_DENSE, ids=[c.id for c in L1_DENSE])
def test_l1_second_launch_of_a_batch(c):
    """Batch 2^22 + 2^21 + 3 of one-tile elements: chunk_of_tiles() cuts it into two launches, the second from e0 = 2^22."""
    _dense_case(c)


@pytest.mark.parametrize("c", L2, ids=[c.id for c in L2])
def test_l2_three_transposition_launches(c):
    """Batch 2 x 65535 + 7 through nt_prepass, Bt not shared: launch_transpose_t() transposes it in three launches."""
    _dense_case(c)


@pytest.mark.parametrize("c", L6, ids=[c.id for c in L6])
def test_l6_tall_and_wide_single_launches(c):
    """More than 65536 rows (columns) of tiles on the single launches' 1-D grids."""
    _dense_case(c)


# ---- L5: gridDim.y ---------------------------------------------------------------------------------------------------------
def _grid_y():
    """Rows of tiles (of blocks) that no longer fit the device's gridDim.y -- or, on a device whose gridDim.y is beyond what
    the memory budget reaches, the 65535 from which the library itself leaves the 2-D grid."""
    y = g.device_max_grid_dim_y(0)
    print(f"\nhipDeviceAttributeMaxGridDimY = {y}")
    return y if lc.GRID_Y <= y <= lc.GRID_Y + 1024 else lc.GRID_Y


@pytest.mark.parametrize("cid", ["l5_ordered_float_add_min", "l5_widen_ordered_half"])
def test_l5_rows_of_tiles_beyond_grid_dim_y(cid):
    """N = 64 Y + 65: the 2-D single launch asks for Y + 2 rows of tiles in gridDim.y."""
    _dense_case(lc.BY_ID[cid], n=lc.TILE * _grid_y() + 65)


@pytest.mark.parametrize("cid", ["l5_split"])
def test_l5_blocks_beyond_grid_dim_y(cid):
    """N = 256 Y + 257 under MM_PATH_SPLIT: its packing launch asks for Y + 2 blocks in gridDim.y.  Small integers are exact
    on this path (each fits the first bf16 plane), so every row is compared with float64 exactly: that is inside the
    documented 2^-19 normwise bound, and stricter than a band-by-band self-comparison."""
    _dense_case(lc.BY_ID[cid], n=lc.SPLIT_BLOCK * _grid_y() + 257)


# ---- packed words in torch -------------------------------------------------------------------------------------------------
def _bit_weights():
    w = torch.ones(32, dtype=torch.int64, device=_dev()) << torch.arange(32, device=_dev())
    return torch.where(w >= 1 << 31, w - (1 << 32), w).to(torch.int32)


def _pack(x):
    """bool / uint8 (..., cols) -> int32 (..., ceil(cols / 32)): column j is bit j & 31 of word j >> 5, padding bits 0 --
    numpy.packbits(bitorder="little") viewed as uint32, written in torch."""
    cols = x.shape[-1]
    w = lc.words(cols)
    if x.dim() > 1 and x.shape[0] >= 1 << 16:              # 32 int32 per word while it is formed: in pieces
        out = torch.empty(x.shape[:-1] + (w,), dtype=torch.int32, device=x.device)
        for sl in _pieces(x.shape[0]):
            out[sl] = _pack(x[sl])
        return out
    bits = torch.zeros(x.shape[:-1] + (w * 32,), dtype=torch.int32, device=x.device)
    bits[..., :cols] = x != 0
    return (bits.view(x.shape[:-1] + (w, 32)) * _bit_weights()).sum(-1, dtype=torch.int32)


def _unpack(p, cols):
    """int32 (..., W) -> bool (..., cols); padding bits and further words are ignored."""
    w = lc.words(cols)
    bits = (p[..., :w].unsqueeze(-1) >> torch.arange(32, device=p.device, dtype=torch.int32)) & 1
    return bits.reshape(p.shape[:-1] + (w * 32,))[..., :cols] != 0


def _popcount(x):
    x = x - ((x >> 1) & 0x55555555)
    x = (x & 0x33333333) + ((x >> 2) & 0x33333333)
    x = (x + (x >> 4)) & 0x0F0F0F0F
    return ((x * 0x01010101) >> 24) & 0xFF


def _garbage_padding(p, cols, gen):
    """p with random bits where its rows' padding bits are: the products must ignore them."""
    tail = cols & 31
    if tail:
        junk = _random_words(gen, p.shape[:-1]) & ~((1 << tail) - 1)
        p[..., -1] |= junk
    return p


# ---- L1, packed ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["l1_bits_matmul_shared_b"])
def test_l1_bits_matmul_second_launch(cid):
    c = lc.BY_ID[cid]
    assert lc.kernel_name(c) == c.kernel
    gen = _gen(11)
    kw, mw = lc.words(c.k), lc.words(c.m)
    # one bit in eight set, so that about half of C's are; the padding bits are as random as the rest: ignored
    a = _random_words(gen, (c.batch, c.n, kw)) & _random_words(gen, (c.batch, c.n, kw)) & _random_words(gen, (c.batch, c.n, kw))
    b = _random_words(gen, (c.k, mw)) & _random_words(gen, (c.k, mw)) & _random_words(gen, (c.k, mw))
    out = Guarded(torch.int32, c.batch * c.n * mw)
    got = g.bits_matmul(a, b, c.k, c.m, out=out.dense(c.batch, c.n, mw))
    torch.cuda.synchronize()
    bf = _unpack(b, c.m).double()
    for i, sl in enumerate(_pieces(c.batch)):
        ref = _pack(torch.matmul(_unpack(a[sl], c.k).double(), bf) > 0)
        _assert_equal(got[sl], ref, sl.start, c.id, out.sentinel, i == 0)
    out.assert_guards()


@pytest.mark.parametrize("cid", ["l1_bits_count_xor_shared_bt"])
def test_l1_bits_count_second_launch(cid):
    c = lc.BY_ID[cid]
    assert lc.kernel_name(c) == c.kernel
    gen = _gen(12)
    kw = lc.words(c.k)
    a, bt = _random_words(gen, (c.batch, c.n, kw)), _random_words(gen, (c.m, kw))   # padding bits random: ignored
    out = Guarded(torch.int32, c.batch * c.n * c.m, -7)
    got = g.bits_matmul_count(a, bt, c.k, op=c.extra["op"], out=out.dense(c.batch, c.n, c.m))
    torch.cuda.synchronize()
    mask = torch.tensor([-1, (1 << (c.k & 31)) - 1], dtype=torch.int32, device=_dev())
    for i, sl in enumerate(_pieces(c.batch, 4 * PIECES)):
        x = (a[sl].unsqueeze(-2) ^ bt) & mask                      # (piece, n, m, words)
        ref = _popcount(x).sum(-1, dtype=torch.int32)
        _assert_equal(got[sl], ref, sl.start, c.id, out.sentinel, i == 0)
    out.assert_guards()


# ---- L3: on-chip closures -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["l3_closure_float", "l3_closure_float_witness"])
def test_l3_second_closure_launch(cid):
    """Batch 2^20 + 2^19 + 5 of 4-vertex graphs: Floyd-Warshall over the batch in four broadcast steps for D (all of it), and
    tests/_closure_ref.py's relaxation rule for W on the first 4096 graphs, the last 4096 and the 4096 around e0 = 2^20."""
    c = lc.BY_ID[cid]
    n, batch, witness = c.n, c.batch, c.extra["witness"]
    cfg = g.make_config(c.dtype, c.map_op, c.reduce_op)
    assert g.kernel_name_closure(cfg, n, batch, witness) == c.kernel
    gen = _gen(21)
    d0 = _ints(gen, (batch, n, n), 1, 200, torch.float32)
    d = Guarded(torch.float32, batch * n * n)
    d.flat.copy_(d0.view(-1))
    w = Guarded(torch.int32, batch * n * n, -77) if witness else None
    g.closure_(d.dense(batch, n, n), w.dense(batch, n, n) if witness else None, dtype=c.dtype, map_op=c.map_op,
               reduce_op=c.reduce_op)
    torch.cuda.synchronize()
    ref = d0.clone()
    for v in range(n):                                             # the right-hand side is evaluated first, as numpy does
        ref = torch.minimum(ref, ref[:, :, v].unsqueeze(-1) + ref[:, v, :].unsqueeze(-2))
    assert bool((ref != d0).float().mean() > 0.1), "the closure changes too little of its input"
    for i, sl in enumerate(_pieces(batch)):
        _assert_equal(d.dense(batch, n, n)[sl], ref[sl], sl.start, c.id, d.sentinel, i == 0)
    d.assert_guards()
    if witness:
        e0 = lc.CLOSURE_GRAPHS
        for sl in (slice(0, 4096), slice(e0 - 2048, e0 + 2048), slice(batch - 4096, batch)):
            dd = d0[sl].cpu().numpy()
            ww = dd.astype("int32")
            ww[...] = -1
            for v in range(n):
                cr._relax(dd, ww, dd[:, :, v][:, :, None] + dd[:, v, :][:, None, :], v, c.reduce_op)
            got_w = w.dense(batch, n, n)[sl].cpu().numpy()
            assert (dd == ref[sl].cpu().numpy()).all()
            assert (got_w == ww).all(), (cid, sl, int((got_w != ww).any((1, 2)).argmax()) + sl.start)
        assert bool(((w.flat >= -1) & (w.flat < n)).all()), "a witness was not written, or names no vertex"
        w.assert_guards()


@pytest.mark.parametrize("cid", ["l3_bits_closure"])
def test_l3_second_bits_closure_launch(cid):
    c = lc.BY_ID[cid]
    n, batch = c.n, c.batch
    assert g.kernel_name_bits_closure(n, batch) == c.kernel
    gen = _gen(22)
    graph = _ints(gen, (batch, n, n), 0, 8, torch.uint8) == 0         # one edge in eight
    d = Guarded(torch.int32, batch * n)
    d.flat.copy_(_garbage_padding(_pack(graph), n, gen).view(-1))
    g.bits_closure_(d.dense(batch, n, 1))
    torch.cuda.synchronize()
    ref = graph.clone()
    for v in range(n):                                             # Boolean Floyd-Warshall on the unpacked batch
        ref |= ref[:, :, v].unsqueeze(-1) & ref[:, v, :].unsqueeze(-2)
    ref = _pack(ref)
    for i, sl in enumerate(_pieces(batch)):
        _assert_equal(d.dense(batch, n, 1)[sl], ref[sl], sl.start, c.id, d.sentinel, i == 0)
    d.assert_guards()


# ---- L4: the grid-stride part of the conversions -------------------------------------------------------------------------
def _convert(fn, src, dst, rows, cols, ld_src, ld_dst, batch, stride_src, stride_dst):
    g._enqueue(_dev(), fn, src.data_ptr(), dst.data_ptr(), rows, cols, ld_src, ld_dst, batch, stride_src, stride_dst)
    torch.cuda.synchronize()


@pytest.mark.parametrize("cid", ["l4_pack_bits"])
def test_l4_pack_bits_beyond_the_grid_cap(cid):
    """5 x 630 000 x 70 bytes, rows 72 bytes apart: 1.5 x the 2^22 wavefronts of work one pass of the grid covers."""
    c = lc.BY_ID[cid]
    batch, rows, cols, ld = c.batch, c.n, c.m, c.extra["ld"]
    gen = _gen(31)
    src = _ints(gen, (batch, rows, ld), 0, 2, torch.uint8) * _ints(gen, (batch, rows, ld), 1, 256, torch.uint8)   # half are 0
    w = lc.words(cols)
    ld_dst, stride_dst = w + 1, rows * (w + 1) + 8
    out = Guarded(torch.int32, batch * stride_dst)
    _convert(g.lib().mm_bits_pack_enqueue, src, out.flat, rows, cols, ld, ld_dst, batch, rows * ld, stride_dst)
    elements = out.flat.view(batch, stride_dst)
    for e in range(batch):
        got = elements[e, :rows * ld_dst].view(rows, ld_dst)
        ref = _pack(src[e, :, :cols])                              # (bytes 70 and 71 of a row are not columns)
        assert bool((ref[:, -1] >> (cols & 31) == 0).all())
        _assert_equal(got[:, :w], ref, 0, f"{c.id} element {e}", out.sentinel, e == 0)
        out.assert_fill(got[:, w:], "the gap word of a row")
    out.assert_fill(elements[:, rows * ld_dst:], "the gap between two elements")
    out.assert_guards()


@pytest.mark.parametrize("cid", ["l4_unpack_bits"])
def test_l4_unpack_bits_beyond_the_grid_cap(cid):
    """5 x 630 000 x 108 bytes from reference-packed words: 1.27 x the 2^28 bytes one pass of the grid covers.  The output
    holds 0 and 1 only, so the 16 distinct values are asked of the packed words it is read from."""
    c = lc.BY_ID[cid]
    batch, rows, cols = c.batch, c.n, c.m
    gen = _gen(32)
    w = lc.words(cols)
    src = _random_words(gen, (batch, rows, w + 1))                 # padding bits and a gap word of random bits
    assert _distinct(src[..., :w]) >= 16
    ld_dst, stride_dst = cols + 4, rows * (cols + 4) + 64
    out = Guarded(torch.uint8, batch * stride_dst)
    _convert(g.lib().mm_bits_unpack_enqueue, src, out.flat, rows, cols, w + 1, ld_dst, batch, rows * (w + 1), stride_dst)
    elements = out.flat.view(batch, stride_dst)
    for e in range(batch):
        got = elements[e, :rows * ld_dst].view(rows, ld_dst)
        for sl in _pieces(rows, 4):
            ref = _unpack(src[e, sl], cols).to(torch.uint8)
            _assert_equal(got[sl, :cols], ref, sl.start, f"{c.id} element {e}", out.sentinel, False)
        out.assert_fill(got[:, cols:], "the gap bytes of a row")
    out.assert_fill(elements[:, rows * ld_dst:], "the gap between two elements")
    out.assert_guards()


@pytest.mark.parametrize("cid", ["l4_transpose_bits"])
def test_l4_transpose_bits_beyond_the_grid_cap(cid):
    """5 x 5 rows x 35 000 003 columns: 1.3 x the 2^22 wavefronts of work one pass of the grid covers; the reference
    transpose is torch shifts on the device, one element at a time."""
    c = lc.BY_ID[cid]
    batch, rows, cols = c.batch, c.n, c.m
    gen = _gen(33)
    cw = lc.words(cols)
    src = _random_words(gen, (batch, rows, cw))                    # the last word's padding bits are random: ignored
    out = Guarded(torch.int32, batch * cols)
    got = g.transpose_bits(src, cols, out=out.dense(batch, cols, 1))
    torch.cuda.synchronize()
    for e in range(batch):
        ref = torch.zeros(cols, dtype=torch.int32, device=_dev())
        for i in range(rows):
            ref |= _unpack(src[e, i], cols).to(torch.int32) << i
        assert bool((ref >> rows == 0).all())                      # the result's padding bits
        _assert_equal(got[e, :, 0], ref, 0, f"{c.id} element {e}", out.sentinel, e == 0)
    out.assert_guards()
