"""GPU tests of the bit-packed Boolean calls (mm_bits_*, pack_bits / unpack_bits / bits_matmul / bits_addmm_ / bits_closure_).
The oracle is tests/_bits_ref.py: numpy on bool arrays.  Everything is compared exactly, word for word -- the padding bits of
every output must be 0, and guard words, gap words (beyond a row's own words, up to its ld) and the space between the
elements of a batch must come back untouched."""
import ctypes
import functools

import numpy as np
import pytest

import _bits_ref as br
import gemm_hls_amd as g
from _bits_rig import Dev, _first_difference, _layout, _pattern, _poison_padding, _rows_of
from _knobs import knob  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu


def gemm(a, b, seed=None, *, ld_extra=(0, 0, 0), ld=None, stride_c_extra=0, shift=(0, 0, 0), poison=False, batch=None, rng=None,
         want_name=None):
    """mm_bits_gemm_launch on bool operands a (Ba, n, k), b (Bb, k, m) -- Ba, Bb in {1, batch}: 1 is a broadcast -- and an
    optional bool seed (batch, n, m) for the accumulating form.  Gap words of the inputs hold random bits, those of C a
    pattern that must survive; poison: the padding bits of A, B and the seed are ones.  Asserts that C equals the reference
    word for word and returns element 0 of what the GPU wrote, as a bool array."""
    rng = rng or np.random.default_rng(0)
    n, k, m = a.shape[1], a.shape[2], b.shape[2]
    batch = batch or max(a.shape[0], b.shape[0])
    kw, mw = br.words(k), br.words(m)
    lda, ldb, ldc = ld or (kw + ld_extra[0], mw + ld_extra[1], mw + ld_extra[2])
    pa, pb = br.pack(a), br.pack(b)
    want = br.matmul(a, b) | (seed if seed is not None else False)
    want = np.broadcast_to(want, (batch, n, m))
    pc = br.pack(seed) if seed is not None else None
    if poison:
        pa, pb = _poison_padding(pa, k), _poison_padding(pb, m)
        pc = _poison_padding(pc, m) if pc is not None else None
    sa, sb = (n - 1) * lda + kw + 5, (k - 1) * ldb + mw + 3
    sa, sb = (sa + 3) // 4 * 4, (sb + 3) // 4 * 4          # batch strides that keep the tile kernel's alignment
    sc = ((n - 1) * ldc + mw + stride_c_extra + 1) // 2 * 2
    rand = lambda count: rng.integers(0, 1 << 32, size=count, dtype=np.uint64).astype(np.uint32)
    da = Dev(_layout(pa, lda, sa, rand(pa.shape[0] * sa)), shift[0])
    db = Dev(_layout(pb, ldb, sb, rand(pb.shape[0] * sb)), shift[1])
    c_fill = _pattern(batch * sc, 3)
    c_host = _layout(pc, ldc, sc, c_fill) if pc is not None else c_fill.reshape(batch, sc).copy()
    dc = Dev(c_host, shift[2])
    if want_name is not None:
        assert g.kernel_name_bits_gemm(n, k, m, lda, ldb, ldc, batch) == want_name
    rc = g.lib().mm_bits_gemm_launch(0, da.ptr, db.ptr, dc.ptr, n, k, m, lda, ldb, ldc, batch,
                                     sa if a.shape[0] > 1 else 0, sb if b.shape[0] > 1 else 0, sc, int(seed is not None), None)
    assert rc == 0, (rc, g.lib().mm_last_error().decode())
    got = dc.fetch()
    rows = _rows_of(got, n, mw, ldc)
    assert np.array_equal(rows, br.pack(want)), _first_difference(rows, br.pack(want), "words", "#x")
    assert np.array_equal(got, _layout(rows, ldc, sc, c_fill)), "a gap word of C was written"
    return br.unpack(rows[0], m)


def _operands(n, k, m, rng, batch_a=1, batch_b=1):
    p = br.density(k)
    return rng.random((batch_a, n, k)) < p, rng.random((batch_b, k, m)) < p


def _assert_informative(ref, n, m):
    if n * m >= 1024:
        d = ref.mean()
        assert 0.2 <= d <= 0.8, f"the reference's output density {d:.3f} would hide errors"


# every issue shape, and one shape just inside and just outside each threshold of the kernels: the 64-row tile (64, 65 above),
# the plain kernel's 64-word tile and the rule's M > 2048, the tile kernel's 128-word tile
SHAPES = [(1, 1, 1), (5, 33, 31), (64, 64, 64), (65, 95, 129), (130, 1, 70), (257, 513, 255), (300, 1000, 700), (96, 4100, 64),
          (3, 40, 2048), (3, 40, 2049), (2, 33, 4096), (2, 33, 4097)]


@pytest.mark.parametrize("n,k,m", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_bits_product_against_numpy(n, k, m, knob):
    """Natural ld (the plain kernel serves: ld = ceil(M / 32) is odd or M <= 2048), then an ld the tile kernel's rule accepts,
    under the default rule and with each kernel forced."""
    rng = np.random.default_rng(n * 1000003 + k * 1009 + m)
    a, b = _operands(n, k, m, rng)
    mw = br.words(m)
    ld4 = (br.words(k), (mw + 3) // 4 * 4, (mw + 1) // 2 * 2)
    rule = "bits_tile" if m > 2048 else "bits_plain"
    ref = gemm(a, b, rng=rng, want_name=rule if ld4[1:] == (mw, mw) else "bits_plain")
    _assert_informative(ref, n, m)
    gemm(a, b, ld=ld4, rng=rng, want_name=rule)
    for variant, name in ((0, "bits_plain"), (1, "bits_tile")):
        knob("bits_variant", variant)
        gemm(a, b, ld=ld4, rng=rng, want_name=name)


@pytest.mark.parametrize("variant", [0, 1], ids=["plain", "tile"])
def test_bits_product_special_operands(variant, knob):
    knob("bits_variant", variant)
    n, k, m = 65, 95, 129
    ld = (3, 8, 6)
    rng = np.random.default_rng(7)
    a, b = _operands(n, k, m, rng)
    zero = gemm(np.zeros_like(a), b, ld=ld, rng=rng)                               # all-zero A: every slab is skipped
    assert not zero.any()
    ones = gemm(np.ones_like(a), np.ones_like(b), ld=ld, rng=rng, poison=True)     # all ones: C all ones, its padding 0
    assert ones.all()
    single = np.zeros_like(a)
    single[0, 37, k - 1] = True                                                    # one bit, in A's last valid column
    got = gemm(single, b, ld=ld, rng=rng, poison=True)
    assert np.array_equal(got[37], b[0, k - 1]) and not np.delete(got, 37, axis=0).any()
    # K = 0 in the plain form: the empty OR
    dc = Dev(_pattern(n * 6, 3).reshape(n, 6))
    assert g.lib().mm_bits_gemm_launch(0, None, None, dc.ptr, n, 0, m, 0, 0, 6, 1, 0, 0, 0, 0, None) == 0
    out = dc.fetch()
    assert not out[:, :5].any() and np.array_equal(out[:, 5], _pattern(n * 6, 3).reshape(n, 6)[:, 5])


FEATURE_SHAPES = [(65, 95, 129), (257, 513, 255)]


def _tile_ld(k, m, extra=0):
    mw = br.words(m)
    return (br.words(k) + (3 if extra else 0), (mw + 3) // 4 * 4 + 4 * extra, (mw + 1) // 2 * 2 + 2 * extra)


@pytest.mark.parametrize("variant", [0, 1], ids=["plain", "tile"])
@pytest.mark.parametrize("n,k,m", FEATURE_SHAPES, ids=["65x95x129", "257x513x255"])
def test_bits_product_accumulate_ld_padding_and_alignment(n, k, m, variant, knob):
    knob("bits_variant", variant)
    name = ("bits_plain", "bits_tile")[variant]
    rng = np.random.default_rng(n + 31 * variant)
    a, b = _operands(n, k, m, rng)
    seed = rng.random((1, n, m)) < 0.1
    ld = _tile_ld(k, m)
    # accumulate onto a random C; two calls on the halves of K equal one call on all of it
    full = gemm(a, b, seed, ld=ld, rng=rng, want_name=name)
    h = k // 2
    first = gemm(a[:, :, :h], b[:, :h], seed, ld=(br.words(h), ld[1], ld[2]), rng=rng)
    both = gemm(a[:, :, h:], b[:, h:], first[None], ld=(br.words(k - h), ld[1], ld[2]), rng=rng)
    assert np.array_equal(both, full) and (full != seed[0]).any() and (full != br.matmul(a, b)[0]).any()
    # ld larger than the row in all three operands: input gaps hold random bits, C's gaps a pattern that must survive
    gemm(a, b, ld=_tile_ld(k, m, 1), rng=rng, want_name=name)
    gemm(a, b, seed, ld=_tile_ld(k, m, 1), stride_c_extra=10, rng=rng, want_name=name)
    # padding bits of A, B and the seeded C poisoned with ones
    gemm(a, b, seed, ld=ld, poison=True, rng=rng)
    gemm(a, b, ld=_tile_ld(k, m, 1), poison=True, rng=rng)
    # each base pointer moved by one word (4-byte aligned only): the plain kernel serves, the same bits
    for shift in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)):
        gemm(a, b, seed, ld=ld, shift=shift, poison=True, rng=rng, want_name=name)


@pytest.mark.parametrize("variant", [0, 1], ids=["plain", "tile"])
@pytest.mark.parametrize("n,k,m", FEATURE_SHAPES, ids=["65x95x129", "257x513x255"])
def test_bits_product_batches(n, k, m, variant, knob):
    knob("bits_variant", variant)
    rng = np.random.default_rng(n + 17 * variant)
    ld = _tile_ld(k, m, 1)
    seed = rng.random((3, n, m)) < 0.1
    for ba, bb in ((3, 3), (1, 3), (3, 1)):                         # full, A broadcast, B broadcast
        a, b = _operands(n, k, m, rng, ba, bb)
        gemm(a, b, ld=ld, batch=3, rng=rng)
        gemm(a, b, seed, ld=ld, batch=3, stride_c_extra=2 * n, rng=rng, poison=True)   # stride_c beyond one matrix
    knob("batch_chunk", 2)                                           # two launches: 2 + 1
    gemm(a, b, seed, ld=ld, batch=3, rng=rng)


def _cuda(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


def _words(t):
    return t.cpu().numpy().view(np.uint32)


def test_bits_matmul_binding_column_slice_view_and_out(knob):
    import torch
    rng = np.random.default_rng(11)
    n, k, m = 65, 64, 129                       # a = words 1 and 2 of a 5-word packed matrix: a column slice, no copy
    wide = rng.random((n, 160)) < br.density(k)
    b = rng.random((k, m)) < br.density(k)
    p = g.pack_bits(_cuda(wide))
    view = p[:, 1:3]
    assert not view.is_contiguous() and view.data_ptr() == p.data_ptr() + 4
    pb = g.pack_bits(_cuda(b))
    want = br.matmul(wide[:, 32:96], b)
    got = g.bits_matmul(view, pb, k, m)
    assert got.dtype == torch.int32 and tuple(got.shape) == (n, 5)
    assert np.array_equal(_words(got), br.pack(want))
    # k below the slice's bits: the rest of the last word is padding
    assert np.array_equal(_words(g.bits_matmul(view, pb[:50], 50, m)), br.pack(br.matmul(wide[:, 32:82], b[:50])))
    # out with a wider row: the words beyond ceil(m / 32) are left alone; bits_addmm_ on the same view accumulates
    out = torch.full((n, 8), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    g.bits_matmul(view, pb, k, m, out=out[:, :6])
    assert np.array_equal(_words(out)[:, :5], br.pack(want)) and (_words(out)[:, 5:] == 0x5A5A5A5A).all()
    seed = rng.random((n, m)) < 0.1
    c = g.pack_bits(_cuda(seed))
    assert g.bits_addmm_(c, view, pb, k, m) is c
    assert np.array_equal(_words(c), br.pack(want | seed))
    # 3-D operands and a broadcast with batch stride 0
    a3 = rng.random((3, n, k)) < br.density(k)
    got3 = g.bits_matmul(g.pack_bits(_cuda(a3)), pb.unsqueeze(0).expand(3, -1, -1), k, m)
    assert np.array_equal(_words(got3), br.pack(br.matmul(a3, b)))


def test_bits_matmul_agrees_with_the_byte_path():
    rng = np.random.default_rng(12)
    n, k, m = 257, 513, 255
    a, b = (x[0] for x in _operands(n, k, m, rng))
    got = g.unpack_bits(g.bits_matmul(g.pack_bits(_cuda(a)), g.pack_bits(_cuda(b)), k, m), m, dtype=__import__("torch").uint8)
    byte = g.matmul(_cuda(a.astype(np.uint8)), _cuda(b.astype(np.uint8)), dtype="uint8_t", map_op="And", reduce_op="Max")
    assert np.array_equal(got.cpu().numpy(), byte.cpu().numpy())
    _assert_informative(byte.cpu().numpy() != 0, n, m)


@pytest.mark.parametrize("cols", [1, 31, 32, 33, 1000])
def test_pack_unpack_round_trip(cols):
    import torch
    rng = np.random.default_rng(cols)
    x = rng.integers(0, 3, size=(2, 37, cols)).astype(np.uint8) * 127       # 0, 127 and 254: nonzero bytes other than 1 pack to 1
    p = g.pack_bits(_cuda(x))
    assert p.dtype == torch.int32 and tuple(p.shape) == (2, 37, br.words(cols))
    assert np.array_equal(_words(p), br.pack(x))                             # padding bits 0
    assert np.array_equal(g.unpack_bits(p, cols).cpu().numpy(), x != 0)
    assert np.array_equal(g.unpack_bits(p, cols, dtype=torch.uint8).cpu().numpy(), (x != 0).astype(np.uint8))
    assert np.array_equal(_words(g.pack_bits(_cuda(x != 0))), br.pack(x))    # torch.bool in
    # a strided source through the binding: a column slice of a wider byte matrix, no copy
    wide = rng.integers(0, 2, size=(37, cols + 9)).astype(np.uint8)
    assert np.array_equal(_words(g.pack_bits(_cuda(wide)[:, 3:3 + cols])), br.pack(wide[:, 3:3 + cols]))


@pytest.mark.parametrize("cols", [33, 1000])
def test_pack_unpack_strided_source_and_destination(cols):
    """The C ABI with ld and batch strides beyond the rows on both sides: gap bytes and gap words keep their pattern, the
    padding bits of poisoned packed input are ignored."""
    import torch
    rng = np.random.default_rng(cols + 1)
    rows, batch, w = 19, 3, br.words(cols)
    x = rng.integers(0, 2, size=(batch, rows, cols)).astype(np.uint8) * 9
    ld_b, st_b = cols + 7, rows * (cols + 7) + 13
    ld_w, st_w = w + 2, rows * (w + 2) + 5
    src = rng.integers(0, 256, size=(batch, st_b)).astype(np.uint8)
    for r in range(rows):
        src[:, r * ld_b:r * ld_b + cols] = x[:, r]
    dsrc = torch.from_numpy(src).to("cuda:0")
    fill = _pattern(batch * st_w, 4)
    dst = Dev(fill.reshape(batch, st_w))
    assert g.lib().mm_bits_pack_launch(0, dsrc.data_ptr(), dst.ptr, rows, cols, ld_b, ld_w, batch, st_b, st_w, None) == 0
    got = dst.fetch()
    want = _layout(br.pack(x), ld_w, st_w, fill)
    assert np.array_equal(got, want)
    # unpack from that layout with poisoned padding into a strided byte buffer
    poisoned = Dev(_layout(_poison_padding(br.pack(x), cols), ld_w, st_w, rng.integers(0, 1 << 32, size=batch * st_w, dtype=np.uint64).astype(np.uint32)))
    out = torch.full((batch, st_b), 0xA5, dtype=torch.uint8, device="cuda:0")
    assert g.lib().mm_bits_unpack_launch(0, poisoned.ptr, out.data_ptr(), rows, cols, ld_w, ld_b, batch, st_w, st_b, None) == 0
    want_b = np.full((batch, st_b), 0xA5, np.uint8)
    for r in range(rows):
        want_b[:, r * ld_b:r * ld_b + cols] = x[:, r] != 0
    assert np.array_equal(out.cpu().numpy(), want_b)


# ---- closure ------------------------------------------------------------------------------------------------------------
CLOSURE_N = [1, 33, 64, 65, 127, 200, 257, 520, 1030]   # 64 and 65: both sides of the one block size that ships


@functools.lru_cache(maxsize=None)
def _graph(n, skip=0):
    """(graph, closure) of the first seed of 0..4 (after `skip` accepted ones) whose reference closure is informative: density
    in [0.05, 0.80] and different from the input (n >= 33).  Never skips: a size without such a seed fails."""
    found = 0
    for seed in range(5):
        d = br.graph(n, seed)
        c = br.closure(d)
        if n < 33 or (0.05 <= c.mean() <= 0.80 and (c != d).any()):
            if found == skip:
                return d, c
            found += 1
    raise AssertionError(f"no seed in 0..4 gives an informative closure at n = {n}")


def closure(d, ldd=None, stride_extra=0, poison=False, rng=None):
    """mm_bits_closure_launch on (batch, n, n) bool graphs; gaps hold random bits that must survive.  Returns the bool result."""
    rng = rng or np.random.default_rng(1)
    batch, n, _ = d.shape
    w = br.words(n)
    ldd = ldd or w
    stride = (n - 1) * ldd + w + stride_extra
    p = br.pack(d)
    if poison:
        p = _poison_padding(p, n)
    fill = rng.integers(0, 1 << 32, size=batch * stride, dtype=np.uint64).astype(np.uint32)
    dev = Dev(_layout(p, ldd, stride, fill))
    rc = g.lib().mm_bits_closure_launch(0, dev.ptr, n, ldd, batch, stride, None)
    assert rc == 0, (rc, g.lib().mm_last_error().decode())
    got = dev.fetch()
    rows = _rows_of(got, n, w, ldd)
    assert np.array_equal(got, _layout(rows, ldd, stride, fill)), "a gap word of D was written"
    assert np.array_equal(rows, br.pack(br.unpack(rows, n))), "padding bits of D are not 0"
    return br.unpack(rows, n)


@pytest.mark.parametrize("n", CLOSURE_N)
def test_bits_closure_against_warshall(n):
    d, want = _graph(n)
    assert g.kernel_name_bits_closure(n) == ("bits_closure_onchip" if n <= 64 else "bits_closure_blocked")
    got = closure(d[None])[0]
    assert np.array_equal(got, want), f"{(got != want).sum()} entries differ"
    # ldd larger than the row, poisoned gaps and poisoned padding (an even and an odd ldd: both product kernels in step 3)
    for extra in (1, 2):
        assert np.array_equal(closure(d[None], ldd=br.words(n) + extra, stride_extra=3, poison=True)[0], want)
    # idempotent: a second call changes nothing
    assert np.array_equal(closure(want[None])[0], want)


@pytest.mark.parametrize("n", [40, 200], ids=["onchip-40", "blocked-200"])
def test_bits_closure_batch_of_five_equals_each_alone(n, knob):
    graphs = [br.graph(n, seed) for seed in range(5)]
    wants = [br.closure(x) for x in graphs]
    assert len({x.tobytes() for x in wants}) == 5
    alone = [closure(x[None])[0] for x in graphs]
    for got, want in zip(alone, wants):
        assert np.array_equal(got, want)
    batch = closure(np.stack(graphs), ldd=br.words(n) + 1, stride_extra=7, poison=True)
    assert np.array_equal(batch, np.stack(wants))
    knob("batch_chunk", 2)          # the blocked form's second and third workspace chunk: 2 + 2 + 1 graphs
    assert np.array_equal(closure(np.stack(graphs), stride_extra=7), np.stack(wants))


def test_bits_closure_binding_and_the_byte_path():
    import torch
    n = 257
    d, want = _graph(n)
    p = g.pack_bits(_cuda(d))
    assert g.bits_closure_(p) is p
    assert np.array_equal(_words(p), br.pack(want))
    byte = _cuda(d.astype(np.uint8))
    g.closure_(byte, dtype="uint8_t", map_op="And", reduce_op="Max")
    assert np.array_equal(g.unpack_bits(p, n, dtype=torch.uint8).cpu().numpy(), byte.cpu().numpy())
    # a batch through the binding, n given explicitly on a tensor with more rows' worth of words
    d3 = np.stack([br.graph(70, s) for s in range(3)])
    p3 = torch.zeros((3, 70, 4), dtype=torch.int32, device="cuda:0")
    p3[:, :, :3] = g.pack_bits(_cuda(d3))
    p3[:, :, 3] = 0x77777777
    g.bits_closure_(p3, 70)
    assert np.array_equal(_words(p3)[:, :, :3], br.pack(np.stack([br.closure(x) for x in d3])))
    assert (_words(p3)[:, :, 3] == 0x77777777).all()
