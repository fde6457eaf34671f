"""GPU tests of the bit-packed product over GF(2) (mm_bits_gf2_*, bits_matmul_gf2 / bits_addmm_gf2_).  The oracle is
tests/_bits_gf2_ref.py: the integer product of the bool arrays, mod 2.  Everything is compared exactly, word for word -- the
padding bits of every output must be 0, and guard words, gap words (beyond a row's own words, up to its ld) and the space
between the elements of a batch must come back untouched.  Operands have density 0.5."""
import numpy as np
import pytest

import _bits_gf2_ref as gr
import gemm_hls_amd as g
from _bits_rig import Dev, _first_difference, _layout, _pattern, _poison_padding, _rows_of
from _knobs import knob  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

TILE_MIN = 128                 # the serving rule's N and M (include/mm_bits_gf2.h)
NAMES = ("bits_gf2_plain", "bits_gf2_tile")


def gf2(a, b, seed=None, *, ref=None, ld_extra=(0, 0, 0), ld=None, stride_c_extra=0, shift=(0, 0, 0), poison=False, batch=None,
        rng=None, want_name=None):
    """mm_bits_gf2_launch on bool operands a (Ba, n, k), b (Bb, k, m) -- Ba, Bb in {1, batch}: 1 is a broadcast -- and an
    optional bool seed (batch, n, m) for the accumulating form; ref: gr.matmul(a, b) where the caller has it already.  Gap
    words of the inputs hold random bits, those of C a pattern that must survive; poison: the padding bits of A, B and the
    seed are ones.  Asserts that C equals the reference word for word and returns element 0 of what the GPU wrote, as a bool
    array."""
    rng = rng or np.random.default_rng(0)
    n, k, m = a.shape[1], a.shape[2], b.shape[2]
    batch = batch or max(a.shape[0], b.shape[0])
    kw, mw = gr.words(k), gr.words(m)
    lda, ldb, ldc = ld or (kw + ld_extra[0], mw + ld_extra[1], mw + ld_extra[2])
    pa, pb = gr.pack(a), gr.pack(b)
    want = (gr.matmul(a, b) if ref is None else ref) ^ (seed if seed is not None else False)
    want = np.broadcast_to(want, (batch, n, m))
    pc = gr.pack(seed) if seed is not None else None
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
        assert g.kernel_name_bits_gf2(n, k, m, lda, ldb, ldc, batch) == want_name
    rc = g.lib().mm_bits_gf2_launch(0, da.ptr, db.ptr, dc.ptr, n, k, m, lda, ldb, ldc, batch,
                                    sa if a.shape[0] > 1 else 0, sb if b.shape[0] > 1 else 0, sc, int(seed is not None), None)
    assert rc == 0, (rc, g.lib().mm_last_error().decode())
    got = dc.fetch()
    rows = _rows_of(got, n, mw, ldc)
    assert np.array_equal(rows, gr.pack(want)), _first_difference(rows, gr.pack(want), "words", "#x")
    assert np.array_equal(got, _layout(rows, ldc, sc, c_fill)), "a gap word of C was written"
    return gr.unpack(rows[0], m)


def _operands(n, k, m, rng, batch_a=1, batch_b=1):
    return rng.random((batch_a, n, k)) < 0.5, rng.random((batch_b, k, m)) < 0.5


def _assert_informative(ref, n, m):
    if n * m >= 1024:
        d = ref.mean()
        assert 0.2 <= d <= 0.8, f"the reference's output density {d:.3f} would hide errors"   # (K = 1: 0.25, else 0.5)


def _tile_ld(k, m, extra=0):
    mw = gr.words(m)
    return (gr.words(k) + (3 if extra else 0), (mw + 3) // 4 * 4 + 4 * extra, (mw + 1) // 2 * 2 + 2 * extra)


# either side of each kernel's edges: the 128-row and 64-row tiles (64, 65, 129, 130, 257), a K that is no multiple of 4 (a
# nibble group straddling K) or of 32, 129 slabs (4100), the 128-word tile (4096, 4097), a row whose last 16-byte access
# straddles its word count (129 -> 5 words, 4130 -> 130 words); and both sides of the serving rule's N and M
SHAPES = [(1, 1, 1), (5, 33, 31), (64, 64, 64), (65, 95, 129), (130, 1, 70), (257, 513, 255), (300, 1000, 700), (96, 4100, 64),
          (3, 40, 4096), (3, 40, 4097), (129, 37, 4130), (TILE_MIN, 37, TILE_MIN), (TILE_MIN - 1, 37, TILE_MIN),
          (TILE_MIN, 37, TILE_MIN - 1)]


@pytest.mark.parametrize("n,k,m", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_bits_gf2_against_numpy(n, k, m, knob):
    """Natural ld, then an ld the tile kernel's rule accepts, under the default rule and with each kernel forced."""
    rng = np.random.default_rng(n * 1000003 + k * 1009 + m)
    a, b = _operands(n, k, m, rng)
    ref = gr.matmul(a, b)
    _assert_informative(ref, n, m)
    mw = gr.words(m)
    ld4 = _tile_ld(k, m)
    rule = NAMES[n >= TILE_MIN and m >= TILE_MIN]
    gf2(a, b, ref=ref, rng=rng, want_name=rule if mw % 2 == 0 else "bits_gf2_plain")   # (ldb and ldc even: the tile's rule)
    gf2(a, b, ref=ref, ld=ld4, rng=rng, want_name=rule)
    for variant in (0, 1):
        knob("bits_gf2_variant", variant)
        gf2(a, b, ref=ref, ld=ld4, rng=rng, want_name=NAMES[variant])


@pytest.mark.parametrize("variant", [0, 1], ids=["plain", "tile"])
def test_bits_gf2_special_operands(variant, knob):
    knob("bits_gf2_variant", variant)
    n, k, m = 65, 95, 129
    ld = (3, 8, 6)
    rng = np.random.default_rng(7)
    a, b = _operands(n, k, m, rng)
    assert not gf2(np.zeros_like(a), b, ld=ld, rng=rng, want_name=NAMES[variant]).any()      # all-zero A
    # all ones with poisoned padding: the sum of K ones -- all ones for odd K, all zero for even K (under OR: all ones); a
    # live padding bit of A or a live row of B at k >= K flips every output
    assert gf2(np.ones_like(a), np.ones_like(b), ld=ld, rng=rng, poison=True).all()
    assert not gf2(np.ones((1, n, 94), bool), np.ones((1, 94, m), bool), ld=ld, rng=rng, poison=True).any()
    single = np.zeros_like(a)
    single[0, 37, k - 1] = True                                                             # one bit, in A's last valid column
    got = gf2(single, b, ld=ld, rng=rng, poison=True)
    assert np.array_equal(got[37], b[0, k - 1]) and not np.delete(got, 37, axis=0).any()
    eye = np.eye(k, dtype=bool)[None]                                                       # A I = A, m = k
    assert np.array_equal(gf2(a, eye, ld=(3, 4, 4), rng=rng, poison=True, want_name=NAMES[variant]), a[0])
    # K = 0 in the plain form: the empty sum
    dc = Dev(_pattern(n * 6, 3).reshape(n, 6))
    assert g.lib().mm_bits_gf2_launch(0, None, None, dc.ptr, n, 0, m, 0, 0, 6, 1, 0, 0, 0, 0, None) == 0
    out = dc.fetch()
    assert not out[:, :5].any() and np.array_equal(out[:, 5], _pattern(n * 6, 3).reshape(n, 6)[:, 5])


FEATURE_SHAPES = [(65, 95, 129), (257, 513, 255)]


@pytest.mark.parametrize("variant", [0, 1], ids=["plain", "tile"])
@pytest.mark.parametrize("n,k,m", FEATURE_SHAPES, ids=["65x95x129", "257x513x255"])
def test_bits_gf2_accumulate_ld_padding_and_alignment(n, k, m, variant, knob):
    knob("bits_gf2_variant", variant)
    name = NAMES[variant]
    rng = np.random.default_rng(n + 31 * variant)
    a, b = _operands(n, k, m, rng)
    ref = gr.matmul(a, b)
    seed = rng.random((1, n, m)) < 0.5
    ld = _tile_ld(k, m)
    # C ^ A B onto a random C; two calls on the halves of K equal one call on all of it
    full = gf2(a, b, seed, ref=ref, ld=ld, rng=rng, want_name=name)
    h = k // 2
    first = gf2(a[:, :, :h], b[:, :h], seed, ld=(gr.words(h), ld[1], ld[2]), rng=rng)
    both = gf2(a[:, :, h:], b[:, h:], first[None], ld=(gr.words(k - h), ld[1], ld[2]), rng=rng)
    assert np.array_equal(both, full) and (full != seed[0]).any() and (full != ref[0]).any()
    # the same product applied twice restores the seed's valid bits (its poisoned padding comes back 0)
    again = gf2(a, b, full[None], ref=ref, ld=ld, rng=rng, poison=True, want_name=name)
    assert np.array_equal(again, seed[0])
    # ld larger than the row in all three operands: input gaps hold random bits, C's gaps a pattern that must survive
    gf2(a, b, ref=ref, ld=_tile_ld(k, m, 1), rng=rng, want_name=name)
    gf2(a, b, seed, ref=ref, ld=_tile_ld(k, m, 1), stride_c_extra=10, rng=rng, want_name=name)
    # padding bits of A, B and the seeded C poisoned with ones
    gf2(a, b, seed, ref=ref, ld=ld, poison=True, rng=rng)
    gf2(a, b, ref=ref, ld=_tile_ld(k, m, 1), poison=True, rng=rng)
    # each base pointer moved by one word (4-byte aligned only): the plain kernel serves, the same bits
    for shift in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)):
        gf2(a, b, seed, ref=ref, ld=ld, shift=shift, poison=True, rng=rng, want_name=name)


@pytest.mark.parametrize("variant", [0, 1], ids=["plain", "tile"])
@pytest.mark.parametrize("n,k,m", FEATURE_SHAPES, ids=["65x95x129", "257x513x255"])
def test_bits_gf2_batches(n, k, m, variant, knob):
    knob("bits_gf2_variant", variant)
    rng = np.random.default_rng(n + 17 * variant)
    ld = _tile_ld(k, m, 1)
    seed = rng.random((3, n, m)) < 0.5
    for ba, bb in ((3, 3), (1, 3), (3, 1)):                         # full, A broadcast, B broadcast
        a, b = _operands(n, k, m, rng, ba, bb)
        ref = gr.matmul(a, b)
        gf2(a, b, ref=ref, ld=ld, batch=3, rng=rng)
        gf2(a, b, seed, ref=ref, ld=ld, batch=3, stride_c_extra=2 * n, rng=rng, poison=True)   # stride_c beyond one matrix
    knob("batch_chunk", 2)                                           # two launches: 2 + 1
    gf2(a, b, seed, ref=ref, ld=ld, batch=3, rng=rng)


def test_bits_gf2_batch_beyond_one_launch():
    """2^22 + 5 elements of 1 x 32 x 32 with B broadcast: one tile each, so the batch is cut after 2^22 elements and the
    second launch starts from the pointers for_each_bits_chunk advanced."""
    batch = (1 << 22) + 5
    rng = np.random.default_rng(22)
    a = rng.integers(0, 1 << 32, size=batch, dtype=np.uint64).astype(np.uint32)
    b = rng.integers(0, 1 << 32, size=32, dtype=np.uint64).astype(np.uint32)
    want = np.zeros(batch, np.uint32)
    for k in range(32):
        want ^= np.where((a >> np.uint32(k)) & np.uint32(1), b[k], np.uint32(0)).astype(np.uint32)
    da, db, dc = Dev(a), Dev(b), Dev(_pattern(batch, 5))
    assert g.kernel_name_bits_gf2(1, 32, 32, 1, 1, 1, batch) == "bits_gf2_plain"
    rc = g.lib().mm_bits_gf2_launch(0, da.ptr, db.ptr, dc.ptr, 1, 32, 32, 1, 1, 1, batch, 1, 0, 1, 0, None)
    assert rc == 0, (rc, g.lib().mm_last_error().decode())
    got = dc.fetch()
    assert np.array_equal(got[:1 << 22], want[:1 << 22]), _first_difference(got[:1 << 22], want[:1 << 22], "words", "#x")
    assert np.array_equal(got[1 << 22:], want[1 << 22:]), "the second launch's elements"
    assert want[-5:].all() and len(set(want[-5:])) == 5              # (informative: five different nonzero words)


def _cuda(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


def _words(t):
    return t.cpu().numpy().view(np.uint32)


def test_bits_matmul_gf2_binding_and_the_counting_product():
    import torch
    rng = np.random.default_rng(12)
    n, k, m = 257, 513, 255
    a, b = (x[0] for x in _operands(n, k, m, rng))
    pa, pb = g.pack_bits(_cuda(a)), g.pack_bits(_cuda(b))
    got = g.bits_matmul_gf2(pa, pb, k, m)
    assert got.dtype == torch.int32 and tuple(got.shape) == (n, gr.words(m))
    counts = g.bits_matmul_count(pa, g.transpose_bits(pb, m), k, "And")
    assert torch.equal(g.unpack_bits(got, m, dtype=torch.uint8).to(torch.int32), counts & 1)
    want = gr.matmul(a, b)
    _assert_informative(want, n, m)
    assert np.array_equal(_words(got), gr.pack(want))
    # a = words 1 and 2 of a wider packed matrix: a column slice, no copy
    wide = rng.random((n, 160)) < 0.5
    b64 = rng.random((64, m)) < 0.5
    p = g.pack_bits(_cuda(wide))
    view = p[:, 1:3]
    assert not view.is_contiguous() and view.data_ptr() == p.data_ptr() + 4
    pb64 = g.pack_bits(_cuda(b64))
    want64 = gr.matmul(wide[:, 32:96], b64)
    assert np.array_equal(_words(g.bits_matmul_gf2(view, pb64, 64, m)), gr.pack(want64))
    # out with a wider row: the words beyond ceil(m / 32) are left alone
    out = torch.full((n, 12), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    g.bits_matmul_gf2(view, pb64, 64, m, out=out[:, :10])
    assert np.array_equal(_words(out)[:, :8], gr.pack(want64)) and (_words(out)[:, 8:] == 0x5A5A5A5A).all()
    # bits_addmm_gf2_ on a 3-D c with 2-D operands: every element takes the same product
    seed = rng.random((3, n, m)) < 0.5
    c = g.pack_bits(_cuda(seed))
    assert g.bits_addmm_gf2_(c, view, pb64, 64, m) is c
    assert np.array_equal(_words(c), gr.pack(seed ^ want64))
