"""GPU tests of the packed counting calls (mm_bits_count_*, mm_bits_transpose_*; bits_matmul_count / bits_addmm_count_ /
transpose_bits).  The oracle is tests/_bits_count_ref.py: numpy on bool arrays.  Every comparison is exact; guard words, gap
words and gap elements (beyond a row's own, up to its ld) and the space between the elements of a batch must come back
untouched.  Operands have density 0.5, and wherever N M >= 1024 and K >= 64 the reference's counts are asserted to take at
least 8 distinct values (Binomial(64, 1/4) has sigma 3.5), so that a constant or saturated result cannot pass."""
import numpy as np
import pytest

import _bits_count_ref as cr
import gemm_hls_amd as g
from _bits_rig import Dev, _first_difference, _layout, _pattern, _poison_padding, _rows_of
from _knobs import knob  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

SLAB = 256     # k per slab of both kernels (8 words)


def _pack(x):
    return cr.pack(x) if x.shape[-1] else np.zeros(x.shape[:-1] + (0,), np.uint32)


def _up4(x):
    return (x + 3) // 4 * 4


def _assert_informative(ref, n, k, m):
    if n * m >= 1024 and k >= 64:
        assert cr.distinct_values(ref) >= 8, f"the reference takes {cr.distinct_values(ref)} values: it would hide errors"


def count(a, bt, op="And", seed=None, *, ld_extra=(0, 0, 0), shift=(0, 0, 0), poison=(False, False), batch=None, rng=None,
          want_name=None, null_operands=False, base=None):
    """mm_bits_count_launch on bool operands a (Ba, n, k), bt (Bb, m, k) -- Ba, Bb in {1, batch}: 1 is a broadcast -- and an
    optional int32 seed (batch, n, m) for the accumulating form.  Gap words of the inputs hold random bits, gap elements of C
    a pattern that must survive; poison: the padding bits of a / of bt are ones.  Asserts that C equals the reference
    exactly and returns the reference, (batch, n, m) int32.  base: cr.count(a, bt, op), where the caller has it already."""
    rng = rng or np.random.default_rng(0)
    n, k, m = a.shape[1], a.shape[2], bt.shape[1]
    batch = batch or max(a.shape[0], bt.shape[0])
    kw = cr.words(k)
    lda, ldbt, ldc = kw + ld_extra[0], kw + ld_extra[1], m + ld_extra[2]
    pa, pb = _pack(a), _pack(bt)
    base = cr.count(a, bt, op) if base is None else base
    _assert_informative(base, n, k, m)
    want = base if seed is None else ((base.astype(np.int64) + seed) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
    want = np.broadcast_to(want, (batch, n, m))
    if poison[0]:
        pa = _poison_padding(pa, k)
    if poison[1]:
        pb = _poison_padding(pb, k)
    sa, sb = _up4((n - 1) * lda + kw + 5), _up4((m - 1) * ldbt + kw + 3)   # batch strides that keep the tile kernel's alignment
    sc = _up4((n - 1) * ldc + m + 3)
    rand = lambda cnt: rng.integers(0, 1 << 32, size=cnt, dtype=np.uint64).astype(np.uint32)   # noqa: E731
    da = Dev(_layout(pa, lda, sa, rand(pa.shape[0] * sa)), shift[0])
    db = Dev(_layout(pb, ldbt, sb, rand(pb.shape[0] * sb)), shift[1])
    c_fill = _pattern(batch * sc, 3)
    c_host = _layout(seed.view(np.uint32), ldc, sc, c_fill) if seed is not None else c_fill.reshape(batch, sc).copy()
    dc = Dev(c_host, shift[2])
    if want_name is not None:
        assert g.kernel_name_bits_count(n, k, m, lda, ldbt, ldc, batch) == want_name
    rc = g.lib().mm_bits_count_launch(0, cr.OPS[op], 0 if null_operands else da.ptr, 0 if null_operands else db.ptr, dc.ptr, n, k, m,
                                      lda, ldbt, ldc, batch, sa if a.shape[0] > 1 else 0, sb if bt.shape[0] > 1 else 0, sc,
                                      int(seed is not None), None)
    assert rc == 0, (rc, g.lib().mm_last_error().decode())
    got = dc.fetch()
    rows = _rows_of(got, n, m, ldc)
    assert np.array_equal(rows.view(np.int32), want), _first_difference(rows.view(np.int32), want, "elements", "")
    assert np.array_equal(got, _layout(rows, ldc, sc, c_fill)), "a gap element of C was written"
    return want


def _operands(n, k, m, rng, batch_a=1, batch_b=1):
    return rng.random((batch_a, n, k)) < 0.5, rng.random((batch_b, m, k)) < 0.5


def _tile_ld(k, m):
    """ld extras with which the tile kernel's rule holds."""
    kw = cr.words(k)
    return (_up4(kw) - kw, _up4(kw) - kw, _up4(m) - m)


# every issue shape, and one K just inside and one just outside the slab of 256 k
SHAPES = [(1, 1, 1), (5, 33, 31), (64, 64, 64), (65, 95, 129), (130, 1, 70), (128, 256, 128), (129, 257, 127), (257, 513, 255),
          (3, 4100, 200), (66, SLAB, 70), (66, SLAB + 1, 70)]


@pytest.mark.parametrize("op", ["And", "Xor"])
@pytest.mark.parametrize("n,k,m", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_count_against_numpy_under_both_kernels(n, k, m, op, knob):
    """The natural ld and an ld the tile kernel's rule accepts, with each kernel forced; the resolver's name asserted."""
    rng = np.random.default_rng(n * 1000003 + k * 1009 + m)
    a, bt = _operands(n, k, m, rng)
    natural_serves = cr.words(k) % 4 == 0 and m % 4 == 0
    base = cr.count(a, bt, op)
    for variant in (0, 1):
        knob("bits_count_variant", variant)
        count(a, bt, op, rng=rng, base=base, want_name="bits_count_tile" if variant and natural_serves else "bits_count_plain")
        count(a, bt, op, rng=rng, base=base, ld_extra=_tile_ld(k, m), want_name="bits_count_tile" if variant else "bits_count_plain")


def test_ld_rule_and_tile_threshold_under_the_default_rule():
    """2 x 32768 outputs are 256 started tiles of 128 x 128: the rule takes the tile kernel where every ld is a multiple of 4
    (extras 0 and 4 on ld = 4, 4, 32768) and the plain one otherwise (extra 1); 255 tiles run the plain kernel."""
    assert g.get_tuning("bits_count_variant") == -1
    rng = np.random.default_rng(11)
    a, bt = _operands(2, 128, 32768, rng)
    for extra, name in ((0, "bits_count_tile"), (1, "bits_count_plain"), (4, "bits_count_tile")):
        for op in ("And", "Xor"):
            count(a, bt, op, rng=rng, ld_extra=(extra, extra, extra), want_name=name)
    for ld_extra, name in (((1, 0, 0), "bits_count_plain"), ((0, 1, 0), "bits_count_plain"), ((0, 0, 1), "bits_count_plain")):
        count(a, bt, "Xor", rng=rng, ld_extra=ld_extra, want_name=name)
    count(a, bt[:, :32640], "And", rng=rng, want_name="bits_count_plain")
    count(a, bt[:, :32641], "And", rng=rng, ld_extra=(0, 0, 3), want_name="bits_count_tile")


@pytest.mark.parametrize("op", ["And", "Xor"])
def test_misaligned_base_is_demoted_silently(op, knob):
    """A base shifted by one word: the resolver still names the tile kernel (shape and ld alone), the launch runs the plain
    one, the values are the same."""
    knob("bits_count_variant", 1)
    rng = np.random.default_rng(12)
    a, bt = _operands(130, 300, 70, rng)
    for shift in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 2, 3)):
        count(a, bt, op, rng=rng, ld_extra=_tile_ld(300, 70), shift=shift, want_name="bits_count_tile")
        seed = rng.integers(-1 << 31, 1 << 31, size=(1, 130, 70)).astype(np.int32)
        count(a, bt, op, seed, rng=rng, ld_extra=_tile_ld(300, 70), shift=shift, want_name="bits_count_tile")


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("op", ["And", "Xor"])
def test_poisoned_padding_never_counts(op, variant, knob):
    """Padding bits all ones in both operands (And counts them unless both are masked; Xor counts them when exactly one is)
    and in one operand alone (Xor counts them unless that one is masked)."""
    knob("bits_count_variant", variant)
    rng = np.random.default_rng(13)
    for n, k, m in ((65, 95, 129), (5, 33, 31), (130, 257, 70), (3, 1, 2)):
        a, bt = _operands(n, k, m, rng)
        for poison in ((True, True), (True, False), (False, True)):
            count(a, bt, op, rng=rng, ld_extra=_tile_ld(k, m), poison=poison)


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("op", ["And", "Xor"])
def test_accumulation_wraps_mod_2_32(op, variant, knob):
    knob("bits_count_variant", variant)
    rng = np.random.default_rng(14)
    for n, k, m in ((65, 95, 129), (130, 600, 70)):
        a, bt = _operands(n, k, m, rng)
        seed = rng.integers(-1 << 31, 1 << 31, size=(1, n, m)).astype(np.int32)
        seed[0, n // 2, m // 2] = 0x7FFFFFFF
        assert (seed < 0).any()
        want = count(a, bt, op, seed, rng=rng, ld_extra=_tile_ld(k, m))
        assert want[0, n // 2, m // 2] < 0                      # the sum went past 2^31 - 1 and wrapped
        count(a, bt, op, seed, rng=rng, ld_extra=(1, 2, 3))


@pytest.mark.parametrize("variant", [0, 1])
def test_batches_broadcasts_and_chunks(variant, knob):
    knob("bits_count_variant", variant)
    rng = np.random.default_rng(15)
    n, k, m = 70, 300, 130
    for op in ("And", "Xor"):
        a1, bt3 = _operands(n, k, m, rng, 1, 3)
        count(a1, bt3, op, rng=rng, ld_extra=_tile_ld(k, m))                     # a shared by the batch
        a3, bt1 = _operands(n, k, m, rng, 3, 1)
        seed = rng.integers(-1 << 31, 1 << 31, size=(3, n, m)).astype(np.int32)
        count(a3, bt1, op, seed, rng=rng, ld_extra=_tile_ld(k, m))               # bt shared by the batch
        count(a3, bt1, op, rng=rng, ld_extra=(1, 0, 1))
    knob("batch_chunk", 2)                                                       # 5 elements: chunks of 2, 2, 1
    a5, bt5 = _operands(n, k, m, rng, 5, 5)
    count(a5, bt5, "Xor", rng=rng, ld_extra=_tile_ld(k, m))
    seed = rng.integers(-1 << 31, 1 << 31, size=(5, n, m)).astype(np.int32)
    count(a5, bt5[:1], "And", seed, rng=rng, ld_extra=_tile_ld(k, m), batch=5)


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("op", ["And", "Xor"])
def test_k_zero_writes_zero_or_keeps_c(op, variant, knob):
    knob("bits_count_variant", variant)
    rng = np.random.default_rng(16)
    a, bt = np.zeros((1, 70, 0), bool), np.zeros((2, 132, 0), bool)
    assert not count(a, bt, op, rng=rng).any()                                   # the plain form: C = 0
    assert not count(a, bt, op, rng=rng, null_operands=True).any()               # a and bt are not read
    seed = rng.integers(-1 << 31, 1 << 31, size=(2, 70, 132)).astype(np.int32)
    assert np.array_equal(count(a, bt, op, seed, rng=rng, null_operands=True), seed)   # accumulating: a no-op


# ---- the torch binding ---------------------------------------------------------------------------------------------------
def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x).view(np.int32) if x.dtype == np.uint32 else np.ascontiguousarray(x)).to("cuda:0")


def test_binding_count_equals_boolean_product_and_xor_identity():
    import torch
    rng = np.random.default_rng(17)
    n, k, m = 67, 200, 133
    a, bt = rng.random((n, k)) < 0.05, rng.random((m, k)) < 0.05                  # sparse: about a third of the counts are 0
    pa, pbt = _dev(cr.pack(a)), _dev(cr.pack(bt))
    c_and = g.bits_matmul_count(pa, pbt, k)
    assert c_and.dtype == torch.int32 and tuple(c_and.shape) == (n, m)
    assert np.array_equal(c_and.cpu().numpy(), cr.count(a, bt, "And"))
    zero = (c_and == 0).float().mean().item()
    assert 0.1 < zero < 0.9, zero
    boolean = g.unpack_bits(g.bits_matmul(pa, g.transpose_bits(pbt, k), k, m), m)
    assert torch.equal(c_and > 0, boolean)
    c_xor = g.bits_matmul_count(pa, pbt, k, op="Xor")
    pop = lambda p, cols: g.unpack_bits(p, cols, dtype=torch.uint8).sum(-1, dtype=torch.int32)   # noqa: E731
    assert torch.equal(c_xor, pop(pa, k)[:, None] + pop(pbt, k)[None, :] - 2 * c_and)
    assert np.array_equal(c_xor.cpu().numpy(), cr.count(a, bt, "Xor"))


def test_binding_strides_batches_and_accumulation():
    import torch
    rng = np.random.default_rng(18)
    n, k, m = 40, 64, 50
    a, bt = rng.random((3, n, 160)) < 0.5, rng.random((m, 160)) < 0.5
    wide_a, wide_bt = _dev(cr.pack(a)), _dev(cr.pack(bt))                         # 5 words per row; words 1..2 are columns 32..95
    sl_a, sl_bt = wide_a[:, :, 1:3], wide_bt[:, 1:3]
    assert sl_a.stride(-2) == 5 and not sl_a.is_contiguous()
    want = cr.count(a[:, :, 32:96], bt[None, :, 32:96], "Xor")
    got = g.bits_matmul_count(sl_a, sl_bt.expand(3, m, 2), k, op="Xor")
    assert tuple(got.shape) == (3, n, m) and np.array_equal(got.cpu().numpy(), want)
    big = torch.full((3, n, 64), 7, dtype=torch.int32, device="cuda:0")
    c = big[:, :, :m]                                                              # a row stride of its own
    assert g.bits_addmm_count_(c, sl_a, sl_bt, k, op="Xor") is c
    assert np.array_equal(c.cpu().numpy(), want + 7) and (big[:, :, m:] == 7).all()
    out = torch.empty((3, n, m), dtype=torch.int32, device="cuda:0")
    assert g.bits_matmul_count(sl_a, sl_bt, 60, out=out) is out                   # k inside the words: the rest is padding
    assert np.array_equal(out.cpu().numpy(), cr.count(a[:, :, 32:92], bt[None, :, 32:92], "And"))


def test_triangle_count_of_a_small_graph():
    import torch
    rng = np.random.default_rng(19)
    n = 90
    upper = np.triu(rng.random((n, n)) < 0.3, 1)
    adj = upper | upper.T
    p = _dev(cr.pack(adj))
    paths = g.bits_matmul_count(p, p, n)                                           # symmetric: A x A^T = A x A
    triangles = (paths * g.unpack_bits(p, n, dtype=torch.uint8).to(torch.int32)).sum().item() / 6
    ai = adj.astype(np.int64)
    want = np.trace(ai @ ai @ ai) / 6
    assert want > 100 and triangles == want


# ---- the packed transpose --------------------------------------------------------------------------------------------------
def transpose(x, *, ld_extra=(0, 0), poison=False, rng=None):
    """mm_bits_transpose_launch on a bool (batch, rows, cols); exact against numpy, the destination's padding 0, gap words
    untouched.  Returns the destination's rows, packed."""
    rng = rng or np.random.default_rng(0)
    batch, rows, cols = x.shape
    cw, rw = cr.words(cols), cr.words(rows)
    ld_src, ld_dst = cw + ld_extra[0], rw + ld_extra[1]
    ps = cr.pack(x)
    if poison:
        ps = _poison_padding(ps, cols)
    ss, sd = (rows - 1) * ld_src + cw + 3, (cols - 1) * ld_dst + rw + 2
    rand = rng.integers(0, 1 << 32, size=batch * ss, dtype=np.uint64).astype(np.uint32)
    src = Dev(_layout(ps, ld_src, ss, rand))
    d_fill = _pattern(batch * sd, 4)
    dst = Dev(d_fill.reshape(batch, sd).copy())
    rc = g.lib().mm_bits_transpose_launch(0, src.ptr, dst.ptr, rows, cols, ld_src, ld_dst, batch, ss, sd, None)
    assert rc == 0, (rc, g.lib().mm_last_error().decode())
    got = dst.fetch()
    out = _rows_of(got, cols, rw, ld_dst)
    assert np.array_equal(out, cr.pack(cr.transpose(x))), "transpose differs (padding bits included)"
    assert np.array_equal(got, _layout(out, ld_dst, sd, d_fill)), "a gap word of the destination was written"
    assert np.array_equal(src.fetch(), _layout(ps, ld_src, ss, rand)), "the source was written"
    return out


T_SHAPES = [(1, 1), (31, 33), (64, 32), (65, 95), (257, 513), (1000, 70)]


@pytest.mark.parametrize("rows,cols", T_SHAPES, ids=["x".join(map(str, s)) for s in T_SHAPES])
def test_transpose_against_numpy(rows, cols):
    rng = np.random.default_rng(rows * 1009 + cols)
    x = rng.random((1, rows, cols)) < 0.5
    transpose(x, rng=rng)
    transpose(x, rng=rng, ld_extra=(1, 4), poison=True)
    transpose(rng.random((3, rows, cols)) < 0.5, rng=rng, ld_extra=(4, 1), poison=True)


def test_transpose_twice_returns_the_source_with_clean_padding():
    import torch
    rng = np.random.default_rng(20)
    x = rng.random((2, 75, 203)) < 0.5
    p = _dev(_poison_padding(cr.pack(x), 203))
    t = g.transpose_bits(p, 203)
    assert tuple(t.shape) == (2, 203, 3) and np.array_equal(t.cpu().numpy().view(np.uint32), cr.pack(cr.transpose(x)))
    back = g.transpose_bits(t, 75)
    assert np.array_equal(back.cpu().numpy().view(np.uint32), cr.pack(x))         # the padding cleared
    out = torch.full((203, 5), -1, dtype=torch.int32, device="cuda:0")
    assert g.transpose_bits(p[1], 203, out=out) is out
    assert np.array_equal(out[:, :3].cpu().numpy().view(np.uint32), cr.pack(cr.transpose(x[1]))) and (out[:, 3:] == -1).all()


# ---- seeded fuzz ---------------------------------------------------------------------------------------------------------
def test_seeded_fuzz_over_both_kernels(knob):
    """40 cases, N, M <= 300, K <= 1200, on both sides of the 64 and 128 tiles and of the slab, random op, ld extras, batch,
    accumulation and kernel."""
    rng = np.random.default_rng(2024)
    edges = [1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300]
    k_edges = [1, 31, 32, 33, 255, 256, 257, 511, 512, 513, 1200]
    for case in range(40):
        n, m = (int(rng.choice(edges)) if rng.random() < 0.5 else int(rng.integers(1, 301)) for _ in range(2))
        k = int(rng.choice(k_edges)) if rng.random() < 0.5 else int(rng.integers(1, 1201))
        op = ("And", "Xor")[int(rng.integers(2))]
        batch = int(rng.choice([1, 1, 2, 3]))
        ba, bb = (batch, batch) if rng.random() < 0.5 else ((1, batch) if rng.random() < 0.5 else (batch, 1))
        a, bt = _operands(n, k, m, rng, ba, bb)
        seed = rng.integers(-1 << 31, 1 << 31, size=(batch, n, m)).astype(np.int32) if rng.random() < 0.5 else None
        ld_extra = _tile_ld(k, m) if rng.random() < 0.5 else tuple(int(v) for v in rng.integers(0, 6, size=3))
        variant = int(rng.integers(2))
        knob("bits_count_variant", variant)
        kw = cr.words(k)
        serves = all(v % 4 == 0 for v in (kw + ld_extra[0], kw + ld_extra[1], m + ld_extra[2]))
        try:
            count(a, bt, op, seed, rng=rng, ld_extra=ld_extra, batch=batch,
                  want_name="bits_count_tile" if variant and serves else "bits_count_plain")
        except AssertionError as e:
            raise AssertionError(f"case {case}: n {n} k {k} m {m} {op} batch {ba},{bb} seed {seed is not None} ld {ld_extra} "
                                 f"variant {variant}: {e}") from e
