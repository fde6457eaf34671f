"""The log-semiring product on the MI355X (mm_gemm_logsumexp_*): every configuration on both kernels against the numpy
reference (the documented bound for finite outputs, special values exactly), the hybrid's fallback on an adversarial case
the shifted torch pipeline gets wrong -- alone and inside a batch --, accumulation, batches, chunked batches (by the knob and
by the 256 MiB of workspace), determinism, the sandwich maxplus <= lse <= maxplus + log K, an HMM forward pass and
typical-data precision."""
import ctypes
import math
import time

import numpy as np
import pytest

import _lse_ref
import gemm_hls_amd as g
from _knobs import knob as knobs  # noqa: F401  (the fixture, under the name the tests here use)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"
NP = {"half": np.float16, "float": np.float32, "double": np.float64}
GUARD = 12345.0


@pytest.fixture
def lse_variant():
    old = g.get_tuning("lse_variant")
    yield lambda v: g.set_tuning("lse_variant", v)
    g.set_tuning("lse_variant", old)


def _offset_view(x, shape, off):
    """`x` copied into a fresh device buffer at element offset `off` (element-aligned, not 16-byte aligned)."""
    n = int(np.prod(shape))
    buf = torch.full((n + off + 3,), GUARD, dtype=x.dtype, device=DEV)
    v = buf[off:off + n].view(shape)
    v.copy_(x)
    return buf, v


def _run(a, b, dtype, red, path, transposed=False, seed=None, off=1):
    """C through an offset view with guard elements around it; the guards must survive."""
    at, bt = (torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in (a, b))
    _, av = _offset_view(at, tuple(at.shape), off)
    _, bv = _offset_view(bt, tuple(bt.shape), off + 2)
    n = a.shape[1] if transposed else a.shape[0]
    m = b.shape[1]
    init = torch.from_numpy(seed).to(DEV) if seed is not None else torch.zeros((n, m), dtype=at.dtype, device=DEV)
    cbuf, cv = _offset_view(init, (n, m), off + 1)
    if seed is None:
        g.matmul_logsumexp(av, bv, dtype, red, path, transposed, out=cv)
    else:
        g.addmm_logsumexp_(cv, av, bv, dtype, red, path, transposed)
    torch.cuda.synchronize()
    cb = cbuf.cpu().numpy()
    assert (cb[:off + 1] == GUARD).all() and (cb[off + 1 + n * m:] == GUARD).all(), "a guard element was overwritten"
    return cv.cpu().numpy()


SHAPES = [(1, 1, 1), (37, 70001, 5), (300, 64, 272), (65, 129, 63)]


@pytest.mark.parametrize("path", [g.PATH_AUTO, g.PATH_ORDERED], ids=["auto", "ordered"])
@pytest.mark.parametrize("red", ["Max", "Min"])
@pytest.mark.parametrize("dtype", ["half", "float", "double"])
def test_lse_configs_against_reference(dtype, red, path):
    rng = np.random.default_rng(11)
    for (n, k, m) in SHAPES:
        a = rng.uniform(-8, 8, size=(n, k)).astype(NP[dtype])
        b = rng.uniform(-8, 8, size=(k, m)).astype(NP[dtype])
        c = _run(a, b, dtype, red, path)
        _lse_ref.check(c, _lse_ref.logsumexp_ref(a, b, dtype, red), a, b, dtype, red, what=f"{(n, k, m)}")
    # the K x N A, and special values
    # (the first shape: two tiles each way, a one-line last tile, a one-k last slab whose other 15 k are the staging's fill)
    for n, k, m in [(65, 17, 67), (300, 64, 272)]:
        a = rng.uniform(-8, 8, size=(k, n)).astype(NP[dtype])
        b = rng.uniform(-8, 8, size=(k, m)).astype(NP[dtype])
        c = _run(a, b, dtype, red, path, transposed=True)
        _lse_ref.check(c, _lse_ref.logsumexp_ref(a, b, dtype, red, transposed_a=True), a, b, dtype, red, True, f"K x N A {(n, k, m)}")
        seed = rng.uniform(-8, 8, size=(n, m)).astype(NP[dtype])
        c = _run(a, b, dtype, red, path, transposed=True, seed=seed)
        _lse_ref.check(c, _lse_ref.logsumexp_ref(a, b, dtype, red, seed, True), a, b, dtype, red, True, f"K x N A seeded {(n, k, m)}")
    a = rng.uniform(-8, 8, size=(n, k)).astype(NP[dtype])
    a[3, 5] = np.nan
    a[7, :] = -np.inf
    a[9, 2] = np.inf
    a[11, :] = np.inf
    b[4, 100] = -np.inf
    b[2, 101] = -np.inf       # with a[9, 2]: +inf + -inf, a NaN term
    b[:, 200] = -np.inf
    b[10, 201] = np.inf
    c = _run(a, b, dtype, red, path)
    _lse_ref.check(c, _lse_ref.logsumexp_ref(a, b, dtype, red), a, b, dtype, red, what="special values")


def _adversarial(dtype="float", red="Max"):
    """A row block of A that is [0, -120]-like and a column block of B that is [-120, 0]-like: every term of those outputs
    sits about 120 below ra + rb, where exp underflows f32 to zero (exp(-100) is still a denormal)."""
    return _lse_ref.adversarial(dtype, red, 256, 128, 256, slice(64, 128), slice(128, 192), 120)


def test_lse_hybrid_fallback_fixes_what_the_shifted_pipeline_loses(lse_variant):
    a, b = _adversarial()
    at, bt = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    am, bm = at.max(dim=1, keepdim=True).values, bt.max(dim=0, keepdim=True).values
    shifted = (torch.log(torch.exp(at - am) @ torch.exp(bt - bm)) + am + bm).cpu().numpy()
    ref = _lse_ref.logsumexp_ref(a, b)
    block = (slice(64, 128), slice(128, 192))
    assert np.isfinite(ref[block]).all() and (ref[block] < -110).all()
    assert (shifted[block] == -np.inf).all(), "the shifted pipeline was expected to lose these outputs"
    cfg = g.make_config("float", "Add", "Max")
    assert g.kernel_name_logsumexp(cfg, 256, 128, 256) == "lse_hybrid"
    c = g.matmul_logsumexp(at, bt).cpu().numpy()
    _lse_ref.check(c, ref, a, b, what="hybrid")
    assert np.isfinite(c[block]).all()
    lse_variant(2)   # every tile recomputed by the exact kernel
    c2 = g.matmul_logsumexp(at, bt).cpu().numpy()
    _lse_ref.check(c2, ref, a, b, what="all tiles to the fallback")
    lse_variant(0)
    c0 = g.matmul_logsumexp(at, bt).cpu().numpy()
    assert np.array_equal(c0, c2), "the fallback's tiles are the exact kernel's bits"
    for red in ("Min",):
        a, b = _adversarial(red=red)
        lse_variant(-1)
        c = g.matmul_logsumexp(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV), reduce_op=red).cpu().numpy()
        _lse_ref.check(c, _lse_ref.logsumexp_ref(a, b, "float", red), a, b, "float", red, what="Min hybrid")


@pytest.mark.parametrize("path", [g.PATH_AUTO, g.PATH_ORDERED], ids=["auto", "ordered"])
@pytest.mark.parametrize("dtype", ["float", "double"])
def test_lse_accumulate_k_split_k0_and_neg_inf_seed(dtype, path):
    rng = np.random.default_rng(5)
    n, k, m = 130, 200, 70
    a = rng.uniform(-6, 6, size=(n, k)).astype(NP[dtype])
    b = rng.uniform(-6, 6, size=(k, m)).astype(NP[dtype])
    at, bt = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    whole = g.matmul_logsumexp(at, bt, dtype, "Max", path).cpu().numpy()
    c = torch.full((n, m), -math.inf, dtype=at.dtype, device=DEV)    # a seed of -inf adds nothing
    g.addmm_logsumexp_(c, at[:, :120].contiguous(), bt[:120], dtype, "Max", path)
    g.addmm_logsumexp_(c, at[:, 120:].contiguous(), bt[120:], dtype, "Max", path)
    ref = _lse_ref.logsumexp_ref(a, b, dtype)
    _lse_ref.check(whole, ref, a, b, dtype, what="one call")
    _lse_ref.check(c.cpu().numpy(), ref, a, b, dtype, what="K split")
    before = c.clone()
    g.addmm_logsumexp_(c, at[:, :0], bt[:0], dtype, "Max", path)      # K = 0: a no-op
    assert torch.equal(before, c)


def test_lse_batched_broadcast_position_and_determinism():
    rng = np.random.default_rng(9)
    batch, n, k, m = 6, 70, 96, 66
    a = torch.from_numpy(rng.uniform(-5, 5, size=(batch, n, k)).astype(np.float32)).to(DEV)
    b = torch.from_numpy(rng.uniform(-5, 5, size=(batch, k, m)).astype(np.float32)).to(DEV)
    c = g.matmul_logsumexp(a, b)
    assert torch.equal(c, g.matmul_logsumexp(a, b)), "two runs differ"
    for e in range(batch):
        single = g.matmul_logsumexp(a[e], b[e]).cpu().numpy()
        ref = _lse_ref.logsumexp_ref(a[e].cpu().numpy(), b[e].cpu().numpy())
        _lse_ref.check(c[e].cpu().numpy(), ref, a[e].cpu().numpy(), b[e].cpu().numpy(), what=f"element {e}")
        _lse_ref.check(single, ref, a[e].cpu().numpy(), b[e].cpu().numpy(), what=f"single {e}")
    # bits independent of position and of the other elements
    perm = torch.tensor([3, 0, 5, 1, 4, 2])
    cp = g.matmul_logsumexp(a[perm].contiguous(), b[perm].contiguous())
    assert torch.equal(cp, c[perm])
    other = a.clone()
    other[1:] = torch.from_numpy(rng.uniform(-50, 50, size=(batch - 1, n, k)).astype(np.float32)).to(DEV)
    assert torch.equal(g.matmul_logsumexp(other, b)[0], c[0])
    # broadcast A and B (batch stride 0)
    ab = g.matmul_logsumexp(a[0:1].expand(batch, n, k), b)
    bb = g.matmul_logsumexp(a, b[0:1].expand(batch, k, m))
    assert torch.equal(ab, g.matmul_logsumexp(a[0:1].expand(batch, n, k).contiguous(), b))
    assert torch.equal(bb, g.matmul_logsumexp(a, b[0:1].expand(batch, k, m).contiguous()))


@pytest.mark.parametrize("red", ["Max", "Min"])
def test_lse_sandwich_between_tropical_products(red):
    rng = np.random.default_rng(13)
    n, k, m = 200, 300, 180
    a = torch.from_numpy(rng.uniform(-20, 20, size=(n, k)).astype(np.float32)).to(DEV)
    b = torch.from_numpy(rng.uniform(-20, 20, size=(k, m)).astype(np.float32)).to(DEV)
    trop = g.matmul(a, b, "float", "Add", red).double()
    lse = g.matmul_logsumexp(a, b, "float", red).double()
    slack = 1e-4 * (1 + trop.abs())
    if red == "Max":
        assert (trop <= lse + slack).all() and (lse <= trop + math.log(k) + slack).all()
    else:
        assert (trop - math.log(k) - slack <= lse).all() and (lse <= trop + slack).all()


def test_lse_hmm_forward_algorithm():
    rng = np.random.default_rng(21)
    seqs, states, steps, symbols = 64, 512, 50, 16
    log_t = np.log(rng.dirichlet(np.ones(states) * 0.5, size=states)).astype(np.float32)      # (from, to)
    log_e = np.log(rng.dirichlet(np.ones(symbols), size=states)).astype(np.float32)          # (state, symbol)
    log_pi = np.log(rng.dirichlet(np.ones(states))).astype(np.float32)
    obs = rng.integers(0, symbols, size=(seqs, steps))
    lt, le = torch.from_numpy(log_t).to(DEV), torch.from_numpy(log_e).to(DEV)
    alpha = (torch.from_numpy(log_pi).to(DEV)[None, :] + le[:, torch.from_numpy(obs[:, 0]).to(DEV)].T).contiguous()
    for t in range(1, steps):
        alpha = g.matmul_logsumexp(alpha, lt) + le[:, torch.from_numpy(obs[:, t]).to(DEV)].T
    ll = torch.logsumexp(alpha, dim=1).cpu().numpy().astype(np.float64)
    # float64 numpy forward pass
    T64, E64 = log_t.astype(np.float64), log_e.astype(np.float64)
    al = log_pi.astype(np.float64)[None, :] + E64[:, obs[:, 0]].T
    for t in range(1, steps):
        mx = al.max(axis=1, keepdims=True)
        al = np.log(np.exp(al - mx) @ np.exp(T64)) + mx + E64[:, obs[:, t]].T
    want = np.log(np.exp(al - al.max(axis=1, keepdims=True)).sum(axis=1)) + al.max(axis=1)
    assert np.all(np.abs(ll - want) <= 1e-5 * np.abs(want) + 1e-3), np.abs(ll - want).max()


@pytest.mark.parametrize("path", [g.PATH_AUTO, g.PATH_ORDERED], ids=["auto", "ordered"])
def test_lse_typical_data_precision(path):
    rng = np.random.default_rng(17)
    n, k, m = 64, 4096, 64
    a = rng.uniform(-4, 4, size=(n, k)).astype(np.float32)
    b = rng.uniform(-4, 4, size=(k, m)).astype(np.float32)
    c = g.matmul_logsumexp(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV), path=path).cpu().numpy()
    ref = _lse_ref.logsumexp_ref(a, b)
    err = _lse_ref.check(c, ref, a, b, what="typical")
    assert err <= 2.0 ** -14, err


# ---- the fallback inside a batch, and batches that run as several chunks ------------------------------------------------------
C_GUARD = 64   # elements of pattern before the first and after the last C of a batch


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint8)


def run_batch(d, dtype, red, nt=False, path=g.PATH_AUTO, kxn=False, seeded=False, pad_c=0, share=None, a="a"):
    """C (batch, N, M) of the batched call on _lse_ref.fallback_batch()'s operands (`a`: which of its A), under whatever the
    knobs hold.  nt: B handed over as materialised b.mT to the A x B^T call; kxn: A as materialised a.mT with transposed_a;
    share: "a" (A of element 1) or "b" (B of element 4) broadcast with batch stride 0; seeded: accumulate onto d["seed"]; pad_c:
    elements between one C and the next.  C lives in a buffer of finite pattern values that must come back untouched in the
    guards and in the gaps; a plain call starts on the pattern too, and has to overwrite all of it."""
    batch, (n, k, m) = _lse_ref.FB_BATCH, _lse_ref.FB_SHAPE
    ta, tb = torch.tensor(d[a], device=DEV), torch.tensor(d["b"], device=DEV)    # (the shared arrays are read-only: copies)
    if kxn:
        ta = ta.mT.contiguous()
    if nt:
        tb = tb.mT.contiguous()
    if share == "a":
        ta = ta[1:2].expand(batch, *ta.shape[1:])
    if share == "b":
        tb = tb[4:5].expand(batch, *tb.shape[1:])
    sc = n * m + pad_c
    total = 2 * C_GUARD + (batch - 1) * sc + n * m
    pattern = (1000 + np.arange(total) % 251).astype(NP[dtype])    # whole numbers below 2048: exact in half
    buf = torch.from_numpy(pattern).to(DEV)
    c = torch.as_strided(buf, (batch, n, m), (sc, m, 1), C_GUARD)
    if seeded:
        c.copy_(torch.tensor(d["seed"], device=DEV))
        if nt:
            g.addmm_logsumexp_nt_(c, ta, tb, dtype, red, path)
        else:
            g.addmm_logsumexp_(c, ta, tb, dtype, red, path, kxn)
    elif pad_c == 0:
        if nt:
            g.matmul_logsumexp_nt(ta, tb, dtype, red, path, out=c)
        else:
            g.matmul_logsumexp(ta, tb, dtype, red, path, kxn, out=c)
    else:   # a pure-output C with a padded batch stride: the C ABI takes it, the torch wrappers' `out` does not
        fn = g.lib().mm_gemm_logsumexp_nt_enqueue if nt else g.lib().mm_gemm_logsumexp_enqueue
        cfg = g.make_config(dtype, "Add", red, path, kxn)
        rc = fn(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), ctypes.byref(cfg), ta.data_ptr(), tb.data_ptr(),
                c.data_ptr(), n, k, m, batch, ta.stride(0), tb.stride(0), sc, 0)
        assert rc == 0, (rc, g.lib().mm_last_error().decode())
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    inside = np.zeros(total, dtype=bool)
    for e in range(batch):
        inside[C_GUARD + e * sc:C_GUARD + e * sc + n * m] = True
    assert np.array_equal(_bits(got[~inside]), _bits(pattern[~inside])), "a guard or a gap between two C was overwritten"
    return np.stack([got[C_GUARD + e * sc:C_GUARD + e * sc + n * m].reshape(n, m) for e in range(batch)])


FB_FORMS = {   # form -> (run_batch arguments, the reference)
    "plain": ({}, "ref"),
    "kxn_a": (dict(kxn=True), "ref"),
    "seeded": (dict(seeded=True), "ref_seeded"),
    "seeded_padded_c": (dict(seeded=True, pad_c=64), "ref_seeded"),
    "special_values": (dict(a="a_special"), "ref_special"),
}


def check_fallback_inside_a_batch(dtype, red, form, knobs, nt=False):
    """The hybrid on fallback_batch(), debug_poison = 1: every element within the bound of its own reference, the adversarial
    blocks finite, their tiles bit for bit lse_variant = 0's (the exact kernel's), lse_variant = 2 all of lse_variant = 0's,
    and -- float and double -- each benign element NOT lse_variant = 0's bits.  Without the last the equalities would say
    nothing: a flag index without its element term leaves the flags of elements 1.. unwritten, which under debug_poison sends
    all their tiles to the exact kernel."""
    d = _lse_ref.fallback_batch(dtype, red)
    kw, which = FB_FORMS[form]
    kw = dict(kw, nt=nt)
    a, ref = d[kw.get("a", "a")], d[which]
    n, k, m = _lse_ref.FB_SHAPE
    name = g.kernel_name_logsumexp_nt if nt else g.kernel_name_logsumexp
    knobs("debug_poison", 1)
    knobs("lse_variant", -1)
    assert name(g.make_config(dtype, "Add", red), n, k, m, _lse_ref.FB_BATCH) == ("lse_hybrid_nt" if nt else "lse_hybrid")
    c = run_batch(d, dtype, red, **kw)
    knobs("lse_variant", 0)
    c0 = run_batch(d, dtype, red, **kw)
    for e in range(_lse_ref.FB_BATCH):
        _lse_ref.check(c[e], ref[e], a[e], d["b"][e], dtype, red, what=f"{form}: element {e}")
        _lse_ref.check(c0[e], ref[e], a[e], d["b"][e], dtype, red, what=f"{form}: exact, element {e}")
    for e, block in _lse_ref.FB_BLOCKS.items():
        assert np.isfinite(c[e][block]).all(), f"element {e}: the adversarial block"
        tile = _lse_ref.FB_TILES[e]
        assert np.array_equal(_bits(c[e][tile]), _bits(c0[e][tile])), f"element {e}: the flagged tiles are the exact kernel's bits"
    if form == "special_values":
        nan, inf = np.isnan(c), np.isinf(c)
        want_nan, want_inf = np.zeros_like(nan), np.zeros_like(inf)
        want_nan[_lse_ref.FB_NAN[0], _lse_ref.FB_NAN[1], :] = True
        want_inf[_lse_ref.FB_INF_ROW[0], _lse_ref.FB_INF_ROW[1], :] = True
        assert np.array_equal(nan, want_nan) and np.array_equal(inf, want_inf), "NaN / inf outside the row that has to hold them"
        assert (c[_lse_ref.FB_INF_ROW] == (np.inf if red == "Min" else -np.inf)).all()
    for e in sorted(set(range(_lse_ref.FB_BATCH)) - set(_lse_ref.FB_BLOCKS)):
        print(f"{dtype} {red} {form} element {e}: {int((c[e] != c0[e]).sum())} outputs differ between the hybrid and the exact kernel")
        # (half: the two kernels' f32 results round to the same binary16 nearly everywhere -- 0 to 2 of an element's 26 000
        # outputs differ on this data -- so half says nothing here; float and double differ in over 10 000 of them)
        if dtype != "half":
            assert not np.array_equal(_bits(c[e]), _bits(c0[e])), f"benign element {e} carries the exact kernel's bits: was it flagged?"
    knobs("lse_variant", 2)
    c2 = run_batch(d, dtype, red, **kw)
    assert np.array_equal(_bits(c2), _bits(c0)), "every tile through the fallback: the exact kernel's bits"


def fallback_cases(nt):
    return [(dtype, red, form) for form in FB_FORMS for dtype in ("half", "float", "double") for red in ("Max", "Min")
            if not (form == "kxn_a" and (nt or dtype == "half"))]


@pytest.mark.parametrize("dtype,red,form", fallback_cases(nt=False))
def test_lse_fallback_inside_a_batch(dtype, red, form, knobs):
    check_fallback_inside_a_batch(dtype, red, form, knobs)


ARRANGEMENTS = {"per-element": {}, "A broadcast": dict(share="a"), "B broadcast": dict(share="b"),
                "padded stride_c": dict(pad_c=64)}


def check_chunks_by_the_knob(dtype, red, knobs, nt=False):
    """batch_chunk = 2 (2 + 2 + 1: the adversarial elements in chunks 0 and 2, a one-element last chunk) and 1 against the
    whole batch in one go, debug_poison = 1: the same bits, guards and gaps intact (run_batch).  Bits, not the bound: a flag
    left by an earlier chunk would send a later chunk's tile to the exact kernel, whose answer is within the bound too.
    MM_PATH_ORDERED is the exact kernel's own chunk loop."""
    d = _lse_ref.fallback_batch(dtype, red)
    knobs("debug_poison", 1)
    knobs("lse_variant", -1)
    for path in (g.PATH_AUTO, g.PATH_ORDERED):
        for seeded in (False, True):
            ref = d["ref_seeded" if seeded else "ref"]
            for what, kw in ARRANGEMENTS.items():
                kw = dict(kw, nt=nt, path=path, seeded=seeded)
                knobs("batch_chunk", -1)
                whole = run_batch(d, dtype, red, **kw)
                # the element whose own operands a broadcast leaves in place (all of them without one) has its reference
                for e in {"a": [1], "b": [4]}.get(kw.get("share"), range(_lse_ref.FB_BATCH)):
                    _lse_ref.check(whole[e], ref[e], d["a"][e], d["b"][e], dtype, red, what=f"{what}: element {e}")
                for chunk in (2, 1):
                    knobs("batch_chunk", chunk)
                    got = run_batch(d, dtype, red, **kw)
                    assert np.array_equal(_bits(got), _bits(whole)), (what, "seeded" if seeded else "plain", path, chunk)


@pytest.mark.parametrize("red", ["Max", "Min"])
@pytest.mark.parametrize("dtype", ["half", "float", "double"])
def test_lse_batch_chunks_by_the_knob_keep_every_bit(dtype, red, knobs):
    check_chunks_by_the_knob(dtype, red, knobs)


def test_lse_second_workspace_chunk_equals_the_first_period(knobs):
    """dispatch_lse_hybrid's second chunk, reached by the 256 MiB of workspace alone (e0 > 0: the offsets of A, B and C, the
    flag block, EA / EB / S written a second time).  float 128 x 128 x 128: per element the workspace holds EA, EB and S
    (3 x 16384 f32), two 128-entry maxima and 4 flags, 4 (3 * 16384 + 2 * 128) + 4 * 4 = 197 648 bytes, so a chunk is
    2^28 // 197 648 = 1358 elements and 1365 run as 1358 + 7.  The batch is base[e % 7], so every output has to be the bits
    of the element one period earlier; base 3 is adversarial, so both chunks hold flagged tiles (elements 3 and 1361)."""
    n = k = m = 128
    batch, period = 1365, 7
    assert (1 << 28) // (4 * (3 * n * n + 2 * n) + 4 * 4) == 1358 < batch and batch % period == 0
    rng = np.random.default_rng(43)
    a = rng.uniform(-5, 5, size=(period, n, k)).astype(np.float32)
    b = rng.uniform(-5, 5, size=(period, k, m)).astype(np.float32)
    block = (slice(64, 128), slice(0, 64))
    a[3], b[3] = _lse_ref.adversarial("float", "Max", n, k, m, *block, 120, seed=44, spread=5.0)
    assert g.kernel_name_logsumexp(g.make_config("float", "Add", "Max"), n, k, m, batch) == "lse_hybrid"
    index = torch.arange(batch, device=DEV) % period
    ta, tb = torch.from_numpy(a).to(DEV)[index], torch.from_numpy(b).to(DEV)[index]      # gathered on the device
    knobs("debug_poison", 1)
    knobs("lse_variant", -1)
    knobs("batch_chunk", -1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    c = g.matmul_logsumexp(ta, tb)
    torch.cuda.synchronize()
    print(f"hybrid, {batch} x {n}^3 in two workspace chunks: {time.perf_counter() - t0:.3f} s")
    first = c[:period].clone()
    assert torch.equal(c.view(torch.int32).view(batch // period, period, n, m),
                       first.view(torch.int32).expand(batch // period, period, n, m)), "an element differs from its base's first"
    knobs("lse_variant", 0)
    exact = g.matmul_logsumexp(ta[:period], tb[:period]).cpu().numpy()
    first = first.cpu().numpy()
    for e in range(period):
        _lse_ref.check(first[e], _lse_ref.logsumexp_ref(a[e], b[e]), a[e], b[e], what=f"base {e}")
        # (the flags again: a benign element on the exact kernel's bits would have been flagged)
        assert (e == 3) or not np.array_equal(_bits(first[e]), _bits(exact[e])), f"base {e} carries the exact kernel's bits"
    assert np.isfinite(first[3][block]).all() and np.array_equal(_bits(first[3][block]), _bits(exact[3][block]))
