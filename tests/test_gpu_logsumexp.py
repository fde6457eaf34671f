"""The log-semiring product on the MI355X (mm_gemm_logsumexp_*): every configuration on both kernels against the numpy
reference (the documented bound for finite outputs, special values exactly), the hybrid's fallback on an adversarial case
the shifted torch pipeline gets wrong, accumulation, batches, determinism, the sandwich maxplus <= lse <= maxplus + log K,
an HMM forward pass and typical-data precision."""
import math

import numpy as np
import pytest

import _lse_ref
import gemm_hls_amd as g

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
    rng = np.random.default_rng(3)
    n, k, m = 256, 128, 256
    a = rng.uniform(-1, 1, size=(n, k))
    b = rng.uniform(-1, 1, size=(k, m))
    a[64:128, : k // 2] = rng.uniform(-0.5, 0.5, size=(64, k // 2))
    a[64:128, k // 2:] = -120 + rng.uniform(-0.5, 0.5, size=(64, k // 2))
    b[: k // 2, 128:192] = -120 + rng.uniform(-0.5, 0.5, size=(k // 2, 64))
    b[k // 2:, 128:192] = rng.uniform(-0.5, 0.5, size=(k // 2, 64))
    sg = -1 if red == "Min" else 1
    return (sg * a).astype(NP[dtype]), (sg * b).astype(NP[dtype])


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
