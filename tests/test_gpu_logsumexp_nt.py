"""The log-semiring product over an M x K B on the MI355X (mm_gemm_logsumexp_nt_*, matmul_logsumexp_nt /
addmm_logsumexp_nt_): every configuration on both kernels against the numpy reference on bt.T (the header's bound for finite
outputs, special values exactly), equality with the row-major call on a materialised transpose, the hybrid's fallback --
alone and inside a batch --, accumulation, batches, batches chunked by the knob, determinism, and a Viterbi decoder and a forward pass over a "to-state major" transition matrix."""
import math

import numpy as np
import pytest

import _lse_ref
import gemm_hls_amd as g
import test_gpu_logsumexp as rm

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = rm.DEV
NP = rm.NP
GUARD = rm.GUARD
knobs = rm.knobs    # the fixture: set(name, value), every knob put back


@pytest.fixture
def lse_variant():
    old = g.get_tuning("lse_variant")
    yield lambda v: g.set_tuning("lse_variant", v)
    g.set_tuning("lse_variant", old)


def _run(a, bt, dtype, red, path, seed=None, off=1):
    """C of the A x B^T call through offset views (element-aligned, not 16-byte aligned) with guard elements around C; the
    guards must survive."""
    at, btt = (torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in (a, bt))
    _, av = rm._offset_view(at, tuple(at.shape), off)
    _, bv = rm._offset_view(btt, tuple(btt.shape), off + 2)
    n, m = a.shape[0], bt.shape[0]
    init = torch.from_numpy(seed).to(DEV) if seed is not None else torch.zeros((n, m), dtype=at.dtype, device=DEV)
    cbuf, cv = rm._offset_view(init, (n, m), off + 1)
    if seed is None:
        g.matmul_logsumexp_nt(av, bv, dtype, red, path, out=cv)
    else:
        g.addmm_logsumexp_nt_(cv, av, bv, dtype, red, path)
    torch.cuda.synchronize()
    cb = cbuf.cpu().numpy()
    assert (cb[:off + 1] == GUARD).all() and (cb[off + 1 + n * m:] == GUARD).all(), "a guard element was overwritten"
    return cv.cpu().numpy()


def _pair(rng, n, k, m, dtype, lo=-8, hi=8):
    return rng.uniform(lo, hi, size=(n, k)).astype(NP[dtype]), rng.uniform(lo, hi, size=(m, k)).astype(NP[dtype])


def _dev(*xs):
    return [torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in xs]


def _same_numbers(x, y):
    """Equal as numbers, NaN in the same places (the sign of a zero may differ)."""
    return np.array_equal(np.isnan(x), np.isnan(y)) and np.array_equal(x[~np.isnan(x)], y[~np.isnan(y)])


SHAPES = [(1, 1, 1), (300, 64, 272), (65, 129, 63), (37, 4099, 5), (65, 17, 67)]


@pytest.mark.parametrize("path", [g.PATH_AUTO, g.PATH_ORDERED], ids=["auto", "ordered"])
@pytest.mark.parametrize("red", ["Max", "Min"])
@pytest.mark.parametrize("dtype", ["half", "float", "double"])
def test_lse_nt_configs_against_reference_and_the_row_major_call(dtype, red, path):
    rng = np.random.default_rng(11)
    cfg = g.make_config(dtype, "Add", red, path)
    assert g.kernel_name_logsumexp_nt(cfg, 1, 1, 1) == ("lse_hybrid_nt" if path == g.PATH_AUTO else "lse_exact_nt")
    for (n, k, m) in SHAPES:
        a, bt = _pair(rng, n, k, m, dtype)
        c = _run(a, bt, dtype, red, path)
        _lse_ref.check(c, _lse_ref.logsumexp_ref(a, bt.T, dtype, red), a, bt.T, dtype, red, what=f"{(n, k, m)}")
        ta, tb = _dev(a, bt)
        row_major = g.matmul_logsumexp(ta, tb.mT.contiguous(), dtype, red, path).cpu().numpy()
        if path == g.PATH_ORDERED:   # the same per-output sequence: the same bits
            assert np.array_equal(c.view(np.uint8), row_major.view(np.uint8)), (n, k, m)
        else:
            assert _same_numbers(c, row_major), (n, k, m)


@pytest.mark.parametrize("path", [g.PATH_AUTO, g.PATH_ORDERED], ids=["auto", "ordered"])
@pytest.mark.parametrize("red", ["Max", "Min"])
@pytest.mark.parametrize("dtype", ["half", "float", "double"])
def test_lse_nt_special_values(dtype, red, path):
    """A NaN operand, +inf + -inf pairs, an all -inf row (Max) / all +inf row (Min), and their mirror images: torch.logsumexp
    over the terms, exactly (what _lse_ref.check asks of every non-finite reference value)."""
    rng = np.random.default_rng(12)
    n, k, m = 300, 64, 272
    a, bt = _pair(rng, n, k, m, dtype)
    a[3, 5] = np.nan
    a[7, :] = -np.inf
    a[9, 2] = np.inf
    a[11, :] = np.inf
    bt[100, 4] = -np.inf
    bt[101, 2] = -np.inf      # with a[9, 2]: +inf + -inf, a NaN term
    bt[200, :] = -np.inf
    bt[201, 10] = np.inf
    bt[202, :] = np.inf
    bt[203, 7] = np.nan
    c = _run(a, bt, dtype, red, path)
    ref = _lse_ref.logsumexp_ref(a, bt.T, dtype, red)
    assert np.isnan(ref).any() and (ref == np.inf).any() and (ref == -np.inf).any()
    _lse_ref.check(c, ref, a, bt.T, dtype, red, what="special values")
    ta, tb = _dev(a, bt)
    assert _same_numbers(c, g.matmul_logsumexp(ta, tb.mT.contiguous(), dtype, red, path).cpu().numpy())


def test_lse_nt_hybrid_fallback(lse_variant):
    rng = np.random.default_rng(13)
    a, bt = _pair(rng, 300, 64, 272, "float")
    ta, tb = _dev(a, bt)
    lse_variant(2)   # every tile through the fallback
    assert g.kernel_name_logsumexp_nt(g.make_config("float", "Add", "Max"), 300, 64, 272) == "lse_hybrid_nt"
    c2 = g.matmul_logsumexp_nt(ta, tb).cpu().numpy()
    lse_variant(0)
    assert g.kernel_name_logsumexp_nt(g.make_config("float", "Add", "Max"), 300, 64, 272) == "lse_exact_nt"
    c0 = g.matmul_logsumexp_nt(ta, tb).cpu().numpy()
    assert np.array_equal(c0.view(np.uint8), c2.view(np.uint8)), "the fallback's tiles are the exact kernel's bits"
    # outputs whose every term underflows in the shifted product: the flagged tiles get the exact kernel's answer
    for red in ("Max", "Min"):
        a, b = rm._adversarial(red=red)
        ta, tb = _dev(a, b.T)
        ref = _lse_ref.logsumexp_ref(a, b, "float", red)
        block = (slice(64, 128), slice(128, 192))
        assert np.isfinite(ref[block]).all() and (np.abs(ref[block]) > 110).all()
        lse_variant(1)
        c1 = g.matmul_logsumexp_nt(ta, tb, reduce_op=red).cpu().numpy()
        _lse_ref.check(c1, ref, a, b, "float", red, what=f"hybrid {red}")
        lse_variant(0)
        c0 = g.matmul_logsumexp_nt(ta, tb, reduce_op=red).cpu().numpy()
        assert np.array_equal(c1[block].view(np.uint8), c0[block].view(np.uint8)), "the flagged tile is the exact kernel's"


@pytest.mark.parametrize("dtype,red,form", rm.fallback_cases(nt=True))
def test_lse_nt_fallback_inside_a_batch(dtype, red, form, knobs):
    """test_gpu_logsumexp.py's batch of five with two adversarial elements, B handed over as materialised b.mT: "lse_hybrid_nt",
    whose exact kernel reads an M x K B with a batch stride."""
    rm.check_fallback_inside_a_batch(dtype, red, form, knobs, nt=True)


@pytest.mark.parametrize("red", ["Max", "Min"])
@pytest.mark.parametrize("dtype", ["half", "float", "double"])
def test_lse_nt_batch_chunks_by_the_knob_keep_every_bit(dtype, red, knobs):
    rm.check_chunks_by_the_knob(dtype, red, knobs, nt=True)


@pytest.mark.parametrize("path", [g.PATH_AUTO, g.PATH_ORDERED], ids=["auto", "ordered"])
@pytest.mark.parametrize("dtype", ["float", "double"])
def test_lse_nt_accumulate_k_split_k0_and_neg_inf_seed(dtype, path):
    rng = np.random.default_rng(5)
    n, k, m = 130, 200, 70
    a, bt = _pair(rng, n, k, m, dtype, -6, 6)
    ta, tb = _dev(a, bt)
    ref = _lse_ref.logsumexp_ref(a, bt.T, dtype)
    whole = g.matmul_logsumexp_nt(ta, tb, dtype, "Max", path)
    _lse_ref.check(whole.cpu().numpy(), ref, a, bt.T, dtype, what="one call")
    c = torch.full((n, m), -math.inf, dtype=ta.dtype, device=DEV)
    g.addmm_logsumexp_nt_(c, ta, tb, dtype, "Max", path)
    assert torch.equal(c, whole), "a seed of -inf adds nothing"
    c = torch.full((n, m), -math.inf, dtype=ta.dtype, device=DEV)
    g.addmm_logsumexp_nt_(c, ta[:, :120].contiguous(), tb[:, :120].contiguous(), dtype, "Max", path)
    g.addmm_logsumexp_nt_(c, ta[:, 120:].contiguous(), tb[:, 120:].contiguous(), dtype, "Max", path)
    _lse_ref.check(c.cpu().numpy(), ref, a, bt.T, dtype, what="K split")
    before = c.clone()
    g.addmm_logsumexp_nt_(c, ta[:, :0], tb[:, :0], dtype, "Max", path)      # K = 0: a no-op
    assert torch.equal(before, c)


def test_lse_nt_batched_broadcast_position_and_determinism():
    rng = np.random.default_rng(9)
    batch, n, k, m = 4, 70, 96, 66
    a = torch.from_numpy(rng.uniform(-5, 5, size=(batch, n, k)).astype(np.float32)).to(DEV)
    bt = torch.from_numpy(rng.uniform(-5, 5, size=(m, k)).astype(np.float32)).to(DEV)
    c = g.matmul_logsumexp_nt(a, bt.expand(batch, m, k))                     # a broadcast Bt (batch stride 0)
    assert torch.equal(c, g.matmul_logsumexp_nt(a, bt.expand(batch, m, k))), "two runs differ"
    assert torch.equal(c, g.matmul_logsumexp_nt(a, bt.expand(batch, m, k).contiguous()))
    ref_b = bt.cpu().numpy().T
    for e in range(batch):
        ae = a[e].cpu().numpy()
        _lse_ref.check(c[e].cpu().numpy(), _lse_ref.logsumexp_ref(ae, ref_b), ae, ref_b, what=f"element {e}")
        assert torch.equal(g.matmul_logsumexp_nt(a[e], bt), c[e]), "an element's bits depend on its position"
    perm = torch.tensor([3, 0, 1, 2])
    assert torch.equal(g.matmul_logsumexp_nt(a[perm].contiguous(), bt), c[perm])


def test_viterbi_and_forward_over_a_to_state_major_transition_matrix():
    """S = 40 states, T = 12 steps, 5 sequences as the rows of A; trans[j, i] = the score of i -> j, so row j of the matrix
    holds everything state j needs: no transposed copy anywhere.  Viterbi: matmul_argreduce_nt (Add, Max) per step plus the
    emission add in torch, then backtracking over the returned indices, against numpy's best path and score (scores are
    small integers in float, so the sums are exact and np.argmax's first maximum is the contract's smallest k).  Forward:
    matmul_logsumexp_nt per step against a float64 numpy forward pass, within the header's bound accumulated over T."""
    rng = np.random.default_rng(29)
    states, steps, seqs = 40, 12, 5
    trans_to = rng.integers(-8, 1, size=(states, states)).astype(np.float32)      # [to, from]
    emit = rng.integers(-6, 1, size=(steps, seqs, states)).astype(np.float32)
    tt, = _dev(trans_to)
    delta = torch.from_numpy(emit[0]).to(DEV)
    backs = []
    for t in range(1, steps):
        vals, idx = g.matmul_argreduce_nt(delta, tt, "float", "Add", "Max")
        backs.append(idx.cpu().numpy())
        delta = vals + torch.from_numpy(emit[t]).to(DEV)
    d = emit[0].copy()
    ref_backs = []
    for t in range(1, steps):
        cand = d[:, :, None] + trans_to.T[None, :, :]                              # [seq, from, to]
        ref_backs.append(np.argmax(cand, axis=1).astype(np.int32))
        d = cand.max(axis=1) + emit[t]
    assert np.array_equal(delta.cpu().numpy(), d), "best scores"

    def backtrack(bp):
        path = [d.argmax(axis=1)]
        for b in reversed(bp):
            path.append(b[np.arange(seqs), path[-1]])
        return np.array(path[::-1])
    assert np.array_equal(backtrack(backs), backtrack(ref_backs)), "best paths"

    # the forward pass: log-likelihoods of the same chains under the log semiring
    log_t = np.log(rng.dirichlet(np.ones(states) * 0.5, size=states)).astype(np.float32).T.copy()   # [to, from], columns normalised
    log_e = np.log(rng.uniform(0.05, 1.0, size=(steps, seqs, states))).astype(np.float32)
    lt, = _dev(log_t)
    alpha = torch.from_numpy(log_e[0]).to(DEV)
    al = log_e[0].astype(np.float64)
    bound = 0.0
    for t in range(1, steps):
        step = g.matmul_logsumexp_nt(alpha, lt)
        prev = alpha.cpu().numpy()
        bound += float(_lse_ref.bound(prev, log_t.T, _lse_ref.logsumexp_ref(prev, log_t.T)).max()) + 2.0 ** -22 * 64
        alpha = step + torch.from_numpy(log_e[t]).to(DEV)
        al = _lse_ref.lse_terms(al[:, :, None] + log_t.T.astype(np.float64)[None, :, :], 1) + log_e[t].astype(np.float64)
    ll = torch.logsumexp(alpha.double(), dim=1).cpu().numpy()
    want = _lse_ref.lse_terms(al, 1)
    assert np.all(np.abs(ll - want) <= bound), (np.abs(ll - want).max(), bound)
