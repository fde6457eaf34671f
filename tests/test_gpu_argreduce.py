"""GPU tests of argmin / argmax (mm_gemm_argreduce_*, matmul_argreduce / addmm_argreduce_): a Min- or Max-reduced product that
also returns the k that produced each output.  The oracle is the contract's loop (include/mm_gemm.h) written in numpy on
_semiring_ref's operators:
    acc = seed or identity; idx = seed index or -1
    for k ascending: s = Map(a, b); if (Min: s < acc / Max: acc < s): acc = s; idx = index_base + k"""
import ctypes
import zlib

import numpy as np
import pytest

import _semiring_ref as sr
import gemm_hls_amd as g
from _product_ref import oracle

pytestmark = pytest.mark.gpu

GUARD = 64   # elements of guard pattern on each side of C and of I
REDUCTIONS = ("Min", "Max")
ARG_CONFIGS = [(d, mp, rd) for d in sr.DTYPES for mp in sr.OPS for rd in REDUCTIONS]   # 11 x 5 x 2 = 110


def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x).reshape(-1).view(np.uint8).copy()).to("cuda:0")


def _guarded(x):
    pattern = (np.arange(GUARD * x.dtype.itemsize) % 251 + 1).astype(np.uint8).view(x.dtype)
    return np.concatenate([pattern, x.reshape(-1), pattern]), pattern


def argreduce(cfg, a, b, n, k, m, batch=1, sa=0, sb=0, sc=None, c0=None, i0=None, index_base=0, c_offset=0, i_offset=0):
    """The blocking launch on host arrays, C and I inside guarded buffers (checked); returns (C flat, I flat).  c_offset /
    i_offset move C's / I's base by that many elements (a pointer that is not 16-byte aligned)."""
    t = a.dtype
    sc = n * m if sc is None else sc
    size = (batch - 1) * sc + n * m
    c = np.zeros(size, dtype=t) if c0 is None else np.asarray(c0, dtype=t).reshape(-1)
    i = np.full(size, 7, dtype=np.int32) if i0 is None else np.asarray(i0, dtype=np.int32).reshape(-1)
    cbuf, cpat = _guarded(np.concatenate([np.zeros(c_offset, dtype=t), c]))
    ibuf, ipat = _guarded(np.concatenate([np.zeros(i_offset, dtype=np.int32), i]))
    da, db, dc, di = _dev(a), _dev(b), _dev(cbuf), _dev(ibuf)
    cp = dc.data_ptr() + (GUARD + c_offset) * t.itemsize
    rc = g.lib().mm_gemm_argreduce_launch(0, ctypes.byref(cfg), da.data_ptr(), db.data_ptr(), cp,
                                          di.data_ptr() + (GUARD + i_offset) * 4, n, k, m, batch, sa, sb, sc, index_base,
                                          int(c0 is not None), None)
    assert rc == 0, (rc, g.lib().mm_last_error().decode())
    cout, iout = dc.cpu().numpy().view(t), di.cpu().numpy().view(np.int32)
    for out, pat in ((cout, cpat), (iout, ipat)):
        assert out[:GUARD].tobytes() == pat.tobytes() and out[-GUARD:].tobytes() == pat.tobytes(), "guard overwritten"
    return cout[GUARD + c_offset:-GUARD], iout[GUARD + i_offset:-GUARD]


def ordered_values(cfg_dtype, mp, rd, a, b, n, k, m, ta=False, c0=None):
    """C of mm_gemm_batched_launch (plain) / mm_gemm_batched_accumulate_launch (seeded) under MM_PATH_ORDERED."""
    cfg = g.make_config(cfg_dtype, mp, rd, g.PATH_ORDERED, ta)
    c = np.zeros(n * m, dtype=a.dtype) if c0 is None else np.asarray(c0, dtype=a.dtype).reshape(-1).copy()
    da, db, dc = _dev(a), _dev(b), _dev(c)
    launch = g.lib().mm_gemm_batched_launch if c0 is None else g.lib().mm_gemm_batched_accumulate_launch
    rc = launch(0, ctypes.byref(cfg), da.data_ptr(), db.data_ptr(), dc.data_ptr(), n, k, m, 1, 0, 0, 0, None)
    assert rc == 0, g.lib().mm_last_error().decode()
    return dc.cpu().numpy().view(a.dtype).reshape(n, m)


def operands(dtype, mp, rd, n, k, m, rng, ta=False):
    a_shape = (k, n) if ta else (n, k)
    if sr.is_float(dtype):
        return sr.float_operands(dtype, mp, rd, a_shape, (k, m), rng, True, a_row_axis=1 if ta else 0)
    return sr.int_operands(dtype, mp, rd, a_shape, (k, m), rng, a_row_axis=1 if ta else 0)


def seeds(dtype, shape, rng):
    """Full-range seeds with min, max, 0 (and +-0, +-inf, NaN for floating types) planted."""
    t = sr.NP_DTYPES[dtype]
    lo, hi = sr.limits(dtype)
    if sr.is_float(dtype):
        c = rng.uniform(-4, 4, size=shape).astype(t)
        special = [t(0), t(-0.0), lo, hi, t(np.inf), t(-np.inf), t(np.nan)]
    else:
        u = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[np.dtype(t).itemsize]
        c = rng.integers(0, np.iinfo(u).max, size=shape, dtype=u, endpoint=True).view(t)
        special = [t(0), lo, hi]
    flat = c.reshape(-1)
    pos = rng.choice(flat.size, size=flat.size // 8, replace=False)
    flat[pos] = rng.choice(np.array(special, dtype=t), size=pos.size)
    return c


def check(got_c, got_i, want_c, want_i, what):
    assert sr.same_bits(got_c, want_c), (what, "values", sr.first_difference(got_c, want_c))
    assert np.array_equal(got_i, want_i), (what, "indices", sr.first_difference(got_i, want_i))


# tiled ragged, unserved, K x N A, and the 64 x 64 kernel's edge in both A layouts: two tiles each way, a one-line last tile, a
# one-k last slab
SHAPES = [(200, 68, 132, False), (67, 37, 61, False), (132, 36, 72, True), (65, 17, 67, False), (65, 17, 67, True)]


@pytest.mark.parametrize("dtype,mp,rd", ARG_CONFIGS, ids=["-".join(c) for c in ARG_CONFIGS])
def test_argreduce_every_config_both_paths(dtype, mp, rd):
    rng = np.random.default_rng(zlib.crc32(f"{dtype}/{mp}/{rd}".encode()))
    for n, k, m, ta in SHAPES:
        a, b = operands(dtype, mp, rd, n, k, m, rng, ta)
        want_c, want_i = oracle(dtype, mp, rd, a, b, transposed_a=ta)
        ordered = ordered_values(dtype, mp, rd, a, b, n, k, m, ta)
        assert sr.same_bits(want_c, ordered), ("oracle vs MM_PATH_ORDERED", sr.first_difference(want_c, ordered))
        for path in (g.PATH_AUTO, g.PATH_ORDERED):
            cfg = g.make_config(dtype, mp, rd, path, ta)
            c, i = argreduce(cfg, a, b, n, k, m)
            check(c.reshape(n, m), i.reshape(n, m), want_c, want_i, (n, k, m, ta, path, g.kernel_name_argreduce(cfg, n, k, m)))
        # accumulating, seeded with random values (NaN, +-inf, +-0 among them) and random indices
        c0, i0 = seeds(dtype, (n, m), rng), rng.integers(-1, 1000, size=(n, m)).astype(np.int32)
        want_c, want_i = oracle(dtype, mp, rd, a, b, c0, i0, transposed_a=ta, index_base=5)
        assert sr.same_bits(want_c, ordered_values(dtype, mp, rd, a, b, n, k, m, ta, c0))
        for path in (g.PATH_AUTO, g.PATH_ORDERED):
            c, i = argreduce(g.make_config(dtype, mp, rd, path, ta), a, b, n, k, m, c0=c0, i0=i0, index_base=5)
            check(c.reshape(n, m), i.reshape(n, m), want_c, want_i, (n, k, m, ta, path, "seeded"))


@pytest.mark.parametrize("dtype", ["int", "uint8_t", "float", "half", "double", "long"])
@pytest.mark.parametrize("rd", REDUCTIONS)
def test_argreduce_ties_take_the_first_k(dtype, rd):
    rng = np.random.default_rng(3)
    t = sr.NP_DTYPES[dtype]
    for n, k, m in ((128, 64, 128), (65, 33, 63)):
        # a handful of values: most outputs see their extreme at several k
        a = rng.integers(0, 3, size=(n, k)).astype(t)
        b = rng.integers(0, 3, size=(k, m)).astype(t)
        if sr.is_float(dtype):   # signed zeros tie with each other: the first one stays
            a[rng.random(a.shape) < 0.2] = t(-0.0)
        want_c, want_i = oracle(dtype, "Add", rd, a, b)
        assert (want_i > 0).any() and (want_i < k - 1).any()
        for path in (g.PATH_AUTO, g.PATH_ORDERED):
            c, i = argreduce(g.make_config(dtype, "Add", rd, path), a, b, n, k, m)
            check(c.reshape(n, m), i.reshape(n, m), want_c, want_i, (dtype, rd, n, path))


@pytest.mark.parametrize("dtype", ["float", "int", "half"])
def test_argreduce_identity_survives_with_minus_one(dtype):
    t = sr.NP_DTYPES[dtype]
    lo, hi = sr.limits(dtype)
    for n, k, m in ((128, 32, 128), (61, 31, 67)):
        for rd, fill in (("Min", hi), ("Max", lo)):
            a = np.full((n, k), fill, dtype=t)
            b = np.full((k, m), fill, dtype=t)
            if sr.is_float(dtype):   # +-inf paths and NaNs never beat the identity either
                a[:, ::3] = np.inf if rd == "Min" else -np.inf
                b[::5, :] = np.nan
            a[0, 1] = 0                                 # one row of outputs with a real candidate, at k = 1
            b[1, :] = 0
            mp = "Max" if rd == "Min" else "Min"        # Map = max(a, b) keeps fill (Min) / min keeps lowest (Max)
            want_c, want_i = oracle(dtype, mp, rd, a, b)
            assert (want_i[1:] == -1).all() and (want_c[1:] == fill).all()
            for path in (g.PATH_AUTO, g.PATH_ORDERED):
                c, i = argreduce(g.make_config(dtype, mp, rd, path), a, b, n, k, m)
                check(c.reshape(n, m), i.reshape(n, m), want_c, want_i, (dtype, rd, n, path))


@pytest.mark.parametrize("shape", [(256, 96, 128), (61, 90, 67)], ids=["tile", "plain"])
@pytest.mark.parametrize("dtype,mp,rd", [("float", "Add", "Min"), ("int", "Add", "Max"), ("double", "Multiply", "Min")])
def test_argreduce_k_split_composes(shape, dtype, mp, rd):
    n, k, m = shape
    k1 = 40
    rng = np.random.default_rng(11)
    a, b = operands(dtype, mp, rd, n, k, m, rng)
    cfg = g.make_config(dtype, mp, rd)
    whole_c, whole_i = argreduce(cfg, a, b, n, k, m)
    c1, i1 = argreduce(cfg, np.ascontiguousarray(a[:, :k1]), np.ascontiguousarray(b[:k1]), n, k1, m)
    c2, i2 = argreduce(cfg, np.ascontiguousarray(a[:, k1:]), np.ascontiguousarray(b[k1:]), n, k - k1, m, c0=c1, i0=i1,
                       index_base=k1)
    check(c2, i2, whole_c, whole_i, ("K split", shape))
    check(whole_c.reshape(n, m), whole_i.reshape(n, m), *oracle(dtype, mp, rd, a, b), "whole")


@pytest.mark.parametrize("shape", [(8, 70000, 16), (5, 70000, 7)], ids=["tile", "plain"])
def test_argreduce_large_k_indices_are_not_truncated(shape):
    n, k, m = shape
    rng = np.random.default_rng(5)
    a = rng.uniform(1, 2, size=(n, k)).astype(np.float32)
    b = rng.uniform(1, 2, size=(k, m)).astype(np.float32)
    a[: n // 2, 65536] = -100.0      # unique minimum at k = 65536 for the upper rows
    a[n // 2:, 69999] = -100.0       # and at k = 69999 (the last k) for the others
    cfg = g.make_config("float", "Add", "Min")
    c, i = argreduce(cfg, a, b, n, k, m)
    i = i.reshape(n, m)
    assert (i[: n // 2] == 65536).all() and (i[n // 2:] == 69999).all(), np.unique(i)
    assert g.kernel_name_argreduce(cfg, n, k, m) == ("argreduce_tile" if m % 4 == 0 else "argreduce")
    ref = (a[:, :, None] + b[None, :, :]).min(axis=1)
    assert np.array_equal(c.reshape(n, m), ref)


@pytest.mark.parametrize("bcast", ["a", "b"])
@pytest.mark.parametrize("shape", [(64, 32, 128), (33, 30, 45)], ids=["tile", "plain"])
def test_argreduce_batches_broadcast_chunked_and_guarded(bcast, shape):
    n, k, m = shape
    batch, sc = 5, n * m + 12
    rng = np.random.default_rng(17)
    dtype, mp, rd = "float", "Add", "Min"
    nb_a, nb_b = (1, batch) if bcast == "a" else (batch, 1)
    a = np.stack([operands(dtype, mp, rd, n, k, m, rng)[0] for _ in range(nb_a)])
    b = np.stack([operands(dtype, mp, rd, n, k, m, rng)[1] for _ in range(nb_b)])
    sa, sb = (0 if nb_a == 1 else n * k), (0 if nb_b == 1 else k * m)
    cfg = g.make_config(dtype, mp, rd)
    old = g.get_tuning("batch_chunk")
    try:
        for chunk in (-1, 2):
            g.set_tuning("batch_chunk", chunk)
            c, i = argreduce(cfg, a, b, n, k, m, batch, sa, sb, sc)
            for e in range(batch):
                want_c, want_i = oracle(dtype, mp, rd, a[e % nb_a], b[e % nb_b])
                check(c[e * sc:e * sc + n * m].reshape(n, m), i[e * sc:e * sc + n * m].reshape(n, m), want_c, want_i,
                      (bcast, chunk, e))
                if e < batch - 1:   # the gap between elements is not written
                    assert (i[e * sc + n * m:(e + 1) * sc] == 7).all()
    finally:
        g.set_tuning("batch_chunk", old)


@pytest.mark.parametrize("dtype", ["float", "half", "uint8_t"])
def test_argreduce_misaligned_outputs_and_strides_give_the_same_bits(dtype):
    """A shape the tile serves, with C's base, I's base, or the element stride of C and I not 16-byte aligned: the call is
    accepted (mm_gemm.h: the launch is demoted to the predicated kernel, which this test cannot observe -- it checks only
    that the values and indices are right and that nothing outside C and I is written)."""
    n, k, m, batch = 128, 64, 128, 3
    rng = np.random.default_rng(23)
    a, b = operands(dtype, "Add", "Min", n, k, m, rng)
    cfg = g.make_config(dtype, "Add", "Min")
    assert g.kernel_name_argreduce(cfg, n, k, m, batch) == "argreduce_tile"
    want = oracle(dtype, "Add", "Min", a, b)
    for kw in ({"c_offset": 1}, {"i_offset": 1}, {"i_offset": 2}):
        c, i = argreduce(cfg, a, b, n, k, m, **kw)
        check(c.reshape(n, m), i.reshape(n, m), *want, kw)
    sc = n * m + 1                      # element stride: an odd number of elements, so neither C's nor I's is 16-byte aligned
    c, i = argreduce(cfg, a, b, n, k, m, batch, 0, 0, sc)
    for e in range(batch):
        check(c[e * sc:e * sc + n * m].reshape(n, m), i[e * sc:e * sc + n * m].reshape(n, m), *want, ("stride", e))


def _floyd_warshall(w):
    d = w.copy()
    for v in range(d.shape[0]):
        d = np.minimum(d, d[:, v:v + 1] + d[v:v + 1, :])
    return d


@pytest.mark.parametrize("nv,path", [(300, g.PATH_ORDERED), (512, g.PATH_AUTO)], ids=["plain", "tile"])
def test_shortest_paths_with_witnesses_end_to_end(nv, path):
    """Repeated min-plus squaring D <- min(D, D (x) D) with addmm_argreduce_ (D's copy as the operand): the witness of
    (i, j) is an intermediate vertex v with D[i, j] = D[i, v] + D[v, j], or -1 for the direct edge / i == j.  Distances
    equal Floyd-Warshall's; every path expanded through its witnesses walks real edges whose weights sum to the distance."""
    import torch
    rng = np.random.default_rng(nv)
    big = np.int32(1 << 28)           # "no edge": big + big still fits an int32
    w = np.full((nv, nv), big, dtype=np.int32)
    mask = rng.random((nv, nv)) < 8.0 / nv
    w[mask] = rng.integers(1, 100, size=mask.sum())
    np.fill_diagonal(w, 0)
    dev = torch.device("cuda:0")
    d = torch.from_numpy(w).to(dev)
    wit = torch.full((nv, nv), -1, dtype=torch.int32, device=dev)
    assert g.kernel_name_argreduce(g.make_config("int", "Add", "Min", path), nv, nv, nv) == \
        ("argreduce_tile" if path == g.PATH_AUTO else "argreduce")
    for _ in range(int(np.ceil(np.log2(nv))) + 1):
        g.addmm_argreduce_(d, wit, d.clone(), d.clone(), "int", "Add", "Min", path)
    dist, wit = d.cpu().numpy(), wit.cpu().numpy()
    ref = _floyd_warshall(w.astype(np.int64))
    ref[ref >= big] = big
    assert np.array_equal(np.minimum(dist, big), ref)

    def expand(i, j, out, depth=0):
        assert depth < 64
        v = wit[i, j]
        if v < 0:
            out.append((i, j))
            return
        expand(i, v, out, depth + 1)
        expand(v, j, out, depth + 1)

    checked = 0
    for i, j in zip(*np.nonzero((ref < big) & ~np.eye(nv, dtype=bool))):
        if checked >= 3000:
            break
        hops = []
        expand(i, j, hops)
        assert all(w[x, y] < big for x, y in hops), (i, j, hops)
        assert sum(int(w[x, y]) for x, y in hops) == ref[i, j], (i, j, hops)
        checked += 1
    assert checked > 1000


def test_viterbi_backpointers_end_to_end():
    """Max-plus Viterbi over 64 sequences, 128 states, 50 steps: delta_t[s, j] = max_i (delta_{t-1}[s, i] + T[i, j]) + E_t[s, j]
    with the argmax as the backpointer -- one matmul_argreduce per step (B = the transition matrix, shared).  Compared with
    numpy Viterbi, whose np.argmax takes the first maximum: scores are small integers in float, so ties happen."""
    import torch
    rng = np.random.default_rng(29)
    seqs, states, steps = 64, 128, 50
    trans = rng.integers(-8, 1, size=(states, states)).astype(np.float32)
    emit = rng.integers(-6, 1, size=(steps, seqs, states)).astype(np.float32)
    dev = torch.device("cuda:0")
    tt = torch.from_numpy(trans).to(dev)
    delta = torch.from_numpy(emit[0]).to(dev)
    backs = []
    for t in range(1, steps):
        vals, idx = g.matmul_argreduce(delta, tt, "float", "Add", "Max")
        assert idx.dtype == torch.int32 and tuple(idx.shape) == (seqs, states)
        backs.append(idx)
        delta = vals + torch.from_numpy(emit[t]).to(dev)
    # numpy Viterbi
    d = emit[0].copy()
    ref_backs = []
    for t in range(1, steps):
        cand = d[:, :, None] + trans[None, :, :]
        ref_backs.append(np.argmax(cand, axis=1).astype(np.int32))
        d = cand.max(axis=1) + emit[t]
    assert np.array_equal(delta.cpu().numpy(), d)
    for t, (got, want) in enumerate(zip(backs, ref_backs)):
        assert np.array_equal(got.cpu().numpy(), want), t
    # decoded paths agree
    last = d.argmax(axis=1)
    path_ref, path_got = [last], [last]
    for got, want in zip(reversed(backs), reversed(ref_backs)):
        path_ref.append(want[np.arange(seqs), path_ref[-1]])
        path_got.append(got.cpu().numpy()[np.arange(seqs), path_got[-1]])
    assert np.array_equal(np.array(path_got), np.array(path_ref))


def test_torch_api_on_a_non_default_stream():
    import torch
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(31)
    for n, k, m in ((256, 128, 256), (67, 37, 61)):
        a, b = operands("float", "Add", "Min", n, k, m, rng)
        ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            vals, idx = g.matmul_argreduce(ta, tb)
        s.synchronize()
        assert idx.dtype == torch.int32 and vals.dtype == torch.float32 and tuple(vals.shape) == (n, m)
        ref = g.matmul(ta, tb, "float", "Add", "Min", path=g.PATH_ORDERED)
        torch.cuda.synchronize()
        assert sr.same_bits(vals.cpu().numpy(), ref.cpu().numpy())
        check(vals.cpu().numpy(), idx.cpu().numpy(), *oracle("float", "Add", "Min", a, b), (n, "torch"))
    # 3-D and broadcast operands, out= / out_index=, and the in-place form on a batch
    a3 = torch.from_numpy(rng.uniform(-1, 1, size=(3, 64, 32)).astype(np.float32)).to(dev)
    b2 = torch.from_numpy(rng.uniform(-1, 1, size=(32, 64)).astype(np.float32)).to(dev)
    out = torch.empty(3, 64, 64, device=dev)
    out_i = torch.empty(3, 64, 64, dtype=torch.int32, device=dev)
    vals, idx = g.matmul_argreduce(a3, b2, reduce_op="Max", out=out, out_index=out_i)
    assert vals is out and idx is out_i
    ref = g.bmm(a3, b2, "float", "Add", "Max", path=g.PATH_ORDERED)
    assert torch.equal(vals, ref)
    c, ci = vals.clone(), idx.clone()
    g.addmm_argreduce_(c, ci, a3 - 0.5, b2, reduce_op="Max", index_base=32)
    for e in range(3):
        want_c, want_i = oracle("float", "Add", "Max", (a3[e] - 0.5).cpu().numpy(), b2.cpu().numpy(),
                                vals[e].cpu().numpy(), idx[e].cpu().numpy(), index_base=32)
        check(c[e].cpu().numpy(), ci[e].cpu().numpy(), want_c, want_i, ("addmm_argreduce_", e))
    with pytest.raises(g.MMError, match="Min or Max"):
        g.matmul_argreduce(a3, b2, reduce_op="Add")
        torch.cuda.synchronize()
