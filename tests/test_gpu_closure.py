"""GPU tests of the semiring closure (mm_closure_*, closure_): blocked Floyd-Warshall in place, with witnesses.  The oracle is
tests/_closure_ref.py: the library's blocked algorithm restated in numpy in the element type's own arithmetic (bit for bit),
and plain Floyd-Warshall, which it equals on absorptive inputs (checked on the CPU by tests/test_closure_capi.py)."""
import ctypes
import heapq
import zlib

import numpy as np
import pytest

import _closure_ref as cr
import _semiring_ref as sr
import gemm_hls_amd as g

pytestmark = pytest.mark.gpu

GUARD = 64   # elements of guard pattern around D and W, and in the gaps between the graphs of a batch
CONFIGS = cr.CONFIGS   # 11 x 5 x 2 = 110


@pytest.fixture
def block():
    """Sets closure_block for one test and restores it."""
    old = g.get_tuning("closure_block")
    yield lambda b: g.set_tuning("closure_block", b)
    g.set_tuning("closure_block", old)


def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x).reshape(-1).view(np.uint8).copy()).to("cuda:0")


def _pattern(t, count):
    return (np.arange(count * np.dtype(t).itemsize) % 251 + 1).astype(np.uint8).view(t)


def _operand_sets(dtype, mp, rd, n, rng, batch=1):
    """[(graphs, informative)]: the sparse graphs whose closure keeps many values (_closure_ref.graphs), and for the integer
    Add and Multiply maps the dense full-range set as well, whose wrap-around makes every bit depend on the pivot order."""
    sets = [(cr.graphs(dtype, mp, rd, n, rng, batch), True)]
    if cr.wrapping(dtype, mp):
        sets.append((cr.full_range(dtype, n, rng, batch), False))
    return sets


def _bits(x):
    return x.view(sr._UNSIGNED[x.dtype.itemsize])


def closure_capi(cfg, d, witness, stride=None):
    """mm_closure_launch on (batch, n, n) host graphs, placed at `stride` elements apart inside guarded buffers; the guards
    and the gap after every graph must come back untouched.  Returns (D, W or None) as (batch, n, n)."""
    batch, n, _ = d.shape
    t = d.dtype
    nn = n * n
    stride = nn if stride is None else stride

    def guarded(x, fill_t):
        body = np.empty((batch, stride), dtype=fill_t)
        body[:, :nn] = x.reshape(batch, nn)
        body[:, nn:] = _pattern(fill_t, stride - nn)
        return np.concatenate([_pattern(fill_t, GUARD), body.reshape(-1), _pattern(fill_t, GUARD)])

    dd = _dev(guarded(d, t))
    dw = _dev(guarded(np.full(d.shape, 12345, dtype=np.int32), np.int32)) if witness else None
    rc = g.lib().mm_closure_launch(0, ctypes.byref(cfg), dd.data_ptr() + GUARD * t.itemsize,
                                   dw.data_ptr() + GUARD * 4 if witness else None, n, batch, stride, None)
    assert rc == 0, (rc, g.lib().mm_last_error().decode())

    def unpack(buf, x_t):
        out = buf.cpu().numpy().view(x_t)
        guard = _bits(_pattern(x_t, GUARD))
        assert np.array_equal(_bits(out[:GUARD]), guard) and np.array_equal(_bits(out[-GUARD:]), guard), "guard overwritten"
        body = out[GUARD:-GUARD].reshape(batch, stride)
        gaps = _bits(body[:, nn:])
        assert np.array_equal(gaps, np.broadcast_to(_bits(_pattern(x_t, stride - nn)), gaps.shape)), "gap overwritten"
        return body[:, :nn].reshape(batch, n, n).copy()

    return unpack(dd, t), (unpack(dw, np.int32) if witness else None)


def _check_against_restatement(dtype, mp, rd, path, witness, d, got_d, got_w, b, informative=False):
    auto = path == g.PATH_AUTO and not witness
    for e in range(d.shape[0]):
        want_d, want_w = cr.blocked(dtype, mp, rd, d[e], b, witness=witness, auto=auto)
        if informative:
            cr.assert_informative(dtype, mp, rd, d[e], want_d, f"graph {e}")
        if auto and sr.is_float(dtype):
            assert sr.same_values(got_d[e], want_d), (e, sr.first_difference(got_d[e], want_d, by_value=True))
        else:
            assert sr.same_bits(got_d[e], want_d), (e, sr.first_difference(got_d[e], want_d))
        if witness:
            assert np.array_equal(got_w[e], want_w), (e, np.argwhere(got_w[e] != want_w)[:3])


@pytest.mark.parametrize("witness", [False, True], ids=["values", "witness"])
@pytest.mark.parametrize("path", [g.PATH_ORDERED, g.PATH_AUTO], ids=["ordered", "auto"])
@pytest.mark.parametrize("dtype,mp,rd", CONFIGS)
def test_bit_exact_against_blocked_restatement(dtype, mp, rd, path, witness, block):
    """Every configuration, closure_block = 64: n below B (on chip), n = B, n = 2B + 36 (aligned, the tile kernels in
    step 3 under AUTO), and a batch of 3 graphs of n = 2B + 37 with guard patterns in the gaps between them."""
    block(64)
    _run_shapes(dtype, mp, rd, path, witness, 64, ((37, 1), (64, 1), (164, 1), (2 * 64 + 37, 3)))


def _run_shapes(dtype, mp, rd, path, witness, b, shapes):
    """Every operand set of the configuration at every (n, batch) of `shapes`, batches at a padded stride, compared bit
    for bit (witnesses included) with the restatement at block size b; every primary reference must be informative."""
    cfg = g.make_config(dtype, mp, rd, path)
    rng = np.random.default_rng(zlib.crc32(f"{dtype},{mp},{rd}".encode()))
    for n, batch in shapes:
        for d, informative in _operand_sets(dtype, mp, rd, n, rng, batch):
            got_d, got_w = closure_capi(cfg, d, witness, stride=None if batch == 1 else (n * n + 15) // 16 * 16 + 16)
            _check_against_restatement(dtype, mp, rd, path, witness, d, got_d, got_w, b, informative)


# The shipped forms, which closure_block = 64 never reaches.  B = 256 (value-only, elements of at most 4 bytes):
# closure_diag_kernel<..., 256, 8> and closure_panel_kernel<..., 256>; B = 128: closure_diag_kernel<..., 128, 4> on 1024
# threads and panels with bt = 128.  Shapes, the smallest that reach every branch -- B = 256: n = 200 on chip, ragged inside
# class 256; n = 456 = 256 + 200: panels with a ragged bt in class 256, a last panel tile 8 wide, a rank update with K = 200;
# n = 293 = 256 + 37 as a batch of 2 at a padded stride: a class-64 diagonal, a rank update with K % 4 != 0 on the predicated
# kernels.  B = 128: the same at n = 100, 228 = 128 + 100 and 293 = 2 * 128 + 37.
SHIPPED_SHAPES = {256: ((200, 1), (456, 1), (293, 2)), 128: ((100, 1), (228, 1), (293, 2))}


def _shipped_block(dtype, witness):
    """The block size closure_block = -1 chooses."""
    return 256 if not witness and np.dtype(sr.NP_DTYPES[dtype]).itemsize <= 4 else 128


@pytest.mark.parametrize("witness", [False, True], ids=["values", "witness"])
@pytest.mark.parametrize("dtype,mp,rd", CONFIGS)
def test_bit_exact_at_the_shipped_block_sizes(dtype, mp, rd, witness, block):
    """Every configuration under MM_PATH_AUTO with the default closure_block (the diagonal and panel kernels do not depend
    on the path): outside absorptive inputs the blocked algorithm at B itself fixes every bit."""
    block(-1)
    b = _shipped_block(dtype, witness)
    _run_shapes(dtype, mp, rd, g.PATH_AUTO, witness, b, SHIPPED_SHAPES[b])


# one (map, reduce) per dtype for the forms the matrix above does not reach
ONE_PER_DTYPE = [("float", "Multiply", "Min"), ("double", "Add", "Max"), ("half", "Add", "Min"), ("int8_t", "Add", "Min"),
                 ("uint8_t", "Multiply", "Max"), ("int16_t", "Max", "Min"), ("uint16_t", "Add", "Max"),
                 ("int", "Multiply", "Min"), ("unsigned", "Min", "Max"), ("long", "Add", "Min"),
                 ("unsigned long", "Multiply", "Max")]
assert [c[0] for c in ONE_PER_DTYPE] == sr.DTYPES


@pytest.mark.parametrize("witness", [False, True], ids=["values", "witness"])
@pytest.mark.parametrize("dtype,mp,rd", ONE_PER_DTYPE)
def test_bit_exact_at_the_shipped_block_sizes_ordered(dtype, mp, rd, witness, block):
    block(-1)
    b = _shipped_block(dtype, witness)
    _run_shapes(dtype, mp, rd, g.PATH_ORDERED, witness, b, SHIPPED_SHAPES[b])


@pytest.mark.parametrize("dtype,mp,rd", [c for c in ONE_PER_DTYPE if _shipped_block(c[0], False) == 256])
def test_bit_exact_value_only_at_block_128(dtype, mp, rd, block):
    """closure_diag_kernel<..., 128, 4> and the 128 panels without witnesses on elements of at most 4 bytes: reached by the
    knob alone."""
    block(128)
    _run_shapes(dtype, mp, rd, g.PATH_AUTO, False, 128, SHIPPED_SHAPES[128])


def _check_batch_equals_each_graph_alone(dtype, mp, rd, base, batch, stride, b):
    """A batch of base[e % p] (p prime, so no chunk boundary falls on a period) against every base graph run alone, which in
    turn equals the restatement: bit for bit, witnesses included, guards and gaps intact."""
    cfg = g.make_config(dtype, mp, rd)
    alone = [closure_capi(cfg, base[e:e + 1], True) for e in range(len(base))]
    alone_d, alone_w = np.concatenate([a[0] for a in alone]), np.concatenate([a[1] for a in alone])
    _check_against_restatement(dtype, mp, rd, g.PATH_AUTO, True, base, alone_d, alone_w, b)
    which = np.arange(batch) % len(base)
    got_d, got_w = closure_capi(cfg, base[which], True, stride=stride)
    bad = np.flatnonzero((_bits(got_d) != _bits(alone_d)[which]).any(axis=(1, 2)) | (got_w != alone_w[which]).any(axis=(1, 2)))
    assert bad.size == 0, f"{bad.size} graphs differ from the same graph run alone, the first at {bad[:4]}"


def test_second_workspace_chunk_equals_each_graph_alone(block):
    """dispatch_closure's second chunk of graphs (e0 > 0: the offsets of D and W, the pitch of the witness memset).  double
    with witnesses at closure_block = 64 and n = 65: a snapshot is 4160 elements, so the 256 MiB of workspace hold
    2^28 / (2 * 4160 * 8) = 4033 graphs, and 4040 run as 4033 + 7."""
    block(64)
    n, batch = 65, 4040
    assert g.kernel_name_closure(g.make_config("double", "Add", "Min"), n, batch, True) == "closure_blocked"
    base = cr.graphs("double", "Add", "Min", n, np.random.default_rng(17), batch=7)
    for e in range(len(base)):
        cr.assert_informative("double", "Add", "Min", base[e], cr.blocked("double", "Add", "Min", base[e], 64)[0], f"graph {e}")
    _check_batch_equals_each_graph_alone("double", "Add", "Min", base, batch, n * n + 31, 64)


def test_second_onchip_chunk_equals_each_graph_alone():
    """The on-chip form launches 2^20 graphs at a time: 2^20 + 5 graphs of 2 vertices run as two launches.  (4 entries
    cannot meet assert_informative; the 13 graphs differ, and their closures differ from them.)"""
    n, batch = 2, (1 << 20) + 5
    rng = np.random.default_rng(19)
    base = np.where(rng.random((13, n, n)) < 0.4, np.inf, rng.integers(1, 4097, size=(13, n, n)) / 64.0).astype(np.float32)
    want = np.stack([cr.blocked("float", "Add", "Min", x, 128)[0] for x in base])
    assert len({x.tobytes() for x in want}) == 13 and (want != base).any(axis=(1, 2)).sum() >= 6
    _check_batch_equals_each_graph_alone("float", "Add", "Min", base, batch, n * n + 3, 128)


def _torch_closure(d, dtype, mp, rd, witness=False, path=g.PATH_AUTO):
    import torch
    x = torch.from_numpy(np.ascontiguousarray(d)).to("cuda:0")
    w = torch.empty(x.shape, dtype=torch.int32, device=x.device) if witness else None
    g.closure_(x, w, dtype, mp, rd, path)
    return x.cpu().numpy(), (w.cpu().numpy() if witness else None)


def _shortest_inputs(dtype, n, rng, density=0.05):
    """Non-negative integer weights in [1, 100], "no edge" +inf (floats) or max() / 2 (integers), diagonal 0 (A*)."""
    t = sr.NP_DTYPES[dtype]
    none = np.inf if sr.is_float(dtype) else sr.limits(dtype)[1] // 2
    d = np.where(rng.random((n, n)) < density, rng.integers(1, 101, size=(n, n)), 0).astype(np.float64)
    d = np.where(d > 0, d, none).astype(t)
    np.fill_diagonal(d, 0)
    return d


@pytest.mark.parametrize("case", ["float", "int", "negative"])
def test_shortest_paths_equal_floyd_warshall(case):
    rng = np.random.default_rng(7)
    n = 520
    if case == "negative":   # negative edges, no negative cycle: w'(u, v) = w(u, v) + h(u) - h(v) with potentials h
        base = _shortest_inputs("float", n, rng)
        h = rng.integers(0, 50, size=n).astype(np.float32)
        d = np.where(np.isinf(base), base, base + h[:, None] - h[None, :]).astype(np.float32)
        assert (d < 0).any()
        dtype = "float"
    else:
        dtype = case
        d = _shortest_inputs(dtype, n, rng)
    got, _ = _torch_closure(d, dtype, "Add", "Min")
    want, _ = cr.floyd_warshall(dtype, "Add", "Min", d)
    assert sr.same_bits(got, want)


def test_longest_path_in_a_dag_equals_floyd_warshall():
    rng = np.random.default_rng(8)
    n = 520
    d = np.where(rng.random((n, n)) < 0.05, rng.integers(1, 100, size=(n, n)), -np.inf).astype(np.float32)
    d[np.tril_indices(n)] = -np.inf   # edges i -> j only for i < j
    got, _ = _torch_closure(d, "float", "Add", "Max")
    want, _ = cr.floyd_warshall("float", "Add", "Max", d)
    assert sr.same_bits(got, want) and np.isfinite(got).sum() > n


@pytest.mark.parametrize("mp,rd", [("Min", "Max"), ("Max", "Min")], ids=["widest", "minimax"])
@pytest.mark.parametrize("dtype", sr.DTYPES)
def test_widest_and_minimax_paths_equal_floyd_warshall(dtype, mp, rd):
    rng = np.random.default_rng(9)
    n = 300
    d = cr.graphs(dtype, mp, rd, n, rng)[0]
    want, _ = cr.floyd_warshall(dtype, mp, rd, d)
    cr.assert_informative(dtype, mp, rd, d, want)
    for witness in (False, True):
        got, w = _torch_closure(d, dtype, mp, rd, witness)
        assert sr.same_bits(got, want), witness


def test_reachability_equals_floyd_warshall():
    rng = np.random.default_rng(10)
    n = 520
    d = (rng.random((n, n)) < 0.002).astype(np.uint8)
    got, _ = _torch_closure(d, "uint8_t", "And", "Max")
    want, _ = cr.floyd_warshall("uint8_t", "And", "Max", d)
    assert np.array_equal(got, want) and 0 < got.sum() < n * n


def _expand(w, i, j, depth=0):
    assert depth < 4096
    v = w[i, j]
    return [(i, j)] if v < 0 else _expand(w, i, v, depth + 1) + _expand(w, v, j, depth + 1)


def test_witnesses_compose_keep_and_reconstruct_paths():
    rng = np.random.default_rng(11)
    n = 520
    d = _shortest_inputs("float", n, rng)
    np.fill_diagonal(d, np.inf)   # A+: no zero-weight self loops, every improvement passes through another vertex
    got, w = _torch_closure(d, "float", "Add", "Min", witness=True)
    i, j = np.nonzero(w >= 0)
    v = w[i, j]
    assert len(v) > n
    assert np.array_equal(got[i, v] + got[v, j], got[i, j])
    assert sr.same_bits(got[w < 0], d[w < 0])
    for a, b in zip(rng.integers(0, n, 200), rng.integers(0, n, 200)):
        if np.isinf(got[a, b]):
            continue
        path = _expand(w, a, b)
        assert path[0][0] == a and path[-1][1] == b and all(p[1] == q[0] for p, q in zip(path, path[1:]))
        assert all(np.isfinite(d[x, y]) for x, y in path)
        assert sum(float(d[x, y]) for x, y in path) == float(got[a, b])


def _dijkstra(adj, src, n):
    dist = [np.inf] * n
    dist[src] = 0.0
    heap = [(0.0, src)]
    while heap:
        du, u = heapq.heappop(heap)
        if du > dist[u]:
            continue
        for v, wt in adj[u]:
            if du + wt < dist[v]:
                dist[v] = du + wt
                heapq.heappush(heap, (dist[v], v))
    return np.array(dist, dtype=np.float64)


def test_large_sparse_graph_against_dijkstra():
    import torch
    n, deg = 16384, 6
    rng = np.random.default_rng(12)
    src = np.repeat(np.arange(n), deg)
    dst = rng.integers(0, n, size=n * deg)
    wt = rng.integers(1, 101, size=n * deg).astype(np.float32)
    d = torch.full((n, n), float("inf"), dtype=torch.float32, device="cuda:0")
    d[torch.from_numpy(src).cuda(), torch.from_numpy(dst).cuda()] = torch.from_numpy(wt).cuda()   # (duplicates: any one)
    d.fill_diagonal_(0)
    host = d.cpu().numpy()
    g.closure_(d)
    got = d.cpu().numpy()
    adj = [[] for _ in range(n)]
    for u, v in zip(*np.nonzero(np.isfinite(host) & (host > 0))):
        adj[u].append((v, float(host[u, v])))
    for s in rng.integers(0, n, 4):
        assert np.array_equal(got[s].astype(np.float64), _dijkstra(adj, s, n)), s


def test_n4096_equals_repeated_squaring():
    import torch
    n = 4096
    rng = np.random.default_rng(13)
    host = _shortest_inputs("float", n, rng, density=0.002)
    d = torch.from_numpy(host).cuda()
    sq = d.clone()
    for _ in range(12):   # ceil(log2 n) rounds of D <- min(D, D + D)
        prev = sq.clone()
        g.addmm_(sq, prev, prev, "float", "Add", "Min")
    g.closure_(d)
    assert torch.equal(d, sq)


def test_deterministic_and_independent_of_batch_position():
    rng = np.random.default_rng(14)
    n = 600
    graphs = np.stack([_shortest_inputs("float", n, rng) for _ in range(3)])
    runs = [_torch_closure(graphs, "float", "Add", "Min", witness=True) for _ in range(2)]
    assert runs[0][0].tobytes() == runs[1][0].tobytes() and np.array_equal(runs[0][1], runs[1][1])
    for e in range(3):
        alone_d, alone_w = _torch_closure(graphs[e], "float", "Add", "Min", witness=True)
        assert alone_d.tobytes() == runs[0][0][e].tobytes() and np.array_equal(alone_w, runs[0][1][e])
    # value-only, int, a batch that runs as several chunks is the same as one graph at a time
    ints = np.stack([_shortest_inputs("int", 300, rng) for _ in range(2)])
    both, _ = _torch_closure(ints, "int", "Add", "Min")
    for e in range(2):
        assert np.array_equal(both[e], _torch_closure(ints[e], "int", "Add", "Min")[0])


def test_many_small_graphs_in_one_call():
    rng = np.random.default_rng(15)
    batch, n = 4096, 64
    d = np.where(rng.random((batch, n, n)) < 0.1, rng.integers(1, 101, size=(batch, n, n)), np.inf).astype(np.float32)
    assert g.kernel_name_closure(g.make_config("float", "Add", "Min"), n, batch) == "closure_onchip"
    got, w = _torch_closure(d, "float", "Add", "Min", witness=True)
    for e in rng.integers(0, batch, 16):
        want_d, want_w = cr.blocked("float", "Add", "Min", d[e], 128, witness=True)
        assert sr.same_bits(got[e], want_d) and np.array_equal(w[e], want_w), e


def test_torch_api_forms_and_refusals():
    import torch
    rng = np.random.default_rng(16)
    d2 = _shortest_inputs("float", 90, rng)
    x = torch.from_numpy(d2).cuda()
    assert g.closure_(x) is x
    assert sr.same_bits(x.cpu().numpy(), cr.floyd_warshall("float", "Add", "Min", d2)[0])
    d3 = np.stack([_shortest_inputs("double", 70, rng) for _ in range(5)])
    y = torch.from_numpy(d3).cuda()
    wy = torch.empty(y.shape, dtype=torch.int32, device="cuda:0")
    g.closure_(y, wy, "double")
    for e in range(5):
        want_d, want_w = cr.blocked("double", "Add", "Min", d3[e], 128, witness=True)
        assert sr.same_bits(y[e].cpu().numpy(), want_d) and np.array_equal(wy[e].cpu().numpy(), want_w)
    z = torch.zeros(8, 8, device="cuda:0")
    with pytest.raises(g.MMError, match="device tensors"):
        g.closure_(torch.zeros(8, 8))
    with pytest.raises(g.MMError, match="shape"):
        g.closure_(torch.zeros(8, 9, device="cuda:0"))
    with pytest.raises(g.MMError, match="shape"):
        g.closure_(torch.zeros(2, 2, 8, 8, device="cuda:0"))
    with pytest.raises(g.MMError, match="contiguous"):
        g.closure_(torch.zeros(8, 8, device="cuda:0").t())
    with pytest.raises(g.MMError, match="dtype"):
        g.closure_(z, dtype="double")
    with pytest.raises(g.MMError, match="d_witness"):
        g.closure_(z, torch.zeros(8, 8, dtype=torch.int64, device="cuda:0"))
    with pytest.raises(g.MMError, match="d_witness"):
        g.closure_(z, torch.zeros(8, 7, dtype=torch.int32, device="cuda:0"))
    with pytest.raises(g.MMError):
        g.closure_(z, reduce_op="Add")
