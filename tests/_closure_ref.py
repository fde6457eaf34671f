"""numpy restatements of the semiring closure (mm_closure_*, include/mm_gemm.h), in the element type's own arithmetic on
_semiring_ref's operators.

blocked() is the library's algorithm to the letter -- block t covers K = [tB, min(n, (t + 1)B)); for t ascending:
  1. for v in K ascending: D[K,K] <- D[K,K] (+) D[K,v] (x) D[v,K]  (numpy evaluates the right-hand side first)
  2. row panel D[K,J] <- D[K,J] (+) P (x) D[K,J]_old, column panel D[I,K] <- D[I,K] (+) D[I,K]_old (x) P, v in K ascending
  3. D <- D (+) Cc (x) Rc, Cc = D[:,K], Rc = D[K,:]
  (n <= B: step 1 only).  A winner is a strict improvement (Min: s < acc, Max: acc < s); the witness records v.
floyd_warshall() is the textbook recurrence, one v at a time over the whole matrix.  The two agree on absorptive inputs
(tests/test_closure_capi.py checks that), which is what lets the GPU tests use blocked() as their oracle.

TEST INFRASTRUCTURE ONLY."""
import numpy as np

import _semiring_ref as sr

REDUCTIONS = ("Min", "Max")
CONFIGS = [(d, mp, rd) for d in sr.DTYPES for mp in sr.OPS for rd in REDUCTIONS]   # 11 x 5 x 2 = 110


def _relax(acc, wacc, s, v, rd, auto=False):
    """acc <- acc (+) s in place (and wacc <- v where s strictly improves).  auto: floating Min / Max as minNum / maxNum."""
    take = (s < acc) if rd == "Min" else (acc < s)
    if auto and acc.dtype.kind == "f":
        acc[...] = np.fmin(acc, s) if rd == "Min" else np.fmax(acc, s)
    else:
        acc[...] = np.where(take, s, acc)
    if wacc is not None:
        wacc[take] = v


def blocked(dtype, mp, rd, d, block, witness=False, auto=False):
    """(D, W) after the blocked closure of one n x n graph; W is None unless witness.  auto: step 3 as MM_PATH_AUTO's
    value-only rank update evaluates its reduction (valu_tile: minNum / maxNum)."""
    t = sr.NP_DTYPES[dtype]
    d = np.array(d, dtype=t, copy=True)
    n = d.shape[0]
    w = np.full((n, n), -1, dtype=np.int32) if witness else None
    ap = lambda x, y: sr._apply(mp, x, y, t, False)   # noqa: E731
    with np.errstate(all="ignore"):
        for k0 in range(0, n, block):
            k1 = min(n, k0 + block)
            wkk = w[k0:k1, k0:k1] if witness else None
            for v in range(k0, k1):
                _relax(d[k0:k1, k0:k1], wkk, ap(d[k0:k1, v][:, None], d[v, k0:k1][None, :]), v, rd)
            if n <= block:
                break
            p = d[k0:k1, k0:k1].copy()
            out = np.r_[0:k0, k1:n]
            rows, cols = np.ix_(np.arange(k0, k1), out), np.ix_(out, np.arange(k0, k1))
            r_old, c_old = d[rows], d[cols]
            r_acc, c_acc = r_old.copy(), c_old.copy()
            r_w, c_w = (w[rows], w[cols]) if witness else (None, None)
            for i, v in enumerate(range(k0, k1)):
                _relax(r_acc, r_w, ap(p[:, i][:, None], r_old[i][None, :]), v, rd)
                _relax(c_acc, c_w, ap(c_old[:, i][:, None], p[i][None, :]), v, rd)
            d[rows], d[cols] = r_acc, c_acc
            if witness:
                w[rows], w[cols] = r_w, c_w
            cc, rc = d[:, k0:k1].copy(), d[k0:k1, :].copy()
            for i, v in enumerate(range(k0, k1)):
                _relax(d, w, ap(cc[:, i][:, None], rc[i][None, :]), v, rd, auto)
    return d, w


def floyd_warshall(dtype, mp, rd, d, witness=False):
    """Plain Floyd-Warshall: for v ascending, D <- D (+) D[:,v] (x) D[v,:]."""
    t = sr.NP_DTYPES[dtype]
    d = np.array(d, dtype=t, copy=True)
    n = d.shape[0]
    w = np.full((n, n), -1, dtype=np.int32) if witness else None
    with np.errstate(all="ignore"):
        for v in range(n):
            _relax(d, w, sr._apply(mp, d[:, v][:, None], d[v, :][None, :], t, False), v, rd)
    return d, w


# ---- operand sets with an informative closure --------------------------------------------------------------------------
# The closure of a dense random graph collapses to (nearly) one value, which a kernel that broadcast one number would
# reproduce.  graphs() draws, per (type class, map, reduce), graphs whose closure keeps many values; assert_informative() is
# the criterion, and every reference a closure test compares against goes through it.
EDGES_PER_ROW = 3      # sparse graphs: density 3 / n
WEIGHTS = 4096         # distinct edge weights, where the type has room for them


def _int_weight_range(dtype):
    """Edge weights 1 .. W of the non-wrapping integer (Add, *) recipe: sums of two entries stay inside the type."""
    return {1: 40 if dtype == 'uint8_t' else 10, 2: 1024}.get(np.dtype(sr.NP_DTYPES[dtype]).itemsize, WEIGHTS)


def wrapping(dtype, mp):
    """True where a second, full-range operand set applies: integer Add and Multiply maps wrap around, and that is what
    makes the result depend on the pivot order and the block size."""
    return not sr.is_float(dtype) and mp in ("Add", "Multiply")


def full_range(dtype, n, rng, batch=1):
    """Dense NaN-free graphs: floats in [1/16, 2], integers over the type's whole range (wrap-around is exact)."""
    t = sr.NP_DTYPES[dtype]
    shape = (batch, n, n)
    if sr.is_float(dtype):
        return (rng.integers(1, 33, size=shape) / 16).astype(t)
    info = np.iinfo(t)
    return rng.integers(info.min, info.max, size=shape, dtype=t, endpoint=True)


def graphs(dtype, mp, rd, n, rng, batch=1):
    """(batch, n, n) graphs of about EDGES_PER_ROW edges per row whose "no edge" is the element the map absorbs and the
    reduction ignores, where the semiring has one; see the branches for the others."""
    t = sr.NP_DTYPES[dtype]
    shape = (batch, n, n)
    lo, hi = sr.limits(dtype)
    fl = sr.is_float(dtype)
    signed = fl or np.iinfo(t).min < 0
    edge = rng.random(shape) < EDGES_PER_ROW / n
    j = rng.integers(1, WEIGHTS + 1, size=shape)

    def sparse(weights, none):
        return np.where(edge, weights, none).astype(t)

    if mp == "And":
        return _and_graphs(t, rd, shape, rng, fl, signed, edge, j)
    if mp == rd:                      # (Min, Min), (Max, Max): the closure is the graph's extreme value everywhere,
        d = _spread(t, shape, rng, fl, j)   # provided it is off the diagonal: D[a, a] reaches row a and column a only
        d[:, 1 % n, 0] = lo if rd == "Min" else hi
        return d
    if mp in ("Min", "Max"):          # widest path (Min, Max): no edge lowest(); minimax (Max, Min): no edge max()
        none = lo if mp == "Min" else hi
        return np.where(edge, _spread(t, shape, rng, fl, j), none).astype(t)
    if fl:
        if mp == "Add":               # multiples of 1/64; (Add, Max): negative weights, no edge -inf
            return sparse(j / 64.0, np.inf) if rd == "Min" else sparse(-j / 64.0, -np.inf)
        if rd == "Min":               # (Multiply, Min): weights 1 + j / 4096, no edge +inf
            return sparse(1.0 + j / float(WEIGHTS), np.inf)
        return sparse(1.0 / (1.0 + j / float(WEIGHTS)), 0.0)   # (Multiply, Max): their reciprocals, no edge 0
    if mp == "Multiply":
        return _int_multiply_graphs(t, shape, rng)
    return _int_add_graphs(t, rd, shape, rng, signed, edge)


def _name(t):
    return next(k for k, v in sr.NP_DTYPES.items() if v is t)


def _spread(t, shape, rng, fl, j):
    """About WEIGHTS distinct values strictly inside the type's range (never lowest() or max(), the "no edge" values)."""
    if fl:
        return (j / 64.0).astype(t)
    info = np.iinfo(t)
    return rng.integers(int(info.min) + 1, int(info.max) - 1, size=shape, dtype=t, endpoint=True)


def _and_graphs(t, rd, shape, rng, fl, signed, edge, j):
    """The And map yields 0 / 1, so the closure is max(input, reachable) or min(input, 0 / 1).
    (And, Max), floats: the 0 / 1 adjacency (a vertex without an incoming edge stays unreachable: some 0 remain).  Integers: 30 % of the
      vertices have no outgoing edge (rows of 0, which stay 0); elsewhere 45 % zeros, which become 1, among values of at
      least 2, which stay.
    (And, Min): one zero at (a, b) zeroes row a at pivot b and column b at pivot a, and then every entry that is not
      negative: all that a Min can keep is negative input.  Signed types: half of the entries negative, the others above 1
      (they all become 0), zeros on the edges.  Unsigned types have nothing to keep: the closure is 0 by nature."""
    if fl:
        if rd == "Max":
            return edge.astype(t)
        return np.where(edge, 0.0, np.where(rng.random(shape) < 0.5, -j / 64.0, 1.0 + j / 64.0)).astype(t)
    info = np.iinfo(t)
    big = rng.integers(2, info.max, size=shape, dtype=t, endpoint=True)
    if rd == "Max":
        d = np.where(rng.random(shape) < 0.45, t(0), big)
        d[rng.random(shape[:2]) < 0.3] = 0
        return d
    if signed:
        big = np.where(rng.random(shape) < 0.5, rng.integers(info.min, -1, size=shape, dtype=t, endpoint=True), big)
    return np.where(edge, t(0), big)


def _potentials(t, shape, rng, lo, hi):
    """h[u] - h[v] as a (batch, n, n) array, h drawn from [lo, hi]."""
    h = rng.integers(lo, hi, size=shape[:2], endpoint=True)
    return h[:, :, None] - h[:, None, :]


def _int_add_graphs(t, rd, shape, rng, signed, edge):
    """Integer (Add, Min) / (Add, Max) without wrap-around: weights 1 .. W (negated for Max), "no edge" max() / 2 or
    lowest() / 2, so the sum of any two entries stays inside the type.  int8_t has only 63 values between a weight and
    "no edge", so its weights are shifted by potentials, w + h(u) - h(v) with h in [0, 25]: every entry stays within
    25 of the range [1, 63] (a walk with g "no edge" hops telescopes to at least 63 g - 25 (g + 1)), and still no sum wraps.
    Unsigned (Add, Max) has no such form -- a positive cycle through the zeros doubles until it wraps -- so it takes a
    wrapping one: h(u) - h(v) + {0, 2^(bits - 1)} mod 2^bits, dense, whose closure is the larger of x and x + 2^(bits - 1)."""
    info = np.iinfo(t)
    if rd == "Max" and not signed:
        u = np.dtype(t)
        h = rng.integers(0, info.max, size=shape[:2], dtype=t, endpoint=True)
        half = t(1) << t(info.bits - 1)
        with np.errstate(over="ignore"):
            return (h[:, :, None] - h[:, None, :] + np.where(rng.random(shape) < 0.5, half, t(0))).astype(u)
    w = rng.integers(1, _int_weight_range(_name(t)) + 1, size=shape)
    if info.bits == 8 and signed:
        w = w + _potentials(t, shape, rng, 0, 25)
    w, none = (w, int(info.max) // 2) if rd == "Min" else (-w, int(info.min) // 2)
    return np.where(edge, w, none).astype(t)


def _int_multiply_graphs(t, shape, rng):
    """Wrapping products have no absorbing "no edge", and dense full-range operands collapse (0 absorbs, and wins an
    unsigned Min).  Odd values with multiplicative potentials do not: D[u, v] = h(u) w h(v)^-1 mod 2^bits, h odd,
    w in {1, 2^(bits - 1) + 1} (a subgroup: w w = 1).  Every walk from u to v telescopes to h(u) h(v)^-1 times 1 or w, so
    the closure is the smaller (larger) of the two for every entry, and about half of the entries change."""
    info = np.iinfo(t)
    u = sr._UNSIGNED[np.dtype(t).itemsize]
    h = rng.integers(0, np.iinfo(u).max, size=shape[:2], dtype=u, endpoint=True) | u(1)
    with np.errstate(over="ignore"):
        inv = h.copy()                    # Newton: correct to 3 bits, doubling each round
        for _ in range(5):
            inv = inv * (u(2) - h * inv)
        assert np.all(h * inv == 1)
        w = np.where(rng.random(shape) < 0.5, (u(1) << u(info.bits - 1)) | u(1), u(1))
        return (h[:, :, None] * w * inv[:, None, :]).astype(u).view(t)


def stats(d, ref):
    """(share of entries that differ from the input, share of the most common value, number of distinct values)."""
    u = sr._UNSIGNED[ref.dtype.itemsize]
    assert not (ref.dtype.kind == "f" and np.isnan(ref).any()), "the reference holds a NaN"
    bits, counts = np.unique(ref.view(u), return_counts=True)
    return float(np.mean(ref.view(u) != np.asarray(d, dtype=ref.dtype).view(u))), counts.max() / ref.size, bits.size


def assert_informative(dtype, mp, rd, d, ref, what=""):
    """A comparison with a (nearly) constant reference proves little.  `ref`, the closure of graph `d`, must be NaN-free and
      * differ from the input in at least 25 % of its entries,
      * hold no value in more than 60 % of its entries,
      * take at least 64 distinct values (n of them for a graph of n < 64 vertices, whose edges are that few),
    with these exemptions, each asserted to be what it is:
      * map == reduce (Min, Min / Max, Max): the closure is the graph's extreme value everywhere, by nature -- only
        "changed" is asked, and the witness variant carries the information;
      * unsigned (And, Min): all 0 by nature (_and_graphs) -- the same;
      * floating (And, Max): 0 / 1 results, both present, as _semiring_ref.assert_not_degenerate asks;
      * integer Multiply maps: wrapping products have no absorbing "no edge" -- at least 3 distinct values."""
    changed, top, distinct = stats(d, ref)
    what = f"{what} ({dtype}, {mp}, {rd}), n = {ref.shape[0]}: changed {changed:.2f}, top share {top:.2f}, {distinct} distinct"
    assert changed >= 0.25, what
    fl = sr.is_float(dtype)
    if mp == rd:
        assert mp in REDUCTIONS and distinct == 1 and ref[0, 0] == (d.min() if rd == "Min" else d.max()), what
    elif mp == "And" and rd == "Min" and not fl and np.iinfo(ref.dtype).min == 0:
        assert distinct == 1 and ref[0, 0] == 0, what
    elif mp == "And" and rd == "Max" and fl:
        assert set(np.unique(ref).tolist()) == {0, 1}, what
    elif mp == "Multiply" and not fl:
        assert distinct >= 3, what
    else:
        assert top <= 0.60 and distinct >= min(64, ref.shape[0]), what
