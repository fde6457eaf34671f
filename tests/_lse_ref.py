"""numpy restatement of the log-semiring product (include/mm_gemm.h, mm_gemm_logsumexp_*): the terms s_k = A[i,k] + B[k,j]
are formed in the computation type (f32 for half and float, f64 for double) and reduced in float64 (np.longdouble for
double), with torch.logsumexp's special-value rules; and the documented error bound for finite outputs."""
import numpy as np

U = {"half": 2.0 ** -24, "float": 2.0 ** -24, "double": 2.0 ** -53}
COMPUTE = {"half": np.float32, "float": np.float32, "double": np.float64}


def lse_terms(terms, axis):
    """log sum exp over `axis` with torch.logsumexp's special values: a NaN term -> NaN; else any +inf -> +inf; else all
    -inf -> -inf; else the shifted sum."""
    t = np.asarray(terms)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        nan = np.isnan(t).any(axis=axis)
        pinf = (t == np.inf).any(axis=axis)
        mx = np.max(np.where(np.isnan(t), -np.inf, t), axis=axis)
        safe = np.where(np.isfinite(mx), mx, 0)
        r = safe + np.log(np.sum(np.exp(t - np.expand_dims(safe, axis)), axis=axis))
    r = np.where(mx == -np.inf, -np.inf, r)
    r = np.where(pinf, np.inf, r)
    return np.where(nan, np.nan, r)


def logsumexp_ref(a, b, dtype="float", reduce_op="Max", seed=None, transposed_a=False):
    """C (in the reference type: float64, np.longdouble for double) of one problem: a (N, K) -- or (K, N) with
    transposed_a -- b (K, M), seed (N, M) or None."""
    ct = COMPUTE[dtype]
    wide = np.longdouble if dtype == "double" else np.float64
    A = np.asarray(a).T if transposed_a else np.asarray(a)
    sg = -1.0 if reduce_op == "Min" else 1.0
    with np.errstate(invalid="ignore", over="ignore"):
        terms = (A.astype(ct)[:, :, None] + np.asarray(b).astype(ct)[None, :, :]).astype(wide) * sg
    if seed is not None:
        terms = np.concatenate([terms, (np.asarray(seed).astype(wide) * sg)[:, None, :]], axis=1)
    return sg * lse_terms(terms, 1)


def bound(a, b, ref, dtype="float", reduce_op="Max", transposed_a=False):
    """The elementwise bound on |C - C*| for finite outputs (include/mm_gemm.h):
    u (4 (|ra_i| + |rb_j|) + 4 |C*| + 2 K + 512), plus 2^-11 |C*| for half."""
    A = (np.asarray(a).T if transposed_a else np.asarray(a)).astype(np.float64)
    B = np.asarray(b).astype(np.float64)
    sg = -1.0 if reduce_op == "Min" else 1.0
    k = A.shape[1]
    with np.errstate(invalid="ignore"):
        ra = np.max(np.where(np.isnan(A), -np.inf, sg * A), axis=1) if k else np.zeros(A.shape[0])
        rb = np.max(np.where(np.isnan(B), -np.inf, sg * B), axis=0) if k else np.zeros(B.shape[1])
    ra = np.where(np.isfinite(ra), ra, 0)
    rb = np.where(np.isfinite(rb), rb, 0)
    c = np.abs(np.asarray(ref, dtype=np.float64))
    c = np.where(np.isfinite(c), c, 0)
    bnd = U[dtype] * (4 * (np.abs(ra)[:, None] + np.abs(rb)[None, :]) + 4 * c + 2 * k + 512)
    if dtype == "half":
        bnd = bnd + 2.0 ** -11 * c
    return bnd


def check(c, ref, a, b, dtype="float", reduce_op="Max", transposed_a=False, what=""):
    """Special values exactly (NaN, +inf, -inf where the reference has them), finite outputs within the bound; a finite
    reference beyond half's range must be +-inf."""
    c = np.asarray(c, dtype=np.float64)
    r = np.asarray(ref, dtype=np.float64)
    if dtype == "half":   # the rounding on store: finite values beyond 65504 (+ half an ulp) become +-inf
        r = np.where(np.abs(r) >= 65520.0, np.sign(r) * np.inf, r)
    assert np.array_equal(np.isnan(c), np.isnan(r)), f"{what}: NaN positions differ"
    fin = np.isfinite(r)
    assert np.array_equal(c[~fin & ~np.isnan(r)], r[~fin & ~np.isnan(r)]), f"{what}: infinities differ"
    assert np.isfinite(c[fin]).all(), f"{what}: a finite reference gave a non-finite result"
    bnd = bound(a, b, ref, dtype, reduce_op, transposed_a)
    with np.errstate(invalid="ignore"):   # inf - inf where both are the same infinity: masked out below
        err = np.abs(c - r)
    bad = fin & (err > bnd)
    assert not bad.any(), (f"{what}: {int(bad.sum())} outputs beyond the bound, worst err {err[bad].max()} "
                           f"vs bound {bnd[bad].min()}")
    return float(err[fin].max()) if fin.any() else 0.0


# ---- operands that need the hybrid's fallback, and the batch that puts them inside a batched call ----------------------------
NP = {"half": np.float16, "float": np.float32, "double": np.float64}
DEPTH = {"half": 120, "float": 120, "double": 800}   # exp(-depth) is 0 in the computation type, and S below tau (2^-64, f64: 2^-512)


def adversarial(dtype, red, n, k, m, rows, cols, depth, seed=3, spread=1.0):
    """(a (n, k), b (k, m)) of uniform(-spread, spread) data in which rows `rows` of A are about 0 over the first half of K and
    about -depth over the second, and columns `cols` of B the mirror image: every term of that block sits about `depth` below
    ra + rb.  Min: the pair negated.  Asserted here, per call: the reference on the block is finite with |ref| > depth - 10,
    and the shifted pipeline log(exp(a - ra) @ exp(b - rb)) + ra + rb in the computation type returns an infinity on all of
    it -- without the exact kernel's tiles the answer would be wrong."""
    rng = np.random.default_rng(seed)
    h = k // 2
    nr, nc = len(range(*rows.indices(n))), len(range(*cols.indices(m)))
    a = rng.uniform(-spread, spread, size=(n, k))
    b = rng.uniform(-spread, spread, size=(k, m))
    a[rows, :h] = rng.uniform(-0.5, 0.5, size=(nr, h))
    a[rows, h:] = -depth + rng.uniform(-0.5, 0.5, size=(nr, k - h))
    b[:h, cols] = -depth + rng.uniform(-0.5, 0.5, size=(h, nc))
    b[h:, cols] = rng.uniform(-0.5, 0.5, size=(k - h, nc))
    sg = -1 if red == "Min" else 1
    a, b = (sg * a).astype(NP[dtype]), (sg * b).astype(NP[dtype])
    ref = logsumexp_ref(a[rows], b[:, cols], dtype, red)
    assert np.isfinite(ref).all() and (np.abs(ref.astype(np.float64)) > depth - 10).all(), "the block's reference"
    ct = COMPUTE[dtype]
    sa, sb = sg * a.astype(ct), sg * b.astype(ct)
    ra, rb = sa.max(axis=1, keepdims=True), sb.max(axis=0, keepdims=True)
    with np.errstate(divide="ignore", under="ignore"):
        shifted = np.log(np.exp(sa - ra) @ np.exp(sb - rb)) + ra + rb
    assert shifted.dtype == ct and np.isinf(shifted[rows, cols]).all(), "the shifted pipeline was expected to lose the block"
    return a, b


# 3 x 4 tiles of 64 x 64, a two-row last tile row and an eight-column last tile column, K padded from 72 to 128
FB_SHAPE = (130, 72, 200)
FB_BATCH = 5
# element -> (rows, cols) of its adversarial block: element 1 flags tiles 5 and 9 (the ragged tile row), element 4 tiles 2 and 3
FB_BLOCKS = {1: (slice(100, 130), slice(64, 128)), 4: (slice(0, 64), slice(128, 200))}
# the 64 x 64 tiles those blocks touch, as (rows, cols): what the exact kernel recomputes
FB_TILES = {1: (slice(64, 130), slice(64, 128)), 4: (slice(0, 64), slice(128, 200))}
FB_NAN = (2, 70, 30)      # A[e, i, k]: row 70 of element 2 is NaN
FB_INF_ROW = (3, 5)       # A[e, i, :]: row 5 of element 3 is -inf (Min: +inf), every term of it
_FB = {}


def _frozen(x):
    x.setflags(write=False)
    return x


def fallback_batch(dtype, red):
    """The batch of 5 the fallback and chunking tests share (built once per (dtype, red), read-only): elements 0, 2 and 3
    uniform(-5, 5), elements 1 and 4 adversarial() on FB_BLOCKS -- two elements that flag DIFFERENT tiles, in chunks 0 and 2
    of a 2 + 2 + 1 split.  Returns a dict of
      a (5, N, K), b (5, K, M);
      seed (5, N, M): uniform(-8, 8) with one row of -inf (Min: +inf), a term that adds nothing, and for Min a row of -inf
        as well, which is then the output;
      a_special: a with one NaN in element 2 (FB_NAN) and a row of -inf (Min: +inf) in element 3 (FB_INF_ROW);
      ref, ref_seeded, ref_special: the references of all five elements."""
    if (dtype, red) not in _FB:
        n, k, m = FB_SHAPE
        rng = np.random.default_rng(41)
        a = rng.uniform(-5, 5, size=(FB_BATCH, n, k)).astype(NP[dtype])
        b = rng.uniform(-5, 5, size=(FB_BATCH, k, m)).astype(NP[dtype])
        for e, (rows, cols) in FB_BLOCKS.items():
            a[e], b[e] = adversarial(dtype, red, n, k, m, rows, cols, DEPTH[dtype], seed=50 + e, spread=5.0)
        seed = rng.uniform(-8, 8, size=(FB_BATCH, n, m)).astype(NP[dtype])
        seed[:, 101, :] = np.inf if red == "Min" else -np.inf     # the reduction's identity, inside element 1's block
        if red == "Min":
            seed[:, 70, :] = -np.inf                              # a row of -inf absorbs a soft-min: -inf out (in no block)
        ref = np.stack([logsumexp_ref(a[e], b[e], dtype, red) for e in range(FB_BATCH)])
        ref_seeded = np.stack([logsumexp_ref(a[e], b[e], dtype, red, seed[e]) for e in range(FB_BATCH)])
        a_special = a.copy()
        a_special[FB_NAN] = np.nan
        a_special[FB_INF_ROW] = np.inf if red == "Min" else -np.inf
        ref_special = ref.copy()
        for e in (FB_NAN[0], FB_INF_ROW[0]):
            ref_special[e] = logsumexp_ref(a_special[e], b[e], dtype, red)
        parts = dict(a=a, b=b, seed=seed, a_special=a_special, ref=ref, ref_seeded=ref_seeded, ref_special=ref_special)
        _FB[dtype, red] = {key: _frozen(v) for key, v in parts.items()}
    return _FB[dtype, red]
