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
