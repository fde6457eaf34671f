"""numpy references of the product calls that go beyond the plain semiring product of _semiring_ref.reference(): the seeded
(accumulating) product and its (Multiply, Add) bound, the argmin / argmax contract, and the widening products.  Each one is the
contract of include/mm_gemm.h written on _semiring_ref's operators; the feature tests and the shape fuzz share them.

TEST INFRASTRUCTURE ONLY."""
import numpy as np

import _semiring_ref as sr


# ---- accumulating calls (mm_gemm_accumulate_*, mm_gemm_batched_accumulate_*) ----------------------------------------------
def seeded_reference(dtype, mp, rd, a, b, c0, transposed_a=False, auto_minmax=False):
    """Naive (include/Utility.h:18-42) with acc = C[i][j] in place of identity()."""
    t = sr.NP_DTYPES[dtype]
    a = np.asarray(a, dtype=t)
    if transposed_a:
        a = a.T
    acc = np.array(c0, dtype=t, copy=True)
    with np.errstate(all="ignore"):
        for kk in range(a.shape[1]):
            acc = sr._apply(rd, acc, sr._apply(mp, a[:, kk:kk + 1], b[kk:kk + 1, :], t, auto_minmax), t, auto_minmax)
    return acc


MUL_ADD_TOL = {"float": 1e-5, "double": 1e-12, "half": 2e-3}


def within_bound(dtype, got, a, b, c0, ta=False):
    """|C - (C_in + A B)| <= tol (|C_in| + |A||B|) elementwise."""
    exact, scale = sr.exact_and_scale(dtype, a, b, ta) if dtype != "double" else (
        (a.T if ta else a) @ b, np.abs(a.T if ta else a) @ np.abs(b))
    exact = exact + c0.astype(exact.dtype)
    scale = scale + np.abs(c0.astype(exact.dtype)) + np.finfo(sr.NP_DTYPES[dtype]).tiny
    err = float(np.max(np.abs(got.astype(exact.dtype) - exact) / scale))
    return err < MUL_ADD_TOL[dtype], err


# ---- argmin / argmax (mm_gemm_argreduce_*, mm_gemm_argreduce_nt_*) ---------------------------------------------------------
def oracle(dtype, mp, rd, a, b, c0=None, i0=None, transposed_a=False, index_base=0):
    t = sr.NP_DTYPES[dtype]
    a = np.asarray(a, dtype=t)
    if transposed_a:
        a = a.T
    n, k = a.shape
    m = b.shape[1]
    acc = np.full((n, m), sr.identity(dtype, rd), dtype=t) if c0 is None else np.array(c0, dtype=t, copy=True)
    idx = np.full((n, m), -1, dtype=np.int32) if i0 is None else np.array(i0, dtype=np.int32, copy=True)
    with np.errstate(all="ignore"):
        for kk in range(k):
            s = sr._apply(mp, a[:, kk:kk + 1], b[kk:kk + 1, :], t, False)
            take = (s < acc) if rd == "Min" else (acc < s)
            acc = np.where(take, s, acc)
            idx = np.where(take, np.int32(index_base + kk), idx)
    return acc, idx


# ---- widening (mm_gemm_widen_*) -----------------------------------------------------------------------------------------------
def _int_ref(a, b, seed=None):
    s = a.astype(np.int64) @ b.astype(np.int64)
    return (s if seed is None else s + seed.astype(np.int64)).astype(np.int32)      # the cast wraps mod 2^32


def _f32_loop(a, b, seed=None):
    """acc = seed or 0; for k ascending: acc = acc + (float)a * (float)b, each operation rounded to float32 (numpy does not fuse)."""
    a32, b32 = a.astype(np.float32), b.astype(np.float32)
    acc = np.zeros((a.shape[0], b.shape[1]), np.float32) if seed is None else seed.astype(np.float32).copy()
    with np.errstate(all="ignore"):
        for kk in range(a.shape[1]):
            acc = acc + a32[:, kk, None] * b32[None, kk, :]
    return acc


def _check_bound(what, c, a, b, seed=None, rel=1e-6):
    exact = a.astype(np.float64) @ b.astype(np.float64)
    scale = np.abs(a.astype(np.float64)) @ np.abs(b.astype(np.float64))
    if seed is not None:
        exact, scale = exact + seed.astype(np.float64), scale + np.abs(seed.astype(np.float64))
    err, bound = np.abs(c.astype(np.float64) - exact), rel * scale
    bad = np.argwhere(~(err <= bound))
    print(f"{what}: max err / bound = {np.max(err / np.maximum(bound, 1e-300)):.3f}")
    assert bad.size == 0, f"{what}: |c - exact| {err[tuple(bad[0])]!r} above the bound {bound[tuple(bad[0])]!r} at {tuple(bad[0])} ({len(bad)} elements)"
