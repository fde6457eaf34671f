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
