"""numpy restatements of the packed counting calls (mm_bits_count_*, mm_bits_transpose_*) on bool arrays; the storage format is
_bits_ref's (pack / unpack, imported from there)."""
import numpy as np

from _bits_ref import pack, unpack, words  # noqa: F401  (the format, for the tests that import this module)

OPS = {"And": 0, "Xor": 1}


def count_and(a, bt):
    """sum_k a[..., i, k] & bt[..., j, k] of bool arrays (..., n, k) and (..., m, k), as int64."""
    return a.astype(np.int64) @ np.swapaxes(bt, -1, -2).astype(np.int64)


def count(a, bt, op="And", seed=None):
    """The counting product as int32, mod 2^32: op "And" or "Xor" (pop(a) + pop(bt) - 2 and), plus an int32 seed."""
    c = count_and(a, bt)
    if op == "Xor":
        c = a.sum(-1, dtype=np.int64)[..., :, None] + bt.sum(-1, dtype=np.int64)[..., None, :] - 2 * c
    else:
        assert op == "And", op
    if seed is not None:
        c = c + seed.astype(np.int64)
    return (c & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def transpose(x):
    """(..., rows, cols) bool -> (..., cols, rows)."""
    return np.ascontiguousarray(np.swapaxes(x, -1, -2))


def distinct_values(c):
    return len(np.unique(c))
