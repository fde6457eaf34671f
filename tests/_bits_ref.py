"""numpy restatements of the bit-packed Boolean calls (mm_bits_*): the storage format, the product and the closure.  Boolean
matrices are numpy bool arrays; packed ones are uint32 arrays, column j in bit j & 31 of word j >> 5."""
import numpy as np


def words(cols):
    return (cols + 31) // 32


def pack(x, ld=None, fill=0):
    """(..., rows, cols) bool / uint8 -> (..., rows, ld) uint32, ld >= words(cols); nonzero is 1, padding bits are 0, the words
    beyond the row's own hold `fill`."""
    x = np.asarray(x) != 0
    cols = x.shape[-1]
    w = words(cols)
    ld = w if ld is None else ld
    assert ld >= w
    by = np.packbits(x, axis=-1, bitorder="little")
    pad = 4 * w - by.shape[-1]
    by = np.concatenate([by, np.zeros(by.shape[:-1] + (pad,), np.uint8)], axis=-1)
    out = np.full(x.shape[:-1] + (ld,), fill, dtype=np.uint32)
    out[..., :w] = np.ascontiguousarray(by).view("<u4").reshape(x.shape[:-1] + (w,))
    return out


def unpack(p, cols):
    """(..., rows, >= words(cols)) uint32 -> (..., rows, cols) bool; padding bits and further words are ignored."""
    p = np.ascontiguousarray(np.asarray(p)[..., :words(cols)]).astype("<u4")
    by = p.view(np.uint8).reshape(p.shape[:-1] + (4 * words(cols),))
    return np.unpackbits(by, axis=-1, bitorder="little")[..., :cols].astype(bool)


def matmul(a, b):
    """Boolean product of bool arrays (..., n, k) and (..., k, m)."""
    return (a.astype(np.int32) @ b.astype(np.int32)) > 0


def closure(d):
    """Transitive closure (paths of one or more edges) of an (n, n) bool array: Warshall."""
    d = np.array(d, dtype=bool)
    for v in range(d.shape[0]):
        d |= np.outer(d[:, v], d[v, :])
    return d


def density(k):
    """Operand density at which about half the outputs of a product over k are set."""
    return min(1.0, float(np.sqrt(np.log(2.0) / k)))


def graph(n, seed):
    """G(n, 1.5 / n), the closure tests' graphs."""
    return np.random.default_rng(seed * 1000 + n).random((n, n)) < 1.5 / n
