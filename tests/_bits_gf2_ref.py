"""numpy restatements of the bit-packed product over GF(2) (mm_bits_gf2_*): the definition on bool arrays, and the table scheme
of the bits_gf2_tile kernel (the Method of the Four Russians) on packed words, index for index."""
import numpy as np

from _bits_ref import pack, unpack, words  # noqa: F401  (the storage format is the Boolean calls')


def matmul(a, b):
    """Product over GF(2) of bool arrays (..., n, k) and (..., k, m): XOR_k (a AND b)."""
    return ((a.astype(np.int64) @ b.astype(np.int64)) & 1).astype(bool)


SLAB = 32      # k per slab: one word of A per row
GROUPS = 8     # groups of 4 consecutive k per slab, one table of 16 entries each


def tables(pb, k_total, s):
    """T[g][v] of slab s, (8, 16, words): the XOR of rows 32 s + 4 g + b of the packed B over the bits b of v, built in
    Gray-code order -- entry i ^ (i >> 1) is the entry before it XOR row ctz(i).  Rows at k >= k_total count as zero."""
    w = pb.shape[1]
    t = np.zeros((GROUPS, 16, w), np.uint32)
    for g in range(GROUPS):
        rows = [pb[k] if k < k_total else np.zeros(w, np.uint32) for k in range(s * SLAB + 4 * g, s * SLAB + 4 * g + 4)]
        cur = np.zeros(w, np.uint32)
        for i in range(1, 16):
            cur = cur ^ rows[(i & -i).bit_length() - 1]
            t[g][i ^ (i >> 1)] = cur
    return t


def table_product(pa, pb, k_total, m):
    """Packed C (n, words(m)) of packed pa (n, >= words(k_total)) and pb (>= k_total rows, words(m)) by the table scheme: per
    slab and row one entry per nibble of A's word, A's last word masked with the K tail, C's last word with the M tail.
    Padding bits of pa and pb may hold anything."""
    n, mw, kw = pa.shape[0], words(m), words(k_total)
    k_tail = np.uint32((1 << (k_total & 31)) - 1 if k_total & 31 else 0xFFFFFFFF)
    m_tail = np.uint32((1 << (m & 31)) - 1 if m & 31 else 0xFFFFFFFF)
    c = np.zeros((n, mw), np.uint32)
    for s in range(kw):
        t = tables(pb[:, :mw], k_total, s)
        for i in range(n):
            a = int(pa[i, s] & k_tail) if s == kw - 1 else int(pa[i, s])
            for g in range(GROUPS):
                c[i] ^= t[g][(a >> (4 * g)) & 15]
    c[:, -1] &= m_tail
    return c
