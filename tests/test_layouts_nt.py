"""CPU model of valu_tile_nt's Bt slab (gemm_hls_amd/csrc/mm_valu_tile_nt.inc; no GPU needed), for every element size:
  * the eight 1-KiB LDS-DMA pieces (lane-linear destination, 16-byte chunk index ^ (col >> 2) & 3 on the SOURCE) are replayed
    into a byte image, and every (col, k) is found where the kernel's reads look for it;
  * one wavefront's Bt reads of a k-step -- a thread owns columns tx + 16 j and reads KSTEP consecutive k per column -- are
    replayed per hardware service group: the two 32-lane halves of ds_read_b64 (elements of up to 4 bytes: 8-byte reads), the
    four 16-lane groups of ds_read_b128 (8-byte elements: 16-byte reads); bank = (addr / 4) % 64 for both;
  * the column ownership valu_tile uses for a K x M B (tx * 4 + e) is shown to conflict on this image: the reason for the
    other one."""
import itertools

import pytest

from test_layouts import assert_conflict_free_b128, b64_half_banks_disjoint

COLS, ROW_BYTES = 128, 64


def geometry(es):
    """(BK, KSTEP, threads): slab depth, k per LDS read, workgroup size (TI = 4 rows per thread on 512 threads for 8 bytes)."""
    return 64 // es, (2 if es >= 4 else 8 // es), (512 if es == 8 else 256)


def dma_image(es):
    """byte address -> (col, k) of the element whose first byte lies there, after the 8 pieces of one slab."""
    image = {}
    for piece, lane in itertools.product(range(8), range(64)):
        col, pc = piece * 16 + lane // 4, lane % 4
        src_chunk = pc ^ ((col >> 2) & 3)                 # the 16 bytes this lane fetches from its column's 64
        dst = piece * 1024 + lane * 16                    # lane-linear
        for e in range(16 // es):
            image[dst + e * es] = (col, (src_chunk * 16) // es + e)
    return image


def read_addr(es, tx, j, kk):
    """Byte address of the PK read of thread column j at k-step kk."""
    kb = kk * es
    return (tx + 16 * j) * ROW_BYTES + (((kb >> 4) ^ ((tx >> 2) & 3)) * 16) + (kb & 15)


@pytest.mark.parametrize("es", [1, 2, 4, 8])
def test_nt_bt_slab_dma_roundtrip(es):
    bk, kstep, _ = geometry(es)
    image = dma_image(es)
    assert len(image) == COLS * bk and sorted(image.values()) == sorted(itertools.product(range(COLS), range(bk)))
    for tx, j, kk in itertools.product(range(16), range(8), range(0, bk, kstep)):
        a = read_addr(es, tx, j, kk)
        assert a % (kstep * es) == 0                      # the PK read is naturally aligned
        for q in range(kstep):
            assert image[a + q * es] == (tx + 16 * j, kk + q), (tx, j, kk, q)


@pytest.mark.parametrize("es", [1, 2, 4, 8])
def test_nt_bt_reads_of_a_wavefront_are_conflict_free(es):
    bk, kstep, threads = geometry(es)
    for wave, j, kk in itertools.product(range(threads // 64), range(8), range(0, bk, kstep)):
        def addr(lane):
            return read_addr(es, (wave * 64 + lane) % 16, j, kk)
        if kstep * es == 16:
            assert_conflict_free_b128(addr)
        else:
            assert kstep * es == 8
            b64_half_banks_disjoint(addr, range(0, 32))
            b64_half_banks_disjoint(addr, range(32, 64))


@pytest.mark.parametrize("es", [1, 2, 4, 8])
def test_nt_a_reads_keep_valu_tiles_layout(es):
    """A's slab is valu_tile_dma_kernel's: the rows of the 2 (b128: 1-2) ty values a service group holds fall into different slots."""
    bk, kstep, threads = geometry(es)
    ti = 4 if es == 8 else 8
    for wave, i, kk in itertools.product(range(threads // 64), range(ti), range(0, bk, kstep)):
        def addr(lane):
            ty = (wave * 64 + lane) // 16
            row = (ty * 4 + i if i < 4 else 64 + ty * 4 + (i - 4)) if ti == 8 else ty * 4 + i
            kb = kk * es
            return row * ROW_BYTES + (((kb >> 4) ^ (ty & 3)) * 16) + (kb & 15)
        if kstep * es == 16:
            for grp_addrs in ([addr(l) for l in range(h, h + 32)] for h in (0, 32)):
                assert len({(a // 16) % 16 for a in set(grp_addrs)}) == len(set(grp_addrs))
        else:
            b64_half_banks_disjoint(addr, range(0, 32))
            b64_half_banks_disjoint(addr, range(32, 64))


def test_nt_row_major_column_ownership_would_conflict():
    """Columns tx * 4 + e (valu_tile's, right for a K x M slab) put the 16 tx lanes of one read on rows 256 bytes apart."""
    def addr(lane):
        col = (lane % 16) * 4
        return col * ROW_BYTES + ((0 ^ ((col >> 2) & 3)) * 16)
    with pytest.raises(AssertionError):
        b64_half_banks_disjoint(addr, range(0, 32))
