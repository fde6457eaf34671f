"""CPU tests of tests/_limit_cases.py, the cases tests/test_gpu_launch_limits.py runs: each names the kernel its row says,
crosses its limit by at least a quarter of it (L1 - L4; L5 and L6 cross by whole rows of tiles), stays inside its memory
budget, and the limits it was written against are still the ones in the source."""
import os
import re

import pytest

import _limit_cases as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _source(name):
    return open(os.path.join(ROOT, "gemm_hls_amd", "csrc", name)).read()


def _function(text, header):
    """The text of the function that starts at `header`, up to the first line that closes a top-level brace."""
    start = text.index(header)
    return text[start:text.index("\n}\n", start)]


def test_the_literals_are_the_ones_in_the_source():
    capi = _source("mm_capi.hip")
    assert lc.CHUNK_TILES == 1 << 22 and "(1ull << 22) / tiles" in _function(capi, "unsigned chunk_of_tiles(")
    assert lc.TRANSPOSE_MATRICES == 65535
    transpose = _function(_source("mm_transpose.hip"), "int launch_transpose_t(")
    assert "e0 += 65535u" in transpose and "std::min(65535u, count - e0)" in transpose
    assert lc.CLOSURE_GRAPHS == 1 << 20
    for header in ("int dispatch_closure(", "int dispatch_bits_closure("):
        assert re.search(r"const unsigned chunk = 1u << 20;", _function(capi, header)), header
    assert lc.MAX_GRID == 1 << 20
    for name in ("mm_bits.hip", "mm_bits_count.hip"):
        assert _source(name).count("constexpr unsigned long long kMaxGrid = 1ull << 20;") == 1, name
    # the tile chunk_of_tiles() counts in, and the tile and block whose rows the L5 launches count in gridDim.y or past it
    assert "(p.n + 63) / 64) * ((p.m + 63) / 64)" in _function(capi, "unsigned batch_chunk(")
    assert lc.TILE == 64 and "constexpr int kTile = 64," in _source("mm_tile64.h")
    # L5: the three single launches that put rows of tiles (of blocks) into gridDim.y; once one of them goes 1-D, its L5
    # case is an L6 case
    assert lc.GRID_Y == 65535
    assert "dim3(tiles_m, tiles_n)" in _function(_source("mm_ordered.hip"), "int launch_at(")
    assert "dim3(tiles_m, tiles_n)" in _function(_source("mm_widen_ordered.hip"), "int launch_typed(")
    assert _function(_source("mm_mfma_f32_split.hip"), "int launch_mfma_f32_split(").count("dim3(slabs, blocks_") == 3
    assert lc.SPLIT_BLOCK == 256 and "blocks_a = (p.n + 255) / 256, blocks_b = (p.m + 255) / 256" in _source("mm_mfma_f32_split.hip")


def test_chunk_of_tiles_restated():
    assert lc.chunk_of_tiles(1, lc.BATCH_L1) == 1 << 22
    assert lc.chunk_of_tiles(3, lc.BATCH_L1) == (1 << 22) // 3
    assert lc.chunk_of_tiles(1 << 23, 5) == 1 and lc.chunk_of_tiles(1, 7) == 7
    # the batches cut where the GPU tests look: a second launch from e0 = 2^22, three transposition launches, e0 = 2^20
    assert lc.BATCH_L1 - lc.chunk_of_tiles(1, lc.BATCH_L1) == (1 << 21) + 3
    assert -(-lc.BATCH_L2 // lc.TRANSPOSE_MATRICES) == 3
    assert -(-lc.BATCH_L3 // lc.CLOSURE_GRAPHS) == 2


NAMED = [c for c in lc.CASES if c.kernel]


@pytest.mark.parametrize("c", NAMED, ids=[c.id for c in NAMED])
def test_case_names_its_kernel(c):
    name = lc.kernel_name(c)
    assert name.startswith(c.kernel), name
    if c.kernel in ("ordered", "valu_tile"):     # (not ordered_tile, ordered_wide_f16, valu_tile_nt)
        assert name == c.kernel, name


@pytest.mark.parametrize("c", lc.CASES, ids=[c.id for c in lc.CASES])
def test_case_crosses_its_limit_inside_its_budget(c):
    work, limit = lc.work_and_limit(c)
    if c.limit in ("L1", "L2", "L3", "L4"):
        assert 4 * work >= 5 * limit, (work, limit)
    else:
        assert work > limit, (work, limit)
    if c.limit in ("L1", "L2", "L3"):
        assert lc.tiles64(c.n, c.m) == 1                       # one tile per element: the launch boundary is the limit itself
    budget = lc.BUDGET_SPLIT if "split" in c.id else lc.BUDGET
    assert lc.device_bytes(c) < budget, (lc.device_bytes(c) / 2**30, budget / 2**30)


def test_the_strided_part_of_each_conversion_holds_an_element_boundary_and_a_ragged_row_end():
    for c in lc.CASES:
        if c.limit != "L4":
            continue
        work, limit = lc.work_and_limit(c)
        per_element = work // c.batch
        assert (c.batch - 1) * per_element > limit, c.id      # the last element starts in the strided part
        ragged = {"pack_bits": c.m % 64, "unpack_bits": c.m % 256, "transpose_bits": c.m % 32}[c.call]
        assert ragged != 0, c.id


def test_the_l2_cases_fit_one_workspace_chunk():
    for c in lc.CASES:
        if c.limit == "L2":
            km = c.k * c.m * lc.ELEMENT_SIZE[c.dtype]
            assert km <= 1024 and (256 << 20) // km >= c.batch, c.id   # kNtWorkspaceCap, mm_capi.hip dispatch_nt_prepass()
    assert "kNtWorkspaceCap = 256ull << 20" in _source("mm_capi.hip")
