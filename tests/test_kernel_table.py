"""CPU tests of the matrix-core families' kernel tables (mm_mfma_*_kernels.inc, mm_mfma_f64.hip): what mm_kernel_name,
mm_kernel_name_batched and mm_kernel_info answer for the smallest shapes, knob values and layouts that reach every row.  The
expected values were recorded from the library as it was before the tables existed (names by a parallel array, geometry read
off the kernel's name): the tables must describe every kernel exactly as that code did.  No device is touched."""
import os
import re

import pytest

import gemm_hls_amd as g

# (dtype, knob or None, K x N A, n, k, m, mm_kernel_name, mm_kernel_name_batched at batch 1,
#  (tile_n, tile_m, tile_k, wavefronts, inst_n, inst_m, inst_k, ops_per_clk_per_cu), measured_issue_efficiency)
# The single launch picks its tile by the shape (small problems: the 64 x 256 slab kernels); the batched resolver runs a
# ping-pong kernel wherever one serves.  A knob value the library does not have: "unsupported", described as the catch-all.
CASES = [
    ("half", None, False, 256, 256, 256, "mfma_f16_64x256x64_slab64", "mfma_f16_256x256_pingpong_16x16x32", (64, 256, 64, 4, 32, 32, 16, 4096.0), 0.67),
    ("half", ("f16_variant", 100), False, 256, 256, 256, "mfma_f16_256x256_pingpong_32x32x16", "mfma_f16_256x256_pingpong_32x32x16", (256, 256, 32, 8, 32, 32, 16, 4096.0), 0.9),
    ("half", None, False, 256, 128, 256, "mfma_f16_64x256x64_slab64", "mfma_f16_256x256_pingpong_k32", (64, 256, 64, 4, 32, 32, 16, 4096.0), 0.67),
    ("half", None, False, 256, 48, 256, "mfma_f16_64x256x64_slab64", "mfma_f16_64x256x64_slab64", (64, 256, 64, 4, 32, 32, 16, 4096.0), 0.67),
    ("half", None, False, 512, 512, 512, "mfma_f16_64x256x64_slab64", "mfma_f16_256x256_pingpong_16x16x32", (64, 256, 64, 4, 32, 32, 16, 4096.0), 0.67),
    ("half", ("f16_variant", 200), False, 256, 256, 256, "mfma_f16_256x256_pingpong_16x16x32", "mfma_f16_256x256_pingpong_16x16x32", (256, 256, 32, 8, 16, 16, 32, 4096.0), 0.91),
    ("half", ("f16_variant", 11), False, 256, 128, 256, "mfma_f16_256x256_pingpong_k32", "mfma_f16_256x256_pingpong_k32", (256, 256, 32, 8, 32, 32, 16, 4096.0), 0.9),
    ("half", None, False, 4096, 4096, 4096, "mfma_f16_256x256_pingpong_16x16x32", "mfma_f16_256x256_pingpong_16x16x32", (256, 256, 32, 8, 16, 16, 32, 4096.0), 0.91),
    ("half", None, False, 4096, 160, 4096, "mfma_f16_256x256_pingpong_k32", "mfma_f16_256x256_pingpong_k32", (256, 256, 32, 8, 32, 32, 16, 4096.0), 0.9),
    ("half", None, False, 4096, 48, 4096, "mfma_f16_256x256x64_slab64", "mfma_f16_256x256x64_slab64", (256, 256, 64, 8, 32, 32, 16, 4096.0), 0.67),
    ("half", None, True, 256, 256, 256, "mfma_f16_256x256_pingpong_k32_KxN", "mfma_f16_256x256_pingpong_k32_KxN", (256, 256, 32, 8, 32, 32, 16, 4096.0), 0.9),
    ("half", None, True, 256, 48, 256, "mfma_f16_256x256x64_slab64_KxN", "mfma_f16_256x256x64_slab64_KxN", (256, 256, 64, 8, 32, 32, 16, 4096.0), 0.67),
    ("half", ("f16_variant", 0), False, 256, 48, 256, "mfma_f16_256x256x64_slab64", "mfma_f16_256x256x64_slab64", (256, 256, 64, 8, 32, 32, 16, 4096.0), 0.67),
    ("half", ("f16_variant", 4), False, 256, 48, 256, "mfma_f16_128x256x64_slab64", "mfma_f16_128x256x64_slab64", (128, 256, 64, 4, 32, 32, 16, 4096.0), 0.67),
    ("half", ("f16_variant", 5), False, 256, 48, 256, "mfma_f16_64x256x64_slab64", "mfma_f16_64x256x64_slab64", (64, 256, 64, 4, 32, 32, 16, 4096.0), 0.67),
    ("half", ("f16_variant", 99), False, 256, 256, 256, "unsupported", "ordered_wide_f16", (256, 256, 64, 8, 32, 32, 16, 4096.0), 0.67),
    ("int8_t", None, False, 512, 512, 512, "mfma_i8_64x256x128_slab128", "mfma_i8_256x256_pingpong_16x16x64", (64, 256, 128, 4, 32, 32, 32, 8192.0), 0.68),
    ("int8_t", ("i8_variant", 100), False, 512, 512, 512, "mfma_i8_256x256_pingpong_32x32x32", "mfma_i8_256x256_pingpong_32x32x32", (256, 256, 64, 8, 32, 32, 32, 8192.0), 0.92),
    ("int8_t", None, False, 256, 256, 256, "mfma_i8_64x256x128_slab128", "mfma_i8_256x256_pingpong_k64", (64, 256, 128, 4, 32, 32, 32, 8192.0), 0.68),
    ("int8_t", None, False, 256, 96, 256, "mfma_i8_64x256x128_slab128", "mfma_i8_64x256x128_slab128", (64, 256, 128, 4, 32, 32, 32, 8192.0), 0.68),
    ("uint8_t", None, False, 4096, 96, 4096, "mfma_i8_256x256x128_slab128", "mfma_i8_256x256x128_slab128", (256, 256, 128, 8, 32, 32, 32, 8192.0), 0.68),
    ("int8_t", ("i8_variant", 200), False, 512, 512, 512, "mfma_i8_256x256_pingpong_16x16x64", "mfma_i8_256x256_pingpong_16x16x64", (256, 256, 64, 8, 16, 16, 64, 8192.0), 0.92),
    ("int8_t", ("i8_variant", 10), False, 256, 256, 256, "mfma_i8_256x256_pingpong_k64", "mfma_i8_256x256_pingpong_k64", (256, 256, 64, 8, 32, 32, 32, 8192.0), 0.92),
    ("int8_t", None, False, 4096, 4096, 4096, "mfma_i8_256x256_pingpong_16x16x64", "mfma_i8_256x256_pingpong_16x16x64", (256, 256, 64, 8, 16, 16, 64, 8192.0), 0.92),
    ("int8_t", None, False, 4096, 320, 4096, "mfma_i8_256x256_pingpong_k64", "mfma_i8_256x256_pingpong_k64", (256, 256, 64, 8, 32, 32, 32, 8192.0), 0.92),
    ("int8_t", None, True, 256, 256, 256, "mfma_i8_256x256_pingpong_k64_KxN", "mfma_i8_256x256_pingpong_k64_KxN", (256, 256, 64, 8, 32, 32, 32, 8192.0), 0.92),
    ("int8_t", None, True, 256, 96, 256, "mfma_i8_256x256x128_slab128_KxN", "mfma_i8_256x256x128_slab128_KxN", (256, 256, 128, 8, 32, 32, 32, 8192.0), 0.68),
    ("int8_t", ("i8_variant", 0), False, 256, 96, 256, "mfma_i8_256x256x128_slab128", "mfma_i8_256x256x128_slab128", (256, 256, 128, 8, 32, 32, 32, 8192.0), 0.68),
    ("int8_t", ("i8_variant", 5), False, 256, 96, 256, "mfma_i8_64x256x128_slab128", "mfma_i8_64x256x128_slab128", (64, 256, 128, 4, 32, 32, 32, 8192.0), 0.68),
    ("int8_t", ("i8_variant", 99), False, 512, 512, 512, "unsupported", "valu_tile", (256, 256, 128, 8, 32, 32, 32, 8192.0), 0.68),
    ("double", None, False, 64, 64, 64, "mfma_f64_64x64x16_w4x4", "mfma_f64_64x64x16_w4x4", (64, 64, 16, 4, 16, 16, 4, 128.0), 0.97),
    ("double", None, False, 2048, 2048, 2048, "mfma_f64_128x128x16_w4x2", "mfma_f64_128x128x16_w4x2", (128, 128, 16, 4, 16, 16, 4, 128.0), 0.97),
    ("double", None, False, 16384, 16384, 16384, "mfma_f64_256x128x16_w8", "mfma_f64_256x128x16_w8", (256, 128, 16, 8, 16, 16, 4, 128.0), 0.97),
    ("double", ("f64_variant", 0), False, 256, 256, 256, "mfma_f64_256x128x16_w8", "mfma_f64_256x128x16_w8", (256, 128, 16, 8, 16, 16, 4, 128.0), 0.97),
    ("double", ("f64_variant", 1), False, 256, 256, 256, "mfma_f64_128x128x16_w4x2", "mfma_f64_128x128x16_w4x2", (128, 128, 16, 4, 16, 16, 4, 128.0), 0.97),
    ("double", ("f64_variant", 2), False, 256, 256, 256, "mfma_f64_256x128x16_w8_compiler_placed", "mfma_f64_256x128x16_w8_compiler_placed", (256, 128, 16, 8, 16, 16, 4, 128.0), 0.97),
    ("double", ("f64_variant", 3), False, 256, 256, 256, "mfma_f64_128x128x16_w4x2_compiler_placed", "mfma_f64_128x128x16_w4x2_compiler_placed", (128, 128, 16, 4, 16, 16, 4, 128.0), 0.97),
    ("double", ("f64_variant", 4), False, 256, 256, 256, "mfma_f64_64x64x16_w4x4", "mfma_f64_64x64x16_w4x4", (64, 64, 16, 4, 16, 16, 4, 128.0), 0.97),
    ("double", None, True, 256, 256, 256, "mfma_f64_64x64x16_w4x4", "mfma_f64_64x64x16_w4x4", (64, 64, 16, 4, 16, 16, 4, 128.0), 0.97),
]

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gemm_hls_amd", "csrc")
TABLES = {"f16": "mm_mfma_f16_kernels.inc", "i8": "mm_mfma_i8_kernels.inc", "f64": "mm_mfma_f64.hip"}


def rows(family):
    """The names of the family's table, read from its source"""
    body = re.search(r"kTable\[\] = \{(.*?)\n\};", open(os.path.join(CSRC, TABLES[family])).read(), flags=re.S).group(1)
    return re.findall(r'kernel_row<\w+>\("([^"]+)"', body)


FAMILY = {"half": "f16", "int8_t": "i8", "uint8_t": "i8", "double": "f64"}


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-{c[1][0]}={c[1][1]}-" if c[1] else f"{c[0]}-")
def test_kernel_name_and_info_by_shape_knob_and_layout(case):
    dtype, knob, transposed, n, k, m, name, batched, geometry, efficiency = case
    cfg = g.make_config(dtype, "Multiply", "Add", g.PATH_AUTO, transposed)
    old = g.get_tuning(knob[0]) if knob else None
    try:
        if knob:
            g.set_tuning(*knob)
        assert g.kernel_name(cfg, n, k, m) == name
        assert g.kernel_name_batched(cfg, n, k, m, 1) == batched
        i = g.kernel_info(cfg, n, k, m)
        assert (i.tile_n, i.tile_m, i.tile_k, i.wavefronts, i.inst_n, i.inst_m, i.inst_k, i.ops_per_clk_per_cu) == geometry
        assert i.measured_issue_efficiency == efficiency
    finally:
        if knob:
            g.set_tuning(knob[0], old)


def test_the_cases_reach_every_row_of_every_table():
    for family, count in (("f16", 9), ("i8", 8), ("f64", 5)):
        names = rows(family)
        assert len(names) == count and len(set(names)) == count, (family, names)
        reached = {c[6] for c in CASES if FAMILY[c[0]] == family}
        assert reached >= set(names), (family, sorted(set(names) - reached))
