"""The launches that tests/test_gpu_launch_limits.py pushes past a grid limit of the host code: one plain list, checked on
the CPU by tests/test_limit_cases.py (the kernel each case names, how far it crosses its limit, what it allocates) and run
on the GPU by tests/test_gpu_launch_limits.py, which takes every shape from here.

The limits are literals that mirror the source; test_limit_cases.py reads the source text, so a limit that moves turns that
test red instead of silently leaving the GPU tests on the near side of it.

TEST INFRASTRUCTURE ONLY."""
from collections import namedtuple

# ---- the limits ----------------------------------------------------------------------------------------------------------
CHUNK_TILES = 1 << 22        # L1: gemm_hls_amd/csrc/mm_capi.hip chunk_of_tiles(): `(1ull << 22) / tiles` workgroups per launch
TRANSPOSE_MATRICES = 65535   # L2: gemm_hls_amd/csrc/mm_transpose.hip launch_transpose_t(): `e0 += 65535u`, gridDim.y
CLOSURE_GRAPHS = 1 << 20     # L3: mm_capi.hip dispatch_closure() and dispatch_bits_closure(): `chunk = 1u << 20`
MAX_GRID = 1 << 20           # L4: mm_bits.hip and mm_bits_count.hip: `kMaxGrid = 1ull << 20` workgroups, then a grid stride
GRID_Y = 65535               # L5: gridDim.y as the shapes below are budgeted; the GPU test reads the device's own value
TILE = 64                    # the 64 x 64 tile chunk_of_tiles() counts in, and the side of the L5 kernels' tiles
SPLIT_BLOCK = 256            # rows of one packed block of MM_PATH_SPLIT (mm_mfma_f32_split.hip: blocks_a, blocks_b)
TALL = 64 * 65536 + 65       # L6: rows of the tall single launches: 65538 rows of tiles, the last one ragged
WIDE = 64 * 65536 + 68       # L6: columns of the wide ones (a multiple of 4: valu_tile's 16-byte rows)

BATCH_L1 = (1 << 22) + (1 << 21) + 3   # two launches of one-tile elements, the second from e0 = 2^22
BATCH_L2 = 2 * 65535 + 7               # three transposition launches
BATCH_L3 = (1 << 20) + (1 << 19) + 5   # two on-chip closure launches, the second from e0 = 2^20

BUDGET = 2 << 30             # device bytes a test may allocate ...
BUDGET_SPLIT = 4 << 30       # ... and a case named `split`

ELEMENT_SIZE = {"float": 4, "double": 8, "half": 2, "int8_t": 1, "int": 4}


def chunk_of_tiles(tiles, batch):
    """mm_capi.hip's chunk_of_tiles() with the batch_chunk knob at its default, restated."""
    return min(max(1, CHUNK_TILES // tiles), batch)


def tiles64(n, m):
    return ((n + TILE - 1) // TILE) * ((m + TILE - 1) // TILE)


def words(cols):
    return (cols + 31) // 32


# call: the binding's function.  n, k, m: one element's shape (bits_closure_ / closure_: n alone).  shared: the operands
# passed 2-D, one matrix for the whole batch.  kernel: what the call's kernel_name function must start with.  knobs: tuning
# knobs the case pins (name, value).  extra: what only this case needs (index_base, ld, stride_c, op, cols ...).
Case = namedtuple("Case", "id limit call dtype map_op reduce_op path n k m batch kernel shared knobs extra")


def _c(id, limit, call, dtype, ops, n, k, m, batch, kernel, path="auto", shared="", knobs=(), **extra):
    return Case(id, limit, call, dtype, ops[0], ops[1], path, n, k, m, batch, kernel, shared, tuple(knobs), extra)


MUL_ADD, ADD_MIN, ADD_MAX = ("Multiply", "Add"), ("Add", "Min"), ("Add", "Max")

CASES = [
    # ---- L1: 2^22 workgroups per launch of a batch ----
    _c("l1_bmm_float_add_min", "L1", "bmm", "float", ADD_MIN, 2, 4, 4, BATCH_L1, "valu_tile"),
    _c("l1_bmm_float_mul_add_shared_b", "L1", "bmm", "float", MUL_ADD, 2, 8, 4, BATCH_L1, "mfma_f32_", shared="b"),
    _c("l1_bmm_int_ragged", "L1", "bmm", "int", MUL_ADD, 3, 5, 3, BATCH_L1, "ordered"),
    _c("l1_baddbmm_double_add_max", "L1", "baddbmm_", "double", ADD_MAX, 1, 4, 4, BATCH_L1, "valu_tile", stride_c=6),
    _c("l1_argreduce_float_add_min", "L1", "matmul_argreduce", "float", ADD_MIN, 2, 4, 4, BATCH_L1, "argreduce_tile",
       index_base=7),
    _c("l1_wide_int8_ragged", "L1", "matmul_wide", "int8_t", MUL_ADD, 3, 5, 3, BATCH_L1, "widen_ordered"),
    _c("l1_wide_int8_matrix_core_shared_b", "L1", "matmul_wide", "int8_t", MUL_ADD, 1, 32, 16, BATCH_L1, "mfma_i8_",
       shared="b"),
    _c("l1_nt_float_add_min", "L1", "matmul_nt", "float", ADD_MIN, 1, 16, 2, BATCH_L1, "valu_tile_nt"),
    _c("l1_bits_matmul_shared_b", "L1", "bits_matmul", "bits", ("And", "Or"), 2, 40, 40, BATCH_L1, "bits_plain", shared="b"),
    # (m = 20, not 40: 2 x 40 int32 counts per element are 2 GiB of C alone at this batch)
    _c("l1_bits_count_xor_shared_bt", "L1", "bits_matmul_count", "bits", ("Xor", "Add"), 2, 40, 20, BATCH_L1,
       "bits_count_plain", shared="b", op="Xor"),
    # ---- L2: 65535 matrices per transposition launch; Bt is not shared, k * m * element size <= 1024 ----
    _c("l2_nt_prepass_int8", "L2", "matmul_nt", "int8_t", MUL_ADD, 3, 32, 16, BATCH_L2, "nt_prepass"),
    _c("l2_nt_prepass_half", "L2", "matmul_nt", "half", MUL_ADD, 3, 16, 8, BATCH_L2, "nt_prepass"),
    _c("l2_nt_prepass_float", "L2", "matmul_nt", "float", MUL_ADD, 3, 8, 4, BATCH_L2, "nt_prepass"),
    _c("l2_nt_prepass_double", "L2", "matmul_nt", "double", MUL_ADD, 3, 8, 2, BATCH_L2, "nt_prepass"),
    # ---- L3: 2^20 graphs per on-chip closure launch ----
    _c("l3_closure_float", "L3", "closure_", "float", ADD_MIN, 4, 4, 4, BATCH_L3, "closure_onchip", witness=False),
    _c("l3_closure_float_witness", "L3", "closure_", "float", ADD_MIN, 4, 4, 4, BATCH_L3, "closure_onchip", witness=True),
    _c("l3_bits_closure", "L3", "bits_closure_", "bits", ("And", "Or"), 8, 8, 8, BATCH_L3, "bits_closure_onchip"),
    # ---- L4: kMaxGrid = 2^20 workgroups, then the kernel strides.  batch x rows x cols (bytes or bits) ----
    _c("l4_pack_bits", "L4", "pack_bits", "bits", ("", ""), 630_000, 0, 70, 5, "", ld=72),
    # (108 columns, not 100: 5 x 630 000 x 100 bytes are 1.17 x the cap of 2^28 bytes, below the quarter asked for)
    _c("l4_unpack_bits", "L4", "unpack_bits", "bits", ("", ""), 630_000, 0, 108, 5, ""),
    # 5 x 5 rows x 35 000 003 columns: the fourth element boundary lies in the strided part, the last word holds 3 bits
    _c("l4_transpose_bits", "L4", "transpose_bits", "bits", ("", ""), 5, 0, 35_000_003, 5, ""),
    # ---- L5: gridDim.y of a 2-D single launch; n is budgeted with GRID_Y, the GPU test uses the device's value ----
    _c("l5_ordered_float_add_min", "L5", "matmul", "float", ADD_MIN, TILE * GRID_Y + 65, 3, 3, 1, "ordered"),
    _c("l5_widen_ordered_half", "L5", "matmul_wide", "half", MUL_ADD, TILE * GRID_Y + 65, 3, 3, 1, "widen_ordered"),
    _c("l5_split", "L5", "matmul", "float", MUL_ADD, SPLIT_BLOCK * GRID_Y + 257, 16, 8, 1, "mfma_f32_split", path="split"),
    # ---- L6: tall N and wide M on the 1-D single launches ----
    _c("l6_tall_valu_tile", "L6", "matmul", "float", ADD_MIN, TALL, 4, 4, 1, "valu_tile"),
    _c("l6_tall_mfma_f32_64x64", "L6", "matmul", "float", MUL_ADD, TALL, 8, 4, 1, "mfma_f32_64x64", knobs=(("f32_variant", 64),)),
    _c("l6_tall_mfma_f64", "L6", "matmul", "double", MUL_ADD, TALL, 8, 2, 1, "mfma_f64_"),
    _c("l6_tall_ordered_tile", "L6", "matmul", "float", MUL_ADD, TALL, 4, 4, 1, "ordered_tile", path="ordered"),
    _c("l6_tall_argreduce", "L6", "matmul_argreduce", "float", ADD_MIN, TALL, 4, 4, 1, "argreduce_tile", index_base=3),
    _c("l6_tall_nt_valu_tile", "L6", "matmul_nt", "float", ADD_MIN, TALL, 16, 1, 1, "valu_tile_nt"),
    _c("l6_wide_valu_tile", "L6", "matmul", "float", ADD_MIN, 5, 4, WIDE, 1, "valu_tile"),
    _c("l6_wide_ordered", "L6", "matmul", "float", ADD_MIN, 5, 3, WIDE, 1, "ordered"),
]
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)


def work_and_limit(c):
    """(work, limit) in the limit's own unit: what the case launches against what one launch (or one pass of a
    grid-stride kernel) takes."""
    if c.limit == "L1":
        if c.call == "bits_matmul":      # for_each_bits_chunk: tiles of 64 rows x 64 words
            return tiles64(c.n, words(c.m)) * c.batch, CHUNK_TILES
        return tiles64(c.n, c.m) * c.batch, CHUNK_TILES
    if c.limit == "L2":
        return c.batch, TRANSPOSE_MATRICES
    if c.limit == "L3":
        return c.batch, CLOSURE_GRAPHS
    if c.limit == "L4":
        if c.call == "pack_bits":        # one wavefront per 64 columns of a row, 4 wavefronts per workgroup
            return c.batch * c.n * ((c.m + 63) // 64), 4 * MAX_GRID
        if c.call == "unpack_bits":      # one byte per thread, 256 per workgroup
            return c.batch * c.n * c.m, 256 * MAX_GRID
        return c.batch * ((c.n + 63) // 64) * words(c.m), 4 * MAX_GRID   # transpose: a wavefront per 64 rows x one word
    if c.limit == "L5":
        return (c.n + (SPLIT_BLOCK if c.path == "split" else TILE) - 1) // (SPLIT_BLOCK if c.path == "split" else TILE), GRID_Y
    return max((c.n + TILE - 1) // TILE, (c.m + TILE - 1) // TILE), 65536   # L6: rows or columns of tiles beyond anything tested


def device_bytes(c):
    """Bytes of device memory the GPU test of the case holds at its peak, counted generously: operands, outputs with their
    guards and gaps, the reference (or the piece of it compared at a time), the test's largest temporaries, and the
    library's own workspace."""
    GUARDS = 2 * 64 * 8 + (160 << 20)   # ... and 160 MiB for torch's matmul workspace and what else it holds on its own
    if c.call == "pack_bits":
        src, dst = c.batch * c.n * c.extra["ld"], c.batch * c.n * words(c.m) * 4
        return src + dst + GUARDS + 4 * c.n * words(c.m) * 32 * 4   # bytes, words; one element's bits as int32, four times
    if c.call == "unpack_bits":
        src, dst = c.batch * c.n * words(c.m) * 4, c.batch * c.n * c.m
        return src + 3 * dst + GUARDS                           # words, bytes, reference bytes, the comparison's mask
    if c.call == "transpose_bits":
        src, dst = c.batch * c.n * words(c.m) * 4, c.batch * c.m * words(c.n) * 4
        return src + dst + GUARDS + 6 * c.m * 4                 # one row's bits as int32, six times: one element at a time
    if c.call == "bits_closure_":
        d = c.batch * c.n * words(c.n) * 4
        return 2 * d + GUARDS + 8 * c.batch * c.n * c.n          # packed in and out, the unpacked batch and its temporaries
    if c.call == "closure_":
        d = c.batch * c.n * c.n * 4
        return (5 if c.extra["witness"] else 3) * d + GUARDS + 2 * d   # D in, out, reference (and W), two temporaries
    if c.call in ("bits_matmul", "bits_matmul_count"):
        a, b = c.batch * c.n * words(c.k) * 4, c.k * words(c.m) * 4
        out = c.batch * c.n * (c.m if c.call == "bits_matmul_count" else words(c.m)) * 4
        if c.call == "bits_matmul":      # 16 pieces: a piece's rows unpacked, as float64, their products, packed again
            return a + b + out + GUARDS + 800 * (c.batch // 16 + 1) * c.n
        return a + b + out + GUARDS + 8 * (c.batch // 64 + 1) * c.n * c.m * 2 * 4   # 64 pieces: word pairs, eight times
    es, wide = ELEMENT_SIZE[c.dtype], c.call == "matmul_wide"
    ces = 4 if wide else es
    a = (1 if "a" in c.shared else c.batch) * c.n * c.k * es
    b = (1 if "b" in c.shared else c.batch) * c.k * c.m * es
    out = c.batch * c.extra.get("stride_c", c.n * c.m) * ces
    if c.call == "baddbmm_":
        out += c.batch * c.n * c.m * ces                       # the seed's copy
    if c.call == "matmul_argreduce":
        out += c.batch * c.n * c.m * 4
    # the reference is formed and compared in 16 pieces of the batch (of the rows): never whole
    piece = c.batch * c.n // 16 + 1
    if c.reduce_op in ("Min", "Max") or c.dtype == "int":
        temp = 3 * piece * c.k * c.m * 8                       # the mapped products of a piece, in 8 bytes, three times
    else:
        temp = 3 * piece * (c.k + c.m) * 8                     # float64 copies of a piece of A and of its product
    ws = 0
    if c.path == "split":                                      # 24 KiB per 256-row block and 16-k slab of A and of B
        ws = (((c.n + 255) // 256) + ((c.m + 255) // 256)) * ((c.k + 15) // 16) * 24576
    if c.kernel == "nt_prepass":
        ws = c.batch * c.k * c.m * es
    return a + b + out + temp + ws + GUARDS


def _kernel_name(g, c, n):
    if c.call == "bits_matmul":
        return g.kernel_name_bits_gemm(n, c.k, c.m, batch=c.batch)
    if c.call == "bits_matmul_count":
        return g.kernel_name_bits_count(n, c.k, c.m, batch=c.batch)
    if c.call == "bits_closure_":
        return g.kernel_name_bits_closure(n, c.batch)
    paths = {"auto": g.PATH_AUTO, "ordered": g.PATH_ORDERED, "split": g.PATH_SPLIT}
    cfg = g.make_config(c.dtype, c.map_op, c.reduce_op, paths[c.path])
    if c.call == "closure_":
        return g.kernel_name_closure(cfg, n, c.batch, c.extra["witness"])
    if c.call == "matmul":
        return g.kernel_name(cfg, n, c.k, c.m)
    name = {"bmm": g.kernel_name_batched, "baddbmm_": g.kernel_name_batched, "matmul_argreduce": g.kernel_name_argreduce,
            "matmul_wide": g.kernel_name_widen, "matmul_nt": g.kernel_name_nt}[c.call]
    return name(cfg, n, c.k, c.m, c.batch)


def pinned(c):
    """Context manager: the case's knobs set, and put back afterwards."""
    import contextlib

    import gemm_hls_amd as g

    @contextlib.contextmanager
    def manager():
        old = {knob: g.get_tuning(knob) for knob, _ in c.knobs}
        try:
            for knob, value in c.knobs:
                g.set_tuning(knob, value)
            yield
        finally:
            for knob, value in old.items():
                g.set_tuning(knob, value)
    return manager()


def kernel_name(c, n=None):
    """What the case's kernel_name function answers under the case's knobs, for n rows (the case's own by default)."""
    import gemm_hls_amd as g
    with pinned(c):
        return _kernel_name(g, c, c.n if n is None else n)
