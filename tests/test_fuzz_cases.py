"""The case lists of the differential shape fuzz (tests/_fuzz_cases.py, run on the GPU by tests/test_gpu_fuzz.py), checked
without a device: the mm_kernel_name* functions are pure arithmetic.  Walks exactly what the GPU tests run at
MM_FUZZ_SCALE = 1 -- the same seeds and counts -- and asserts a coverage condition; it measures nothing.

REQUIRED is every kernel name the resolvers return at default knobs inside the generator's pools and reference budgets: the
full cross product of the pools was enumerated once and the result is written down here, so that a resolver change that
silently stops serving a kernel shows up as a failure here and as a diff of this list.  Behind each name: "k" where a K x N
A reaches it, "m" where the call takes a base moved by one element (every call but the batched / accumulating one, which
takes it under the k-ordered contracts).  Every name exists plain and seeded, single and batched, and with a broadcast
operand; the closure has no seed and no operand to broadcast."""
import collections

import numpy as np
import pytest

import _closure_ref as cr
import _fuzz_cases as fc
import gemm_hls_amd as g

REQUIRED = {
    "batched": {
        "mfma_f32_128x128x32_w4x2_flush4096": "",
        "mfma_f32_256x256x16_w8_flush4096": "k",
        "mfma_f64_64x64x16_w4x4": "k",
        "mfma_f16_256x256_pingpong_16x16x32": "",
        "mfma_f16_256x256_pingpong_k32": "",
        "mfma_f16_256x256_pingpong_k32_KxN": "k",
        "mfma_f16_256x256x64_slab64_KxN": "k",
        "mfma_f16_64x256x64_slab64": "",
        "mfma_i8_256x256_pingpong_16x16x64": "",
        "mfma_i8_256x256_pingpong_k64": "",
        "mfma_i8_256x256_pingpong_k64_KxN": "k",
        "mfma_i8_256x256x128_slab128_KxN": "k",
        "mfma_i8_64x256x128_slab128": "",
        "ordered": "km",
        "ordered_tile": "km",
        "ordered_wide_f16": "km",
        "valu_tile": "k",
    },
    "argreduce": {"argreduce": "km", "argreduce_tile": "km"},
    "argreduce_nt": {"argreduce_nt": "m", "argreduce_tile_nt": "m"},
    "logsumexp": {"lse_exact": "km", "lse_hybrid": "km"},
    "logsumexp_nt": {"lse_exact_nt": "m", "lse_hybrid_nt": "m"},
    "widen": {
        "mfma_f16_256x256_pingpong_16x16x32_wide": "m",
        "mfma_f16_256x256_pingpong_k32_KxN_wide": "km",
        "mfma_f16_256x256_pingpong_k32_wide": "m",
        "mfma_f16_256x256x64_slab64_KxN_wide": "km",
        "mfma_f16_64x256x64_slab64_wide": "m",
        "mfma_i8_256x256_pingpong_16x16x64_wide": "m",
        "mfma_i8_256x256_pingpong_k64_KxN_wide": "km",
        "mfma_i8_256x256_pingpong_k64_wide": "m",
        "mfma_i8_256x256x128_slab128_KxN_wide": "km",
        "mfma_i8_64x256x128_slab128_wide": "m",
        "widen_ordered": "km",
    },
    "nt": {"nt_prepass": "m", "ordered_nt": "m", "valu_tile_nt": "m"},
    "closure": {"closure_blocked": "m", "closure_onchip": "m"},
}


def _planned(call):
    return [(seed, case) for dtype in fc.CONFIGS[call] for seed, cases in [fc.planned(call, dtype)] for case in cases]


def test_the_plan_covers_every_call_and_is_deterministic():
    assert set(REQUIRED) == set(fc.CALLS) == {call for call, _ in fc.PLAN}
    for (call, dtype), (seed, count) in fc.PLAN.items():
        first = fc.cases(call, dtype, seed, count)
        assert len(first) == count and first == fc.cases(call, dtype, seed, count), (call, dtype)
    assert fc.cases("nt", "float", 1, 8) != fc.cases("nt", "float", 2, 8)


@pytest.mark.parametrize("call", fc.CALLS)
def test_every_case_is_served_and_one_the_c_abi_accepts(call):
    for seed, c in _planned(call):
        name = fc.name_of(c.call, c.dtype, c.mp, c.rd, c.path, c.n, c.k, c.m, c.batch, c.ta, c.witness)
        assert name == c.name and name not in ("unsupported", "invalid"), c     # no case is skipped
        assert name in REQUIRED[call], f"{name} is not in REQUIRED: add it, with the forms it has ({c})"
        assert (c.mp, c.rd) in fc.CONFIGS[call][c.dtype] and c.path in (g.PATH_AUTO, g.PATH_ORDERED), c
        assert c.batch >= 1 and (c.batch > 1 or c.stride == "dense"), c
        if call == "closure":
            assert c.n == c.k == c.m and c.n in fc.CLOSURE_N and c.batch in fc.CLOSURE_BATCHES and not c.ta and not c.seeded, c
            assert c.n ** 3 * c.batch <= fc.budget(call, c.dtype, c.mp, c.rd, c.path), c
            continue
        assert c.batch in fc.BATCHES and c.n * c.k * c.m * c.batch <= fc.budget(call, c.dtype, c.mp, c.rd, c.path), c
        assert not (c.ta and call in fc.NT_CALLS), c                             # A^T B^T is refused
        if call == "batched" and name not in fc.ORDERED_CONTRACT:                # the fast families refuse an offset view
            assert c.misalign is None and c.stride != "c_pad1", c
            assert c.batch == 1 or not any(s * fc._ES[c.dtype] % 16 for s in fc.strides(c)), c
        if c.k >= 4096:                                                          # around the fp32 flush, sized as today
            assert fc.flushes(call, c.dtype, c.mp, c.rd) and c.n <= 300 and c.m <= 160, c


@pytest.mark.parametrize("call", fc.CALLS)
def test_every_reachable_kernel_is_drawn_three_times_and_in_each_of_its_forms(call):
    draws, seen = collections.Counter(), collections.defaultdict(set)
    for _, c in _planned(call):
        draws[c.name] += 1
        seen[c.name].update(fc.forms(c))
        if call == "closure":
            seen[c.name].add("witness" if c.witness else "values")
    for name, extra in REQUIRED[call].items():
        assert draws[name] >= 3, f"{call}: {name} is drawn {draws[name]} times"
        want = {"batch", "witness", "values"} if call == "closure" else {"seeded", "batch", "bcast"}
        want |= ({"kxn"} if "k" in extra else set()) | ({"misalign"} if "m" in extra else set())
        assert want <= seen[name], f"{call}: {name} is never drawn {sorted(want - seen[name])}"
    if call == "closure":   # both kernels at both shipped block sizes
        assert {(c.name, fc.closure_block(c)) for _, c in _planned(call)} == {
            (name, block) for name in REQUIRED[call] for block in (128, 256)}
    print({name: draws[name] for name in REQUIRED[call]})


def test_the_required_list_holds_what_the_library_documents():
    """The kernels include/mm_gemm.h names for these calls at default knobs (pinned variants have their own tests)."""
    names = {name for call in REQUIRED.values() for name in call}
    assert {"ordered", "ordered_tile", "valu_tile", "ordered_wide_f16", "argreduce", "argreduce_tile", "argreduce_nt",
            "argreduce_tile_nt", "lse_hybrid", "lse_exact", "lse_hybrid_nt", "lse_exact_nt", "widen_ordered", "nt_prepass",
            "valu_tile_nt", "ordered_nt", "closure_onchip", "closure_blocked"} <= names
    for family in ("mfma_f32_", "mfma_f64_", "mfma_f16_", "mfma_i8_"):
        assert any(n.startswith(family) for n in REQUIRED["batched"]), family
    for family in ("mfma_f16_", "mfma_i8_"):
        assert any(n.startswith(family) and n.endswith("_KxN") for n in REQUIRED["batched"]), family
    # every matrix-core kernel the batched resolver names for half and int8_t has its wide twin, and nothing else is wide
    narrow = {n + "_wide" for n in REQUIRED["batched"] if n.startswith(("mfma_f16_", "mfma_i8_"))}
    assert narrow == {n for n in REQUIRED["widen"] if n.endswith("_wide")}


def test_the_pools_hold_the_edges_of_the_serving_rules():
    assert {1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 513, 700} <= set(fc.NM_POOL)
    assert {1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 48, 63, 64, 96, 112, 127, 128, 160, 255, 256, 257, 320, 511, 512, 640} == set(fc.K_POOL)
    assert {1, 2, 63, 64, 65, 127, 128, 129, 200, 255, 256, 257, 300, 513} == set(fc.CLOSURE_N)
    assert fc.BATCHES == [1, 2, 3, 5] and fc.CLOSURE_BATCHES == [1, 2, 3]
    drawn = {c.n for call in fc.CALLS if call != "closure" for _, c in _planned(call)}
    assert {1, 700} <= drawn and len(drawn) >= 25            # the whole N pool is in use, not a corner of it
    assert any(c.k >= 4096 for _, c in _planned("batched")) and any(c.k >= 4096 for _, c in _planned("nt"))


@pytest.mark.parametrize("dtype", list(fc.CONFIGS["closure"]))
def test_every_drawn_graph_has_an_informative_closure(dtype):
    """_closure_ref.assert_informative on the restatement of every graph the GPU test will run, at the block size the call
    will use -- for graphs of at least 63 vertices: the closure of 1 or 4 entries cannot take 64 values, and a one-vertex
    graph of these recipes does not change at all (x (+) x (x) x == x is what makes them absorptive)."""
    seed, cases = fc.planned("closure", dtype)
    blocks = collections.Counter()
    for c in cases:
        d = fc.closure_graphs(seed, c)
        assert d.shape == (c.batch, c.n, c.n) and np.array_equal(d, fc.closure_graphs(seed, c))
        blocks[c.name, fc.closure_block(c)] += 1
        assert (c.name == "closure_onchip") == (c.n <= fc.closure_block(c)), c
        if c.n < fc.CLOSURE_INFORMATIVE_MIN_N:
            continue
        for e in range(c.batch):
            want, _ = cr.blocked(c.dtype, c.mp, c.rd, d[e], fc.closure_block(c))
            cr.assert_informative(c.dtype, c.mp, c.rd, d[e], want, f"{c}, graph {e}")
    assert {name for name, _ in blocks} == {"closure_onchip", "closure_blocked"}, blocks
