"""CPU tests of the rules the seeded products of the C ABI share: K = 0 with and without a seed, empty batches, null pointers,
stride_c, and outputs that overlap operands -- for mm_gemm_logsumexp_*, mm_gemm_widen_*, mm_gemm_nt_*, mm_gemm_argreduce_* and
mm_gemm_batched_accumulate_*, each in its enqueue and its launch form, with the exact status and mm_last_error() text.  The
packed product's refusals are pinned under every setting of the batch_chunk knob its dispatcher reads.

Every address is fake and never dereferenced: each call is refused, or is a no-op, before a device is touched.  The expected
values were recorded once from the library as it stood before these checks were written in one place."""
import ctypes

import pytest

import gemm_hls_amd as g

MM_OK, MM_ERR_NO_DEVICE, MM_ERR_BAD_ARGUMENT, MM_ERR_UNSUPPORTED = 0, 1, 2, 3
A0, B0, C0, I0 = 1 << 22, 2 << 22, 3 << 22, 4 << 22
E = 64 * 64

# family: (symbol stem, configuration, takes an index, takes the accumulate flag)
FAMILIES = {
    "logsumexp": ("mm_gemm_logsumexp", ("float", "Add", "Max"), False, True),
    "widen": ("mm_gemm_widen", ("half", "Multiply", "Add"), False, True),
    "nt": ("mm_gemm_nt", ("float", "Multiply", "Add"), False, True),
    "argreduce": ("mm_gemm_argreduce", ("float", "Add", "Min"), True, True),
    "batched_accumulate": ("mm_gemm_batched_accumulate", ("float", "Multiply", "Add"), False, False),
}


def call(family, form, a=A0, b=B0, c=C0, index=I0, n=64, k=64, m=64, batch=4, sa=E, sb=E, sc=E, index_base=0, acc=0):
    """(status, message or None, elapsed or None) of one call."""
    stem, ops, has_index, has_acc = FAMILIES[family]
    cfg = g.make_config(*ops)
    args = [ctypes.byref(cfg), a, b, c] + ([index] if has_index else []) + [n, k, m, batch, sa, sb, sc]
    args += ([index_base] if has_index else []) + ([acc] if has_acc else [])
    t = ctypes.c_double(-1.0)
    if form == "enqueue":
        rc = getattr(g.lib(), stem + "_enqueue")(None, *args)
    else:
        rc = getattr(g.lib(), stem + "_launch")(0, *args, ctypes.byref(t))
    return (rc, g.lib().mm_last_error().decode() if rc else None, t.value if form == "launch" and rc == MM_OK else None)


SPAN = 4 * E * 4   # bytes of four 64 x 64 matrices of 4-byte elements
CASES = {
    "k0_plain": dict(k=0),
    "k0_accumulate": dict(k=0, acc=1),
    "k0_accumulate_null_a_b": dict(k=0, acc=1, a=0, b=0),
    "k0_accumulate_null_c": dict(k=0, acc=1, c=0),
    "k0_accumulate_stride_c": dict(k=0, acc=1, sc=E - 1),
    "k0_accumulate_c_overlaps_a": dict(k=0, acc=1, c=A0 + 64),
    "empty_batch": dict(batch=0, a=0, b=0, c=0, index=0),
    "empty_batch_accumulate": dict(batch=0, acc=1),
    "no_rows": dict(n=0),
    "no_columns_accumulate": dict(m=0, acc=1),
    "null_a": dict(a=0),
    "null_b": dict(b=0),
    "null_c": dict(c=0),
    "null_a_accumulate": dict(a=0, acc=1),
    "null_index": dict(index=0),
    "stride_c": dict(sc=E - 1),
    "stride_c_accumulate": dict(sc=E - 1, acc=1),
    "stride_c_unread_in_a_batch_of_one": dict(sc=0, batch=1, device_needed=True),
    "c_overlaps_a": dict(c=A0 + SPAN - 64),
    "c_overlaps_a_from_below_accumulate": dict(c=A0 - SPAN + 64, acc=1),
    "c_overlaps_b": dict(c=B0 + 64),
    "c_overlaps_broadcast_b_accumulate": dict(b=C0 + 3 * E * 4, sb=0, acc=1),
    "index_overlaps_c": dict(index=C0 + SPAN - 64),
    "index_overlaps_a_accumulate": dict(index=A0 + 64, acc=1),
    "index_base_negative": dict(index_base=-1),
    "index_base_largest_that_fits": dict(index_base=2 ** 31 - 64),
    # C's extent counts in C's own element size: one 64 x 64 matrix ending 64 bytes into A when its elements have 4 bytes --
    # as the widening call's C has over half operands -- and 8128 bytes short of A when they have 2
    "c_of_four_byte_elements_reaches_a": dict(c=A0 - E * 4 + 64, batch=1),
}


def applies(family, name):
    """The index cases are the argreduce calls'; a call without the flag always accumulates, so it has no plain K = 0."""
    _, _, has_index, has_acc = FAMILIES[family]
    return (has_index or "index" not in name) and (has_acc or name != "k0_plain")


def run_case(family, form, name):
    kw = dict(CASES[name])
    kw.pop("device_needed", None)
    return call(family, form, **kw)


KEYS = [(family, name) for family in FAMILIES for name in CASES if applies(family, name)]

OK, NEEDS_DEVICE = (MM_OK, None), (MM_ERR_NO_DEVICE, None)
SIZE_K = (MM_ERR_BAD_ARGUMENT, "size_k must be positive")
NULL = (MM_ERR_BAD_ARGUMENT, "null matrix pointer")
NULL_OR_INDEX = (MM_ERR_BAD_ARGUMENT, "null matrix or index pointer")
STRIDE_C = (MM_ERR_BAD_ARGUMENT, "stride_c 4095 < N * M = 4096: the outputs of the batch would overlap")


def overlap(a, b, c):
    return (MM_ERR_BAD_ARGUMENT, f"c overlaps a or b (bases {a}, {b}, {c})")


def overlap_accumulate(a, b, c):
    return (MM_ERR_BAD_ARGUMENT, f"c overlaps a or b (bases {a}, {b}, {c}): an accumulating call updates C in place and reads A "
            "and B meanwhile; pass a copy")


def overlap_index(a, b, c, i="0x1000000"):
    return (MM_ERR_BAD_ARGUMENT, f"c or c_index overlaps a, b or each other (bases {a}, {b}, {c}, {i})")


# what mm_gemm_logsumexp_* and mm_gemm_nt_* answer; the other families below, where they differ
SEEDED = {
    "k0_plain": SIZE_K,
    "k0_accumulate": OK,
    "k0_accumulate_null_a_b": OK,                 # A and B are unread over no k
    "k0_accumulate_null_c": NULL,
    "k0_accumulate_stride_c": STRIDE_C,
    "k0_accumulate_c_overlaps_a": OK,             # an A of no elements overlaps nothing
    "empty_batch": OK,
    "empty_batch_accumulate": OK,
    "no_rows": OK,
    "no_columns_accumulate": OK,
    "null_a": NULL,
    "null_b": NULL,
    "null_c": NULL,
    "null_a_accumulate": NULL,
    "stride_c": STRIDE_C,
    "stride_c_accumulate": STRIDE_C,
    "stride_c_unread_in_a_batch_of_one": NEEDS_DEVICE,
    "c_overlaps_a": overlap("0x400000", "0x800000", "0x40ffc0"),
    "c_overlaps_a_from_below_accumulate": overlap("0x400000", "0x800000", "0x3f0040"),
    "c_overlaps_b": overlap("0x400000", "0x800000", "0x800040"),
    "c_overlaps_broadcast_b_accumulate": overlap("0x400000", "0xc0c000", "0xc00000"),
    "c_of_four_byte_elements_reaches_a": overlap("0x400000", "0x800000", "0x3fc040"),
}
DIFFERENT = {
    "logsumexp": {},
    "nt": {},
    # the last 64 bytes of a four-matrix A of 4-byte elements lie past the same A of half elements
    "widen": {"c_overlaps_a": NEEDS_DEVICE},
    "argreduce": {
        "k0_accumulate_null_a_b": NULL_OR_INDEX,   # the stricter rule: A, B and the index even over no k
        "k0_accumulate_null_c": NULL_OR_INDEX,
        "null_a": NULL_OR_INDEX,
        "null_b": NULL_OR_INDEX,
        "null_c": NULL_OR_INDEX,
        "null_a_accumulate": NULL_OR_INDEX,
        "null_index": NULL_OR_INDEX,
        "c_overlaps_a": overlap_index("0x400000", "0x800000", "0x40ffc0"),
        "c_overlaps_a_from_below_accumulate": overlap_index("0x400000", "0x800000", "0x3f0040"),
        "c_overlaps_b": overlap_index("0x400000", "0x800000", "0x800040"),
        "c_overlaps_broadcast_b_accumulate": overlap_index("0x400000", "0xc0c000", "0xc00000"),
        "c_of_four_byte_elements_reaches_a": overlap_index("0x400000", "0x800000", "0x3fc040"),
        "index_overlaps_c": overlap_index("0x400000", "0x800000", "0xc00000", "0xc0ffc0"),
        "index_overlaps_a_accumulate": overlap_index("0x400000", "0x800000", "0xc00000", "0x400040"),
        "index_base_negative": (MM_ERR_BAD_ARGUMENT, "index_base -1 is negative"),
        "index_base_largest_that_fits": NEEDS_DEVICE,      # 2^31 - 64 + K - 1 = 2^31 - 1 still fits
    },
    "batched_accumulate": {
        "k0_accumulate_null_a_b": NULL,            # the batched call's checks on a problem that has no k
        "c_overlaps_a": overlap_accumulate("0x400000", "0x800000", "0x40ffc0"),
        "c_overlaps_a_from_below_accumulate": overlap_accumulate("0x400000", "0x800000", "0x3f0040"),
        "c_overlaps_b": overlap_accumulate("0x400000", "0x800000", "0x800040"),
        "c_overlaps_broadcast_b_accumulate": overlap_accumulate("0x400000", "0xc0c000", "0xc00000"),
        "c_of_four_byte_elements_reaches_a": overlap_accumulate("0x400000", "0x800000", "0x3fc040"),
    },
}
EXPECTED = {(family, name): DIFFERENT[family].get(name, SEEDED.get(name)) for family, name in KEYS}


def only_without_a_device(expected):
    """A case recorded as NEEDS_DEVICE passes every argument check: with a device present its fake addresses would reach a
    kernel, so it is skipped there, before any call.  Decided by the expectation itself, for every such case."""
    if expected[0] == MM_ERR_NO_DEVICE and g.lib().mm_init(None) != MM_ERR_NO_DEVICE:
        pytest.skip("a device is present: this call passes every check and would launch on fake addresses")


def test_every_case_has_an_expectation():
    assert all(EXPECTED[key] is not None for key in KEYS)
    assert all(set(DIFFERENT[family]) <= set(CASES) for family in FAMILIES) and set(SEEDED) <= set(CASES)
    assert sorted(EXPECTED_BITS) == sorted(BITS_CASES)
    # the hand-set flag of a case never disagrees with what is expected of it
    for (family, name), expected in EXPECTED.items():
        assert not CASES[name].get("device_needed") or expected == NEEDS_DEVICE, (family, name)


@pytest.mark.parametrize("form", ["enqueue", "launch"])
@pytest.mark.parametrize("family,name", KEYS, ids=[f"{f}-{n}" for f, n in KEYS])
def test_shared_rule(family, name, form):
    status, message = EXPECTED[family, name]
    only_without_a_device(EXPECTED[family, name])
    got = run_case(family, form, name)
    assert got[0] == status and (status == MM_ERR_NO_DEVICE or got[1] == message), got
    if form == "launch" and status == MM_OK:
        assert got[2] == 0.0   # a no-op reports no time


# ---- the packed product: its checks under every setting of the knob its chunking reads ----------------------------------------
def bits_call(form, a=A0, b=B0, c=C0, n=64, k=64, m=64, lda=2, ldb=2, ldc=2, batch=4, sa=128, sb=128, sc=128, acc=0):
    t = ctypes.c_double(-1.0)
    args = (a, b, c, n, k, m, lda, ldb, ldc, batch, sa, sb, sc, acc)
    if form == "enqueue":
        rc = g.lib().mm_bits_gemm_enqueue(None, *args)
    else:
        rc = g.lib().mm_bits_gemm_launch(0, *args, ctypes.byref(t))
    return (rc, g.lib().mm_last_error().decode() if rc else None)


BITS_CASES = {
    "k0_plain": dict(k=0),
    "k0_plain_null_a_b": dict(k=0, a=0, b=0),
    "k0_accumulate": dict(k=0, acc=1),
    "empty_batch": dict(batch=0, a=0, b=0, c=0),
    "no_rows": dict(n=0),
    "no_columns": dict(m=0),
    "null_a": dict(a=0),
    "null_b": dict(b=0),
    "null_c": dict(c=0),
    "lda": dict(lda=1),
    "ldb": dict(ldb=1),
    "ldc": dict(ldc=1),
    "stride_c": dict(sc=127),
    "c_overlaps_a": dict(c=A0 + 4 * 128 * 4 - 4),
    "c_overlaps_b": dict(c=B0 - 4 * 128 * 4 + 4, acc=1),
    "valid": dict(device_needed=True),
    # more elements than one launch's 2^22 workgroups take: the checks pass whatever the slices will be
    "valid_many_elements": dict(a=1 << 30, b=2 << 30, c=3 << 30, batch=1 << 23, n=1, k=1, m=1, lda=1, ldb=1, ldc=1, sa=1, sb=1,
                                sc=1, device_needed=True),
}

LD = "a row stride is below its row's words: lda %d (needs 2), ldb %d (2), ldc %d (2)"
EXPECTED_BITS = {
    "k0_plain": NEEDS_DEVICE,              # the product over no k is all zeros: a launch
    "k0_plain_null_a_b": NEEDS_DEVICE,
    "k0_accumulate": OK,
    "empty_batch": OK,
    "no_rows": OK,
    "no_columns": OK,
    "null_a": NULL,
    "null_b": NULL,
    "null_c": NULL,
    "lda": (MM_ERR_BAD_ARGUMENT, LD % (1, 2, 2)),
    "ldb": (MM_ERR_BAD_ARGUMENT, LD % (2, 1, 2)),
    "ldc": (MM_ERR_BAD_ARGUMENT, LD % (2, 2, 1)),
    "stride_c": (MM_ERR_BAD_ARGUMENT, "stride_c 127 < (N - 1) ldc + ceil(M / 32) = 128: the outputs of the batch would overlap"),
    "c_overlaps_a": overlap("0x400000", "0x800000", "0x4007fc"),
    "c_overlaps_b": overlap("0x400000", "0x800000", "0x7ff804"),
    "valid": NEEDS_DEVICE,
    "valid_many_elements": NEEDS_DEVICE,
}


@pytest.fixture
def batch_chunk():
    old = g.get_tuning("batch_chunk")
    yield lambda v: g.set_tuning("batch_chunk", v)
    g.set_tuning("batch_chunk", old)


@pytest.mark.parametrize("form", ["enqueue", "launch"])
@pytest.mark.parametrize("knob", [-1, 1, 2], ids=["unset", "chunk1", "chunk2"])
@pytest.mark.parametrize("name", sorted(BITS_CASES))
def test_bits_gemm_checks_do_not_depend_on_the_chunking(name, form, knob, batch_chunk):
    status, message = EXPECTED_BITS[name]
    only_without_a_device(EXPECTED_BITS[name])
    batch_chunk(knob)
    kw = dict(BITS_CASES[name])
    kw.pop("device_needed", None)
    got = bits_call(form, **kw)
    assert got[0] == status and (status == MM_ERR_NO_DEVICE or got[1] == message), got
