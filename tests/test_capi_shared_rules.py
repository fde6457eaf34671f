"""CPU tests of the rules the seeded products of the C ABI share: K = 0 with and without a seed, empty batches, null pointers,
stride_c, and outputs that overlap operands -- for mm_gemm_logsumexp_*, mm_gemm_widen_*, mm_gemm_nt_*, mm_gemm_argreduce_* and
mm_gemm_batched_accumulate_*, each in its enqueue and its launch form, with the exact status and mm_last_error() text.  The
packed products' refusals (mm_bits_gemm_*, mm_bits_count_*) are pinned under every setting of the batch_chunk knob their
dispatchers read; those of mm_bits_transpose_*, mm_bits_pack_*, mm_bits_unpack_* and mm_bits_closure_* in both forms.

Every address is fake and never dereferenced: each call is refused, or is a no-op, before a device is touched.  The expected
values were recorded once from the library as it stood before these checks were written in one place."""
import ctypes

import pytest

import gemm_hls_amd as g
from _bits_rig import _Variant

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
    "variant_below": dict(variant=-2),
    "variant_above": dict(variant=2),
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
    "variant_below": (MM_ERR_BAD_ARGUMENT, "bits_variant -2 is not one of -1, 0, 1"),
    "variant_above": (MM_ERR_BAD_ARGUMENT, "bits_variant 2 is not one of -1, 0, 1"),
}


@pytest.fixture
def batch_chunk():
    old = g.get_tuning("batch_chunk")
    yield lambda v: g.set_tuning("batch_chunk", v)
    g.set_tuning("batch_chunk", old)


def run_packed(call, form, case, variant_knob=None):
    """call(form, **case) -- with the family's kernel knob set to the case's "variant" for the call, where it names one."""
    kw = dict(case)
    kw.pop("device_needed", None)
    variant = kw.pop("variant", None)
    if variant is None:
        return call(form, **kw)
    with _Variant(variant_knob, variant):
        return call(form, **kw)


KNOBS = pytest.mark.parametrize("knob", [-1, 1, 2], ids=["unset", "chunk1", "chunk2"])
FORMS = pytest.mark.parametrize("form", ["enqueue", "launch"])


@FORMS
@KNOBS
@pytest.mark.parametrize("name", sorted(BITS_CASES))
def test_bits_gemm_checks_do_not_depend_on_the_chunking(name, form, knob, batch_chunk):
    status, message = EXPECTED_BITS[name]
    only_without_a_device(EXPECTED_BITS[name])
    batch_chunk(knob)
    got = run_packed(bits_call, form, BITS_CASES[name], "bits_variant")
    assert got[0] == status and (status == MM_ERR_NO_DEVICE or got[1] == message), got


# ---- the rest of the packed family: counting product, transpose, pack / unpack, closure ------------------------------------------
def packed_call(stem, form, *args):
    t = ctypes.c_double(-1.0)
    fn = getattr(g.lib(), f"{stem}_{form}")
    rc = fn(None, *args) if form == "enqueue" else fn(0, *args, ctypes.byref(t))
    return (rc, g.lib().mm_last_error().decode() if rc else None)


def count_call(form, op=0, a=A0, b=B0, c=C0, n=64, k=64, m=64, lda=2, ldbt=2, ldc=64, batch=4, sa=128, sb=128, sc=E, acc=0):
    return packed_call("mm_bits_count", form, op, a, b, c, n, k, m, lda, ldbt, ldc, batch, sa, sb, sc, acc)


def convert_call(stem, row_src, row_dst):
    """A call of 64 x 64 matrices, four to the batch, dense on both sides: rows of row_src / row_dst units."""
    def call(form, src=A0, dst=C0, rows=64, cols=64, ld_src=row_src, ld_dst=row_dst, batch=4, ss=64 * row_src, sd=64 * row_dst):
        return packed_call(stem, form, src, dst, rows, cols, ld_src, ld_dst, batch, ss, sd)
    return call


def closure_call(form, d=C0, n=64, ldd=2, batch=4, sd=128):
    return packed_call("mm_bits_closure", form, d, n, ldd, batch, sd)


OPERAND, COUNTS = 4 * 128 * 4, 4 * E * 4      # bytes of four packed 64 x 64 operands, and of their four int32 results
MANY = dict(batch=1 << 23, device_needed=True)   # more elements than one launch's 2^22 workgroups take
COUNT_CASES = {
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
    "ldbt": dict(ldbt=1),
    "ldc": dict(ldc=63),
    "stride_c": dict(sc=E - 1),
    "c_overlaps_a": dict(c=A0 + OPERAND - 4),
    "c_overlaps_a_from_below": dict(c=A0 - COUNTS + 4, acc=1),
    "c_overlaps_b": dict(c=B0 + OPERAND - 4, op=1),
    "c_overlaps_b_from_below": dict(c=B0 - COUNTS + 4, acc=1),
    "valid": dict(device_needed=True),
    "valid_xor_accumulate": dict(op=1, acc=1, device_needed=True),
    "valid_many_elements": dict(MANY, a=1 << 30, b=2 << 30, c=3 << 30, n=1, k=1, m=1, lda=1, ldbt=1, ldc=1, sa=1, sb=1, sc=1),
    "op_below": dict(op=-1),
    "op_above": dict(op=2),
    "variant_below": dict(variant=-2),
    "variant_above": dict(variant=2),
}


def convert_cases(row_src, row_dst, src_bytes, dst_bytes):
    """The cases of a conversion with rows of row_src / row_dst units, whose four source matrices take src_bytes and whose
    four results take dst_bytes."""
    return {
        "empty_batch": dict(batch=0, src=0, dst=0),
        "no_rows": dict(rows=0),
        "no_columns": dict(cols=0),
        "null_src": dict(src=0),
        "null_dst": dict(dst=0),
        "ld_src": dict(ld_src=row_src - 1),
        "ld_dst": dict(ld_dst=row_dst - 1),
        "stride_dst": dict(sd=64 * row_dst - 1),
        "dst_overlaps_src": dict(dst=A0 + src_bytes - 4),
        "dst_overlaps_src_from_below": dict(dst=A0 - dst_bytes + 4),
        "valid": dict(device_needed=True),
        "valid_many_elements": dict(MANY, src=1 << 30, dst=3 << 30, rows=1, cols=1, ld_src=1, ld_dst=1, ss=1, sd=1),
    }


CLOSURE_CASES = {
    "empty_batch": dict(batch=0, d=0),
    "no_vertices": dict(n=0),
    "null_d": dict(d=0),
    "ldd": dict(ldd=1),
    "stride_d": dict(sd=127),
    "valid": dict(device_needed=True),
    "valid_blocked": dict(n=65, ldd=3, sd=195, device_needed=True),
    "valid_many_elements": dict(MANY, d=3 << 30, n=1, ldd=1, sd=1),
}

# family: (the call, its cases, the knob its "variant" cases set)
PACKED = {
    "count": (count_call, COUNT_CASES, "bits_count_variant"),
    "transpose": (convert_call("mm_bits_transpose", 2, 2), convert_cases(2, 2, OPERAND, OPERAND), None),
    "pack": (convert_call("mm_bits_pack", 64, 2), convert_cases(64, 2, 4 * E, OPERAND), None),
    "unpack": (convert_call("mm_bits_unpack", 2, 64), convert_cases(2, 64, OPERAND, 4 * E), None),
    "closure": (closure_call, CLOSURE_CASES, None),
}

def bad(message):
    return (MM_ERR_BAD_ARGUMENT, message)


def convert_expected(ld_src, ld_dst, stride_dst, above, below):
    return {
        "empty_batch": OK,
        "no_rows": OK,
        "no_columns": OK,
        "null_src": NULL,
        "null_dst": NULL,
        "ld_src": bad("a row stride is below its row: " + ld_src),
        "ld_dst": bad("a row stride is below its row: " + ld_dst),
        "stride_dst": bad(f"destination batch stride {stride_dst}: the outputs of the batch would overlap"),
        "dst_overlaps_src": bad(f"the destination overlaps the source (bases 0x400000, {above})"),
        "dst_overlaps_src_from_below": bad(f"the destination overlaps the source (bases 0x400000, {below})"),
        "valid": NEEDS_DEVICE,
        "valid_many_elements": NEEDS_DEVICE,
    }


COUNT_LD = "a row stride is below its row: lda %d (needs 2 words), ldbt %d (2 words), ldc %d (64 elements)"
EXPECTED_PACKED = {
    "count": {
        "k0_plain": NEEDS_DEVICE,              # the counts over no k are all zeros: a launch
        "k0_plain_null_a_b": NEEDS_DEVICE,
        "k0_accumulate": OK,
        "empty_batch": OK,
        "no_rows": OK,
        "no_columns": OK,
        "null_a": NULL,
        "null_b": NULL,
        "null_c": NULL,
        "lda": bad(COUNT_LD % (1, 2, 64)),
        "ldbt": bad(COUNT_LD % (2, 1, 64)),
        "ldc": bad(COUNT_LD % (2, 2, 63)),
        "stride_c": bad("stride_c 4095 < (N - 1) ldc + M = 4096: the outputs of the batch would overlap"),
        "c_overlaps_a": bad("c overlaps a or bt (bases 0x400000, 0x800000, 0x4007fc)"),
        "c_overlaps_a_from_below": bad("c overlaps a or bt (bases 0x400000, 0x800000, 0x3f0004)"),
        "c_overlaps_b": bad("c overlaps a or bt (bases 0x400000, 0x800000, 0x8007fc)"),
        "c_overlaps_b_from_below": bad("c overlaps a or bt (bases 0x400000, 0x800000, 0x7f0004)"),
        "valid": NEEDS_DEVICE,
        "valid_xor_accumulate": NEEDS_DEVICE,
        "valid_many_elements": NEEDS_DEVICE,
        "op_below": bad("op -1 is not MM_BITS_COUNT_AND (0) or MM_BITS_COUNT_XOR (1)"),
        "op_above": bad("op 2 is not MM_BITS_COUNT_AND (0) or MM_BITS_COUNT_XOR (1)"),
        "variant_below": bad("bits_count_variant -2 is not one of -1, 0, 1"),
        "variant_above": bad("bits_count_variant 2 is not one of -1, 0, 1"),
    },
    "transpose": convert_expected("source 1 (needs 2), destination 2 (2)", "source 2 (needs 2), destination 1 (2)", 127,
                                  "0x4007fc", "0x3ff804"),
    "pack": convert_expected("source 63 (needs 64), destination 2 (2)", "source 64 (needs 64), destination 1 (2)", 127,
                             "0x403ffc", "0x3ff804"),
    "unpack": convert_expected("source 1 (needs 2), destination 64 (64)", "source 2 (needs 2), destination 63 (64)", 4095,
                               "0x4007fc", "0x3fc004"),
    "closure": {
        "empty_batch": OK,
        "no_vertices": OK,
        "null_d": NULL,
        "ldd": bad("ldd 1 is below the row's 2 words"),
        "stride_d": bad("stride_d 127 < (n - 1) ldd + ceil(n / 32) = 128: the graphs of the batch would overlap"),
        "valid": NEEDS_DEVICE,
        "valid_blocked": NEEDS_DEVICE,
        "valid_many_elements": NEEDS_DEVICE,
    },
}


def test_every_packed_case_has_an_expectation():
    for family, (_, cases, _) in PACKED.items():
        assert sorted(EXPECTED_PACKED[family]) == sorted(cases), family
        for name, case in cases.items():
            assert not case.get("device_needed") or EXPECTED_PACKED[family][name] == NEEDS_DEVICE, (family, name)


def check_packed(family, name, form):
    call, cases, variant_knob = PACKED[family]
    status, message = EXPECTED_PACKED[family][name]
    only_without_a_device(EXPECTED_PACKED[family][name])
    got = run_packed(call, form, cases[name], variant_knob)
    assert got[0] == status and (status == MM_ERR_NO_DEVICE or got[1] == message), got


@FORMS
@KNOBS
@pytest.mark.parametrize("name", sorted(COUNT_CASES))
def test_bits_count_checks_do_not_depend_on_the_chunking(name, form, knob, batch_chunk):
    batch_chunk(knob)
    check_packed("count", name, form)


PACKED_KEYS = [(family, name) for family in PACKED if family != "count" for name in sorted(PACKED[family][1])]


@FORMS
@pytest.mark.parametrize("family,name", PACKED_KEYS, ids=[f"{f}-{n}" for f, n in PACKED_KEYS])
def test_packed_conversion_and_closure_checks(family, name, form):
    check_packed(family, name, form)
