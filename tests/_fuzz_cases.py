"""The deterministic case generator of the differential shape fuzz (tests/test_gpu_fuzz.py, checked on the CPU by
tests/test_fuzz_cases.py).  It needs the library, for the pure-arithmetic mm_kernel_name_* functions, but no GPU.

cases(call, dtype, seed, count) returns `count` Case records for one product call and operand type.  Dimensions come from
pools built around the serving rules of include/mm_gemm.h -- K % 4 / M % 4, the 16-byte chunk of the A x B^T pre-pass, the
matrix-core kernels' K % 16 / 32 / 64 / 128 with K >= 128 / 256 / 512, the 64 x 64 kernels' slab of 16 with its one-k tail, the
padding to 64 of the log-sum-exp hybrid, the block sizes of the closure -- not from uniform ranges.  Every case is one the C
ABI accepts: a C stride padded by one element and a base moved by one element are drawn only where the call takes them (every
call but the batched / accumulating one, which takes them under the k-ordered contracts: "ordered", "ordered_tile",
"ordered_wide_f16", and whose fast families want every matrix of a batch 16-byte aligned -- a batch whose dense strides are
not is drawn again).

Two things bound a case.  The numpy reference it will be compared with: a case whose N * K * M * batch is beyond the
budget of its reference (a loop over k, a BLAS product, an N x K x M array of log-sum-exp terms, N^3 for the closure) is
drawn again.  And coverage: from a stream of 40 * count candidates the generator takes, greedily, the candidate that adds
most to "every kernel name three times, and once in each of its forms" (seeded, batch > 1, K x N A, a broadcast operand, a
moved base; a K around the fp32 flush counts as one more), and fills up with the stream's first candidates once nothing is missing.  Both are pure functions of (call,
dtype, seed, count) and of the resolvers, so a failure reproduces from its record.

TEST INFRASTRUCTURE ONLY."""
import collections
import zlib

import numpy as np

import gemm_hls_amd as g

CALLS = ("batched", "argreduce", "argreduce_nt", "logsumexp", "logsumexp_nt", "widen", "nt", "closure")
NT_CALLS = ("argreduce_nt", "logsumexp_nt", "nt")          # B stored M x K: no K x N A

NM_POOL = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 511, 513, 700]
M_UNITS = [1, 2, 3, 7, 8, 15, 16, 17, 31, 32, 33, 40, 64, 65]   # times the family's M multiple (test_gpu_fuzz._shapes)
K_POOL = [1, 2, 3, 4, 5, 15, 16, 17,                            # the 64 x 64 kernels' slab of 16 and its one-k tail
          31, 32, 33, 48, 63, 64, 96, 112, 127, 128, 160, 255, 256, 257, 320, 511, 512, 640]
K_MAX = 700
BATCHES = [1, 2, 3, 5]
CLOSURE_N = [1, 2, 63, 64, 65, 127, 128, 129, 200, 255, 256, 257, 300, 513]
CLOSURE_BATCHES = [1, 2, 3]
STRIDES = ("dense", "a_bcast", "b_bcast", "c_pad64", "c_pad1")
FORMS = ("seeded", "batch", "kxn", "bcast", "misalign")

MA = ("Multiply", "Add")
#  dtype: (K step, M multiple, N multiple of a K x N A) of the (Multiply, Add) matrix-core family
_MFMA_STEPS = {"float": (8, 4, 4), "double": (8, 2, 2), "half": (16, 8, 8), "int8_t": (32, 16, 16), "uint8_t": (32, 16, 16)}
_VALU_STEPS = (4, 4, 4)
_ES = {"float": 4, "double": 8, "half": 2, "int8_t": 1, "uint8_t": 1, "int16_t": 2, "int": 4, "long": 8}

_ARG = [("Add", "Min"), ("Add", "Max"), ("Multiply", "Max")]
_LSE = [("Add", "Max"), ("Add", "Min")]
CONFIGS = {
    "batched": {"float": [MA, ("Add", "Min")], "double": [MA, ("Add", "Max")], "half": [MA], "int8_t": [MA], "uint8_t": [MA],
                "int": [MA], "long": [("Min", "Max")], "int16_t": [MA]},
    "argreduce": {d: _ARG for d in ("float", "half", "int", "uint8_t", "double", "long")},
    "argreduce_nt": {d: _ARG for d in ("float", "half", "int", "uint8_t", "double", "long")},
    "logsumexp": {d: _LSE for d in ("half", "float", "double")},
    "logsumexp_nt": {d: _LSE for d in ("half", "float", "double")},
    "widen": {"int8_t": [MA], "half": [MA]},
    "nt": {"float": [MA, ("Add", "Min")], "double": [MA], "half": [MA], "int8_t": [MA], "uint8_t": [MA], "int": [MA],
           "long": [("Min", "Max")]},
    "closure": {"float": [("Add", "Min")], "double": [("Add", "Max")], "half": [("Min", "Max")], "int8_t": [("Add", "Min")],
                "int": [("Multiply", "Min")], "long": [("Add", "Min")]},
}

# the batched / accumulating call refuses an offset view or an odd stride for its fast families; these names take them
ORDERED_CONTRACT = ("ordered", "ordered_tile", "ordered_wide_f16")

Case = collections.namedtuple("Case", "call dtype mp rd path n k m batch ta seeded stride misalign witness name draw")


def forms(case):
    """The forms of FORMS a case exercises."""
    return tuple(f for f, on in zip(FORMS, (case.seeded, case.batch > 1, case.ta, case.stride in ("a_bcast", "b_bcast"),
                                            case.misalign is not None)) if on)


def strides(case):
    """(stride_a, stride_b, stride_c) in elements: 0 for a broadcast operand, C dense or padded by 64 or by 1 element."""
    sa = 0 if case.stride == "a_bcast" else case.n * case.k
    sb = 0 if case.stride == "b_bcast" else case.k * case.m
    return sa, sb, case.n * case.m + {"c_pad64": 64, "c_pad1": 1}.get(case.stride, 0)


def name_of(call, dtype, mp, rd, path, n, k, m, batch, ta=False, witness=False):
    """What the call's resolver names for this problem (static strings, no device touched)."""
    cfg = g.make_config(dtype, mp, rd, path, ta)
    if call == "closure":
        return g.kernel_name_closure(cfg, n, batch, witness)
    fn = {"batched": g.kernel_name_batched, "argreduce": g.kernel_name_argreduce, "argreduce_nt": g.kernel_name_argreduce_nt,
          "logsumexp": g.kernel_name_logsumexp, "logsumexp_nt": g.kernel_name_logsumexp_nt, "widen": g.kernel_name_widen,
          "nt": g.kernel_name_nt}[call]
    return fn(cfg, n, k, m, batch)


def steps(call, dtype, mp, rd):
    """(K step, M multiple, N multiple of a K x N A) of the fast family that serves this configuration."""
    ks, mm, nm = _MFMA_STEPS.get(dtype, _VALU_STEPS) if (mp, rd) == MA else _VALU_STEPS
    if call in NT_CALLS:   # K and M in 16-byte chunks of elements
        epc = 16 // _ES[dtype]
        ks, mm = max(ks, epc), max(mm, epc)
    return ks, mm, nm


def flushes(call, dtype, mp, rd):
    """Whether one case in eight sits around the fp32 accumulator flush (every 4096 k)."""
    return dtype == "float" and (mp, rd) == MA and call in ("batched", "nt")


def budget(call, dtype, mp, rd, path):
    """The largest N * K * M * batch (closure: n^3 * batch) whose numpy reference stays well below a second."""
    if call == "closure":
        # n = 300 in a batch of 3 and n = 513 alone (513^3 = 135 005 697); numpy's binary16 is ten times slower: n = 300 alone
        return 1 << 25 if dtype == "half" else 140_000_000
    if call in ("logsumexp", "logsumexp_nt"):
        return 1 << 20 if dtype == "double" else 1 << 22   # an N x K x M array of terms in float64 / (slow) longdouble
    if (mp, rd) == MA and path == g.PATH_AUTO:
        if dtype in ("float", "double") or (dtype == "half" and call in ("batched", "widen")):
            return 1 << 30                              # a BLAS product in float64
        if call == "widen":
            return 1 << 25                              # an int64 product
    return 1 << 23                                      # a loop over k on N x M arrays in the element type


def k_candidates(kstep, flush):
    ks = sorted(set(K_POOL) | set(range(kstep, K_MAX + 1, kstep)))
    return ks + ([4096, 4096 + kstep, 8192 - kstep, 8192 + 2 * kstep] if flush else [])


def m_candidates(mmul):
    return sorted(set(NM_POOL) | {u * mmul for u in M_UNITS})


def _draw(call, dtype, rng, draw):
    """One candidate: a Case that the C ABI accepts and whose reference fits the budget."""
    pick = lambda xs: xs[int(rng.integers(len(xs)))]   # noqa: E731
    while True:
        mp, rd = pick(CONFIGS[call][dtype])
        path = g.PATH_ORDERED if rng.random() < 1 / 3 else g.PATH_AUTO
        if call == "closure":
            n, batch = pick(CLOSURE_N), pick(CLOSURE_BATCHES)
            witness = bool(rng.random() < 0.5)
            if n ** 3 * batch > budget(call, dtype, mp, rd, path):
                continue
            stride = pick(("dense", "c_pad64", "c_pad1")) if batch > 1 else "dense"
            misalign = "c" if rng.random() < 1 / 6 else None
            return Case(call, dtype, mp, rd, path, n, n, n, batch, False, False, stride, misalign, witness,
                        name_of(call, dtype, mp, rd, path, n, n, n, batch, False, witness), draw)
        kstep, mmul, nmul = steps(call, dtype, mp, rd)
        ta = call not in NT_CALLS and bool(rng.random() < 1 / 3)
        n = pick(NM_POOL)
        m = pick(M_UNITS) * mmul if rng.random() < 0.6 else pick(NM_POOL)
        k = pick(K_POOL) if rng.random() < 0.6 else int(rng.integers(1, K_MAX // kstep + 1)) * kstep
        if flushes(call, dtype, mp, rd) and rng.random() < 1 / 8:
            k = pick([4096, 4096 + kstep, 8192 - kstep, 8192 + 2 * kstep])
            n, m = min(n, 300), min(m, 160)
        if ta and rng.random() < 0.7:
            n = (n + nmul - 1) // nmul * nmul          # a K x N A is served by the fast kernels when N is a multiple
        batch = pick(BATCHES)
        if n * k * m * batch > budget(call, dtype, mp, rd, path):
            continue
        seeded = bool(rng.random() < 0.5)
        name = name_of(call, dtype, mp, rd, path, n, k, m, batch, ta)
        unaligned_ok = call != "batched" or name in ORDERED_CONTRACT
        stride = pick(STRIDES if unaligned_ok else STRIDES[:4]) if batch > 1 else "dense"
        operands = ("a", "b", "c", "i") if call.startswith("argreduce") else ("a", "b", "c")
        misalign = pick(operands) if unaligned_ok and rng.random() < 1 / 6 else None
        case = Case(call, dtype, mp, rd, path, n, k, m, batch, ta, seeded, stride, misalign, False, name, draw)
        if not unaligned_ok and batch > 1 and any(s * _ES[dtype] % 16 for s in strides(case)):
            continue   # (an odd N x M, N x K or K x M: the fast families want every element of the batch 16-byte aligned)
        return case


def cases(call, dtype, seed, count):
    """`count` cases of `call` on `dtype`, the same list for the same arguments."""
    rng = np.random.default_rng([zlib.crc32(f"{call}/{dtype}".encode()), seed])
    stream = [_draw(call, dtype, rng, i) for i in range(40 * count)]
    draws, seen, picked = collections.Counter(), set(), []

    def marks(c):   # the forms, and a K around the fp32 flush, which a kernel must meet as well
        return forms(c) + (("flush",) if c.k >= 4096 else ())

    def gain(c):
        return (draws[c.name] < 3) + sum((c.name, f) not in seen for f in marks(c))

    left = list(stream)
    while left and len(picked) < count:
        best = max(left, key=gain)                      # the first of the best: deterministic
        if gain(best) == 0:
            break
        left.remove(best)
        picked.append(best)
        draws[best.name] += 1
        seen.update((best.name, f) for f in marks(best))
    picked += left[:count - len(picked)]
    return sorted(picked, key=lambda c: c.draw)


# ---- what tests/test_gpu_fuzz.py runs, and tests/test_fuzz_cases.py walks ---------------------------------------------------
#  (call, dtype): (seed, count at MM_FUZZ_SCALE = 1).  Two dozen cases each; fewer where a case costs more on the host -- the
#  closure's restatement is n^3 in numpy, and numpy's binary16 is slow -- so that no group takes longer than the slowest of
#  the older fuzz tests.  tests/test_fuzz_cases.py says whether a count still reaches everything.
PLAN = {(call, dtype): (1, 24) for call in CALLS for dtype in CONFIGS[call]}
PLAN.update({("closure", dtype): (1, 6) for dtype in CONFIGS["closure"]})
PLAN.update({("closure", "half"): (1, 5), ("closure", "int"): (1, 5), ("argreduce", "half"): (1, 18), ("argreduce_nt", "half"): (1, 18)})


def planned(call, dtype, scale=1):
    """(seed, the cases) of one group of the plan, the counts multiplied by `scale`."""
    seed, count = PLAN[call, dtype]
    return seed, cases(call, dtype, seed, count * scale)


def case_rng(seed, case):
    """The generator a case's operands are drawn from: a function of the group's seed and the case's place in the stream."""
    return np.random.default_rng([seed, case.draw, zlib.crc32(f"{case.call}/{case.dtype}".encode())])


CLOSURE_INFORMATIVE_MIN_N = 63   # (a graph of 1 or 2 vertices has 1 or 4 entries: _closure_ref.assert_informative cannot hold)


def closure_block(case):
    """The block size closure_block = -1 chooses: what the restatement must run at."""
    return 256 if not case.witness and _ES[case.dtype] <= 4 else 128


def closure_graphs(seed, case):
    """The (batch, n, n) graphs of a closure case (_closure_ref.graphs: sparse, with an informative closure)."""
    import _closure_ref as cr
    return cr.graphs(case.dtype, case.mp, case.rd, case.n, case_rng(seed, case), case.batch)
