"""Every (dtype, map, reduce) on full-range and edge-valued operands, subnormals through every (Multiply, Add) family, and
MM_PATH_SPLIT across the exponent range (run with -m gpu on an MI355X).

The rest of the suite mostly feeds the kernels the reference's draws (integers 1..10, reals in [1, 10)).  Here the
operands come from tests/_semiring_ref.py: every bit pattern of the integer types with 0, +-1, min and max planted; floating
operands of both signs spread over most of the exponent range with +-0, subnormals, the smallest normal, the largest
finite value, +-inf and NaN planted.  The yardstick is that module's numpy restatement of Naive (include/Utility.h:18-42),
written apart from the C oracle (tests/test_oracle.py pins the two against each other on all 275 configurations).

Contracts asserted (include/mm_gemm.h):
- MM_PATH_ORDERED: Naive's bits on every configuration and every operand set (NaN payloads aside).
- MM_PATH_AUTO: integer configurations Naive's bits; floating-point configurations run by the k-ordered kernels (Multiply
  and And reductions, the And map, shapes the register tile does not take) Naive's bits; the register-tiled VALU kernel
  Naive's values with IEEE minNum / maxNum for Min / Max (+0 == -0); floating (Multiply, Add) on the matrix cores and the
  wide-accumulate kernel within the bounds their families assert elsewhere, plus an absolute underflow term."""
import math
import zlib

import numpy as np
import pytest

import _oracle
import _semiring_ref as sr
import gemm_hls_amd as g

pytestmark = pytest.mark.gpu

KNOBS = ("f32_variant", "f64_variant", "f16_variant", "i8_variant", "band_rows", "valu_variant", "f32_splitk", "ordered_variant",
         "split_variant", "half_contract")


@pytest.fixture(autouse=True)
def _default_tuning():
    """Every test starts and ends on the library's own choices (knobs are process-wide)."""
    for knob in KNOBS:
        g.set_tuning(knob, -1)
    yield
    for knob in KNOBS:
        g.set_tuning(knob, -1)


PATHS = {"ordered": g.PATH_ORDERED, "auto": g.PATH_AUTO}
# (label, (n, k, m), A stored K x N, knobs): the row-major shape reaches the DMA-staged register tile (and the matrix cores
# for (Multiply, Add)); valu_variant 0 its synchronous staging, 2 the 8-rows-per-thread form of the 8-byte types; the K x N
# shape the synchronous transposed tile (and, K % 8 != 0, the VALU (Multiply, Add) of float / double); the ragged shape the
# predicated kernels; ordered_variant 0 the 64 x 64 anchor of the k-ordered contract.
RUNS = [("dma", (130, 128, 144), False, {}),
        ("sync", (130, 128, 144), False, {"valu_variant": 0}),
        ("rows8", (130, 128, 144), False, {"valu_variant": 2}),
        ("kxn", (132, 68, 100), True, {}),
        ("ragged", (37, 30, 22), False, {}),
        ("anchor", (130, 128, 144), False, {"ordered_variant": 0})]
MFMA = {"float": "mfma_f32_", "double": "mfma_f64_", "half": "mfma_f16_", "int8_t": "mfma_i8_", "uint8_t": "mfma_i8_"}

# (Multiply, Add) bounds of the floating families, as their own tests assert them (tests/_bounds.py NORTH_STAR_F32;
# tests/test_gpu_baseline_sizes.py test_f64_f16_mixed_sign), each with an absolute underflow term of K x the smallest
# subnormal: a chain of K fused multiply-adds rounds at most K times at the subnormal quantum.
REL = {"float": 1e-5, "double": 1e-13}


def _expected_kernel(dtype, mp, rd, path, shape, transposed_a, knobs):
    """The family include/mm_gemm.h says serves the launch (a prefix for the matrix-core families)."""
    n, k, m = shape
    tile = k % 4 == 0 and m % 4 == 0 and (not transposed_a or n % 4 == 0) and mp != "And" and rd in ("Add", "Min", "Max")
    if path == "ordered":
        return "ordered_tile" if tile and knobs.get("ordered_variant", -1) != 0 else "ordered"
    if (mp, rd) == ("Multiply", "Add") and dtype in MFMA:
        if shape == (130, 128, 144):
            return MFMA[dtype]
        if dtype == "half":
            return "ordered_wide_f16"
    return "valu_tile" if tile else "ordered"


def _where(ctx, c, want, idx):
    return f"{ctx}: first mismatch at {idx}: device {c[idx]!r}, reference {want[idx]!r}"


def _check_bound(ctx, dtype, c, a, b, transposed_a, wide_half_ref=None):
    exact, scale = sr.exact_and_scale(dtype, a, b, transposed_a)
    assert np.unique(exact).size >= 3, f"{ctx}: degenerate exact result"
    k = b.shape[0]
    tiny = np.finfo(sr.NP_DTYPES[dtype]).smallest_subnormal.astype(exact.dtype)
    assert np.all(np.isfinite(c)), f"{ctx}: non-finite output {sr.first_difference(c, np.nan_to_num(c))}"
    err = np.abs(c.astype(exact.dtype) - exact)
    if dtype == "half":
        # one rounding of the result to binary16 + fp32 accumulation noise (test_gpu_baseline_sizes.py); the rounding of a
        # result in the binary16 subnormal range is the 2^-25 term
        bound = 2.0 ** -11 * np.abs(exact) + 1e-6 * scale + 2.0 ** -25
    else:
        bound = REL[dtype] * scale + k * tiny
    bad = np.argwhere(err > bound)
    assert bad.size == 0, (f"{ctx}: |c - exact| above the bound at {tuple(bad[0])}: device {c[tuple(bad[0])]!r}, exact "
                           f"{exact[tuple(bad[0])]!r}, bound {bound[tuple(bad[0])]!r} ({bad.shape[0]} elements)")
    if wide_half_ref is not None:   # the wide contract: at most one binary16 ulp from the oracle's one-rounding Naive
        ulps = np.abs(c.view(np.int16).astype(np.int32) - wide_half_ref.view(np.int16).astype(np.int32))
        assert ulps.max() <= 1, f"{ctx}: {ulps.max()} ulps from the wide-accumulate Naive at {np.unravel_index(ulps.argmax(), ulps.shape)}"


class _Operands:
    """Operand sets and references of one configuration, drawn once per (shape, layout) and shared by every run."""

    def __init__(self, dtype, mp, rd):
        self.dtype, self.mp, self.rd = dtype, mp, rd
        self._sets, self._refs = {}, {}

    def sets(self, shape, transposed_a, path):
        n, k, m = shape
        key = (shape, transposed_a)
        if key not in self._sets:
            rng = np.random.default_rng(zlib.crc32(f"{self.dtype} {self.mp} {self.rd} {shape}".encode()))
            a_shape, axis = ((k, n), 1) if transposed_a else ((n, k), 0)
            d, mp, rd = self.dtype, self.mp, self.rd
            if not sr.is_float(d):
                s = {"full_range": sr.int_operands(d, mp, rd, a_shape, (k, m), rng, a_row_axis=axis)}
            else:
                s = {"finite": sr.float_operands(d, mp, rd, a_shape, (k, m), rng, non_finite=False, a_row_axis=axis),
                     "non_finite": sr.float_operands(d, mp, rd, a_shape, (k, m), rng, non_finite=True, a_row_axis=axis)}
                if (mp, rd) == ("Multiply", "Add"):   # the tolerance families: finite results only
                    s["finite_no_overflow"] = sr.float_operands(d, mp, rd, a_shape, (k, m), rng, non_finite=False, largest=False,
                                                                a_row_axis=axis)
            self._sets[key] = s
        s = self._sets[key]
        if sr.is_float(self.dtype) and (self.mp, self.rd) == ("Multiply", "Add"):
            names = ["finite_no_overflow"] if path == "auto" else ["finite", "non_finite", "finite_no_overflow"]
            return {nm: s[nm] for nm in names}
        return s

    def reference(self, shape, transposed_a, set_name, auto_minmax=False):
        key = (shape, transposed_a, set_name, auto_minmax)
        if key not in self._refs:
            a, b = self._sets[(shape, transposed_a)][set_name]
            ref = sr.reference(self.dtype, self.mp, self.rd, a, b, transposed_a=transposed_a, auto_minmax=auto_minmax)
            sr.assert_not_degenerate(ref, self.mp, self.rd, f"{self.dtype} ({self.mp}, {self.rd}) {set_name} {shape}")
            self._refs[key] = ref
        return self._refs[key]


@pytest.mark.parametrize("dtype,mp,rd", sr.CONFIGS, ids=lambda v: str(v).replace(" ", "_"))
def test_semiring_matrix_on_full_range_operands(dtype, mp, rd):
    """One configuration of the 275, through every kernel that serves it at the shapes of RUNS, under MM_PATH_ORDERED and
    MM_PATH_AUTO, on full-range and edge-valued operands."""
    ops = _Operands(dtype, mp, rd)
    itemsize = np.dtype(sr.NP_DTYPES[dtype]).itemsize
    hi = sr.limits(dtype)[1]
    for label, shape, transposed_a, knobs in RUNS:
        if label == "rows8" and itemsize != 8:
            continue
        n, k, m = shape
        for path_name, path in PATHS.items():
            for knob, value in knobs.items():
                g.set_tuning(knob, value)
            try:
                name = g.kernel_name(g.make_config(dtype, mp, rd, path, transposed_a), n, k, m)
                want_name = _expected_kernel(dtype, mp, rd, path_name, shape, transposed_a, knobs)
                assert name.startswith(want_name), (dtype, mp, rd, path_name, label, name, want_name)
                for set_name, (a, b) in ops.sets(shape, transposed_a, path_name).items():
                    ctx = (f"{dtype} ({mp}, {rd}) {path_name} {label} {n}x{k}x{m}{' K x N A' if transposed_a else ''} "
                           f"kernel {name} operands {set_name}")
                    c, _ = g.matmul_capi(a, b, dtype, mp, rd, path=path, transposed_a=transposed_a)
                    exact_kernel = name in ("ordered", "ordered_tile") or not sr.is_float(dtype)
                    if exact_kernel:
                        want = ops.reference(shape, transposed_a, set_name)
                        assert sr.same_bits(c, want), _where(ctx, c, want, sr.first_difference(c, want))
                    elif (mp, rd) == ("Multiply", "Add"):
                        _check_bound(ctx, dtype, c, a, b, transposed_a)
                    else:
                        assert name == "valu_tile", ctx
                        want = ops.reference(shape, transposed_a, set_name, auto_minmax=True)
                        assert sr.same_values(c, want), _where(ctx, c, want, sr.first_difference(c, want, by_value=True))
                    if set_name == "non_finite" and (mp, rd) == ("Add", "Min"):
                        # Naive's semantics: inf + b is never below the identity max(), so the row stays at max(), not inf
                        assert np.all(c[sr.INF_ROW] == hi), f"{ctx}: the all-+inf row of A gives {c[sr.INF_ROW][:4]}, not max()"
            finally:
                for knob in knobs:
                    g.set_tuning(knob, -1)


# ---- subnormals through the (Multiply, Add) families ------------------------------------------------------------------
EMIN = {"float": -126, "double": -1022, "half": -14}
MANT = {"float": 23, "double": 52, "half": 10}
# (label, dtype, (n, k, m), knobs, kernel-name prefix)
SUBNORMAL_CASES = [("f32_256x256", "float", (300, 128, 272), {"f32_variant": 8}, "mfma_f32_256x256"),
                   ("f32_64x64", "float", (130, 128, 144), {}, "mfma_f32_64x64"),
                   ("f32_splitk", "float", (512, 4096, 512), {}, "mfma_f32_64x64x32_w4x2_splitk"),
                   ("f32_streamk", "float", (2560, 512, 2560), {}, "mfma_f32_128x128x32_w4x2_streamk"),
                   ("f64", "double", (130, 128, 144), {}, "mfma_f64_"),
                   ("f16", "half", (130, 128, 144), {}, "mfma_f16_"),
                   ("wide_f16", "half", (130, 68, 100), {}, "ordered_wide_f16")]


def _signed(rng, shape, lo_exp, hi_exp):
    """+-[1, 2) * 2^e, e uniform in [lo_exp, hi_exp), in float64 (callers round to the element type)."""
    sign = rng.choice(np.array([-1.0, 1.0]), size=shape)
    return sign * np.ldexp(rng.uniform(1.0, 2.0, size=shape), rng.integers(lo_exp, hi_exp, size=shape))


def subnormal_operands(dtype, n, k, m, kind, rng):
    """kind "subnormal_a": A subnormal (the smallest and the largest subnormal planted), B scaled so that every product is
    a normal number -- a flush of A to zero leaves an O(1) error.  kind "subnormal_products": A and B normal, every
    product, partial sum and result below the smallest normal."""
    t = sr.NP_DTYPES[dtype]
    emin = EMIN[dtype]
    if kind == "subnormal_a":
        fi = np.finfo(t)
        a = _signed(rng, (n, k), emin - MANT[dtype] + 2, emin).astype(t)
        a[np.abs(a) >= fi.smallest_normal] = fi.smallest_normal - fi.smallest_subnormal     # rounded up onto 2^emin
        flat = a.reshape(-1)
        idx = rng.choice(flat.size, size=2 * k, replace=False)
        flat[idx] = rng.choice(np.array([fi.smallest_subnormal, fi.smallest_normal - fi.smallest_subnormal,
                                         -fi.smallest_subnormal], dtype=t), size=idx.size)
        # |b| >= 2^(MANT - 1): every product of a drawn |a| >= 2^(emin - MANT + 2) is normal (the planted smallest
        # subnormals give subnormal products, inside the bound's absolute term)
        b = _signed(rng, (k, m), MANT[dtype] - 1, MANT[dtype] + 2).astype(t)
    else:
        hi = (emin - math.ceil(math.log2(k))) // 2 - 1        # |a b| < 2^(2 hi + 2), K of them < 2^emin
        a = _signed(rng, (n, k), hi - 4, hi).astype(t)
        b = _signed(rng, (k, m), hi - 4, hi).astype(t)
    return a, b


@pytest.mark.parametrize("case", SUBNORMAL_CASES, ids=lambda c: c[0])
@pytest.mark.parametrize("kind", ["subnormal_a", "subnormal_products"])
def test_subnormals_through_every_multiply_add_family(case, kind):
    """MFMA C / D never flush and A / B follow MODE.denorm, which hipcc leaves at "keep": no family may flush.  (i) A
    subnormal, products normal: a flush shows as an O(1) error; (ii) products, partial sums and results subnormal: the
    family's bound including its absolute underflow term; half results in the binary16 subnormal range also within one ulp
    of the one-rounding Naive (rounding on store).  At the small shapes the k-ordered kernels and the VALU
    min / max tiles take the same operands and give Naive's bits (values, for the minNum / maxNum tile)."""
    label, dtype, (n, k, m), knobs, prefix = case
    rng = np.random.default_rng(len(label) * 7 + len(kind))
    a, b = subnormal_operands(dtype, n, k, m, kind, rng)
    t = sr.NP_DTYPES[dtype]
    fi = np.finfo(t)
    if kind == "subnormal_a":
        assert np.all((np.abs(a) < fi.smallest_normal) & (a != 0))
    else:
        exact, _ = sr.exact_and_scale(dtype, a, b)
        assert np.all(np.abs(exact) < fi.smallest_normal) and np.mean(exact != 0) > 0.99
    for knob, value in knobs.items():
        g.set_tuning(knob, value)
    name = g.kernel_name(g.make_config(dtype), n, k, m)
    ctx = f"{dtype} (Multiply, Add) auto {label} {n}x{k}x{m} kernel {name} operands {kind}"
    assert name.startswith(prefix), ctx
    c, _ = g.matmul_capi(a, b, dtype)
    # half: the one-ulp rule against the one-rounding Naive holds where f32 accumulation is exact enough for it -- the
    # subnormal results here (products and sums far above f32's quantum); with mixed signs and normal results the
    # cancellation can cost more, and the family's bound is the contract (test_f64_f16_mixed_sign)
    wide = None
    if dtype == "half" and kind == "subnormal_products":
        wide = _oracle.naive("half", "Multiply", "Add", a, b, wide_half=True)
        assert np.mean(np.abs(wide.astype(np.float64)) < fi.smallest_normal) > 0.99 and np.unique(wide).size > 16
    _check_bound(ctx, dtype, c, a, b, False, wide)
    for knob in knobs:
        g.set_tuning(knob, -1)
    if n * k * m > 130 * 128 * 144:
        return
    for path_name, mp, rd in [("ordered", "Multiply", "Add"), ("ordered", "Multiply", "Min"), ("ordered", "Add", "Max"),
                              ("auto", "Multiply", "Min"), ("auto", "Multiply", "Max"), ("auto", "Add", "Min")]:
        path = PATHS[path_name]
        name = g.kernel_name(g.make_config(dtype, mp, rd, path), n, k, m)
        assert name == _expected_kernel(dtype, mp, rd, path_name, (n, k, m), False, {}), name
        ctx = f"{dtype} ({mp}, {rd}) {path_name} {n}x{k}x{m} kernel {name} operands {kind}"
        c, _ = g.matmul_capi(a, b, dtype, mp, rd, path=path)
        want = sr.reference(dtype, mp, rd, a, b, auto_minmax=path_name == "auto")
        if dtype == "half" and kind == "subnormal_products" and rd != "Add":
            # binary16 products of these operands sit at the quantum 2^-24 (or round to 0): a min / max of them takes two or
            # three values -- which of them is exactly what the rounding of the product decides
            assert np.unique(want).size >= 2, ctx
        else:
            sr.assert_not_degenerate(want, mp, rd, ctx)
        same = sr.same_bits if path_name == "ordered" else sr.same_values
        assert same(c, want), _where(ctx, c, want, sr.first_difference(c, want, by_value=path_name == "auto"))


# ---- MM_PATH_SPLIT across the exponent range --------------------------------------------------------------------------
SPLIT_EXPONENTS = [100, 60, 0, -60, -100, -108, -112, -116, -120, -126, "subnormal"]
SPLIT_FULL_BITS_FROM = -112     # include/mm_gemm.h MM_PATH_SPLIT: the 2^-19 normwise bound holds for |operands| >= 2^-112
SPLIT_ABS = 2.0 ** -134         # and below that each operand is represented to within 2^-134 absolute


@pytest.mark.parametrize("tile", [256, 512], ids=["tile256", "tile128"])
@pytest.mark.parametrize("e", SPLIT_EXPONENTS, ids=str)
def test_split_path_across_the_exponent_range(e, tile):
    """A = +-[1, 2) 2^e, B = +-[1, 2) 2^-e: products O(1), operands normal, finite and below 2^127 -- and, from 2^-116 down,
    so small that x - bf16(x) falls below bf16's smallest normal and the second and third planes lose bits.  Asserted:
    the 2^-19 normwise bound where the documented range claims it, and everywhere the documented bound
    |c - AB| <= 2^-19 |A||B| + 2^-134 (sum_k |a_ik| + sum_k |b_kj|)."""
    n, k, m = 300, 96, 272
    rng = np.random.default_rng(zlib.crc32(f"split {e}".encode()))
    if e == "subnormal":     # fp32-subnormal A next to the largest B that stays below 2^127
        a = _signed(rng, (n, k), -149, -126).astype(np.float32)
        b = _signed(rng, (k, m), 125, 126).astype(np.float32)
    else:
        a = _signed(rng, (n, k), e, e + 1).astype(np.float32)
        b = _signed(rng, (k, m), -e, -e + 1).astype(np.float32)
    assert np.all(np.isfinite(a)) and np.all(np.isfinite(b)) and np.all(a != 0)
    g.set_tuning("split_variant", tile)
    name = g.kernel_name(g.make_config("float", path=g.PATH_SPLIT), n, k, m)
    assert name == "mfma_f32_split_bf16x3"
    c, _ = g.matmul_capi(a, b, path=g.PATH_SPLIT)
    exact, scale = sr.exact_and_scale("float", a, b)
    err = np.abs(c - exact)
    normwise = float(np.max(err / scale))
    abs_term = SPLIT_ABS * (np.abs(a).astype(np.float64).sum(axis=1)[:, None] + np.abs(b).astype(np.float64).sum(axis=0)[None, :])
    ctx = f"float (Multiply, Add) split e={e} {n}x{k}x{m} split_variant {tile} kernel {name}: normwise {normwise:.3e}"
    print(ctx)
    over = np.argwhere(err > 2.0 ** -19 * scale + abs_term)
    assert over.size == 0, f"{ctx}: above the documented bound first at {tuple(over[0])}"
    if e != "subnormal" and -SPLIT_FULL_BITS_FROM >= e >= SPLIT_FULL_BITS_FROM:
        assert normwise < 2.0 ** -19, ctx
