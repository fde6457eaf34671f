"""An independent numpy restatement of the semiring product, and the operand sets that probe its edges.

reference() is Naive (include/Utility.h:18-42, as oracle/mm_oracle.c's header describes it) written again without the C
oracle:  acc = identity; for k ascending: acc = Reduce(acc, Map(a[n, k], b[k, m])), vectorised over (n, m).
- Integers: Add and Multiply in the unsigned type of the same width (wrap-around mod 2^width, well defined in numpy and
  in C for unsigned types), viewed back; Min / Max are typed compares written as std::min / std::max; And is
  (a != 0) & (b != 0) as 0 / 1.  Identities as include/mm_gemm.h states them: Add 0, Multiply 1, And 1, Min max(),
  Max lowest().
- float / double / half: every operation in the element type, one rounding each, nothing fused.  numpy's binary16 + and *
  are correctly rounded (computed in float32, which has more than 2 * 11 + 2 bits, then rounded once).
- auto_minmax=True: floating-point Min / Max as MM_PATH_AUTO's register-tiled kernels document them (IEEE minNum /
  maxNum: a NaN operand is dropped); signed-zero ties are left open, so compare such results by value.

exact_and_scale() gives the (Multiply, Add) tolerance families their yardstick: the exact value and sum |a||b| in a
wider type (float64 for half and float, np.longdouble for double).

TEST INFRASTRUCTURE ONLY."""
import numpy as np

NP_DTYPES = {"float": np.float32, "double": np.float64, "half": np.float16, "int8_t": np.int8,
             "uint8_t": np.uint8, "int16_t": np.int16, "uint16_t": np.uint16, "int": np.int32,
             "unsigned": np.uint32, "long": np.int64, "unsigned long": np.uint64}
DTYPES = list(NP_DTYPES)
FLOATS = ("float", "double", "half")
OPS = ("Add", "Multiply", "And", "Min", "Max")
CONFIGS = [(d, mp, rd) for d in DTYPES for mp in OPS for rd in OPS]   # 11 x 5 x 5 = 275
_UNSIGNED = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}


def is_float(dtype):
    return dtype in FLOATS


def limits(dtype):
    """(lowest(), max()) of mm_common.h's Limits<T>."""
    t = NP_DTYPES[dtype]
    info = np.finfo(t) if is_float(dtype) else np.iinfo(t)
    return t(info.min), t(info.max)


def identity(dtype, op):
    t = NP_DTYPES[dtype]
    lo, hi = limits(dtype)
    return {"Add": t(0), "Multiply": t(1), "And": t(1), "Min": hi, "Max": lo}[op]


def _apply(op, x, y, t, auto_minmax):
    """Op<op, T>::apply(x, y) on arrays of type t."""
    if op == "And":
        return ((x != 0) & (y != 0)).astype(t)
    if op == "Min":
        if auto_minmax and t in (np.float16, np.float32, np.float64):
            return np.fmin(x, y)
        return np.where(y < x, y, x)        # std::min(x, y): y if y < x else x
    if op == "Max":
        if auto_minmax and t in (np.float16, np.float32, np.float64):
            return np.fmax(x, y)
        return np.where(x < y, y, x)        # std::max(x, y): y if x < y else x
    if np.issubdtype(t, np.integer):
        u = _UNSIGNED[np.dtype(t).itemsize]
        xu, yu = x.astype(t).view(u), y.astype(t).view(u)
        r = xu + yu if op == "Add" else xu * yu
        return r.astype(u).view(t)
    r = x + y if op == "Add" else x * y
    return r.astype(t)


def reference(dtype, map_op, reduce_op, a, b, transposed_a=False, auto_minmax=False):
    """C = A (map, reduce) B by Naive's definition; a is N x K (K x N with transposed_a), b is K x M."""
    t = NP_DTYPES[dtype]
    a = np.asarray(a, dtype=t)
    b = np.asarray(b, dtype=t)
    if transposed_a:
        a = a.T
    n, k = a.shape
    m = b.shape[1]
    assert b.shape[0] == k
    acc = np.full((n, m), identity(dtype, reduce_op), dtype=t)
    with np.errstate(all="ignore"):
        for kk in range(k):
            mapped = _apply(map_op, a[:, kk:kk + 1], b[kk:kk + 1, :], t, auto_minmax)
            acc = _apply(reduce_op, acc, mapped, t, auto_minmax)
    return acc


def wide_type(dtype):
    """The type exact_and_scale() computes in, or None when this platform has none wide enough."""
    if dtype in ("half", "float"):
        return np.float64
    if dtype == "double":
        return np.longdouble if np.finfo(np.longdouble).nmant >= 63 else None
    raise ValueError(dtype)


def exact_and_scale(dtype, a, b, transposed_a=False):
    """(A B, |A| |B|) of finite operands in wide_type(dtype)."""
    w = wide_type(dtype)
    a = np.asarray(a).astype(w)
    b = np.asarray(b).astype(w)
    if transposed_a:
        a = a.T
    return a @ b, np.abs(a) @ np.abs(b)


def same_bits(x, y):
    """Bit equality with every NaN taken as one value (which NaN payload an operation hands on is not specified)."""
    if x.dtype.kind != "f":
        return np.array_equal(x, y)
    u = _UNSIGNED[x.dtype.itemsize]
    nx, ny = np.isnan(x), np.isnan(y)
    return np.array_equal(nx, ny) and np.array_equal(x.view(u)[~nx], y.view(u)[~ny])


def same_values(x, y):
    """Equality by value: +0 == -0, every NaN one value."""
    if x.dtype.kind != "f":
        return np.array_equal(x, y)
    nx, ny = np.isnan(x), np.isnan(y)
    return np.array_equal(nx, ny) and np.array_equal(x[~nx], y[~ny])


def first_difference(x, y, by_value=False):
    """Index of the first element where x and y differ (in the sense of same_bits / same_values), or None."""
    if x.dtype.kind == "f":
        nx, ny = np.isnan(x), np.isnan(y)
        if by_value:
            diff = (nx != ny) | (~nx & ~ny & (x != y))
        else:
            u = _UNSIGNED[x.dtype.itemsize]
            diff = (nx != ny) | (~nx & ~ny & (x.view(u) != y.view(u)))
    else:
        diff = x != y
    idx = np.argwhere(diff)
    return None if idx.size == 0 else tuple(int(i) for i in idx[0])


def binary_result(map_op, reduce_op):
    """True when every output is 0 or 1 (an And reduction, or an And map under a non-Add reduction)."""
    return reduce_op == "And" or (map_op == "And" and reduce_op != "Add")


def assert_not_degenerate(ref, map_op, reduce_op, what):
    """A comparison of two constant arrays proves nothing: the reference must take several values."""
    vals = np.unique(ref[~np.isnan(ref)] if ref.dtype.kind == "f" else ref)
    if binary_result(map_op, reduce_op):
        assert set(vals.tolist()) == {0, 1}, f"degenerate reference for {what}: values {vals[:8]}"
    else:
        assert vals.size >= 3, f"degenerate reference for {what}: values {vals[:8]}"


# ---- operand sets ----------------------------------------------------------------------------------------------------
def int_specials(dtype):
    """0, 1, -1 / all-ones, min, max (and 2^31, 2^32 - 1, 2^32 for the 64-bit types)."""
    t = NP_DTYPES[dtype]
    info = np.iinfo(t)
    vals = [0, 1, info.max, info.min]
    if info.min < 0:
        vals.append(-1)
    else:
        vals.append(info.max)                 # all ones
    if info.bits == 64:
        vals += [2 ** 31, 2 ** 32 - 1, 2 ** 32]
    return np.array(vals, dtype=object).astype(t)


def float_specials(dtype, non_finite, largest=True):
    """+-0, the smallest and the largest subnormal, the smallest normal, (the largest finite value), and with non_finite
    +-inf and NaN -- each with both signs."""
    t = NP_DTYPES[dtype]
    fi = np.finfo(t)
    tiny_sub = fi.smallest_subnormal
    big_sub = t(fi.smallest_normal - tiny_sub)
    vals = [t(0), tiny_sub, big_sub, fi.smallest_normal]
    if largest:
        vals.append(fi.max)
    vals = vals + [-v for v in vals]
    if non_finite:
        vals += [t(np.inf), t(-np.inf), t(np.nan)]
    return np.array(vals, dtype=t)


def _plant(rng, arr, values, rate):
    flat = arr.reshape(-1)
    count = rng.binomial(flat.size, min(rate, 1.0))
    idx = rng.choice(flat.size, size=count, replace=False)
    flat[idx] = rng.choice(values, size=count)


def _zero_rate(map_op, k):
    """Zeros planted for an And map or reduction, so that about half of the k-chains see a zero mapped value: an Add map
    needs both operands zero, every other map one of them."""
    return np.sqrt(0.7 / k) if map_op == "Add" else 0.35 / k


def int_operands(dtype, map_op, reduce_op, a_shape, b_shape, rng, a_row_axis=0):
    """Uniform over every bit pattern of the type; the specials planted; one row of A all min(), one column of B all
    max(); odd values for a Multiply reduction, zeros planted for And.  a_row_axis: the axis of A that indexes the output's rows (1 for a K x N A)."""
    t = NP_DTYPES[dtype]
    u = _UNSIGNED[np.dtype(t).itemsize]
    a = rng.integers(0, np.iinfo(u).max, size=a_shape, dtype=u, endpoint=True).view(t)
    b = rng.integers(0, np.iinfo(u).max, size=b_shape, dtype=u, endpoint=True).view(t)
    k = b_shape[0]
    specials = int_specials(dtype)
    if reduce_op == "And":
        specials = specials[specials != 0]
    for arr in (a, b):
        _plant(rng, arr, specials, 1.0 / k)
    lo, hi = limits(dtype)
    row = 1 % a.shape[a_row_axis]
    if a_row_axis == 0:
        a[row, :] = lo
    else:
        a[:, row] = lo
    b[:, 2 % b.shape[1]] = hi
    if reduce_op == "Multiply":   # odd mapped values: products do not collapse to 0 mod 2^width
        a |= t(1)
        if map_op == "Add":       # odd + even
            b &= ~t(1)
        else:
            b |= t(1)
    if "And" in (map_op, reduce_op):
        for arr in (a, b):
            _plant(rng, arr, np.array([0], dtype=t), _zero_rate(map_op, k))
    _zero_row(a, map_op, a_row_axis)
    return a, b


def float_window(dtype, map_op, reduce_op):
    """Binary exponents drawn from [-w, w): wide where the reduction cannot overflow, near 1 for a Multiply reduction."""
    if reduce_op == "Multiply":
        return None
    if map_op == "Multiply":
        return {"half": 3, "float": 56, "double": 500}[dtype]
    return {"half": 5, "float": 110, "double": 1000}[dtype]


def float_operands(dtype, map_op, reduce_op, a_shape, b_shape, rng, non_finite, largest=True, a_row_axis=0):
    """Random signs; exponents spread over float_window(); the specials of float_specials() planted at about one per
    k-chain of each operand; with non_finite, one row of A all +inf (a_row_axis: as int_operands)."""
    t = NP_DTYPES[dtype]
    k = b_shape[0]
    w = float_window(dtype, map_op, reduce_op)

    def draw(shape, near_one_scale=1.0):
        sign = rng.choice(np.array([-1.0, 1.0]), size=shape)
        if w is None:      # a Multiply reduction: magnitudes 2^[-1/4, 1/4) keep a chain of K products inside the range
            mag = near_one_scale * np.exp2(rng.uniform(-0.25, 0.25, size=shape))
        else:
            mag = np.ldexp(rng.uniform(1.0, 2.0, size=shape), rng.integers(-w, w, size=shape))
        return (sign * mag).astype(t)

    a = draw(a_shape)
    # (Add, Multiply): a + b near +-1, so a B of magnitude ~1/8 next to an A of ~1
    b = draw(b_shape, 0.125 if (w is None and map_op == "Add") else 1.0)
    specials = float_specials(dtype, non_finite, largest)
    if reduce_op in ("Multiply", "And"):
        specials = specials[specials != 0]
    for arr in (a, b):
        _plant(rng, arr, specials, 0.5 / k)
    if "And" in (map_op, reduce_op):
        for arr in (a, b):
            _plant(rng, arr, np.array([0.0, -0.0], dtype=t), _zero_rate(map_op, k))
    _zero_row(a, map_op, a_row_axis)
    if non_finite:
        if a_row_axis == 0:
            a[INF_ROW, :] = np.inf
        else:
            a[:, INF_ROW] = np.inf
    return a, b


INF_ROW = 3   # the row of A that float_operands(non_finite=True) sets to +inf
ZERO_ROW = 5  # the row of A that is all zero under an And map: a row of outputs whose mapped values are all 0


def _zero_row(a, map_op, a_row_axis):
    if map_op == "And":
        if a_row_axis == 0:
            a[ZERO_ROW % a.shape[0], :] = 0
        else:
            a[:, ZERO_ROW % a.shape[1]] = 0
