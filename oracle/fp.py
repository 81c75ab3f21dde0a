"""The rounding model and the bound comparison that every host restatement and every test shares: the formats' constants, one-rounding fp32
helpers, the seeded grid of exactly representable inputs, bit views, and THE check of a result against a reference and an elementwise bound.
numpy only; nothing here is measured from a kernel. It lives in oracle/ because oracle/attention_oracle.py and oracle/trunk_rows_oracle.py
need it as much as the helpers under tests/ do.

The comparison is written once because it is the place where a NaN can hide: `ratio.max() > 1.0` is False for a NaN, and so is `err > tol`.
worst_ratio() maps every non-finite error to infinity, and assert_within() fails unless `worst <= 1.0` holds."""
import numpy as np

U32 = 2.0 ** -24      # fp32 unit roundoff (half an ulp of a value in [1, 2))
X1ULP = 2.0 ** -23    # one fp32 ulp: what the ISA documents for v_exp_f32 / v_rcp_f32 / v_rsq_f32 / v_log_f32, and an MFMA's internal adds
H16 = 2.0 ** -11      # fp16 half ulp of a normal value, relative
Z16 = 2.0 ** -25      # half the fp16 subnormal spacing: the absolute rounding error of a value below N16
N16 = 2.0 ** -14      # fp16's smallest normal; the exponent field of every subnormal and of zero
F16_MAX = 65504.0     # the largest finite fp16
F16_EDGE = 65520.0    # the least magnitude that rounds to an fp16 infinity
LOG2E32 = np.float32(1.4426950408889634)


def gamma(k):
    """the error factor of k chained fp32 roundings"""
    return k * U32 / (1 - k * U32)


def r16(y):
    """the absolute error of the fp16 rounding of a value of magnitude at most y"""
    return np.maximum(H16 * y, Z16)


def fma32(a, b, c):
    """fp32(a * b + c) with ONE rounding, each operand first taken to fp32 (no change for one that is fp32 already): the fp64 product of two
    fp32 is exact, and so is its fp64 sum with a third wherever the result's rounding could tell"""
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    return (a * b + c).astype(np.float32)


def exp2_32(t):
    """fp32 exp2 of the fp32 value of t; results that underflow or overflow do so silently, as v_exp_f32's do"""
    with np.errstate(under="ignore", over="ignore"):
        return np.exp2(t.astype(np.float32)).astype(np.float32)


def grid(shape, seed, scale=1.0, dtype=np.float32):
    """seeded multiples of 1/8 in [-2, 2], times `scale` (a power of two): exact in fp16 as in fp32, so every dtype holds the same values"""
    rng = np.random.default_rng([seed, *shape, 7])
    return (rng.integers(-16, 17, size=shape) / 8.0 * scale).astype(dtype)


def bits(a):
    """the bit patterns of a 2- or 4-byte array, as unsigned integers"""
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def same_bits(a, b):
    """dtype, shape and every bit equal (NaN payloads and the sign of zero included)"""
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


def worst_ratio(got, ref, bnd):
    """(largest |got - ref| / bound, its index: a tuple of ints, one per axis). An element with bound 0 must be exact; a non-finite error (a NaN
    or an infinity in `got` where the reference is finite) is infinitely far; nothing to compare is 0.0 at an index of zeros."""
    got, ref, bnd = np.broadcast_arrays(*(np.asarray(a, np.float64) for a in (got, ref, bnd)))
    if got.size == 0:
        return 0.0, (0,) * got.ndim
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.divide(err, bnd, out=err)
        i = np.unravel_index(np.argmax(ratio), ratio.shape)  # (the first NaN if there is one)
        if np.isnan(ratio[i]):  # 0 / 0, or a non-finite error: the cases spelled out (a clean comparison never comes here)
            err = np.abs(got - ref)
            err = np.where(np.isfinite(err), err, np.inf)
            ratio = np.where(err == 0, 0.0, err / bnd)
            i = np.unravel_index(np.argmax(ratio), ratio.shape)
    return float(ratio[i]), tuple(int(k) for k in i)


def assert_within(got, ref, bnd, label, where=None):
    """Fails unless every |got - ref| <= bnd (a NaN anywhere fails). The message names `label`, how many elements are outside, the worst
    one's index, the three values there and where(index) if given. Returns the worst ratio. Prints nothing: the callers report."""
    worst, at = worst_ratio(got, ref, bnd)
    if not worst <= 1.0:
        got, ref, bnd = np.broadcast_arrays(*(np.asarray(a, np.float64) for a in (got, ref, bnd)))
        outside = int((~(np.abs(got - ref) <= bnd)).sum())
        raise AssertionError(f"{label}: {outside} element(s) outside the bound, worst |got - ref| / bound = {worst:.4g} at {at}"
                             f"{'' if where is None else ' (' + str(where(at)) + ')'}: got {float(got[at])!r}, reference {float(ref[at])!r}, bound {float(bnd[at]):.3e}")
    return worst
