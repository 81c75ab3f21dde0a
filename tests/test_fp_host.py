"""CPU (-m "not gpu"): oracle/fp.py, the comparison and the rounding model every other test stands on, checked against itself: a NaN or an
infinity anywhere fails the bound check and is named, a zero bound demands equality, the edge worst == 1.0 passes; the grid holds the same
values in every format; fma32 rounds once."""
import numpy as np
import pytest

from oracle import attention_oracle as ao
from oracle import fp

SHAPES = [(7,), (3, 5), (2, 3, 4)]
PLANTS = [pytest.param(np.nan, id="nan"), pytest.param(np.inf, id="+inf"), pytest.param(-np.inf, id="-inf")]


def clean(shape):
    """(got, ref, bnd): got inside the bound everywhere, at most half of it used"""
    rng = np.random.default_rng([len(shape), *shape])
    ref = rng.standard_normal(shape)
    bnd = 1e-3 * (1 + rng.random(shape))
    return ref + 0.5 * bnd * rng.uniform(-1, 1, shape), ref, bnd


def last_but_one(shape):
    return tuple(n - 1 for n in shape[:-1]) + (shape[-1] - 2,)


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_a_clean_array_passes_and_the_index_points_at_the_worst_element(shape):
    got, ref, bnd = clean(shape)
    worst, at = fp.worst_ratio(got, ref, bnd)
    assert 0 < worst <= 0.5 and len(at) == len(shape) and all(type(k) is int for k in at)
    assert fp.assert_within(got, ref, bnd, "clean") == worst
    at = last_but_one(shape)
    got[at] = ref[at] + 0.75 * bnd[at]
    assert fp.worst_ratio(got, ref, bnd) == (pytest.approx(0.75), at)


@pytest.mark.parametrize("v", PLANTS)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_a_planted_non_finite_value_is_infinitely_far(shape, v):
    got, ref, bnd = clean(shape)
    at = last_but_one(shape)
    got[at] = v
    assert fp.worst_ratio(got, ref, bnd) == (np.inf, at)
    assert fp.worst_ratio(got.astype(np.float16), ref, bnd)[0] == np.inf  # in the outputs' own type too
    with pytest.raises(AssertionError, match="planted: 1 element"):
        fp.assert_within(got, ref, bnd, "planted")
    # the forms this replaces cannot see the NaN: the maximum of the ratios is NaN, and NaN > 1.0 is False
    if np.isnan(v):
        with np.errstate(invalid="ignore"):
            assert not (np.abs(got - ref) / bnd).max() > 1.0 and not (np.abs(got - ref) > bnd).any()


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_a_zero_bound_demands_equality(shape):
    got, ref, bnd = clean(shape)
    at = last_but_one(shape)
    bnd[at], got[at] = 0.0, ref[at]
    assert fp.worst_ratio(got, ref, bnd)[0] <= 0.5 and fp.assert_within(got, ref, bnd, "exact") <= 0.5
    assert fp.worst_ratio(np.zeros(shape), np.zeros(shape), np.zeros(shape)) == (0.0, (0,) * len(shape))
    got[at] = np.nextafter(ref[at], np.inf)
    assert fp.worst_ratio(got, ref, bnd) == (np.inf, at)
    with pytest.raises(AssertionError, match="bound 0.000e\\+00"):
        fp.assert_within(got, ref, bnd, "one ulp off")


def test_nothing_to_compare_and_the_edge_of_the_bound():
    for shape in ((0,), (0, 5), (2, 0, 3)):
        e = np.zeros(shape)
        assert fp.worst_ratio(e, e, e) == (0.0, (0,) * len(shape)) and fp.assert_within(e, e, e, "empty") == 0.0
    ref, bnd = np.arange(8.0), np.full(8, 0.25)  # (exactly representable: the error IS the bound)
    got = ref.copy()
    got[5] += 0.25
    assert fp.worst_ratio(got, ref, bnd) == (1.0, (5,)) and fp.assert_within(got, ref, bnd, "edge") == 1.0
    got[5] = np.nextafter(got[5], np.inf)
    with pytest.raises(AssertionError, match=r"edge: 1 element\(s\) outside the bound.*at \(5,\) \(column 5\): got 5.25"):
        fp.assert_within(got, ref, bnd, "edge", where=lambda at: f"column {at[0]}")
    got[2] = np.nan
    with pytest.raises(AssertionError, match=r"2 element\(s\) outside the bound.*= inf at \(2,\)"):
        fp.assert_within(got, ref, bnd, "two")


def test_a_nan_in_the_attention_forward_fails_the_check_of_the_gpu_test():
    """tests/test_attention_gpu.py's check_bound is fp.assert_within on ao.reference_and_bound with ao.locator: a correct output (the
    emulation) with one NaN in a live row fails it. The comparison it had, `ratio.max() > 1.0`, lets it pass."""
    qkv, cu = ao.FAMILIES["realistic1"]([5, 97, 33], 2, 11)
    ref, bnd = ao.reference_and_bound(qkv, cu, 2, 2)
    got = ao.emulate(qkv, cu, 2, 2)
    assert fp.assert_within(got, ref, bnd, "clean", ao.locator(cu, 2)) <= 1.0
    got[100, 7] = np.nan
    with np.errstate(invalid="ignore"):
        assert not float((np.abs(got.astype(np.float64) - ref) / bnd).max()) > 1.0   # the hole
    with pytest.raises(AssertionError, match=r"at \(100, 7\) \(sequence 1, len 97, head 0\): got nan"):
        fp.assert_within(got, ref, bnd, "planted", ao.locator(cu, 2))


def test_the_grid_holds_the_same_values_in_every_format():
    for shape, scale in (((64,), 1.0), ((33, 70), 4.0), ((5, 6, 7), 2.0 ** -4), ((40, 40), 64.0)):
        g32, g16 = fp.grid(shape, 3, scale), fp.grid(shape, 3, scale, np.float16)
        assert g32.dtype == np.float32 and g16.dtype == np.float16 and g32.shape == g16.shape == shape
        assert np.array_equal(g32.astype(np.float64), g16.astype(np.float64))              # fp16-exact, the same values
        k = g32.astype(np.float64) / (scale / 8)
        assert np.array_equal(k, np.rint(k)) and np.abs(k).max() == 16 and len(np.unique(k)) > 16   # multiples of scale / 8 in [-2, 2] scale
        assert not np.array_equal(g32, fp.grid(shape, 4, scale)) and fp.same_bits(g32, fp.grid(shape, 3, scale))
    assert not fp.same_bits(g32, g16) and not fp.same_bits(g32, g32[:-1]) and not fp.same_bits(np.float32([0.0]), np.float32([-0.0]))
    assert fp.bits(g16).dtype == np.uint16 and fp.bits(g32).dtype == np.uint32 and fp.same_bits(np.float32([np.nan]), np.float32([np.nan]))


def test_fma32_rounds_once():
    rng = np.random.default_rng(9)
    a, b, c = (rng.standard_normal(20000).astype(np.float32) * np.float32(2.0) ** rng.integers(-8, 9, 20000).astype(np.float32) for _ in range(3))
    exact = a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)   # the product of two fp32 is exact in fp64; the sum errs by 2^-53 relative
    got = fp.fma32(a, b, c)
    assert got.dtype == np.float32
    half_ulp = np.spacing(np.abs(got)).astype(np.float64) / 2
    assert (np.abs(got.astype(np.float64) - exact) <= half_ulp * (1 + 2.0 ** -20)).all()
    # ... which two roundings do not keep: somewhere among 20000 the separately rounded product shows
    assert (np.abs((a * b + c).astype(np.float64) - exact) > half_ulp * (1 + 2.0 ** -20)).any()
    i, j, k = (rng.integers(-2000, 2001, 5000) for _ in range(3))
    assert np.array_equal(fp.fma32(i.astype(np.float32), j.astype(np.float32), k.astype(np.float32)), (i * j + k).astype(np.float32))
    # Python floats are taken to fp32 first, as the literals of a kernel are
    assert fp.fma32(np.float32([3.0]), 0.1, 0.2)[0] == np.float32(np.float64(3.0) * np.float64(np.float32(0.1)) + np.float64(np.float32(0.2)))
    assert fp.r16(1.0) == fp.H16 and fp.r16(0.0) == fp.Z16 and fp.r16(fp.N16) == fp.Z16 and fp.gamma(1) == fp.U32 / (1 - fp.U32)
    with np.errstate(over="ignore"):
        assert np.float16(fp.F16_MAX) == np.float16(65504) and np.isinf(np.float16(fp.F16_EDGE)) and np.isfinite(np.float16(np.nextafter(fp.F16_EDGE, 0.0)))
    assert fp.exp2_32(np.float32([-200.0, 0.0, 200.0])).tolist() == [0.0, 1.0, np.inf]
