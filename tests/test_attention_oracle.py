"""CPU (-m "not gpu"): oracle/attention_oracle.py, the yardstick of tests/test_attention_gpu.py, checked against itself.

The bound of |device - fp64 reference| is derived from formats (see the oracle's docstring), so two things must be shown without a GPU:
it is not too TIGHT -- a second, independent statement of each kernel's dataflow (`emulate`: fp32 scores, fp16 p at the kernel's rounding
point, jobs of 96 with the rescale) sits inside it on every designed input family -- and it is not too LOOSE: each of the index / masking /
rescale defects a kernel of this shape can have, switched on in `emulate`, is pushed OUTSIDE it by at least one of the designed inputs.
"""
import numpy as np
import pytest

from oracle import attention_oracle as ao
from oracle import fp

LENS = [1, 2, 3, 15, 16, 17, 18, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 130, 160, 191, 192, 193, 224, 255, 256, 257, 288, 289, 300,
        383, 384, 385, 480, 481, 511, 512]
HEADS = 2
KERNELS = (1, 2, 3)


@pytest.mark.parametrize("family", sorted(ao.FAMILIES))
def test_emulation_sits_inside_the_bound(family):
    qkv, cu = ao.FAMILIES[family](LENS, HEADS, 11)
    for kernel in KERNELS:
        ref, bnd = ao.reference_and_bound(qkv, cu, HEADS, kernel)
        assert np.isfinite(bnd).all() and (bnd > 0).all()
        full = ao.reference(qkv, cu, HEADS)
        assert np.allclose(ref, ao.cls_rows(full, cu) if kernel == 3 else full, rtol=0, atol=1e-12)  # (fp64; BLAS may order a one-row product apart)
        r = fp.assert_within(ao.emulate(qkv, cu, HEADS, kernel), ref, bnd, f"{family} kernel {kernel}", ao.locator(cu, kernel))
        print(f"{family} kernel {kernel}: emulate worst |err| / bound = {r:.3f}")


def test_bound_is_of_the_size_of_two_fp16_roundings():
    """The bound is dominated by the two fp16 roundings (of p and of the output). On unit-scale realistic rows each is at most 2^-11 max |v|;
    a bound beyond three of them would let real defects through."""
    qkv, cu = ao.FAMILIES["realistic1"](LENS, HEADS, 5)
    vmax = float(np.abs(qkv[:, 2 * 64 * HEADS:].astype(np.float64)).max())
    for kernel in KERNELS:
        bnd = ao.bound(qkv, cu, HEADS, kernel)
        print(f"kernel {kernel}: bound max {bnd.max():.3e} = {bnd.max() / (2.0 ** -11 * vmax):.3f} x 2^-11 max|v|")
        assert bnd.max() <= 3 * 2.0 ** -11 * vmax and (bnd >= 2.0 ** -25).all()


def test_onehot_is_bit_exact_and_its_margin_holds():
    qkv, cu, expected = ao.onehot(LENS, HEADS, 3)
    for b, n in enumerate(LENS):  # the margin claim, from the fp64 scores: winner 125, every other key <= 100, so p_other <= e^-25 < 2^-36
        Q, K, _ = (x.astype(np.float64) for x in ao.split(qkv, cu, HEADS, b))
        S = np.sort(Q @ K.transpose(0, 2, 1) / 8.0, axis=2)
        assert (S[:, :, -1] == 125.0).all()
        assert n == 1 or (S[:, :, -2] <= 100.0).all()
    assert np.exp(-25.0) < 2.0 ** -36
    for kernel in KERNELS:
        got = ao.emulate(qkv, cu, HEADS, kernel)
        exp = ao.cls_rows(expected, cu) if kernel == 3 else expected
        assert np.array_equal(got.view(np.uint16), exp.view(np.uint16)), kernel
        ref, bnd = ao.reference_and_bound(qkv, cu, HEADS, kernel)
        fp.assert_within(exp, ref, bnd, f"onehot kernel {kernel}", ao.locator(cu, kernel))


def test_uniform_ones_are_bit_known():
    lens = list(range(1, 513))
    qkv, cu = ao.uniform_ones(lens, 1, 0)
    for kernel in KERNELS:
        got = ao.emulate(qkv, cu, 1, kernel)
        for b, n in enumerate(lens):
            rows = got[b:b + 1] if kernel == 3 else got[cu[b]:cu[b + 1]]
            e = ao.uniform_ones_expected(n, kernel)
            assert (rows == e).all(), (kernel, n, rows[0, 0], e)
            if kernel == 2 or n & (n - 1) == 0:
                assert e == np.float16(1.0)
            # the expected value does not hinge on how the reciprocal is rounded: one fp32 ulp either way gives the same fp16 p
            x = np.float32(1.0) / np.float32(n)
            assert np.float16(np.nextafter(x, np.float32(0))) == np.float16(x) == np.float16(np.nextafter(x, np.float32(2)))


# where each defect can show: (family, kernel) pairs tried in order; the one-hot family is compared under its bound like the rest
def _inputs(family):
    if family == "onehot":
        return ao.onehot(LENS, HEADS, 3)[:2]
    return ao.FAMILIES[family](LENS, HEADS, 11)


MUTATION_CASES = {
    "a_extra_key": [("uniform_indicators", 2), ("uniform_indicators", 1), ("uniform_indicators", 3)],
    "b_drop_last": [("uniform_indicators", 2), ("uniform_indicators", 1), ("uniform_indicators", 3), ("stair_up", 2)],
    "c_swap_v": [("onehot", 2), ("onehot", 1), ("realistic4", 3)],  # (kernel 3 sees one query: it needs weights spread over the keys)
    "d_skip_o_rescale": [("stair_up", 2), ("spike8", 2)],
    "e_skip_l_rescale": [("stair_up", 2), ("spike8", 2)],
    "f_patch_prev": [("uniform_indicators", 2), ("stair_up", 2)],
    "f_patch_none": [("uniform_indicators", 2), ("stair_up", 2)],
    "g_next_head_k": [("onehot", 2), ("onehot", 1), ("onehot", 3)],
    "h_first_block_q": [("onehot", 2), ("onehot", 1)],
    "i_job_shift": [("onehot", 2), ("stair_up", 2)],
}


@pytest.mark.parametrize("kernel", KERNELS)
def test_a_planted_nan_fails_the_check_of_the_gpu_test(kernel):
    """One NaN in a live row of a correct output: the comparison tests/test_attention_gpu.py applies must fail and name the element. (A
    `ratio.max() > 1.0` does not: the maximum is NaN and the comparison False.)"""
    lens = [5, 97, 33]
    qkv, cu = ao.FAMILIES["realistic1"](lens, HEADS, 11)
    ref, bnd = ao.reference_and_bound(qkv, cu, HEADS, kernel)
    got = ao.emulate(qkv, cu, HEADS, kernel)
    assert fp.assert_within(got, ref, bnd, "clean", ao.locator(cu, kernel)) <= 1.0
    row = 1 if kernel == 3 else 5 + 40
    got[row, 64 + 3] = np.nan
    assert fp.worst_ratio(got, ref, bnd) == (np.inf, (row, 67))
    with pytest.raises(AssertionError, match=r"1 element\(s\) outside the bound.*\(%d, 67\).*sequence 1, len 97, head 1.*got nan" % row):
        fp.assert_within(got, ref, bnd, "planted", ao.locator(cu, kernel))


def test_every_mutation_has_cases():
    assert sorted(MUTATION_CASES) == sorted(ao.MUTATIONS)


@pytest.mark.parametrize("mutation", ao.MUTATIONS)
def test_mutation_violates_the_bound(mutation):
    caught = []
    for family, kernel in MUTATION_CASES[mutation]:
        qkv, cu = _inputs(family)
        ref, bnd = ao.reference_and_bound(qkv, cu, HEADS, kernel)
        fp.assert_within(ao.emulate(qkv, cu, HEADS, kernel), ref, bnd, f"{family} kernel {kernel}")  # the unmutated dataflow passes the same check
        for mut_job in ((1, 2, 5) if mutation in ("d_skip_o_rescale", "e_skip_l_rescale") else (1,)):
            r = fp.worst_ratio(ao.emulate(qkv, cu, HEADS, kernel, mutation, mut_job), ref, bnd)[0]
            print(f"mutation {mutation} (job {mut_job}) on {family}, kernel {kernel}: worst |err| / bound = {r:.3g} -> {'missed' if r <= 1.0 else 'CAUGHT'}")
            caught.append(not r <= 1.0)
    assert caught[0], f"{mutation} slips through its first designed input"
    assert all(caught), f"{mutation} slips through some designed input: {caught}"
