"""CPU: the reference of the forward GEMM suite (tests/gemm_ref.py) checked against itself. The fp32 chain of gelu_erf2 against the fp64 GELU
within the derived bound over every finite fp16 value and a dense fp32 sweep; each GELU mutation thrown out, the unclamped polynomial (the
code before the clamp) exactly where it goes wrong; a second implementation of the GEMM's dataflow inside the realistic-rows bound and equal to
the exact grid result, each deliberate defect thrown out by the grid comparison; the launcher's kernel choice (mdr_test_gemm_choice, host
integers only) pinned on a table of literals. No device and no kernel runs here."""
import ctypes

import numpy as np
import pytest
import torch

import gemm_ref as ref
from guarded import E_INVALID, OK
from oracle import fp


def gelu_inputs():
    h = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16)
    h = h[np.isfinite(h)].astype(np.float32)
    assert h.size == 63488
    sweep = np.linspace(-40.0, 40.0, 1_600_001).astype(np.float32)  # steps of 5e-5
    return np.concatenate([h, sweep])


@pytest.fixture(scope="module")
def gelu_points():
    u = gelu_inputs()
    return u, ref.gelu64(u), ref.gelu_bound(u)


def test_gelu32_within_the_bound_of_gelu64(gelu_points):
    u, want, bnd = gelu_points
    got = ref.gelu32(u)
    assert np.isfinite(got).all()
    got16 = got.astype(np.float16).astype(np.float64)
    err = np.abs(got16 - want)
    i = int(np.argmax(err / bnd))
    print(f"RATIO gelu32 worst |err| / bound = {err[i] / bnd[i]:.4f} at u = {float(u[i])!r}; largest fp32 |err| {np.abs(got - want)[np.abs(u) <= 8].max():.3e} on [-8, 8]")
    assert (err <= bnd).all(), (float(u[i]), got16[i], want[i], bnd[i])
    # the fp32 value alone against the fp32 part of the bound
    assert (np.abs(got.astype(np.float64) - want) <= ref.gelu_err32(u)).all()
    # from the clamp on: exactly u on the right, exactly zero on the left
    far = np.abs(u) >= ref.CLAMP
    assert (got[far & (u > 0)] == u[far & (u > 0)]).all() and (got[far & (u < 0)] == 0).all()
    assert ref.gelu32(np.zeros(1, np.float32))[0] == 0


def test_the_clamp_changes_no_bit_at_or_below_16(gelu_points):
    u = gelu_points[0]
    near = np.abs(u) <= ref.CLAMP
    a, b = ref.gelu32(u[near]), ref.gelu32(u[near], "no_clamp")
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("mutation", ref.GELU_MUTATIONS)
def test_each_gelu_mutation_leaves_the_bound(gelu_points, mutation):
    u, want, bnd = gelu_points
    with np.errstate(over="ignore"):
        got16 = ref.gelu32(u, mutation).astype(np.float16).astype(np.float64)
    err = np.abs(got16 - want)
    bad = ~(err <= bnd)  # (a NaN is bad)
    assert bad.any(), mutation
    print(f"mutation {mutation}: {int(bad.sum())} of {u.size} points outside the bound, the smallest |u| among them {float(np.abs(u[bad]).min())!r}")
    if mutation == "no_clamp":
        # the record of the defect: the polynomial turns around beyond its fit -- every |u| >= 24 is wrong (non-finite from 25 on), nothing at or below 16 is
        assert bad[np.abs(u) >= 24].all()
        assert not bad[np.abs(u) <= ref.CLAMP].any()
        assert float(np.abs(u[bad]).min()) > 23.0
        g24 = ref.gelu32(np.array([24.0, -24.0, 25.0, -25.0], np.float32), "no_clamp")
        assert abs(g24[0]) > 1e20 and not np.isfinite(g24[2:].astype(np.float16)).any()


def test_torch_bound_is_the_numpy_bound():
    u = np.concatenate([np.linspace(-40, 40, 4001), [1000.0, -1000.0, 0.0]])
    g, bnd = ref.gelu_bound_torch(torch.from_numpy(u))
    assert np.allclose(g.numpy(), ref.gelu64(u), rtol=1e-12, atol=0) and np.allclose(bnd.numpy(), ref.gelu_bound(u), rtol=1e-12, atol=0)


def grid_case(M, N, K, seed):
    return fp.grid((M, K), seed, dtype=np.float16), fp.grid((N, K), seed + 1, dtype=np.float16), ref.grid_bias(N, seed + 2), fp.grid((M, N), seed + 3, dtype=np.float16)


def expected_grid(x, w, b, res, epilogue, res_added=True):
    if epilogue == 0:
        return ref.round16(ref.exact(x, w, b))
    if epilogue == 2:
        return ref.exact(x, w, b, res if res_added else None).astype(np.float32)
    return ref.exact(x, w, b).astype(np.float32)


@pytest.mark.parametrize("N,K", ref.SMALL_NK)
def test_emulation_equals_the_grid_and_stays_inside_the_bound(N, K):
    for M in (129, 300):
        x, w, b, res = grid_case(M, N, K, 3)
        for epi in (0, 2, 3):
            for added in ((True, False) if epi == 2 else (True,)):
                got = ref.emulate(x, w, b, epi, res, added)
                want = expected_grid(x, w, b, res, epi, added)
                assert got.dtype == want.dtype and np.array_equal(got, want), (M, epi, added)
        u = ref.exact(x, w, b)
        worst, at = fp.worst_ratio(ref.emulate(x, w, b, 1), ref.gelu64(u), ref.gelu_bound(u))
        assert worst <= 1.0, ("grid gelu", M, worst, at)
        x, w, _ = ref.realistic(M, N, K, 11)
        b, res = ref.bias(N, 11), ref.realistic(M, 64, N, 12)[0]
        for epi in (0, 1, 2, 3):
            for added in ((True, False) if epi == 2 else (True,)):
                r, bnd = ref.reference_and_bound(x, w, b, epi, res, added)
                worst, at = fp.worst_ratio(ref.emulate(x, w, b, epi, res, added), r, bnd)
                assert worst <= 1.0, ("realistic", M, epi, added, worst, at)


def test_the_grid_reaches_the_gelu_cliff():
    """the share of grid pre-activations beyond |u| = 24, where the unclamped polynomial was wrong: what makes the grid GELU test of the GPU suite
    fail on the code before the clamp"""
    for (N, K), least in (((256, 64), 0.01), ((256, 256), 0.2)):
        x, w, b, _ = grid_case(300, N, K, 3)
        share = float((np.abs(ref.exact(x, w, b)) >= 24).mean())
        print(f"N={N} K={K}: {share:.3f} of the grid pre-activations at |u| >= 24")
        assert share >= least


@pytest.mark.parametrize("mutation", ref.GEMM_MUTATIONS)
def test_each_gemm_defect_is_thrown_out_by_the_grid(mutation):
    M, N, K = 129, 256, 256
    x, w, b, res = grid_case(M, N, K, 3)
    x, w = np.abs(x), np.abs(w)  # sums of a few hundred, where an fp16 ulp is 16 quanta of the grid: most values round, some from just beside a tie
    thrown = []
    for epi in (0, 3):
        got, want = ref.emulate(x, w, b, epi, res, mutation=mutation), expected_grid(x, w, b, res, epi)
        assert np.array_equal(ref.emulate(x, w, b, epi, res), want)
        thrown.append(not np.array_equal(got, want))
        print(f"defect {mutation} epilogue {epi}: {int((got != want).sum())} of {got.size} elements differ")
    assert thrown[0], mutation                                  # every defect shows in the fp16 output
    assert thrown[1] or mutation == "double_round16"             # and all but the fp16 rounding in the fp32 output


def test_exact_refuses_inputs_off_the_grid():
    x, w, b, _ = grid_case(17, 64, 64, 3)
    with pytest.raises(AssertionError):
        ref.exact((x.astype(np.float32) / 3).astype(np.float16), w, b)
    with pytest.raises(AssertionError):
        ref.exact(x, w, b + np.float32(1e-3))
    with pytest.raises(AssertionError):
        ref.round16(np.array([70000.0]))


def test_flavour_mirror_on_the_documented_cases():
    """forced selections and their fall-backs, and the three classes the M_est test of the GPU suite relies on (256 compute units): the answers
    of the function launch_gemm switches on (gemm_ref.flavour -> mdr_test_gemm_choice)"""
    f = ref.flavour
    assert [f(k, 300, 300, 256, 256, 0, 256) for k in (1, 2, 4, 6, 7)] == ["small", "mid", "persist", "big", "quad"]
    assert f(2, 300, 300, 192, 64, 0, 256) == "small" and f(2, 300, 300, 64, 64, 0, 256) == "small"   # no multiple of 128: 64x64 tiles
    assert f(4, 300, 300, 192, 64, 0, 256) == "small" and f(6, 300, 300, 128, 128, 0, 256) == "persist"
    assert f(7, 300, 300, 256, 64, 0, 256) == "persist" and f(7, 300, 300, 256, 192, 0, 256) == "persist" and f(7, 300, 300, 256, 384, 0, 256) == "quad"
    got = [f(0, 300, est, 3072, 256, 0, 256) for est in (1, 300, 4096, 70000)]
    assert got[0] in ("small", "mid") and got[1] in ("small", "mid") and {"quad", "big"} <= set(got[2:]), got


# (kernel, M_cap, M_est, N, K, epilogue, num_cus) -> kernel id: 1 = 64x64, 2 = 128x128, 4 = persistent 256x128, 6 / 7 = 256x256 on eight / four waves.
# One row per branch of gemm_choose (csrc/mdr_gemm_choice.h); the values are those of the Python mirror the GPU suite used before the hook existed.
CHOICES = [
    ((0, 300, 300, 768, 768, 0, 256), 1),             # few tiles, small wins the byte count
    ((0, 2400, 2400, 2304, 768, 0, 256), 2),          # few tiles, mid wins
    ((0, 2400, 2400, 768, 3072, 0, 256), 1),
    ((0, 30720, 20480, 2304, 768, 0, 256), 6),        # QKV at bench size: big
    ((0, 30720, 20480, 768, 768, 3, 256), 7),         # out-projection: quad (one round)
    ((0, 30720, 20480, 3072, 768, 1, 256), 6),        # FFN1
    ((0, 30720, 20480, 768, 3072, 3, 256), 7),        # FFN2 (K >= 2048)
    ((0, 30720, 20480, 768, 3072, 2, 256), 7),        # epilogue 2 decides as 3
    ((0, 65536, 43691, 1024, 1024, 0, 256), 6),
    ((0, 65536, 43691, 4096, 1024, 1, 256), 2),       # N above the bias slot: one-tile whatever M
    ((0, 65536, 43691, 1024, 4096, 3, 256), 7),
    ((0, 30720, 20480, 384, 768, 0, 256), 2),         # too few persistent tiles
    ((0, 30720, 20480, 1920, 768, 0, 256), 4),        # N % 256 != 0
    ((0, 30720, 20480, 768, 192, 0, 256), 6),         # K % 128 != 0: no quad
    ((0, 30720, 20480, 768, 320, 0, 256), 6),
    ((0, 1500000, 1000000, 768, 768, 3, 256), 4),     # fp32 output of 4 GiB and more: no 32-bit store offsets
    ((0, 1500000, 1000000, 768, 768, 0, 256), 6),     # the fp16 output still fits
    ((0, 700000, 700000, 256, 3072, 0, 256), 6),      # A of 4 GiB and more: no quad
    ((0, 22016, 22016, 768, 768, 0, 256), 7),         # 86 row tiles (the 258-tile step)
    ((0, 11009, 11009, 3072, 256, 0, 256), 6),
    ((0, 300, 4096, 3072, 256, 0, 256), 7),           # M_est alone decides ...
    ((0, 300, 70000, 3072, 256, 0, 256), 6),          # ... both ways
    ((0, 30720, 20480, 2304, 768, 0, 304), 6),        # another CU count
    ((0, 30720, 20480, 768, 3072, 3, 304), 7),
    ((0, 30720, 20480, 768, 768, 0, 64), 6),
    ((0, 2400, 2400, 2304, 768, 0, 64), 6),
    ((7, 300, 300, 256, 128, 0, 256), 4),             # forced 7, K < 256
    ((7, 300, 300, 512, 256, 0, 256), 7),
    ((6, 300, 300, 384, 64, 0, 256), 4),              # forced 6, N % 256 != 0
    ((4, 300, 300, 3200, 64, 0, 256), 1),             # forced 4, N above the bias slot
    ((2, 300, 300, 320, 64, 0, 256), 1),              # forced 2, N % 128 != 0
    ((7, 9000000, 300, 256, 256, 0, 256), 4),         # forced 7 / 6 past the 32-bit guards
    ((6, 9000000, 300, 256, 256, 3, 256), 4),
    ((6, 9000000, 300, 256, 256, 0, 256), 4),
]


def test_the_kernel_choice_on_one_case_per_branch():
    for args, kernel in CHOICES:
        got, res_added, _ = ref.choice(*args)
        assert got == kernel and res_added == (kernel in (1, 2)), (args, kernel, got, res_added)


def raw_choice(*args):
    from multihop_dense_retrieval_amd import _lib
    return _lib.lib().mdr_test_gemm_choice(*args)


def test_the_choice_hook_refuses_bad_arguments():
    good = dict(kernel=0, M=300, M_est=300, N=256, K=256, epilogue=0, num_cus=256)
    assert raw_choice(*good.values(), None, None, None) == OK
    for change in (dict(kernel=3), dict(kernel=8), dict(epilogue=4), dict(M_est=0), dict(N=96), dict(num_cus=0)):
        out = ctypes.c_int(-7)
        assert raw_choice(*{**good, **change}.values(), ctypes.byref(out), None, None) == E_INVALID, change
        assert out.value == -7, change


def test_every_out_pointer_of_the_choice_hook_may_be_null():
    args = (6, 22016, 22016, 768, 768, 0, 256)
    want = ref.choice(*args)
    assert want == (6, False, 85)
    assert raw_choice(*args, None, None, None) == OK
    for i in range(3):
        outs = [ctypes.c_int(-7) for _ in range(3)]
        assert raw_choice(*args, *[ctypes.byref(o) if j == i else None for j, o in enumerate(outs)]) == OK
        assert [o.value for o in outs] == [int(want[j]) if j == i else -7 for j in range(3)]


def test_walk_row_tiles():
    """86 row tiles x 3 column tiles of 256 = 258 tiles on 256 workgroups: the one complete round is 85 row tiles, the 86th goes to the 128x128 tail;
    the 256x128 kernel walks all 86; the one-tile kernels walk none."""
    assert [ref.choice(k, 22016, 22016, 768, 768, 0, 256) for k in (6, 7, 4, 1)] == [(6, False, 85), (7, False, 85), (4, False, 86), (1, True, 0)]
