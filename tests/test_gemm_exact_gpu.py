"""GPU (-m gpu): the encoder's forward GEMMs in isolation (mdr_test_gemm_ex, include/mdr_hip.h) against tests/gemm_ref.py, at the smallest
shapes that can break. EVERY output element is compared; nothing is averaged.

Three bars. On the grid (gemm_ref: x, w, bias and residual multiples of 1/8 of magnitude at most 2, so every fp32 sum is exact in any order)
fp32 outputs must EQUAL the integer result bit for bit and fp16 outputs its one round-to-nearest-even: every index map, K-loop prologue,
counted wait, deferred store and tile seam without a tolerance. The GELU epilogue is held to gemm_ref.gelu_bound, derived from the rounding
points listed above gelu_erf2 (csrc/mdr_encoder_gemm.inl). Realistic rows are held to gemm_ref.reference_and_bound (the accumulation term the
Linear backward's dX uses). The host suite (tests/test_gemm_host.py) shows that a second implementation stays inside the bounds and that each
deliberate defect leaves them. No tolerance here was read off a device.

Every output lives in a buffer with 64 guard rows of a finite sentinel on both sides; the guards and the rows at or behind *m_dev must keep
their bits in every call of this file (run() asserts it).

Kernels 0 (the heuristic), 1 (64x64), 2 (128x128), 4 (persistent 256x128), 6 and 7 (persistent 256x256 on eight and four waves); a forced
kernel whose condition the shape does not meet falls back; gemm_ref.flavour asks the library which kernel a call lands on (the function the
launcher itself switches on) and the tests assert it through res_added and bit-equality.
"""
import ctypes

import numpy as np
import pytest
import torch

import gemm_ref as ref
from guarded import E_INVALID, E_STATE, OK, SENTINEL, Guarded, dev
from multihop_dense_retrieval_amd._lib import ptr
from oracle import fp
from oracle.fp import bits

pytestmark = pytest.mark.gpu

GUARD = 64        # rows in front of and behind the call's own
ONE_TILE = ("small", "mid")
KERNEL_OF = {"small": 1, "mid": 2, "persist": 4, "big": 6, "quad": 7}
ALL_NK = [pytest.param(N, K, id=f"N{N}-K{K}") for N, K in ref.SMALL_NK]


def num_cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def raw_call(x, w, b, res, M, M_est, m_dev, N, K, out, epilogue, kernel, flag):
    from multihop_dense_retrieval_amd import _lib
    return _lib.lib().mdr_test_gemm_ex(ptr(x), ptr(w), ptr(b), ptr(res), M, M_est, ptr(m_dev), N, K, ptr(out), epilogue, kernel, flag, 0, _lib.current_stream_ptr())


def run_dev(tx, tw, tb, epilogue, kernel, tres=None, m=None, M_est=None):
    """One call on device tensors. -> (the whole guarded buffer [GUARD + M + GUARD, N] on the device, res_added) after asserting MDR_OK and that
    the guards and the rows at or behind m kept their bits."""
    from multihop_dense_retrieval_amd import _lib
    M, K = tx.shape
    N = tw.shape[0]
    out = Guarded(M, (N,), torch.float16 if epilogue in (0, 1) else torch.float32, GUARD, GUARD)
    m_dev = None if m is None else torch.tensor([m], dtype=torch.int32, device="cuda")
    flag = ctypes.c_int(-1)
    _lib.check(raw_call(tx, tw, tb, tres, M, M if M_est is None else M_est, m_dev, N, K, out.own, epilogue, kernel, ctypes.byref(flag)))
    torch.cuda.synchronize()
    assert flag.value in (0, 1)
    out.checked(out.buf, valid=M if m is None else m)  # (on the device: the callers bring to the host what they compare)
    return out.buf, bool(flag.value)


def run(x, w, b, epilogue, kernel, res=None, m=None, M_est=None):
    """One call on numpy inputs -> (numpy [M, N], rows at or behind m still SENTINEL; res_added)."""
    buf, added = run_dev(dev(x), dev(w), dev(b), epilogue, kernel, dev(res) if epilogue == 2 else None, m, M_est)
    return buf[GUARD:GUARD + x.shape[0]].cpu().numpy(), added


def assert_equal(got, want, label):
    assert got.dtype == want.dtype, label
    bad = np.argwhere(~(got == want))
    if bad.size:
        i = tuple(bad[0])
        pytest.fail(f"{label}: differs at {len(bad)} of {got.size} elements; first at {i}: got {float(got[i])!r}, exact {float(want[i])!r}")


def check_bound(got, r, bnd, label, worst_of=None):
    worst = fp.assert_within(got, r, bnd, label)
    if worst_of is not None:
        worst_of[0] = max(worst_of[0], worst)
    return worst


def grid_case(M, N, K, seed, positive=False):
    x, w = fp.grid((M, K), seed, dtype=np.float16), fp.grid((N, K), seed + 1, dtype=np.float16)
    if positive:  # sums of a few hundred: most values are rounded by the fp16 conversion, some from just beside a tie
        x, w = np.abs(x), np.abs(w)
    return x, w, ref.grid_bias(N, seed + 2), fp.grid((M, N), seed + 3, dtype=np.float16)


def expected_grid(x, w, b, res, epilogue, res_added):
    if epilogue == 0:
        return ref.round16(ref.exact(x, w, b))
    return ref.exact(x, w, b, res if epilogue == 2 and res_added else None).astype(np.float32)


def flavour_of(kernel, M, N, K, epilogue, M_est=None):
    return ref.flavour(kernel, M, M if M_est is None else M_est, N, K, epilogue, num_cus())


# ---- 1. the exact grid ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", ALL_NK)
@pytest.mark.parametrize("kernel", ref.KERNELS)
def test_exact_grid_equality(kernel, N, K):
    """epilogues 0, 3 and 2 over the M sweep (and once on all-positive inputs, where the fp16 conversion has to round): equality with the integer
    result; res_added as the flavour promises, the residual in the output exactly where it says so; a fallen-back selection returns the bits of
    the kernel it fell back to."""
    for M, positive in [(M, False) for M in ref.M_SWEEP] + [(300, True)]:
        x, w, b, res = grid_case(M, N, K, 3, positive)
        for epi in (0, 3, 2):
            fl = flavour_of(kernel, M, N, K, epi)
            got, added = run(x, w, b, epi, kernel, res)
            assert added == (fl in ONE_TILE), (kernel, fl, added)
            assert_equal(got, expected_grid(x, w, b, res, epi, added), f"kernel {kernel} ({fl}) M={M} N={N} K={K} epilogue {epi}")
            if kernel != 0 and fl != ref.NOMINAL[kernel]:
                other, added1 = run(x, w, b, epi, KERNEL_OF[fl], res)
                assert added1 == added and np.array_equal(bits(got), bits(other)), f"kernel {kernel} fell back to {fl} but differs from kernel {KERNEL_OF[fl]}"


def test_the_sweep_reaches_every_flavour_and_every_fallback():
    seen = {(k, flavour_of(k, 300, N, K, 0)) for k in ref.KERNELS for N, K in ref.SMALL_NK}
    for k, fl in ((1, "small"), (2, "mid"), (2, "small"), (4, "persist"), (4, "small"), (6, "big"), (6, "persist"), (6, "small"), (7, "quad"),
                  (7, "persist"), (7, "small")):
        assert (k, fl) in seen, (k, fl)
    big_short = [K for N, K in ref.SMALL_NK if flavour_of(6, 300, N, K, 0) == "big"]
    assert {64, 128, 192} <= set(big_short)  # one to three K-tiles on the 2-slot ring of the 256x256 kernel


# ---- 2. m_dev edges ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", [pytest.param(256, 256, id="N256-K256"), pytest.param(192, 64, id="N192-K64"), pytest.param(256, 64, id="N256-K64")])
@pytest.mark.parametrize("kernel", ref.KERNELS)
def test_rows_behind_m_dev_do_not_exist(kernel, N, K):
    """m in {0, 1, M - 1, M}; rows at or behind m of x and res hold NaN and +-Inf: the outputs in front of m are finite, exact, and the bits of the
    call on the first m rows alone; nothing at or behind m is written (run() asserts it), so m = 0 writes nothing."""
    M = 300
    x, w, b, res = grid_case(M, N, K, 17)
    for m in (0, 1, M - 1, M):
        xb, rb = x.copy(), res.copy()
        xb[m:], rb[m:] = np.nan, np.inf
        xb[m + 1::2], rb[m + 1::2] = -np.inf, np.nan
        for epi in (0, 1, 2, 3):
            got, added = run(xb, w, b, epi, kernel, rb, m=m)
            assert np.isfinite(got[:m]).all()
            if m == 0:
                continue
            alone, added1 = run(x[:m], w, b, epi, kernel, res[:m], M_est=M)  # (the same M_est: the same flavour for kernel 0)
            assert added1 == added and np.array_equal(bits(got[:m]), bits(alone)), (m, epi)
            if epi != 1:
                assert_equal(got[:m], expected_grid(x[:m], w, b, res[:m], epi, added), f"kernel {kernel} m={m} epilogue {epi}")


# ---- 3. M_est ------------------------------------------------------------------------------------------------------------------------------
def test_m_est_picks_the_flavour_and_never_the_result():
    """kernel 0 reads the host's ESTIMATE only: at (300, 3072, 256) the estimates 1 .. 70000 walk from a one-tile kernel through both 256x256
    kernels; every flavour returns the same bits (epilogue 2: the same z, with the residual where res_added says so)."""
    M, N, K = 300, 3072, 256
    x, w, b, res = grid_case(M, N, K, 19)
    ests = (1, 300, 4096, 70000)
    for epi in (0, 1, 2, 3):
        fls = [flavour_of(0, M, N, K, epi, e) for e in ests]
        assert fls[0] in ONE_TILE and fls[1] in ONE_TILE and len(set(fls)) >= 3 and {"big", "quad"} & set(fls), fls
        outs = []
        for e, fl in zip(ests, fls):
            got, added = run(x, w, b, epi, 0, res, M_est=e)
            assert added == (fl in ONE_TILE), (e, fl)
            if epi == 2 and added:
                got = got - res.astype(np.float32)  # exact on the grid
            outs.append(got)
        for e, o in zip(ests[1:], outs[1:]):
            assert np.array_equal(bits(o), bits(outs[0])), (epi, e)
        if epi != 1:
            assert_equal(outs[0], expected_grid(x, w, b, None, epi, False), f"M_est epilogue {epi}")


# ---- 4. several tiles per workgroup at short K -------------------------------------------------------------------------------------------
def device_grid(shape, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randint(-16, 17, shape, generator=g, device="cuda").to(torch.float32) / 8).half()


def exact_dev(tx, tw, tb):
    """the exact result on the device in float64, with gemm_ref.exact's conditions"""
    assert tx.shape[1] <= 4096 and float(tx.abs().max()) <= 2 and float(tw.abs().max()) <= 2
    z = tx.double() @ tw.double().T + tb.double()
    total = tx.abs().double() @ tw.abs().double().T + tb.abs().double()
    assert float(total.max()) * 64 <= 2.0 ** 24 and bool((z.float().double() == z).all()) and float(z.abs().max()) < fp.F16_MAX
    return z


MULTI = ([pytest.param(4, 2817, K, id=f"k4-M2817-K{K}") for K in (64, 128, 192, 256, 448)]
         + [pytest.param(6, 11009, K, id=f"k6-M11009-K{K}") for K in (64, 128, 192, 256, 384)]
         + [pytest.param(7, 11009, K, id=f"k7-M11009-K{K}") for K in (256, 384)])


@pytest.mark.parametrize("kernel,M,K", MULTI)
def test_several_tiles_per_workgroup_at_short_k(kernel, M, K):
    """The persistent kernels where a workgroup owns two tiles or more and K is shorter than the eight K-steps over which the 256x128 kernel
    spreads a tile's stores (its flush of the pending fragments), and the 256x256 kernels with complete rounds plus a 128x128 tail. Grid
    inputs made on the device, the exact result from a float64 matmul there. Epilogues 0 and 3 for equality, 1 within gelu_bound."""
    N = 3072
    fl = flavour_of(kernel, M, N, K, 0)
    assert fl == ref.NOMINAL[kernel]
    most, tail = ref.persistent_walk(kernel, M, N, K, num_cus())
    assert most >= 2, "no workgroup owns two tiles: the grid changed, choose M again"
    assert fl == "persist" or tail > 0, "the 128x128 tail is empty: choose M again"
    tx, tw = device_grid((M, K), 100 + K), device_grid((N, K), 200 + K)
    tb = device_grid((N,), 300 + K).float()
    z = exact_dev(tx, tw, tb)
    for epi in (0, 3, 1):
        buf, added = run_dev(tx, tw, tb, epi, kernel, m=M)
        got = buf[GUARD:GUARD + M]
        assert not added
        if epi == 1:
            g, bnd = ref.gelu_bound_torch(z)
            err = (got.double() - g).abs()
            err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
            ratio = torch.where(err == 0, torch.zeros_like(err), err / bnd)
            worst = float(ratio.max())
            print(f"RATIO kernel {kernel} M={M} K={K} gelu worst |err| / bound = {worst:.4f}")
            assert worst <= 1.0, (worst, int(ratio.argmax()))
        else:
            want = z.float().half() if epi == 0 else z.float()  # (z is exact in fp32: one rounding to fp16)
            bad = got != want
            assert not bool(bad.any()), f"epilogue {epi}: {int(bad.sum())} of {M * N} elements differ; first at flat index {int(bad.flatten().nonzero()[0])}"


# ---- 5. the GELU ladder --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ref.KERNELS)
def test_gelu_ladder(kernel):
    """u = a_m + bias_n over [-40, 40.25) in steps of 2^-10, and around +-1000 and +-65504: within gelu_bound of fp16(gelu64(u)), finite
    everywhere, exactly fp16(u) or +-0 from |u| = 16 on. At or below 16 the device and the emulation (which the host suite shows to be the
    unclamped chain there, bit for bit) differ only in the exponential (1 ulp of t by the ISA) and in whether u s + u / 2 is contracted:
        |device32 - emulation32| <= |u| (X1ULP Phi(-|u|) + U32) + U32 |g| = d,   |device16 - emulation16| <= d + 2 r(|g| + e32 + d)."""
    x, w, b, u = ref.ladder()
    fl = flavour_of(kernel, x.shape[0], 256, 256, 1)
    got, _ = run(x, w, b, 1, kernel)
    assert np.isfinite(got).all(), f"{int((~np.isfinite(got)).sum())} non-finite outputs, the smallest |u| among them {np.abs(u[~np.isfinite(got)]).min()!r}"
    want, bnd = ref.gelu64(u), ref.gelu_bound(u)
    worst = check_bound(got, want, bnd, f"kernel {kernel} ({fl}) ladder")
    print(f"RATIO kernel {kernel} ({fl}) GELU ladder worst |err| / bound = {worst:.4f}")
    far = np.abs(u) >= ref.CLAMP
    with np.errstate(over="ignore"):
        u16 = u.astype(np.float16)
    assert np.isfinite(u16).all()
    assert (got[far & (u > 0)] == u16[far & (u > 0)]).all() and (got[far & (u < 0)] == 0).all()
    near = ~far
    un, emu = u[near].astype(np.float64), ref.gelu32(u[near])
    g = np.abs(ref.gelu64(un))
    d = np.abs(un) * (fp.X1ULP * 0.5 * torch.special.erfc(torch.from_numpy(np.abs(un) / np.sqrt(2.0))).numpy() + fp.U32) + fp.U32 * g
    tol = d + 2 * fp.r16(g + ref.gelu_err32(un) + d)
    diff = np.abs(got[near].astype(np.float64) - emu.astype(np.float16).astype(np.float64))
    print(f"kernel {kernel}: {int((diff != 0).sum())} of {diff.size} outputs at |u| <= 16 differ from the emulation's fp16, worst |diff| / tolerance {float((diff / tol).max()):.4f}")
    assert (diff <= tol).all()


# ---- 6. GELU on the grid -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", ALL_NK)
@pytest.mark.parametrize("kernel", ref.KERNELS)
def test_gelu_on_the_grid(kernel, N, K):
    """u is exact, and a share of it lies beyond |u| = 24 (3 % at K = 64, 29 % at K = 256), where the unclamped polynomial returned 1e21 and inf."""
    worst = [0.0]
    for M in (1, 17, 129, 300):
        x, w, b, _ = grid_case(M, N, K, 3)
        u = ref.exact(x, w, b)
        got, _ = run(x, w, b, 1, kernel)
        check_bound(got, ref.gelu64(u), ref.gelu_bound(u), f"kernel {kernel} M={M} N={N} K={K} grid gelu", worst)
        far = np.abs(u) >= ref.CLAMP
        assert (got[far & (u > 0)] == u[far & (u > 0)].astype(np.float16)).all() and (got[far & (u < 0)] == 0).all()
    print(f"RATIO kernel {kernel} N={N} K={K} grid GELU worst |err| / bound = {worst[0]:.4f}")


# ---- 7. realistic rows ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", ALL_NK)
def test_realistic_rows_within_the_derived_bound(N, K):
    """All four epilogues on every flavour: inside the derived bound, the same bits from every flavour (epilogue 2 without the residual: the bits of
    epilogue 3) and from a second run."""
    for M in (129, 300):
        x, w, _ = ref.realistic(M, N, K, 11)
        b, res = ref.bias(N, 11), ref.realistic(M, 64, N, 12)[0]
        for epi in (0, 1, 2, 3):
            first = {}
            worst = [0.0]
            for kernel in ref.KERNELS:
                got, added = run(x, w, b, epi, kernel, res)
                r, bnd = ref.reference_and_bound(x, w, b, epi, res, added)
                check_bound(got, r, bnd, f"kernel {kernel} M={M} N={N} K={K} epilogue {epi}", worst)
                cls = added if epi == 2 else True  # (only epilogue 2 has two classes of results)
                if cls not in first:
                    first[cls] = got
                    again, _ = run(x, w, b, epi, kernel, res)
                    assert np.array_equal(bits(got), bits(again)), "two runs differ"
                assert np.array_equal(bits(got), bits(first[cls])), f"kernel {kernel} returns other bits than the kernels before it"
            if epi == 2 and False in first:
                plain, _ = run(x, w, b, 3, 1)
                assert np.array_equal(bits(first[False]), bits(plain))
            print(f"RATIO realistic M={M} N={N} K={K} epilogue {epi} worst |err| / bound = {worst[0]:.4f}")


# ---- 8. NaN locality -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ref.KERNELS)
def test_nan_reaches_only_its_row_or_column(kernel):
    M, N, K = 150, 256, 256
    x, w, b, _ = grid_case(M, N, K, 23)
    for epi in (0, 1, 3):
        clean, _ = run(x, w, b, epi, kernel)
        xb = x.copy()
        xb[70, 5] = np.nan
        got, _ = run(xb, w, b, epi, kernel)
        rows = np.arange(M) != 70
        assert np.isnan(got[70]).all() and np.array_equal(bits(got[rows]), bits(clean[rows])), epi
        wb = w.copy()
        wb[9, 3] = np.nan
        got, _ = run(x, wb, b, epi, kernel)
        cols = np.arange(N) != 9
        assert np.isnan(got[:, 9]).all() and np.array_equal(bits(got[:, cols]), bits(clean[:, cols])), epi


# ---- 9. host validation --------------------------------------------------------------------------------------------------------------------
def test_host_validation_writes_nothing():
    from multihop_dense_retrieval_amd import _lib
    lib = _lib.lib()
    M, N, K = 70, 256, 128
    x, w, b, res = (dev(a) for a in grid_case(M, N, K, 37))
    out = torch.full((M, N), SENTINEL, dtype=torch.float32, device="cuda")
    flag = ctypes.c_int(-1)
    cases = [
        ("NULL A", E_INVALID, dict(x=None)), ("NULL W", E_INVALID, dict(w=None)), ("NULL bias", E_INVALID, dict(b=None)), ("NULL out", E_INVALID, dict(out=None)),
        ("M = 0", E_INVALID, dict(M=0)), ("M < 0", E_INVALID, dict(M=-3)), ("N = 0", E_INVALID, dict(N=0)), ("N = 96", E_INVALID, dict(N=96)),
        ("N < 0", E_INVALID, dict(N=-64)), ("K = 0", E_INVALID, dict(K=0)), ("K = 100", E_INVALID, dict(K=100)), ("K < 0", E_INVALID, dict(K=-64)),
        ("epilogue -1", E_INVALID, dict(epilogue=-1)), ("epilogue 4", E_INVALID, dict(epilogue=4)), ("kernel -1", E_INVALID, dict(kernel=-1)),
        ("kernel 3", E_INVALID, dict(kernel=3)), ("kernel 5", E_INVALID, dict(kernel=5)), ("kernel 8", E_INVALID, dict(kernel=8)),
        ("epilogue 2 without res", E_INVALID, dict(epilogue=2)), ("res with epilogue 0", E_INVALID, dict(res=res)),
        ("res with epilogue 3", E_INVALID, dict(res=res, epilogue=3)), ("M_est = 0", E_INVALID, dict(M_est=0)), ("M_est < 0", E_INVALID, dict(M_est=-5)),
        # the persistent kernels leave the residual to the caller, who has to be able to hear that
        ("epilogue 2, persistent, nobody to tell", E_STATE, dict(res=res, epilogue=2, kernel=4, flag=None)),
        ("epilogue 2, 256x256, nobody to tell", E_STATE, dict(res=res, epilogue=2, kernel=6, flag=None)),
    ]
    for label, code, change in cases:
        a = dict(x=x, w=w, b=b, res=None, M=M, M_est=M, m_dev=None, N=N, K=K, out=out, epilogue=0, kernel=1, flag=ctypes.byref(flag))
        a.update(change)
        rc = raw_call(**a)
        assert rc == code, (label, rc)
        assert lib.mdr_last_error(), label
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()), "a rejected call wrote something"
    # and the same call with somebody to tell, or on a one-tile kernel without, is fine
    assert raw_call(x, w, b, res, M, M, None, N, K, out, 2, 4, ctypes.byref(flag)) == OK and flag.value == 0
    assert raw_call(x, w, b, res, M, M, None, N, K, out, 2, 1, None) == OK
    torch.cuda.synchronize()
