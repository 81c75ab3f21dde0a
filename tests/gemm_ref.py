"""Host restatement of ONE forward GEMM call of the encoder (mdr_test_gemm_ex, include/mdr_hip.h): the exact result on a grid of inputs, the
erf-GELU in fp64 and as the fp32 chain of gelu_erf2 (csrc/mdr_encoder_gemm.inl) with switchable mutations, derived error bounds, a second
implementation of the GEMM's dataflow with switchable defects, and the host's kernel choice as the library reports it (mdr_test_gemm_choice: the
function the launcher switches on, not a copy of it). numpy (erfc in float64 through torch's CPU kernel); nothing here is measured from a kernel. Test helper (tests/test_gemm_host.py, tests/test_gemm_exact_gpu.py).

Layout: x float16 [M, K], w float16 [N, K], b float32 [N], res None or float16 [M, N].
Epilogues: 0 = fp16(z), 1 = fp16(gelu(z)), 2 = z + res in fp32 (the persistent kernels leave the residual out and say so), 3 = z in fp32,
z = x w^T + b accumulated in fp32.

The grid
--------
x, w multiples of 1/8 of magnitude at most 2 (oracle/fp.py, grid), b and res multiples of 1/8 of magnitude at most 2: every product is a
multiple of 1/64 of magnitude at most 4, so any fp32 sum of K <= 4096 of them plus the bias and the residual is a whole number of 1/64 that
stays below 2^24 of them: exact in any order. exact() asserts that condition. fp32 outputs must EQUAL it, fp16 outputs its one
round-to-nearest-even.

The GELU bound
--------------
From the rounding points listed above gelu_erf2, for an EXACT fp32 u, g = u Phi(u), a = min(|u|, 16):
  2. t = Phi(-a): PHI_ERR = 2.1e-7 (the file's stated maximum for the fp32 chain; the host test re-checks it over every finite fp16 u and a
     dense fp32 sweep), + 2^-23 t <= 2^-24 for the 1-ulp v_exp_f32 of the ISA (t <= 1/2).
  3. s = 1/2 - t: 2^-25 (half an ulp of a value below 1/2).
  4. u s: 2^-25 |u| (half an ulp of a value of magnitude at most |u| / 2) where it is not contracted; the sum: 2^-24 |g'|, g' the computed value.
  So the error of s is at most PHI_ERR + 2^-24 + 2^-25, multiplied by |u|; with the product's 2^-25 |u| that is |u| (PHI_ERR + 2^-23); the last
  add loses half an ulp of the result, counted twice to cover |g'| instead of |g|:
      e32 = |u| (PHI_ERR + X1ULP) + 2 U32 |g|.
  For a > 16 the clamp replaces Phi(-a) by Phi(-16) < 1e-57: covered by PHI_ERR.
  5. the fp16 rounding r(y) = max(H16 y, Z16) of a value of magnitude at most y (oracle/fp.py, r16):
      gelu_bound = e32 + r(|g| + e32).
When u itself carries an error du (realistic rows), |gelu'| <= 1.13 turns it into 1.13 du and the terms above are taken at |u| + du.

The realistic-rows bound
------------------------
z: K products (exact in fp32) added in some order, at most one ulp lost per addition: linear_grad_ref.gemm_accum_bound, the term the
backward's dX uses (the same GEMM); then the fp32 add of the bias and, for epilogue 2, of the residual: half an ulp of the computed sum each.
      ez = K X1ULP (|x| |w|^T) + U32 (|z| + ez) [+ U32 (|z + res| + ez)]
fp32 outputs: ez. Epilogue 0: ez + r(|z| + ez). Epilogue 1: as above with du = ez.
"""
import ctypes

import numpy as np
import torch

import linear_grad_ref as lref
from linear_grad_ref import PHI_ERR, bias, realistic  # noqa: F401
from oracle.fp import F16_MAX, H16, U32, X1ULP, Z16, exp2_32, fma32, r16

GELU_MUTATIONS = ("no_clamp", "no_half_x", "sign_lost")
GEMM_MUTATIONS = ("drop_k_tile", "row_off_by_one", "neighbour_bias", "double_round16")
GELU_SLOPE = 1.13   # max |gelu'| = 1.1289 at u = sqrt 2 ... (Phi(u) + u phi(u) peaks at u^2 = 2)
CLAMP = 16.0

KERNELS = (0, 1, 2, 4, 6, 7)
SMALL_NK = [(64, 64), (192, 64), (128, 128), (256, 64), (256, 128), (256, 192), (256, 256), (256, 384), (512, 256)]
M_SWEEP = [1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300]   # -1, 0, +1 around an MFMA tile and the 64-, 128- and 256-row tiles


# ---- makers --------------------------------------------------------------------------------------------------------------------------------
def grid_bias(N, seed):
    """float32: seeded multiples of 1/8 in [-2, 2]."""
    return (np.random.default_rng([seed, N, 11]).integers(-16, 17, size=N) / 8.0).astype(np.float32)


def ladder():
    """(x float16 [M, 256], w float16 [256, 256], b float32 [256], u float32 [M, 256]) of the GELU ladder: x[m, 0] = a_m, w[n, 0] = 1, everything
    else zero, so the accumulator of (m, n) is a_m exactly and u = fp32(a_m + b_n) by the epilogue's one add (exact except in the +-65504 rows).
    a: the multiples of 1/4 over [-40, 40], +-1000, +-65504; b: the 256 multiples of 2^-10 in [0, 1/4), shuffled."""
    a = np.concatenate([np.arange(-160, 161) / 4.0, [1000.0, -1000.0, 65504.0, -65504.0]])
    rng = np.random.default_rng(5)
    order = rng.permutation(a.size)
    a = a[order]
    M, N, K = a.size, 256, 256
    x, w = np.zeros((M, K), np.float16), np.zeros((N, K), np.float16)
    x[:, 0], w[:, 0] = a, 1.0
    b = (rng.permutation(256) * 2.0 ** -10).astype(np.float32)
    assert (x[:, 0].astype(np.float64) == a).all() and b.max() < 0.25
    u = x[:, :1].astype(np.float32) + b[None, :]
    return x, w, b, u


# ---- the exact result on the grid ----------------------------------------------------------------------------------------------------------
def exact(x, w, b, res=None):
    """float64 [M, N]: x w^T + b (+ res), after asserting that every fp32 partial sum in any order is exact (see the module docstring)."""
    X, W, B = x.astype(np.float64), w.astype(np.float64), np.asarray(b, np.float64)
    R = None if res is None else res.astype(np.float64)
    q = 1.0 / 64
    for a in (X, W):
        assert (a * 8 == np.round(a * 8)).all() and np.abs(a).max(initial=0) <= 2, "x and w must be multiples of 1/8 of magnitude at most 2"
    for a in (B,) + (() if R is None else (R,)):
        assert (a / q == np.round(a / q)).all(), "bias and residual must be multiples of 1/64"
    total = np.abs(X) @ np.abs(W).T + np.abs(B)[None, :] + (0 if R is None else np.abs(R))
    assert x.shape[1] <= 4096 and (total.size == 0 or total.max() / q <= 2.0 ** 24), "the grid no longer guarantees exact fp32 sums"
    z = X @ W.T + B[None, :]
    if R is not None:
        z = z + R
    assert (z.astype(np.float32) == z).all()
    return z


def round16(z):
    """the one round-to-nearest-even of float64 values to float16, asserting that none leaves the fp16 range"""
    assert z.size == 0 or np.abs(z).max() < F16_MAX, "an exact value leaves the fp16 range"
    return z.astype(np.float16)


# ---- GELU ----------------------------------------------------------------------------------------------------------------------------------
def gelu64(u):
    """u Phi(u) in float64, Phi through erfc so that the negative tail keeps its relative accuracy."""
    u = np.asarray(u, np.float64)
    return u * 0.5 * torch.special.erfc(torch.from_numpy(np.ascontiguousarray(-u / np.sqrt(2.0)))).numpy()


def gelu32(u, mutation=None):
    """gelu_erf2 on fp32 u, one rounding per FMA, exp2 in fp32, u s and the last sum rounded separately. mutation (None: the kernel's formula):
    no_clamp = the polynomial at |u| instead of min(|u|, 16) (the code before the clamp); no_half_x = the + u / 2 dropped; sign_lost = 1/2 - t
    without the sign of u."""
    assert mutation is None or mutation in GELU_MUTATIONS
    f32 = np.float32
    u = np.asarray(u, f32)
    a = np.abs(u) if mutation == "no_clamp" else np.minimum(np.abs(u), f32(CLAMP))
    with np.errstate(over="ignore", invalid="ignore"):
        p = fma32(a, -1.982813420e-05, 6.620948925e-04)
        for c in (-7.759194708e-03, 5.296392132e-02, 4.590664427e-01, 1.151119066e+00):
            p = fma32(p, a, c)
        e = fma32(p, a, 1.0)
        t = exp2_32(-e)
        s = f32(0.5) - t
        if mutation != "sign_lost":
            s = np.copysign(s, u)
        if mutation == "no_half_x":
            return (u * s).astype(f32)
        return (u * s).astype(f32) + f32(0.5) * u  # the product and the sum round separately (the packed multiply and add of the kernel)


def gelu_err32(u, du=0.0):
    """e32 of the docstring (float64): the absolute error of the device's fp32 GELU value, u known to within du."""
    u = np.asarray(u, np.float64)
    au = np.abs(u) + du
    return GELU_SLOPE * du + au * (PHI_ERR + X1ULP) + 2 * U32 * (np.abs(gelu64(u)) + GELU_SLOPE * du)


def gelu_bound(u, du=0.0):
    """the absolute error allowed for the fp16 GELU output"""
    e = gelu_err32(u, du)
    return e + r16(np.abs(gelu64(u)) + e)


def gelu_bound_torch(u):
    """gelu_bound(u) (du = 0) and gelu64(u) on torch float64 tensors, for outputs too large to bring to the host: -> (reference, bound)"""
    u = u.double()
    g = u * 0.5 * torch.special.erfc(-u / np.sqrt(2.0))
    e = u.abs() * (PHI_ERR + X1ULP) + 2 * U32 * g.abs()
    return g, e + torch.clamp(H16 * (g.abs() + e), min=Z16)


# ---- realistic rows ------------------------------------------------------------------------------------------------------------------------
def reference_and_bound(x, w, b, epilogue, res=None, res_added=True):
    """(reference, bound) float64 [M, N] of one call on realistic rows; asserts that nothing leaves the fp16 range."""
    X, W = x.astype(np.float64), w.astype(np.float64)
    z = X @ W.T + np.asarray(b, np.float64)[None, :]
    ez = lref.gemm_accum_bound(np.abs(X), np.abs(W).T, x.shape[1])
    ez = ez + U32 * (np.abs(z) + ez)
    if epilogue == 2:
        if res_added:
            z = z + res.astype(np.float64)
            ez = ez + U32 * (np.abs(z) + ez)
        return z, ez
    if epilogue == 3:
        return z, ez
    if epilogue == 0:
        assert float((np.abs(z) + ez).max(initial=0)) < F16_MAX
        return z, ez + r16(np.abs(z) + ez)
    assert float((np.abs(z) + ez).max(initial=0)) < F16_MAX
    return gelu64(z), gelu_bound(z, ez)


def emulate(x, w, b, epilogue, res=None, res_added=True, mutation=None):
    """A second implementation of the kernels' dataflow: K in tiles of 64, each as two MFMA steps of 32, accumulated in fp32; the bias added in
    fp32; then the epilogue. float16 or float32 [M, N].

    mutation switches ONE defect on: drop_k_tile = the last K-tile never added; row_off_by_one = output row m computed from x row m + 1 (the last
    from itself); neighbour_bias = the bias of column n + 1 (the last: of column n - 1); double_round16 = fp16 outputs rounded to 12 significant
    bits first and to fp16 after."""
    assert mutation is None or mutation in GEMM_MUTATIONS
    f32 = np.float32
    M, K = x.shape
    xf, wf = x.astype(f32), w.astype(f32)
    if mutation == "row_off_by_one":
        xf = np.concatenate([xf[1:], xf[-1:]])
    acc = np.zeros((M, w.shape[0]), f32)
    k_end = K - 64 if mutation == "drop_k_tile" else K
    for k in range(0, k_end, 32):
        acc = acc + xf[:, k:k + 32] @ wf[:, k:k + 32].T
    bb = np.asarray(b, f32)
    if mutation == "neighbour_bias":
        bb = np.concatenate([bb[1:], bb[-2:-1]])
    v = acc + bb[None, :]
    if epilogue == 1:
        v = gelu32(v)
    if epilogue == 2 and res_added:
        v = v + res.astype(f32)
    if epilogue in (2, 3):
        return v
    if mutation == "double_round16":
        with np.errstate(divide="ignore"):
            ex = np.floor(np.log2(np.maximum(np.abs(v.astype(np.float64)), 2.0 ** -14)))
        step = 2.0 ** (ex - 11)   # half an fp16 ulp
        v = (np.round(v.astype(np.float64) / step) * step).astype(f32)
    return v.astype(np.float16)


# ---- the host's kernel choice: asked of the library (mdr_test_gemm_choice, include/mdr_hip.h), which answers without a device ---------------
NOMINAL = {1: "small", 2: "mid", 4: "persist", 6: "big", 7: "quad"}


def choice(kernel, M_cap, M_est, N, K, epilogue, num_cus):
    """(kernel id, res_added, row tiles of 256 of the persistent walk at M_est valid rows) of gemm_choose (csrc/mdr_gemm_choice.h), the function
    launch_gemm switches on, for the call mdr_test_gemm_ex(kernel, M = M_cap, M_est, N, K, epilogue) on num_cus compute units."""
    from multihop_dense_retrieval_amd import _lib
    out = [ctypes.c_int(-1) for _ in range(3)]
    _lib.check(_lib.lib().mdr_test_gemm_choice(kernel, M_cap, M_est, N, K, epilogue, num_cus, *[ctypes.byref(o) for o in out]))
    return out[0].value, bool(out[1].value), out[2].value


def flavour(kernel, M_cap, M_est, N, K, epilogue, num_cus):
    """The kernel a forced selection (the hooks never read the environment) lands on: "small" (64x64), "mid" (128x128), "persist" (256x128),
    "big" (256x256, eight waves) or "quad" (256x256, four waves). The one-tile kernels add the residual of epilogue 2, the others do not."""
    return NOMINAL[choice(kernel, M_cap, M_est, N, K, epilogue, num_cus)[0]]


def persistent_walk(kernel, M, N, K, num_cus):
    """(most tiles one workgroup owns, tail tiles) of the persistent kernel a selection lands on at M valid rows: the XCD split of
    gemm_persist_kernel / gemm_big_kernel / gemm_quad_kernel (XCD x owns tiles [T x / 8, T (x + 1) / 8) and walks them round-robin over its
    num_cus / 8 workgroups), over the row tiles the host counts; the 256x256 kernels finish the rows behind them on 128x128 tail tiles."""
    kid, _, ntm = choice(kernel, M, M, N, K, 0, num_cus)
    assert kid in (4, 6, 7), kid
    G = num_cus // 8
    ntn = N // 128 if kid == 4 else N // 256
    tail = ((max(0, M - ntm * 256) + 127) // 128) * (N // 128)
    T = ntm * ntn
    most = max((T * (x + 1) // 8 - T * x // 8 + G - 1) // G for x in range(8))
    return most, tail
