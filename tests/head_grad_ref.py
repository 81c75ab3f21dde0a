"""Host restatement of ONE head-Linear backward call (mdr_head_backward, include/mdr_head_grad.h): the three formulas in fp64, a derived
elementwise error bound, an fp32 replica of the kernels' dataflow and makers for the inputs. numpy only; nothing here is measured from a
kernel. Test helper (tests/test_head_grad_host.py, tests/test_head_grad_gpu.py).

Layout: x float16 [M, K], w float16 [N, K], dy float32 [M, N]; every row is valid.

    dX = fp16(dY W)            dW = dY^T X (+ old)            db = column sums of dY (+ old)

The bound
---------
u = 2^-24 (fp32 unit roundoff). The operands are exact (fp16 and fp32 values), but a product dy * w or dy * x has up to 35 significant bits:
it is no longer exact in fp32, unlike the fp16 x fp16 products of tests/linear_grad_ref.py. So the bound is the standard one for a length-n
fp32 sum of ROUNDED products: each product carries one rounding (1 + d), |d| <= u, and each of the n - 1 additions one more, so a term
passes through at most n roundings whatever the order of the additions, and (1 + u)^n - 1 <= (n + 1) u as long as n^2 u <= 1 (n <= 4096; asserted).
A fused multiply-add rounds less (the product is not rounded on its own) and stays inside. With t the terms of one output element:

    dW_nk: t_m = dy_mn x_mk, n = M terms;  with accumulate the old value is one more term (n = M + 1):   EdW = (n + 1) u sum |t|
    db_n:  t_m = dy_mn, the same count and the same formula (its terms are exact; the additions are what is bounded)
    dX_mk: t_n = dy_mn w_nk, n = N terms:  e = (N + 1) u sum |t|, then ONE fp16 rounding r(y) = max(2^-11 y, 2^-25) of a value of
           magnitude at most |dX| + e:   EdX = e + r(|dX| + e)

The bound holds for any summation order (chunked or not, fused or not), so it does not pin the implementation. Every constant is a format's
or a count; no term was read off a device. The bound has no term for an overflow: reference_and_bound asserts that dX stays inside fp16.
"""
import numpy as np

from oracle.fp import F16_MAX, U32, fma32, r16

CHUNK = 128  # token rows per chunk of the dW / db sums (kHgChunk of csrc/mdr_head_grad.hip)

# The shapes of the GPU test: one row, the TINY and DEEP batch sizes of the chain tests, one row past a 64-row tile, the training batch
# (two chunks, the second ragged); a one-tile, a multi-tile, a non-square and the model's (N, K).
M_SWEEP = [1, 4, 6, 65, 150]
NK = [(128, 128), (256, 256), (64, 192), (768, 768)]


def chunks(M):
    return (M + CHUNK - 1) // CHUNK


def reference_and_bound(x, w, dy, old_dw=None, old_db=None):
    """{"dx", "dw", "db"} -> (reference, bound), float64."""
    M, K = x.shape
    N = w.shape[0]
    assert max(M + 1, N) <= 4096
    X, W, DY = x.astype(np.float64), w.astype(np.float64), dy.astype(np.float64)
    dx = DY @ W
    e = (N + 1) * U32 * (np.abs(DY) @ np.abs(W))
    edx = e + r16(np.abs(dx) + e)
    assert float((np.abs(dx) + edx).max()) < F16_MAX, "dX leaves the fp16 range: scale dy down"
    odw = np.zeros((N, K)) if old_dw is None else old_dw.astype(np.float64)
    odb = np.zeros(N) if old_db is None else old_db.astype(np.float64)
    dw = DY.T @ X + odw
    edw = (M + 1 + (old_dw is not None)) * U32 * (np.abs(DY).T @ np.abs(X) + np.abs(odw))
    db = DY.sum(axis=0) + odb
    edb = (M + 1 + (old_db is not None)) * U32 * (np.abs(DY).sum(axis=0) + np.abs(odb))
    return {"dx": (dx, edx), "dw": (dw, edw), "db": (db, edb)}


def emulate(x, w, dy, old_dw=None, old_db=None):
    """The kernels' dataflow in numpy: every step one fp32 fused multiply-add (oracle.fp.fma32), dX over n in order and rounded to fp16 once,
    dW and db over the rows of a chunk in order, the chunks added in order, the old value last. Returns (dx float16 [M, K], dw float32
    [N, K], db float32 [N])."""
    f32 = np.float32
    M, K = x.shape
    N = w.shape[0]
    xf, wf, dyf = x.astype(f32), w.astype(f32), dy.astype(f32)
    acc = np.zeros((M, K), f32)
    for n in range(N):
        acc = fma32(dyf[:, n:n + 1], wf[n:n + 1, :], acc)
    with np.errstate(over="ignore"):
        dx = acc.astype(np.float16)
    dw, db = None, None
    for c in range(chunks(M)):
        pw, pb = np.zeros((N, K), f32), np.zeros(N, f32)
        for m in range(c * CHUNK, min((c + 1) * CHUNK, M)):
            pw = fma32(dyf[m][:, None], xf[m][None, :], pw)
            pb = pb + dyf[m]
        dw, db = (pw, pb) if c == 0 else (dw + pw, db + pb)
    if old_dw is not None:
        dw = dw + old_dw.astype(f32)
    if old_db is not None:
        db = db + old_db.astype(f32)
    return dx, dw, db


# ---- makers --------------------------------------------------------------------------------------------------------------------------------
def realistic(M, N, K, seed, dy_scale=1.0):
    """(x float16, w float16, dy float32): N(0, 1) activations, weights x 0.02, N(0, 1) gradients times dy_scale (a loss scale) with all 24
    bits of their significands in use."""
    rng = np.random.default_rng([seed, M, N, K, 9])
    x = rng.standard_normal((M, K)).astype(np.float16)
    w = (0.02 * rng.standard_normal((N, K))).astype(np.float16)
    dy = (dy_scale * rng.standard_normal((M, N))).astype(np.float32)
    return x, w, dy


def old_values(N, K, seed):
    rng = np.random.default_rng([seed, N, K, 10])
    return rng.standard_normal((N, K)).astype(np.float32), rng.standard_normal(N).astype(np.float32)


def bias(N, seed):
    return (0.1 * np.random.default_rng([seed, N, 5]).standard_normal(N)).astype(np.float32)
