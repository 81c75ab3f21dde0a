"""Host restatement of ONE Linear backward call (mdr_linear_backward, include/mdr_linear_grad.h): the four formulas in fp64, a derived
elementwise error bound, an fp32 / fp16 emulation of the kernels' dataflow (with switchable mutations) and makers for the inputs. numpy
(erfc in float64 through torch's CPU kernel); nothing here is measured from a kernel. Test helper (tests/test_linear_grad_host.py,
tests/test_linear_grad_gpu.py).

Layout: x float16 [M, K], w float16 [N, K], dy float16 [M, N], pre None or the float16 pre-activation u [M, N], m = valid rows (None: M).

Formulas, on the first m rows (the others do not exist for the call):
    dZ = dY o gelu'(u),  gelu'(u) = Phi(u) + u phi(u)   (pre None: dZ = dY)
    dX = dZ W            dW = dZ^T X (+ old)            db = column sums of dZ (+ old)

The bound
---------
Derived from the rounding points listed at the top of csrc/mdr_linear_grad.inl. u = 2^-24 (fp32 half ulp), X = 2^-23 (one fp32 ulp: the
rounding of an MFMA's internal adds is not documented as nearest-even, and the ISA documents v_exp_f32 as accurate to 1 ulp), h = 2^-11
(fp16 half ulp of a normal), z = 2^-25 (half the fp16 subnormal spacing). Each line bounds the absolute error of the device's value.

1. Operands are fp16: exact. A product of two fp16 is exact in fp32 -- but the fp16 MFMA does not add the products of one instruction as
   exact numbers. It aligns them to the largest EXPONENT FIELD among them (the sum of the two operands' fields) and keeps 24 bits below it,
   cutting the rest off towards zero. For normal operands 2^field <= |a b|, so the cut is below one ulp of the largest product: that is the
   "one ulp lost per addition" of lines 3 and 4. A subnormal operand, and a zero, carries fp16's SMALLEST field, 2^-14, whatever its value:
   its product sits up to ten bits lower than its field says, and a sum of such products comes out with as many bits fewer. (Seen where the
   chain test runs FFN2's dW over four CLS rows: a column of GELU outputs that is subnormal in every row, 63 x 2^-22 and 2^-22, times dy of
   2^-13 and 2^-3: the smaller product arrives cut to a multiple of 2^(-14 - 3 - 24).) With v' = max(|v|, 2^-14), each of the at most 32
   products of an instruction errs by less than 2^-24 max_i a'_i b'_i <= 2^-24 (sum_i |a_i b_i| + sum_i (a'_i b'_i - |a_i b_i|)); the
   first sum is what lines 3 and 4 count already, the second is the term
       F(a, b) = 32 * 2^-24 * sum_i (a'_i b'_i - |a_i b_i|) = 16 X sum_i (a'_i b'_i - |a_i b_i|),
   which is zero when no operand is subnormal or zero. Zeros are counted because nothing documents that the alignment skips them.
2. gelu'. Phi: the forward's tail polynomial, stated max |Phi error| 2.1e-7 (csrc/mdr_encoder_gemm.inl), + u for the fp32 add of 1/2.
   phi(u) = exp2(u^2 c) k, c = -log2(e) / 2, k = 1 / sqrt(2 pi): u^2 is exact (22 bits), the product with c errs by 2 u |arg| (the
   constant and the rounding), which the exponential turns into a relative ln 2 * 2 u |arg|; the exponential itself X; the constant k, its
   product and the product with u: 3 u; a flushed subnormal result: 2^-126. The final add: u |gelu'|. So
       dg = 2.1e-7 + u + |u phi(u)| (X + 3 u + 2 ln 2 u |arg|) + |u| 2^-126 + u |gelu'(u)|.
   dZ = fp16(fp32(dy) * g): the fp32 product u |dy g|, then the fp16 rounding r(y) = max(h y, z) of a value of magnitude at most y:
       e = |dy| dg + u |dy gelu'|,   EdZ = e + r(|dZ| + e).          (pre None: EdZ = 0)
3. dX_mk: N products added in fp32 in some order, at most one ulp lost per addition, then the exact + 0.0f and the fp16 rounding:
       e = sum_n EdZ_mn |w_nk| + N X sum_n (|dZ_mn| + EdZ_mn) |w_nk| + F(|dZ| + EdZ, w),   EdX = e + r(|dX| + e).
4. dW_nk: the rows of a chunk in slabs of 64 (zero rows behind m are added too), the S chunks in order, then the old value: at most
   mpad + S + 1 additions, mpad = m rounded up to whole slabs, no fp16 term:
       EdW = sum_m EdZ_mn |x_mk| + (mpad + S + 1) X (sum_m (|dZ_mn| + EdZ_mn) |x_mk| + |old_nk|) + F(|dZ| + EdZ, x).
5. db_n: fewer additions than that in any order the kernel uses:
       Edb = sum_m EdZ_mn + (mpad + S + 1) X (sum_m (|dZ_mn| + EdZ_mn) + |old_n|).

Every constant is a format's, a count, the ISA's 1 ulp or the forward's stated 2.1e-7 (which the host test re-checks for the derivative over
every finite fp16 u); no term was read off a device. The emulation below is a second implementation of the dataflow: the host test shows
that it stays inside the bound and that each mutation leaves it.
"""
import numpy as np
import torch

from oracle.fp import F16_MAX, N16, U32, X1ULP, exp2_32, fma32, r16

PHI_ERR = 2.1e-7
SLAB = 64        # token rows per staged slab of the weight-gradient kernel
TILE = 128       # edge of a dW tile
TARGET_WGS = 512
C_EXP = -0.72134752044448170   # -log2(e) / 2
K_PHI = 0.3989422804014327     # 1 / sqrt(2 pi)

MUTATIONS = ("extra_row", "missing_row", "drop_last_chunk", "dw_transposed", "dx_from_w", "db_missing_last_slab", "accumulate_ignored",
             "db_without_dz", "gelu_no_uphi")

# The shapes of the GPU tests (the host test runs the emulation over the same ones).
SMALL_NK = [(64, 64), (192, 64), (64, 192), (128, 128), (256, 384)]
MODEL_NK = [(768, 768), (2304, 768), (3072, 768), (768, 3072)]
M_SWEEP = [1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 300]   # 63 .. 65 and 127 .. 129: -1, 0, +1 around one and two chunks of 64 rows
# (M, N, K) at training row counts: the smallest M at which a chunk of lg_wgrad_kernel holds three slabs or more, so that its register double
# buffer reaches the steady state (put slab i, issue i + 1, compute i, put i + 1, ...), with S >= 3 partials to reduce and a ragged last
# chunk. The three wide model Linears (3, 7 and 9 slabs per chunk), a small-tile shape, the 64-wide remainder quarter on either side of a
# 128 tile, and FFN2 at the M from which its dX leaves the one-tile GEMMs (17 slabs per chunk). assert_large() states the properties; the
# host test holds it against the library's split, so a change of the split constants fails there instead of shrinking the coverage.
# The host emulation runs over every one of them (a few seconds each).
# The two reader shapes: the answer reader's fused QKV (S = 3, 704 rows per chunk, a last chunk of 643) and its out-projection (S = 7, 320
# rows per chunk, a last chunk of 131), at the same smallest M as the retriever's.
LARGE_MNK = [(2051, 768, 768), (2051, 2304, 768), (2051, 3072, 768), (11011, 256, 384), (33000, 64, 192), (33000, 192, 64), (4099, 768, 3072),
             (2051, 3072, 1024), (2051, 1024, 1024)]
# The four Linears of the answer reader at ELECTRA-large geometry (width 1024, FFN 4096): fused QKV, out-projection (and the pooler), FFN1
# (the GELU path in the model), FFN2. M = 300 like MODEL_NK: several dW tiles in both directions at a width no roberta-base shape has, and
# dX as a forward GEMM with (N, K) = (1024, 3072), (1024, 1024), (1024, 4096) and (4096, 1024).
READER_NK = [(3072, 1024), (1024, 1024), (4096, 1024), (1024, 4096)]
# The reader's pooler: packed_linear on the B CLS rows of a batch, no device-side row count. One row, a row count that is no multiple of
# the MFMA's four-row groups, and one whole slab: the smallest, an odd and the largest batch the reader trains at.
POOLER_MNK = [(1, 1024, 1024), (3, 1024, 1024), (64, 1024, 1024)]
# The reader's FFN Linears have 32 x 8 = 256 dW tiles, so the split is S = 2 at EVERY M (512 / 256): two chunks however long. 2051 rows are
# the smallest M of LARGE_MNK's kind: 1088 rows per chunk (17 slabs: the steady state of the slab loop, as long a chain as FFN2's at 4099
# rows), a last chunk of 963 rows = 16 slabs, the last one 3 rows. assert_two_chunks() states it; assert_large() cannot (it wants S >= 3).
TWO_CHUNK_MNK = [(2051, 4096, 1024), (2051, 1024, 4096)]
# The smallest M, and a ragged one, at which dX of the reader's QKV and FFN1 leaves the one-tile GEMMs on 256 compute units (8 ceil(M / 256)
# >= 384: M >= 12033): dX is then a persistent forward GEMM with N = 1024 and K = 3072 / 4096 (gemm_choose's K >= 2048 branch), and a chunk
# of FFN1's dW (S = 2) is a chain of 97 slabs. FFN2's dX has GEMM N = 4096 > kPersistBiasMax and stays on the one-tile kernels at any M.
# Too large for the host emulation (minutes in numpy's fp32 slab loop): the GPU test runs them on the exact grid alone.
PERSIST_DX_MNK = [(12300, 3072, 1024), (12300, 4096, 1024)]


def assert_large(shapes=None, chunks_of=None):
    """Every shape of LARGE_MNK: rows_per_chunk >= 192 (three slabs: the prefetch branch of the slab loop is taken twice in a row), S >= 3,
    M no multiple of the slab and the last chunk shorter than the others. Over the list: some last chunk ends on FEWER slabs than the others
    (the loop ends early) and some on as many with a partial last slab (the zero-fill inside the steady state). Returns
    [(M, N, K, S, rows_per_chunk, rows of the last chunk)]."""
    out = []
    for M, N, K in (LARGE_MNK if shapes is None else shapes):
        S, rpc = (chunks_of or chunks)(M, N, K)
        last = M - (S - 1) * rpc
        assert rpc >= 3 * SLAB and S >= 3 and M % SLAB != 0 and 0 < last < rpc, (M, N, K, S, rpc, last)
        out.append((M, N, K, S, rpc, last))
    fewer = [(last + SLAB - 1) // SLAB < rpc // SLAB for *_, rpc, last in out]
    assert any(fewer) and not all(fewer), out
    return out


def assert_two_chunks(shapes=None, chunks_of=None):
    """Every shape of TWO_CHUNK_MNK: exactly S = 2 chunks of three slabs or more (the slab loop's steady state), M no multiple of the slab and
    a last chunk that is shorter than the first and not empty. Returns [(M, N, K, S, rows_per_chunk, rows of the last chunk)]."""
    out = []
    for M, N, K in (TWO_CHUNK_MNK if shapes is None else shapes):
        S, rpc = (chunks_of or chunks)(M, N, K)
        last = M - (S - 1) * rpc
        assert S == 2 and rpc >= 3 * SLAB and M % SLAB != 0 and 0 < last < rpc, (M, N, K, S, rpc, last)
        out.append((M, N, K, S, rpc, last))
    return out


def chunks(M, N, K):
    """(S, rows_per_chunk) of mdr_linear_backward_chunks: a function of (M, N, K) alone (the host test compares it with the library's)."""
    tiles = ((N + TILE - 1) // TILE) * ((K + TILE - 1) // TILE)
    slabs = (M + SLAB - 1) // SLAB
    want = max(1, min((TARGET_WGS + tiles - 1) // tiles, slabs))
    per = (slabs + want - 1) // want
    return (slabs + per - 1) // per, per * SLAB


def gelu_grad64(u):
    """Phi(u) + u phi(u) in float64."""
    u = np.asarray(u, np.float64)
    Phi = 0.5 * torch.special.erfc(torch.from_numpy(-u / np.sqrt(2.0))).numpy()
    return Phi + u * np.exp(-0.5 * u * u) / np.sqrt(2.0 * np.pi)


def gelu_grad_bound(u):
    """dg of the docstring: the absolute error of the device's fp32 gelu'(u)."""
    u = np.abs(np.asarray(u, np.float64))
    arg = u * u * -C_EXP
    uphi = u * np.exp(-0.5 * u * u) / np.sqrt(2.0 * np.pi)
    return PHI_ERR + U32 + uphi * (X1ULP + 3 * U32 + 2 * np.log(2.0) * U32 * arg) + u * 2.0 ** -126 + U32 * np.abs(gelu_grad64(u))


def gelu_grad32(u, mutation=None):
    """The kernel's fp32 gelu'(u): the forward's tail polynomial at min(|u|, 16) for Phi, one exp2 for phi."""
    f32 = np.float32
    u = np.asarray(u, np.float16).astype(f32)
    a = np.minimum(np.abs(u), f32(16))
    p = fma32(a, -1.982813420e-05, 6.620948925e-04)
    for c in (-7.759194708e-03, 5.296392132e-02, 4.590664427e-01, 1.151119066e+00):
        p = fma32(p, a, c)
    e = fma32(p, a, 1.0)
    s = np.copysign(f32(0.5) - exp2_32(-e), u)
    dens = exp2_32(u * u * f32(C_EXP)) * f32(K_PHI)
    if mutation == "gelu_no_uphi":
        return s + f32(0.5)
    return (s + f32(0.5)) + u * dens


def gemm_accum_bound(abs_a, abs_b, terms):
    """The fp32 accumulation term of a GEMM whose operands are exact: `terms` products added in some order, at most one ulp lost per addition
    (line 3 of the docstring). Shared with tests/gemm_ref.py: dX IS a forward GEMM."""
    return terms * X1ULP * (abs_a @ abs_b)


def field_floor_term(abs_a, abs_b):
    """F of line 1 of the docstring for abs_a @ abs_b: what the fp16 MFMA's alignment to the largest exponent field costs beyond one ulp per
    addition when an operand is subnormal or zero. Zero for normal operands."""
    return 16 * X1ULP * (np.maximum(abs_a, N16) @ np.maximum(abs_b, N16) - abs_a @ abs_b)


def aligned_dw(x, dy):
    """dW = dY^T X of at most 32 rows as line 1 of the docstring describes ONE fp16 MFMA: every non-zero product cut towards zero at
    2^(f - 24), f the largest sum of exponent fields among them (a subnormal's field is -14). float64 [N, K]. A model for the host test of
    the term F, not a statement about any other case."""
    assert x.shape[0] <= 32
    X, DY = x.astype(np.float64), dy.astype(np.float64)
    field = lambda v: np.floor(np.log2(np.maximum(np.abs(v), N16)))  # noqa: E731
    prod = DY.T[:, :, None] * X[None, :, :]
    f = np.where(prod != 0, field(DY).T[:, :, None] + field(X)[None, :, :], -np.inf).max(axis=1, keepdims=True)
    lsb = 2.0 ** np.where(np.isfinite(f), f - 24, 0.0)
    return (np.trunc(prod / lsb) * lsb).sum(axis=1)


def subnormal_columns_case():
    """(x, w, dy) float16, M = 4, N = 256, K = 384: FFN2's dW over four CLS rows with every 16th column of x subnormal in every row -- the row
    with the largest dy holds 1 or 2 x 2^-22, the others 33 .. 63 x 2^-22 under a dy 2^-8 times smaller."""
    M, N, K = 4, 256, 384
    x, w, dy = realistic(M, N, K, 17)
    dy = (dy.astype(np.float32) * np.float32(2.0) ** np.array([-10, -10, -2, -10], np.float32)[:, None]).astype(np.float16)
    rng = np.random.default_rng([17, 4])
    cols = np.arange(1, K, 16)
    sub = -rng.integers(33, 64, size=(M, len(cols)))
    sub[2] = -rng.integers(1, 3, size=len(cols))
    x[:, cols] = (sub * 2.0 ** -22).astype(np.float16)
    assert ((np.abs(x[:, cols]) < N16) & (x[:, cols] != 0)).all()
    return x, w, dy


def reference_and_bound(x, w, dy, pre=None, m=None, old_dw=None, old_db=None):
    """{"dz", "dx", "dw", "db"} -> (reference, bound), float64. dz and dx have m rows. Asserts that nothing leaves the fp16 range (the bound
    has no term for an overflow)."""
    M, K = x.shape
    N = w.shape[0]
    m = M if m is None else int(m)
    S, _ = chunks(M, N, K)
    X, W, DY = x[:m].astype(np.float64), w.astype(np.float64), dy[:m].astype(np.float64)
    if pre is None:
        dz, edz = DY, np.zeros_like(DY)
    else:
        u = pre[:m].astype(np.float64)
        g = gelu_grad64(u)
        dz = DY * g
        e = np.abs(DY) * gelu_grad_bound(u) + U32 * np.abs(dz)
        edz = e + r16(np.abs(dz) + e)
        assert m == 0 or float((np.abs(dz) + edz).max()) < F16_MAX, "dZ leaves the fp16 range: scale dy down"
    adz = np.abs(dz) + edz
    dx = dz @ W
    e = edz @ np.abs(W) + gemm_accum_bound(adz, np.abs(W), N) + field_floor_term(adz, np.abs(W))
    edx = e + r16(np.abs(dx) + e)
    assert m == 0 or float((np.abs(dx) + edx).max()) < F16_MAX, "dX leaves the fp16 range: scale w down"
    cnt = ((m + SLAB - 1) // SLAB * SLAB + S + 1) * X1ULP
    odw = np.zeros((N, K)) if old_dw is None else old_dw.astype(np.float64)
    odb = np.zeros(N) if old_db is None else old_db.astype(np.float64)
    dw = dz.T @ X + odw
    edw = edz.T @ np.abs(X) + cnt * (adz.T @ np.abs(X) + np.abs(odw)) + field_floor_term(adz.T, np.abs(X))
    db = dz.sum(axis=0) + odb
    edb = edz.sum(axis=0) + cnt * (adz.sum(axis=0) + np.abs(odb))
    return {"dz": (dz, edz), "dx": (dx, edx), "dw": (dw, edw), "db": (db, edb)}


def emulate(x, w, dy, pre=None, m=None, old_dw=None, old_db=None, mutation=None):
    """The kernels' dataflow in numpy: dZ = fp16(fp32 dy * fp32 gelu'), dX = fp16 of an fp32 product over the valid rows, dW and db as fp32 sums
    slab by slab inside a chunk (rows at or behind m are zero-filled), the chunks added in order, the old value last. Returns (dx float16 [m, K],
    dw float32 [N, K], db float32 [N]).

    mutation (None: the correct dataflow) switches ONE defect on, for the tests that prove the bound notices it:
    extra_row: row m (which exists in the buffers) taken as valid; missing_row: row m - 1 zero-filled; drop_last_chunk: the last chunk's partial
    never added (S > 1); dw_transposed: dW written as [K, N] (N = K); dx_from_w: dX = dZ W^T (N = K); db_missing_last_slab: db without the last
    slab of rows; accumulate_ignored: the old value not added; db_without_dz: db from dY instead of dZ; gelu_no_uphi: gelu' = Phi alone."""
    assert mutation is None or mutation in MUTATIONS
    f32 = np.float32
    M, K = x.shape
    N = w.shape[0]
    m = M if m is None else int(m)
    S, rpc = chunks(M, N, K)
    me = m
    if mutation == "extra_row":
        me = min(m + 1, M)
    elif mutation == "missing_row":
        me = max(m - 1, 0)
    dyf = dy.astype(f32)
    if pre is None:
        dz = dyf
    else:
        with np.errstate(over="ignore", invalid="ignore"):
            dz = (dyf * gelu_grad32(pre, mutation)).astype(np.float16).astype(f32)
    xf, wf = x.astype(f32), w.astype(f32)
    with np.errstate(over="ignore"):
        dx = (dz[:me] @ (wf.T if mutation == "dx_from_w" else wf)).astype(np.float16)[:m]
    if dx.shape[0] < m:
        dx = np.concatenate([dx, np.zeros((m - dx.shape[0], K), np.float16)])
    dbsrc = dyf if mutation == "db_without_dz" else dz
    dw, db = np.zeros((N, K), f32), np.zeros(N, f32)
    last_slab = (max(me, 1) - 1) // SLAB * SLAB
    for c in range(S):
        if mutation == "drop_last_chunk" and S > 1 and c == S - 1:
            continue
        pw, pb = np.zeros((N, K), f32), np.zeros(N, f32)
        for r0 in range(c * rpc, min((c + 1) * rpc, me), SLAB):
            r1 = min(r0 + SLAB, me)
            pw = pw + dz[r0:r1].T @ xf[r0:r1]
            if not (mutation == "db_missing_last_slab" and r0 == last_slab):
                pb = pb + dbsrc[r0:r1].sum(axis=0, dtype=f32)
        dw, db = dw + pw, db + pb
    if mutation == "dw_transposed":
        dw = np.ascontiguousarray(dw.T)
    if mutation != "accumulate_ignored":
        if old_dw is not None:
            dw = dw + old_dw.astype(f32)
        if old_db is not None:
            db = db + old_db.astype(f32)
    return dx, dw, db


# ---- makers --------------------------------------------------------------------------------------------------------------------------------
def realistic(M, N, K, seed, dy_scale=1.0):
    """(x, w, dy) float16: N(0, 1) activations, weights x 0.02, N(0, 1) gradients times dy_scale (a loss scale)."""
    rng = np.random.default_rng([seed, M, N, K, 3])
    x = rng.standard_normal((M, K)).astype(np.float16)
    w = (0.02 * rng.standard_normal((N, K))).astype(np.float16)
    dy = (dy_scale * rng.standard_normal((M, N))).astype(np.float16)
    return x, w, dy


def bias(N, seed):
    return (0.1 * np.random.default_rng([seed, N, 5]).standard_normal(N)).astype(np.float32)
