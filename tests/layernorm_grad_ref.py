"""Host restatement of ONE LayerNorm backward call (mdr_layernorm_backward, include/mdr_layernorm_grad.h): the formulas in fp64, a derived
elementwise error bound, an fp32 / fp16 emulation of the kernel's dataflow (with switchable mutations) and makers for the inputs. numpy
only; nothing here is measured from a kernel. Test helper (tests/test_layernorm_grad_host.py, tests/test_layernorm_grad_gpu.py).

Layout: inp float32 or float16 [M, H], res None / float16 / float32 [M, H], dy16 None or float16 [M, H], dy2 None or float16 / float32
[M, H], g float32 [H], m = valid rows (None: M).

Formulas, on the first m rows (the others do not exist for the call), all per row:
    x = inp + res      mu = mean(x)      A = mean((x - mu)^2) + eps      r = A^-1/2      t = (x - mu) r   (xhat)
    dy = dy16 + dy2    a = dy g          c1 = mean(a)                    c2 = mean(a t)
    dx = r (a - c1 - t c2)               dg = sum over rows of dy t (+ old)              db = sum over rows of dy (+ old)

The bound
---------
Derived from the rounding points listed at the top of csrc/mdr_layernorm_grad.hip. u = 2^-24 (fp32 unit roundoff), D = H / 64 + 6 (the
additions a term of a row sum passes through: the lane's H / 64 elements in sequence, then a 6-level butterfly). First order in u; the
neglected products of two error terms are covered by a final factor 1 + 2^-10, as in oracle/trunk_rows_oracle.py. Each line bounds the
absolute error of the device's value.

1. x, mu, r, t: the forward's arithmetic, so the forward's derivation (oracle/trunk_rows_oracle.py, `bound`): dx_i (one rounded add, none
   without a residual), dmu, e_i, rho_A, rho_r (the relative error of rstd, v_rsq_f32 at the ISA's 1 ulp), and
       Et_i = r (dmu + e_i)(1 + rho_r) + |t_i| (rho_r + u).
   stats() repeats those lines and returns the intermediate terms that `bound` keeps to itself; the host test checks that they reproduce
   `bound` itself at g = 1, b = 0.
2. dy = fp32(dy16) + fp32(dy2): Edy = u |dy| for the one rounded add, 0 when only one is given (fp16 and fp32 operands are exact).
3. a = dy g: Ea = |g| Edy + u (|a| + |g| Edy).
4. c1 = mean(a): Ec1 = mean(Ea) + D u mean(|a| + Ea) + 3 u |c1| (the summation, then the division by H: 3 u also covers a division that is
   not correctly rounded; the forward's dmu line).
5. p = a t: Ep = |t| Ea + (|a| + Ea) Et + u (|p| + |t| Ea + (|a| + Ea) Et) (the product's rounding; fused into the sum it is absent).
   c2 = mean(p): Ec2 = mean(Ep) + D u mean(|p| + Ep) + 3 u |c2|.
6. q = t c2: Eq = |t| Ec2 + (|c2| + Ec2) Et + u (|q| + |t| Ec2 + (|c2| + Ec2) Et).
   w = (a - c1) - q: E1 = Ea + Ec1 + u (|a - c1| + Ea + Ec1), Ew = E1 + Eq + u (|w| + E1 + Eq).
   dx = r w: Edx = r (1 + rho_r) Ew + |dx| (rho_r + u) + u r (1 + rho_r) Ew.
   dx32 is not rounded again; dx16 is the fp16 rounding of that fp32 value, accepted by the monotonic rule of oracle/trunk_rows_oracle.py:
   RNE16(ref - bound) <= out <= RNE16(ref + bound).
7. dg_e = sum over rows of dy t: a term errs by Eterm = |t| Edy + (|dy| + Edy) Et + u (|dy t| + |t| Edy + (|dy| + Edy) Et); the sum adds
   wave by wave, the chunks in sixteen strands (strand j: chunks j, j + 16, ... in order; then the strands in order) and the old value last, at
   most Nadd = rows_per_chunk / 4 + 4 + S + 1 additions per element:
       Edg = sum(Eterm) + Nadd u (sum(|dy t| + Eterm) + |old|).
   db_e = sum over rows of dy: Edb = sum(Edy) + Nadd u (sum(|dy| + Edy) + |old|).

Every constant is a format's, a count or the ISA's 1 ulp; no term was read off a device. reference_and_bound asserts that |dx| + bound stays
below 65504: the bound has no term for an fp16 overflow. The emulation below is a second implementation of the dataflow: the host test shows
that it stays inside the bound and that each mutation leaves it.
"""
import numpy as np

from oracle import trunk_rows_oracle as tr
from oracle.fp import F16_MAX, U32

MAX_CHUNKS = 1024             # target number of workgroups ...
MAX_PARTIAL_BYTES = 4 << 20   # ... as far as the partial sums [S][2][H] stay within 4 MiB
WAVES = 4
STRANDS = 16                  # chains of the partial-sum reduction over the chunks
EPS = 1e-5

MUTATIONS = ("no_c1", "no_c2", "no_rstd", "no_g", "stats_without_residual", "no_eps", "dg_from_x", "dy2_dropped", "extra_row", "missing_row",
             "drop_last_chunk", "accumulate_ignored")

# The shapes of the GPU tests (the host test runs the emulation over the same ones).
HS = [64, 192, 256, 768, 1024]
M_SWEEP = [1, 2, 3, 4, 5, 7, 8, 9, 300]
# (H, M) at training row counts: the smallest M at the shipping widths at which a wave of ln_grad_kernel walks three rows or more with dg and db
# carried in registers (rows_per_chunk >= 12), the last chunk is ragged, and a strand of grad_strand_reduce_kernel adds more than sixteen
# chunks (S > 16 * 16). assert_large() states the properties; the host test holds it against the library's split. The host emulation runs
# over every one of them (under a second each).
LARGE_HM = [(768, 5461), (1024, 4101), (192, 8200), (256, 8200)]
# (in, residual, dy16, dy2). The first three are the trunk's: post_ln of csrc/mdr_encoder_trunk.inl with residual_fp32 = 0 (fp32 sums + the fp16
# stream; both gradients come back in fp16), 1 (fp32 sums + the fp32 stream; the stream's gradient in fp32) and 2 (fp16 Linear output + the fp32
# stream). The others complete the operand combinations.
TRUNK_COMBOS = [("f32", "res16", True, "f16"), ("f32", "res32", True, "f32"), ("f16", "res32", True, "f32")]
OTHER_COMBOS = [("f32", "none", True, None), ("f16", "none", None, "f32"), ("f16", "res16", True, "f16"), ("f32", "res32", None, "f32")]
COMBOS = TRUNK_COMBOS + OTHER_COMBOS
# family -> whether it also runs under a loss scale of 2^8 (the constant and 1e-3 rows have rstd = 316 and up: max |dx| 2.3e3 at unit scale, 6e5
# under 2^8, outside fp16)
FAMILIES = {"unit": True, "mean30": True, "outlier40": True, "const": False, "small_1e-3": False}


def chunks(M, H):
    """(S, rows_per_chunk) of mdr_layernorm_backward_chunks: a function of (M, H) alone (the host test compares it with the library's)."""
    if M < 1 or H < 64 or H > 1024 or H % 64:
        return 0, 0
    cap = min(MAX_CHUNKS, MAX_PARTIAL_BYTES // (8 * H))
    rpc = ((M + cap - 1) // cap + 3) // 4 * 4
    return (M + rpc - 1) // rpc, rpc


def assert_large(shapes=None, chunks_of=None):
    """Every shape of LARGE_HM: rows_per_chunk >= 12, M no multiple of it, S > 256. Returns [(H, M, S, rows_per_chunk)]."""
    out = []
    for H, M in (LARGE_HM if shapes is None else shapes):
        S, rpc = (chunks_of or chunks)(M, H)
        assert rpc >= 3 * WAVES and M % rpc != 0 and S > STRANDS * STRANDS, (H, M, S, rpc)
        out.append((H, M, S, rpc))
    return out


def large_ms(M, H):
    """valid-row counts for a shape of LARGE_HM: none; one inside a chunk in the middle, with hundreds of whole chunks behind it (a call on
    those rows alone is cut otherwise: its sums are compared through the bound); M - 2, for which a call on those rows alone is cut alike
    (compared bit for bit); all"""
    S, rpc = chunks(M, H)
    ms = (0, (S // 2) * rpc + rpc - 1, M - 2, M)
    assert ms[1] % rpc and ms[1] + 100 * rpc < M and chunks(ms[2], H)[1] == rpc != chunks(ms[1], H)[1], (M, H, ms)
    return ms


def split_ms(H=64):
    """Two M for which the rows are cut into S >= 3 chunks of >= 8 rows that do not divide M: a wave walks several rows, the last chunk is
    ragged and the partial sums are reduced. Found by calling chunks()."""
    out = []
    for M in range(4 * MAX_CHUNKS + 1, 16 * MAX_CHUNKS):
        S, rpc = chunks(M, H)
        if S >= 3 and rpc >= 8 and M % rpc and (not out or rpc != chunks(out[-1], H)[1]):
            out.append(M)
            if len(out) == 2:
                return out
    raise AssertionError("no split shape found")


def _mean(a):
    return a.sum(-1, keepdims=True) / a.shape[-1]


def stats(x, ex, eps):
    """The forward's derivation (oracle/trunk_rows_oracle.py, bound) up to t = xhat: dict(mu, d, r, t, Et, rho_r), [rows, H] or [rows, 1]."""
    H = x.shape[-1]
    D = H // 64 + 6
    eps = np.float64(eps)
    mu = _mean(x)
    d = x - mu
    A = _mean(d * d) + eps
    r = 1.0 / np.sqrt(A)
    dmu = _mean(ex) + D * U32 * _mean(np.abs(x)) + 3 * U32 * np.abs(mu)
    e = ex + U32 * (np.abs(d) + dmu + ex)
    rho_A = (2 * _mean(np.abs(d) * e) + _mean((dmu + e) ** 2)) / A + (D + 5) * U32
    with np.errstate(divide="ignore", invalid="ignore"):
        hi = np.where(rho_A < 1, (1 - np.minimum(rho_A, 1 - 1e-300)) ** -0.5 * (1 + 2 * U32) - 1, np.inf)
    lo = 1 - (1 + rho_A) ** -0.5 * (1 - 2 * U32)
    rho_r = np.maximum(hi, lo)
    t = d * r
    Et = r * (dmu + e) * (1 + rho_r) + np.abs(t) * (rho_r + U32)
    return dict(mu=mu, d=d, r=r, t=t, Et=Et, rho_r=rho_r)


def _dy64(dy16, dy2, m):
    """-> (dy, Edy) float64 [m, H]"""
    parts = [p[:m].astype(np.float64) for p in (dy16, dy2) if p is not None]
    assert parts, "dy16 and dy2 are both None"
    dy = parts[0] if len(parts) == 1 else parts[0] + parts[1]
    return dy, (U32 * np.abs(dy) if len(parts) == 2 else np.zeros_like(dy))


def reference_and_bound(inp, res, dy16, dy2, g, eps=EPS, m=None, old_dg=None, old_db=None):
    """{"dx", "dg", "db"} -> (reference, bound), float64. dx has m rows. Asserts that the bound says something (rho_A < 1) and that nothing
    leaves the fp16 range."""
    M, H = inp.shape
    m = M if m is None else min(max(int(m), 0), M)
    S, rpc = chunks(M, H)
    D = H // 64 + 6
    x, ex = tr.ln_inputs(inp[:m], None if res is None else res[:m])
    st = stats(x, ex, eps)
    r, t, Et, rho_r = st["r"], st["t"], st["Et"], st["rho_r"]
    assert np.isfinite(rho_r).all(), "the bound says nothing here (rho_A >= 1): not a family to test with"
    at = np.abs(t)
    G = np.asarray(g, np.float64)
    dy, Edy = _dy64(dy16, dy2, m)
    a = dy * G
    Ea = np.abs(G) * Edy + U32 * (np.abs(a) + np.abs(G) * Edy)
    c1 = _mean(a)
    Ec1 = _mean(Ea) + D * U32 * _mean(np.abs(a) + Ea) + 3 * U32 * np.abs(c1)
    p = a * t
    Ep = at * Ea + (np.abs(a) + Ea) * Et
    Ep = Ep + U32 * (np.abs(p) + Ep)
    c2 = _mean(p)
    Ec2 = _mean(Ep) + D * U32 * _mean(np.abs(p) + Ep) + 3 * U32 * np.abs(c2)
    q = t * c2
    Eq = at * Ec2 + (np.abs(c2) + Ec2) * Et
    Eq = Eq + U32 * (np.abs(q) + Eq)
    E1 = Ea + Ec1
    E1 = E1 + U32 * (np.abs(a - c1) + E1)
    w = a - c1 - q
    Ew = E1 + Eq
    Ew = Ew + U32 * (np.abs(w) + Ew)
    dx = r * w
    Edx = r * (1 + rho_r) * Ew
    Edx = (Edx + np.abs(dx) * (rho_r + U32) + U32 * Edx) * (1 + 2.0 ** -10)
    assert m == 0 or float((np.abs(dx) + Edx).max()) < F16_MAX, "dx leaves the fp16 range: scale dy down"
    nadd = (rpc // WAVES + 4 + S + 1) * U32
    odg = np.zeros(H) if old_dg is None else old_dg.astype(np.float64)
    odb = np.zeros(H) if old_db is None else old_db.astype(np.float64)
    term = dy * t
    Eterm = at * Edy + (np.abs(dy) + Edy) * Et
    Eterm = Eterm + U32 * (np.abs(term) + Eterm)
    dg = term.sum(axis=0) + odg
    Edg = (Eterm.sum(axis=0) + nadd * ((np.abs(term) + Eterm).sum(axis=0) + np.abs(odg))) * (1 + 2.0 ** -10)
    db = dy.sum(axis=0) + odb
    Edb = (Edy.sum(axis=0) + nadd * ((np.abs(dy) + Edy).sum(axis=0) + np.abs(odb))) * (1 + 2.0 ** -10)
    return {"dx": (dx, Edx), "dg": (dg, Edg), "db": (db, Edb)}


def _wave_sum(v):
    """the xor butterfly 32, 16, .. 1 over the last axis (64 lanes), fp32: every lane ends with the same value; lane 0's is returned [rows, 1]"""
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lanes ^ o]
    return v[:, :1]


def _lane_view(a):
    """[rows, H] -> [rows, 64 lanes, elements per lane] in the kernel's per-lane element order, and whether the 16-byte path is taken"""
    R, H = a.shape
    if H % 256 == 0:  # lane l holds groups i of the four columns (l + 64 i) * 4 ..
        return a.reshape(R, H // 256, 64, 4).transpose(0, 2, 1, 3).reshape(R, 64, H // 64), True
    return a.reshape(R, H // 64, 64).transpose(0, 2, 1), False  # lane l holds columns l + 64 i


def _lane_unview(v, H):
    R = v.shape[0]
    if H % 256 == 0:
        return v.reshape(R, 64, H // 256, 4).transpose(0, 2, 1, 3).reshape(R, H)
    return v.transpose(0, 2, 1).reshape(R, H)


def _row_sum(lv, vec, grouped):
    """the kernel's row sum of per-lane values [rows, 64, n] in fp32: the lane's elements in index order (grouped: ((x0 + x1) + x2) + x3 per
    group of four first, as the statistics' first sum does on the 16-byte path), then the butterfly"""
    f32 = np.float32
    s = np.zeros(lv.shape[:2], f32)
    if vec and grouped:
        for i in range(0, lv.shape[2], 4):
            s = s + (((lv[:, :, i] + lv[:, :, i + 1]) + lv[:, :, i + 2]) + lv[:, :, i + 3])
    else:
        for k in range(lv.shape[2]):
            s = s + lv[:, :, k]
    return _wave_sum(s)


def emulate(inp, res, dy16, dy2, g, eps=EPS, m=None, old_dg=None, old_db=None, mutation=None):
    """The kernel's dataflow in numpy, every operation rounded to fp32 (no fused multiply-add): returns (dx16 float16 [m, H], dx32 float32
    [m, H], dg float32 [H], db float32 [H]).

    mutation (None: the correct dataflow) switches ONE defect on, for the tests that prove the bound notices it:
    no_c1 / no_c2: the mean term left out of dx; no_rstd: dx without the factor rstd; no_g: a = dy; stats_without_residual: mu and rstd from
    `inp` alone; no_eps: rstd = var^-1/2; dg_from_x: dg = sum dy x; dy2_dropped: dy = dy16; extra_row: row m (which exists in the buffers) taken
    as valid for dg and db; missing_row: row m - 1 left out of them; drop_last_chunk: the last chunk's partial never added (S > 1);
    accumulate_ignored: the old value not added."""
    assert mutation is None or mutation in MUTATIONS
    f32 = np.float32
    M, H = inp.shape
    m = M if m is None else min(max(int(m), 0), M)
    S, rpc = chunks(M, H)
    me = m
    if mutation == "extra_row":
        me = min(m + 1, M)
    elif mutation == "missing_row":
        me = max(m - 1, 0)
    x = inp[:me].astype(f32)
    xs = x
    if res is not None:
        x = x + res[:me].astype(f32)
        if mutation != "stats_without_residual":
            xs = x
    dy = None
    for part in ((dy16,) if mutation == "dy2_dropped" and dy16 is not None else (dy16, dy2)):
        if part is not None:
            dy = part[:me].astype(f32) if dy is None else dy + part[:me].astype(f32)
    gf = np.asarray(g, f32)
    xl, vec = _lane_view(xs)
    Hf = f32(H)
    with np.errstate(all="ignore"):
        mu = _row_sum(xl, vec, True) / Hf
        dl = xl - mu[:, :, None]
        var = _row_sum(dl * dl, vec, False) / Hf
        rstd = (f32(1) / np.sqrt((var if mutation == "no_eps" else var + f32(eps)).astype(np.float64))).astype(f32)
        xh = (xs - mu) * rstd
        a = dy if mutation == "no_g" else dy * gf
        c1 = _row_sum(_lane_view(a)[0], vec, False) / Hf
        c2 = _row_sum(_lane_view(a * xh)[0], vec, False) / Hf
        w = a if mutation == "no_c1" else a - c1
        if mutation != "no_c2":
            w = w - xh * c2
        dx32 = (w if mutation == "no_rstd" else rstd * w).astype(f32)[:m]
        if dx32.shape[0] < m:
            dx32 = np.concatenate([dx32, np.zeros((m - dx32.shape[0], H), f32)])
        dx16 = dx32.astype(np.float16)
        tg = dy * (x if mutation == "dg_from_x" else xh)
        # wave w of chunk c adds rows c * rpc + w, + 4, ... in order; waves in order; the chunks strand by strand (S = 1: the one chunk's sum is the
        # result), the strands in order; the old value last
        pad = S * rpc - me
        tg_p = np.concatenate([tg, np.zeros((pad, H), f32)]).reshape(S, rpc // WAVES, WAVES, H)
        dy_p = np.concatenate([dy, np.zeros((pad, H), f32)]).reshape(S, rpc // WAVES, WAVES, H)
        wg, wb = np.zeros((S, WAVES, H), f32), np.zeros((S, WAVES, H), f32)
        for k in range(rpc // WAVES):
            wg, wb = wg + tg_p[:, k], wb + dy_p[:, k]
        pg = ((wg[:, 0] + wg[:, 1]) + wg[:, 2]) + wg[:, 3]
        pb = ((wb[:, 0] + wb[:, 1]) + wb[:, 2]) + wb[:, 3]
        last = S - 1 if mutation == "drop_last_chunk" and S > 1 else S
        dg = db = None
        for j in range(min(STRANDS, S)):
            sg, sb = np.zeros(H, f32), np.zeros(H, f32)
            for c in range(j, last, STRANDS):
                sg, sb = sg + pg[c], sb + pb[c]
            dg, db = (sg, sb) if dg is None else (dg + sg, db + sb)
        if mutation != "accumulate_ignored":
            if old_dg is not None:
                dg = dg + old_dg.astype(f32)
            if old_db is not None:
                db = db + old_db.astype(f32)
    return dx16, dx32, dg, db


# ---- makers --------------------------------------------------------------------------------------------------------------------------------
def _rows(family, rng, M, H):
    if family == "unit":
        return rng.standard_normal((M, H))
    if family == "mean30":  # the cancellation case
        return rng.standard_normal((M, H)) + 30.0
    if family == "const":   # var = 0: rstd = eps^-1/2
        return np.full((M, H), 2.0)
    if family == "outlier40":
        x = np.full((M, H), 0.01)
        x[np.arange(M), rng.integers(0, H, M)] = 40.0
        return x
    if family == "small_1e-3":
        return 1e-3 * rng.standard_normal((M, H))
    raise ValueError(family)


def make_case(family, combo, M, H, seed, dy_scale=1.0):
    """dict(inp, res, dy16, dy2, g) for one of COMBOS: x = inp + res keeps the family's character (the residual is a small N(0, 1) * 2^-4
    perturbation in the family's scale, except for the constant rows, where it is the constant 1); dy = dy16 + dy2 is N(0, 1) * dy_scale in
    sum, split in halves when both are given."""
    in_type, residual, has16, dy2_type = combo
    rng = np.random.default_rng([seed, M, H, sum(map(ord, family + in_type + residual + str(has16) + str(dy2_type)))])
    x = _rows(family, rng, M, H)
    inp = x.astype(np.float16 if in_type == "f16" else np.float32)
    res = None
    if residual != "none":
        r = np.ones((M, H)) if family == "const" else (1e-3 if family == "small_1e-3" else 1.0) * 0.0625 * rng.standard_normal((M, H))
        res = r.astype(np.float16 if residual == "res16" else np.float32)
    g = (1.0 + 0.3 * rng.standard_normal(H)).astype(np.float32)
    d = dy_scale * rng.standard_normal((M, H))
    dy16 = dy2 = None
    if has16 and dy2_type:
        dy16, d = (0.5 * d).astype(np.float16), 0.5 * d
    elif has16:
        dy16 = d.astype(np.float16)
    if dy2_type:
        dy2 = d.astype(np.float16 if dy2_type == "f16" else np.float32)
    return dict(inp=inp, res=res, dy16=dy16, dy2=dy2, g=g)

