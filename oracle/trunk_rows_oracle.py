"""oracle/trunk_rows_oracle.py -- TEST INFRASTRUCTURE, NOT PRODUCT CODE. numpy only; never imports the package under test.

The plain statement of the trunk's packing, embedding, LayerNorm and row kernels (csrc/mdr_encoder_pack_ln.inl and reader_embed_ln_kernel in
csrc/mdr_reader.inl), the derived bound on what a correct fp32 implementation may differ from it, the assertions both
tests/test_trunk_rows_oracle.py (host) and tests/test_trunk_rows_gpu.py (device) apply, and the input families they share.

Integer results (compared for equality)
    lens     (mask != 0).sum(1): any non-zero value is a token
    cu       exclusive scan of lens, cu[B] = total
    order    sequences longest first, ties by lower index
    tok_src  flatnonzero(mask), row-major
    tok_pid  HF create_position_ids_from_input_ids over the WHOLE row from ids != pad_id, sampled at the masked-in positions: the inclusive
             count of non-pad ids up to the position + pad_id where the id is not pad, pad_id where it is

Float results: fp64 from the same fp32 / fp16 inputs
    x = (word[clamp(id)] + pos[clamp(pid)]) + type[ty]      (embeddings)          x = in + residual      (LayerNorm)
    mu = mean(x), var = mean((x - mu)^2) (biased),  y = (x - mu) * (var + eps)^-1/2 * g + b

bound(): what |kernel - fp64| may be, elementwise, for the fp32 outputs
-----------------------------------------------------------------------
u = 2^-24 (fp32 unit roundoff, round to nearest). The kernels' documented arithmetic: x in fp32 with one rounded add per term joined (two for
the embeddings: (w + p) + t); the sum of the H <= 1024 values of a row per lane first (H / 64 terms in sequence; the 16-byte path adds groups of
four) and then over a 6-level butterfly, so every term passes through at most D = H / 64 + 6 additions; mu = sum / H; the TWO-PASS variance
sum((x - mu)^2) in the same order; rstd = rsqrtf(var + eps); y = ((x - mu) * rstd) * g + b with the last multiply-add fused or not. The
derivation (first order in u; the neglected products of two error terms are covered by the final factor 1 + 2^-10):

  dx_i    |x^_i - x_i| <= u |x_i| for one rounded add, u |w + p| + u |x_i| for the embeddings, 0 where nothing is added (the caller passes it:
          ln_inputs / embed_inputs compute it)
  dmu     |mu^ - mu| <= mean(dx) + D u mean|x| + 3 u |mu|          (summation: D u sum|x|; the division: 3 u, which also covers a division that
                                                                    is not correctly rounded)
  the deviations d_i = x_i - mu: d^_i = fl(x^_i - mu^) = d_i + c + e_i with a COMMON part |c| <= dmu and an elementwise part
          e_i <= dx_i + u (|d_i| + dmu + dx_i)
  A = var + eps: sum d^_i^2 - sum d_i^2 = sum (2 d_i (c + e_i) + (c + e_i)^2), and sum d_i c = 0 exactly, so
          |A^ - A| / A <= rho_A = [2 mean(|d| e) + mean((dmu + e)^2)] / A + (D + 5) u
          ((D + 5) u: the squares, the D additions, the division by H and the addition of eps, all on non-negative terms, hence relative)
  rstd    v_rsq_f32 is accurate to 1 ulp = 2 u relative (AMD Instinct CDNA3 / CDNA4 ISA reference guide, V_RSQ_F32: "1ULP accuracy"; rsqrtf
          lowers to it, with an exact power-of-two rescale around it for denormal arguments). So r^ / r lies in
          [(1 + rho_A)^-1/2 (1 - 2u), (1 - rho_A)^-1/2 (1 + 2u)]; rho_r is the larger distance of the two ends from 1 (infinite if rho_A >= 1: the
          bound then says nothing, and the tests assert that no family gets there)
  t = d r |t^ - t_i| <= dt_i = r (dmu + e_i)(1 + rho_r) + |t_i| (rho_r + u)
  y       |y^ - y_i| <= |g_i| dt_i + u |g_i| (|t_i| + dt_i) + u (|y_i| + |g_i| dt_i)      (unfused: two roundings; fused: only the last)

It grows with |mu| / sigma (dmu r ~ D u |mu| / sigma), with max |x| (dx, mean|x|) and with |g|, as it must. No term was read off a device.
The host test records how much of it a second correct fp32 implementation uses.

fp16 outputs: the expected value is RNE16(fp64 result); the kernel rounds its fp32 y once, so by monotonicity its output lies between
RNE16(ref - bound) and RNE16(ref + bound). Accepted: the expected value, bit for bit, or -- only where ref +- bound straddles a rounding boundary on
that side -- the fp16 value behind that boundary. Nothing else: where the interval straddles no boundary (lo == hi) the bits must be those of
RNE16(ref), signed zeros included.
Correction to the first statement of this rule ("the ONE neighbouring value"): for |y| below about 2^11 * bound the fp16 spacing is finer than the
bound itself (unit-scale outputs near zero; rows with a mean of 100 or 1000, whose bound is 1e-4 .. 1e-3), the interval then crosses several
boundaries and a correctly rounded fp32 implementation lands two or more fp16 steps from RNE16(ref) -- the host test's second implementation did,
at 11 % of the bound. The rule is therefore stated by what monotonicity of the rounding proves: RNE16(ref - bound) <= output <= RNE16(ref + bound).
Where the interval crosses at most one boundary this IS the one-neighbour rule.
"""
import numpy as np

from oracle import fp
from oracle.fp import U32


# ---- integer results ---------------------------------------------------------------------------------------------------------------------
def lens(mask):
    return (np.asarray(mask) != 0).sum(1).astype(np.int32)


def cu(mask):
    return np.concatenate([[0], np.cumsum(lens(mask), dtype=np.int64)]).astype(np.int32)


def order(mask):
    n = lens(mask).astype(np.int64)
    return np.asarray(sorted(range(len(n)), key=lambda i: (-n[i], i)), np.int32)


def tok_src(mask):
    return np.flatnonzero(np.asarray(mask).reshape(-1) != 0).astype(np.int32)


def position_ids_full(ids, pad_id):
    """[B, L]: the position id of every position of the row (position_ids_loop below says the same one position at a time)."""
    notpad = np.asarray(ids) != pad_id
    return np.where(notpad, np.cumsum(notpad, axis=1) + pad_id, pad_id).astype(np.int64)


def position_ids_loop(ids, pad_id):
    ids = np.asarray(ids)
    out = np.full(ids.shape, pad_id, np.int64)
    for b in range(ids.shape[0]):
        count = 0
        for p in range(ids.shape[1]):
            if ids[b, p] != pad_id:
                count += 1
                out[b, p] = count + pad_id
    return out


def tok_pid(ids, mask, pad_id):
    return position_ids_full(ids, pad_id).reshape(-1)[tok_src(mask)].astype(np.int32)


def pack(ids, mask, pad_id):
    c = cu(mask)
    return dict(lens=lens(mask), cu=c, total=np.asarray([c[-1]], np.int32), order=order(mask), tok_src=tok_src(mask), tok_pid=tok_pid(ids, mask, pad_id))


# ---- float results -----------------------------------------------------------------------------------------------------------------------
def layer_norm(x, g, b, eps):
    x = np.asarray(x, np.float64)
    mu = x.sum(-1, keepdims=True) / x.shape[-1]
    d = x - mu
    var = (d * d).sum(-1, keepdims=True) / x.shape[-1]
    return d / np.sqrt(var + np.float64(eps)) * np.asarray(g, np.float64) + np.asarray(b, np.float64)


def ln_inputs(inp, res=None):
    """-> (x, dx): the exact fp64 x = in + residual and the bound on the kernel's fp32 x (one rounded add, none without a residual)."""
    x = np.asarray(inp).astype(np.float64)
    if res is None:
        return x, np.zeros_like(x)
    x = x + np.asarray(res).astype(np.float64)
    return x, U32 * np.abs(x)


def embed_rows(ids_flat, src, pid, word, pos, typ, ty=None, reader_L=None):
    """The table rows a kernel must read for packed tokens with source indices `src`: (word row, position row, type row) indices.
    RoBERTa flavour (reader_L None): position min(pid, max_pos - 1), type row 0. Reader flavour: position src % L, type clamp(ty[src])."""
    src = np.asarray(src, np.int64)
    wid = np.clip(np.asarray(ids_flat, np.int64)[src], 0, word.shape[0] - 1)
    if reader_L is None:
        return wid, np.minimum(np.asarray(pid, np.int64), pos.shape[0] - 1), np.zeros_like(wid)
    tid = np.zeros_like(wid) if ty is None else np.clip(np.asarray(ty, np.int64).reshape(-1)[src], 0, typ.shape[0] - 1)
    return wid, src % reader_L, tid


def embed_inputs(word, pos, typ, wid, prow, trow):
    """-> (x, dx) for x = (word[wid] + pos[prow]) + type[trow]: two rounded adds."""
    w, p, t = (np.asarray(a).astype(np.float64) for a in (word[wid], pos[prow], typ[trow]))
    x = w + p + t
    return x, U32 * np.abs(w + p) + U32 * np.abs(x)


def bound(x, dx, g, b, eps):
    """Elementwise bound on |kernel fp32 output - layer_norm(x, g, b, eps)|; the module docstring derives it."""
    x = np.asarray(x, np.float64)
    H = x.shape[-1]
    g, b, eps = np.asarray(g, np.float64), np.asarray(b, np.float64), np.float64(eps)
    D = H // 64 + 6
    mean = lambda a: a.sum(-1, keepdims=True) / H  # noqa: E731
    mu = mean(x)
    d = x - mu
    A = mean(d * d) + eps
    r = 1.0 / np.sqrt(A)
    dmu = mean(dx) + D * U32 * mean(np.abs(x)) + 3 * U32 * np.abs(mu)
    e = dx + U32 * (np.abs(d) + dmu + dx)
    rho_A = (2 * mean(np.abs(d) * e) + mean((dmu + e) ** 2)) / A + (D + 5) * U32
    with np.errstate(divide="ignore", invalid="ignore"):
        hi = np.where(rho_A < 1, (1 - np.minimum(rho_A, 1 - 1e-300)) ** -0.5 * (1 + 2 * U32) - 1, np.inf)
    lo = 1 - (1 + rho_A) ** -0.5 * (1 - 2 * U32)
    rho_r = np.maximum(hi, lo)
    t = np.abs(d) * r
    dt = r * (dmu + e) * (1 + rho_r) + t * (rho_r + U32)
    y = np.abs(d * r * g + b)
    ag = np.abs(g)
    return (ag * dt + U32 * ag * (t + dt) + U32 * (y + ag * dt)) * (1 + 2.0 ** -10)


# ---- the assertions both tests apply -------------------------------------------------------------------------------------------------------
def bits16(a):
    return np.ascontiguousarray(np.asarray(a, np.float16)).view(np.uint16)


def assert_f32(got, ref, bnd, label=""):
    """Every element of the fp32 output within the bound. -> the largest share of the bound used."""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == ref.shape, (label, got.dtype, got.shape, ref.shape)
    assert np.isfinite(bnd).all(), f"{label}: the bound says nothing here (rho_A >= 1): not a family to test with"
    worst, i = fp.worst_ratio(got, ref, bnd)
    if not worst <= 1.0:
        raise AssertionError(f"{label}: {int((~(np.abs(got.astype(np.float64) - ref) <= bnd)).sum())} fp32 elements outside the bound; worst {worst:.3g} x at {i}: "
                             f"got {got[i]!r}, reference {ref[i]!r}, bound {bnd[i]:.3e}")
    return worst


def _step16(v, up):
    return np.nextafter(v, np.float16(np.inf) if up else np.float16(-np.inf))


def assert_f16(got, ref, bnd, label=""):
    """Every element of the fp16 output equal to RNE16(ref) bit for bit, or, where ref +- bound crosses rounding boundaries, one of the fp16 values
    between RNE16(ref - bound) and RNE16(ref + bound). -> the number of elements that are not RNE16(ref)."""
    got = np.asarray(got)
    assert got.dtype == np.float16 and got.shape == ref.shape, (label, got.dtype, got.shape, ref.shape)
    assert np.isfinite(bnd).all(), f"{label}: the bound says nothing here (rho_A >= 1)"
    with np.errstate(over="ignore"):
        exp = ref.astype(np.float16)
        lo, hi = (ref - bnd).astype(np.float16), (ref + bnd).astype(np.float16)
    same = bits16(got) == bits16(exp)
    ok = np.where(bits16(lo) == bits16(hi), bits16(got) == bits16(lo), (got >= lo) & (got <= hi))
    if not ok.all():
        i = tuple(int(k) for k in np.argwhere(~ok)[0])
        raise AssertionError(f"{label}: {int((~ok).sum())} fp16 elements are outside [RNE16(reference - bound), RNE16(reference + bound)]; first at {i}: got "
                             f"{float(got[i])!r}, reference {ref[i]!r} -> {float(exp[i])!r}, bound {bnd[i]:.3e}")
    return int((~same).sum())


def assert_ints(got, exp, name, label=""):
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape, (label, name, got.shape, exp.shape)
    if not np.array_equal(got, exp):
        i = int(np.flatnonzero(got.reshape(-1) != exp.reshape(-1))[0])
        raise AssertionError(f"{label}: {name} differs in {int((got != exp).sum())} places; first at {i}: got {int(got.reshape(-1)[i])}, expected {int(exp.reshape(-1)[i])}")


def assert_pack(got, ids, mask, pad_id, sentinel, label=""):
    """got: dict of the hook's buffers, each starting as `sentinel`: lens [B], cu [B + 1], total [1], order [B], tok_src / tok_pid [B * L]."""
    exp = pack(ids, mask, pad_id)
    B, T = len(exp["lens"]), int(exp["total"][0])
    for k in ("lens", "cu", "total"):
        assert_ints(got[k], exp[k], k, label)
    assert_ints(got["order"], exp["order"] if B <= 1024 else np.full(B, sentinel, np.int32), "order", label)
    for k in ("tok_src", "tok_pid"):
        assert_ints(got[k][:T], exp[k], k, label)
        assert_ints(got[k][T:], np.full(len(got[k]) - T, sentinel, np.int32), k + " beyond total", label)


# ---- input families ------------------------------------------------------------------------------------------------------------------------
def _affine(rng, H):
    return (1.0 + 0.3 * rng.standard_normal(H)).astype(np.float32), (0.2 * rng.standard_normal(H)).astype(np.float32)


def _unit(rng, R, H):
    g, b = _affine(rng, H)
    return rng.standard_normal((R, H)).astype(np.float32), g, b


def _small(rng, R, H):
    x, g, b = _unit(rng, R, H)
    return x * np.float32(1e-3), g, b


def _mean(m):
    def f(rng, R, H):
        x, g, b = _unit(rng, R, H)
        return x + np.float32(m), g, b
    return f


def _outlier(rng, R, H):
    x, g, b = _unit(rng, R, H)
    x[np.arange(R), rng.integers(0, H, R)] = 60.0
    return x, g, b


def _const(rng, R, H):
    g, b = _affine(rng, H)
    return np.full((R, H), 2.0, np.float32), g, b


def _gamma_zero_neg(rng, R, H):
    x, g, b = _unit(rng, R, H)
    g[::3] = 0.0
    g[1::3] *= -1.0
    return x, g, b


def _beta_large(rng, R, H):
    x, g, b = _unit(rng, R, H)
    return x, g * np.float32(1e-2), np.full(H, 100.0, np.float32)


def _f16_max(rng, R, H):
    g, b = _affine(rng, H)
    x = rng.choice(np.asarray([65504.0, -65504.0, 1.0, 0.0], np.float32), size=(R, H))
    x[:, 0], x[:, 1] = 65504.0, -65504.0
    return x, g, b


def _f16_subnormal(rng, R, H):
    g, b = _affine(rng, H)
    return (rng.integers(-1023, 1024, (R, H)) * (2 * fp.Z16)).astype(np.float32), g, b  # every fp16 subnormal magnitude is k * 2^-24, k < 1024


# name -> (generator(rng, rows, H) -> (x fp32 [rows, H], g, b), the input types it applies to, the eps values it runs with)
LN_FAMILIES = {
    "unit": (_unit, ("f32", "f16"), (1e-5, 1e-12)),
    "small_1e-3": (_small, ("f32", "f16"), (1e-5,)),            # variance 1e-6 below eps: eps decides the result
    "mean100": (_mean(100.0), ("f32",), (1e-5,)),
    "mean1000": (_mean(1000.0), ("f32",), (1e-5,)),
    "outlier60": (_outlier, ("f32", "f16"), (1e-5,)),
    "const2": (_const, ("f32", "f16"), (1e-5,)),                # d^ = 0 exactly: the output is beta
    "gamma_zero_neg": (_gamma_zero_neg, ("f32", "f16"), (1e-5,)),
    "beta100": (_beta_large, ("f32", "f16"), (1e-12,)),
    "f16_max": (_f16_max, ("f16",), (1e-5,)),
    "f16_subnormal": (_f16_subnormal, ("f16",), (1e-5, 1e-12)),
}


def ln_case(family, in_type, residual, rows, H, seed):
    """-> dict(inp, res, g, b): inp in the input type (float32 / float16), res None / float16 / float32 -- a second draw of the family, so that
    in + residual keeps the family's character (twice the mean, the same scale)."""
    gen = LN_FAMILIES[family][0]
    rng = np.random.default_rng([seed, H, rows, sum(map(ord, family + in_type + residual))])
    x, g, b = gen(rng, rows, H)
    inp = x.astype(np.float16) if in_type == "f16" else x
    res = None
    if residual != "none":
        r = gen(rng, rows, H)[0]
        if family in ("mean100", "mean1000") and residual == "res16":
            r = r - np.float32(1000.0 if family == "mean1000" else 100.0)  # fp16 holds no unit spread around 1000: the residual carries none of the mean
        res = r.astype(np.float16) if residual == "res16" else r
    return dict(inp=inp, res=res, g=g, b=b)


def make_pack_case(kind, B, L, pad_id, seed, mask_kind="prefix"):
    """ids, mask int64 [B, L]. kind: the lengths (random / equal / full / decreasing / increasing / zeros = random with rows of length 0 first, last
    and at index 1023). mask_kind: prefix (right-padded), holes (a random subset of that many positions), values (prefix, mask values 2 and -1).
    ids: random with pad_id sprinkled inside the rows, and NON-pad ids at masked-out positions in front of masked-in ones (holes) and behind."""
    rng = np.random.default_rng([seed, B, L, pad_id, sum(map(ord, kind + mask_kind))])
    if kind == "random":
        n = rng.integers(1, L + 1, B)
    elif kind == "equal":
        n = np.full(B, max(1, L // 2))
    elif kind == "full":
        n = np.full(B, L)
    elif kind == "decreasing":  # strictly, as far as L allows: then ties again
        n = np.maximum(1, L - np.arange(B) % L)
        n = np.sort(n)[::-1] if B <= L else n
    elif kind == "increasing":
        n = 1 + np.arange(B) % L
        n = np.sort(n) if B <= L else n
    elif kind == "zeros":
        n = rng.integers(0, L + 1, B)
        n[0] = n[-1] = 0
        n[::7] = 0
        if B > 1023:
            n[1023] = 0
    else:
        raise ValueError(kind)
    mask = np.zeros((B, L), np.int64)
    for b in range(B):
        where = rng.permutation(L)[:n[b]] if mask_kind == "holes" else np.arange(n[b])
        mask[b, where] = 1
    if mask_kind == "values":
        mask *= rng.choice(np.asarray([1, 2, -1], np.int64), size=mask.shape)
    ids = rng.integers(0, 50, (B, L)).astype(np.int64)
    ids[ids == pad_id] = 7
    ids[rng.random((B, L)) < 0.15] = pad_id  # pad ids anywhere, masked in or not
    return ids, mask


# (B, L, lengths, mask kind, pad_id): every listed B and every listed L, each lengths / mask kind, both pad ids; not the cross product
PACK_CASES = [(1, 1, "random", "prefix", 1), (1, 64, "zeros", "prefix", 1), (3, 63, "random", "holes", 1), (4, 64, "equal", "prefix", 0),
              (5, 65, "zeros", "values", 1), (63, 128, "decreasing", "prefix", 1), (64, 129, "increasing", "holes", 0), (65, 512, "random", "values", 1),
              (1000, 63, "random", "holes", 1), (1023, 64, "equal", "prefix", 1), (1024, 65, "zeros", "prefix", 1), (1024, 128, "full", "prefix", 0),
              (1024, 512, "random", "holes", 1), (1025, 129, "random", "holes", 1), (2049, 64, "zeros", "values", 0), (3000, 65, "random", "prefix", 1),
              (3000, 1, "zeros", "prefix", 1)]


def f16_conversion_values():
    """fp32 values whose conversion to fp16 exercises RNE: every tie midpoint of the binade [1, 2) and of a subnormal stretch (lower neighbours of both
    parities), values just beside the ties, the subnormal range and below, the overflow threshold, zeros, infinities, NaN."""
    k = np.arange(1024, dtype=np.float64)
    ties = 1.0 + (k + 0.5) * 2.0 ** -10
    sub_ties = (np.arange(0, 1024) + 0.5) * (2 * fp.Z16)   # (the fp16 subnormal spacing, 2^-24)
    vals = np.concatenate([ties, -ties, np.nextafter(ties.astype(np.float32), np.float32(0)), np.nextafter(ties.astype(np.float32), np.float32(4)),
                           sub_ties, -sub_ties, np.arange(0, 1024) * (2 * fp.Z16), [2.0 ** -25, np.nextafter(np.float32(2.0 ** -25), np.float32(1)), 2.0 ** -26, 1e-30, 1e-45],
                           [65504.0, -65504.0, 65519.0, -65519.0, 65519.996, 65520.0, -65520.0, 65536.0, 1e38, 0.0, -0.0, np.inf, -np.inf, np.nan]])
    return vals.astype(np.float32)


def assert_f16_conversion(got, src, label=""):
    """Bits equal to numpy's RNE astype(float16); NaN only by NaN-ness."""
    with np.errstate(over="ignore"):
        exp = np.asarray(src, np.float32).astype(np.float16)
    got = np.asarray(got)
    assert got.dtype == np.float16 and got.shape == exp.shape
    nan = np.isnan(exp)
    assert np.array_equal(np.isnan(got), nan), f"{label}: NaN-ness differs"
    bad = (bits16(got) != bits16(exp)) & ~nan
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise AssertionError(f"{label}: {int(bad.sum())} conversions differ; first at {i}: {float(np.asarray(src)[i])!r} -> got {float(got[i])!r}, RNE {float(exp[i])!r}")
