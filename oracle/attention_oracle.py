"""Host restatement of ONE attention call (mdr_test_attention, include/mdr_hip.h): an fp64 reference, a derived elementwise error
bound, an fp32 / fp16 emulation of each kernel's dataflow (with switchable mutations), and the designed input families the host and
GPU tests share. numpy only; nothing here is measured from a kernel.

Layout (the hook's): qkv is float16 [T, 3 * hidden], a token's row is Q | K | V, head h owns columns 64 h .. 64 h + 63 of each part;
cu is int [B + 1]; sequence b owns rows cu[b] .. cu[b + 1] - 1. Kernels: 1 one-shot, 2 ring, 3 CLS (query 0 of each sequence only:
outputs are [B, hidden] instead of [T, hidden]).

The bound
---------
u = 2^-24 (fp32 half ulp), h = 2^-11 (fp16 half ulp of a normal), z = 2^-25 (half the fp16 subnormal spacing: the absolute rounding
error of a value below 2^-14), n = keys of the sequence, npad = n rounded up to whole pair-tiles of 32, d = 64. For one query, fp64:
s_j = q.k_j / 8, M = max s, w_j = exp(s_j - M), W = sum w, p_j = w_j / W, ref_c = sum_j p_j v_jc. The device's result is
sum_j P_j v_jc (up to accumulation and the last rounding), P_j the weight key j really gets, and

    |out - ref|_c  <=  sum_j |v_jc| dP_j  +  acc_c  +  fin_c,      dP_j >= |P_j - p_j|.

1. Operands are fp16: exact. Products of two fp16 are exact in fp32 (22 bits).
2. Scores: 64 products accumulated in fp32 in some order (MFMA, or the CLS kernel's fma chain):
   |ds_j| <= g64 sum_i |q_i k_ji| / 8, g64 = 64 u / (1 - 64 u). If q and k sit on grids 2^-a, 2^-b with
   sum |q_i k_ji| 2^(a+b) <= 2^24, every partial sum in any order is an integer of at most 24 bits in grid units: ds = 0 (the scores
   of the grid families are bit-known). The factor 1/8 is exact. A common shift of all scores (the device's own maximum) cancels.
3. exp. Kernels 1, 3: x = fl(s - mx), t = fl(x * fl(log2 e)), e = v_exp_f32(t): relative error of e <= 3 u (M - s_j + 2 max ds) + X.
   X = 2^-23: the ISA documents v_exp_f32 (and v_rcp_f32) as accurate to 1 ulp. Kernel 2, job J (keys 96 J .. 96 J + 95), running
   maximum m_J: t = fma(s, fl(log2 e), fl(-m_J fl(log2 e))): the rounding of the second product is u |m_J| log2 e absolute, the fma and
   the constant each u |t| relative: relative error of e_j = exp(s_j - m_J) <= u |m_J| + 2 u (m_J - s_j + 2 max ds) + X. Every later
   job J' multiplies numerator and denominator alike by alpha_J' = exp2f(fl(fl(m_J'-1 - m_J') fl(log2 e))): relative error
   3 u (m_J' - m_J'-1) + X, and 2 u for the two products o * alpha, l * alpha that round apart. exp(ds_j) - 1 is added for the score
   error. The sum is A_j, the relative error of key j's unrounded weight; v_exp_f32 flushes results below 2^-126: absorbed in z.
4. Sum and reciprocal: n positive terms added in fp32 in some order, plus the l * alpha + csum updates: relative error
   <= (1 + u)^(npad + 4 jobs + 8) - 1; the reciprocal X, the product with it u: together C. The perturbed weights themselves move the
   sum by at most Abar = sum_k p_k A_k. So the unrounded normalised weight has relative error th_j = (1 + A_j)(1 + C) / (1 - Abar) - 1.
5. The fp16 rounding of p. Kernels 1, 3 round the NORMALISED p: r_j = h p_j (1 + th_j) if that is >= 2^-14, else z.
   Kernel 2 rounds e_j = exp(s_j - m_J) <= 1: r_j = h e_j (1 + A_j) or z, and the later alphas and the final 1 / l carry it to
   r_j G_j / W (1 + C) / (1 - Abar) (1 + max A), G_j = exp(m_J - M). This is the absolute term of fp16-subnormal probabilities: up to
   2^-25 per key, times |v|. dP_j = p_j th_j + that.
6. P.V accumulation in fp32: acc_c = a sum_j (p_j + dP_j) |v_jc|. MFMA kernels: a = npad 2^-23 + jobs u -- the rounding of the MFMA's
   internal adds is not documented as nearest-even, a truncating add errs by a whole ulp = 2^-23; + u per o *= alpha. CLS kernel: an
   fma chain, a = n u.
7. The output's fp16 rounding: fin_c = h y if y >= 2^-14 else z, y = |ref_c| + everything above.

Every constant is a format's (2^-11, 2^-14, 2^-24, 2^-23 = one fp32 ulp, 2^-25), a count (64, n, npad, jobs) or the ISA's 1 ulp for
v_exp_f32 / v_rcp_f32; no term was taken from an fp32 CPU restatement or from a device run.
"""
import numpy as np

from oracle.fp import H16, LOG2E32, N16, U32, X1ULP, Z16, exp2_32, fma32

JOB = 96
PAIR = 32

MUTATIONS = ("a_extra_key", "b_drop_last", "c_swap_v", "d_skip_o_rescale", "e_skip_l_rescale", "f_patch_prev", "f_patch_none", "g_next_head_k",
             "h_first_block_q", "i_job_shift")


def split(qkv, cu, heads, b):
    """Q, K, V of sequence b as [heads, n, 64] (dtype of qkv)."""
    hidden = 64 * heads
    rows = qkv[int(cu[b]):int(cu[b + 1])]
    n = rows.shape[0]
    return tuple(rows[:, i * hidden:(i + 1) * hidden].reshape(n, heads, 64).transpose(1, 0, 2) for i in range(3))


def _out(cu, heads, kernel, dtype):
    B = len(cu) - 1
    return np.zeros((B if kernel == 3 else int(cu[-1]), 64 * heads), dtype)


def _store(out, cu, b, kernel, o):  # o: [heads, nq, 64]
    hn, nq, _ = o.shape
    if kernel == 3:
        out[b] = o[:, 0].reshape(-1)
    else:
        out[int(cu[b]):int(cu[b + 1])] = o.transpose(1, 0, 2).reshape(nq, hn * 64)


def _grid_exponent(x):
    """Smallest a with x * 2^a all integers (fp16 inputs: a <= 24)."""
    for a in range(0, 25):
        y = x * 2.0 ** a
        if np.array_equal(y, np.rint(y)):
            return a
    return None


def reference_and_bound(qkv, cu, heads, kernel):
    """(reference, bound) of kernel 1, 2 or 3: float64 [T, hidden] ([B, hidden] for kernel 3). See the module docstring."""
    assert kernel in (1, 2, 3)
    ref, bnd = _out(cu, heads, kernel, np.float64), _out(cu, heads, kernel, np.float64)
    for b in range(len(cu) - 1):
        Q, K, V = (x.astype(np.float64) for x in split(qkv, cu, heads, b))
        if kernel == 3:
            Q = Q[:, :1]
        n = K.shape[1]
        njobs = (n + JOB - 1) // JOB if kernel == 2 else 1
        npad = (n + PAIR - 1) // PAIR * PAIR
        S = Q @ K.transpose(0, 2, 1) / 8.0                      # [h, nq, n]
        absS = np.abs(Q) @ np.abs(K).transpose(0, 2, 1) / 8.0
        a, bb = _grid_exponent(Q), _grid_exponent(K)
        exact = a is not None and bb is not None and absS.max() * 8.0 * 2.0 ** (a + bb) <= 2.0 ** 24
        g64 = 64 * U32 / (1 - 64 * U32)
        dS = np.zeros_like(S) if exact else g64 * absS
        dSmax = dS.max(axis=2, keepdims=True)
        M = S.max(axis=2, keepdims=True)
        w = np.exp(S - M)
        W = w.sum(axis=2, keepdims=True)
        p = w / W
        if kernel == 2:
            job = np.arange(n) // JOB
            mj = np.stack([S[:, :, :min(n, (j + 1) * JOB)].max(axis=2) for j in range(njobs)], axis=2)  # running maximum after job j
            step = np.zeros_like(mj)
            step[:, :, 1:] = 3 * U32 * (mj[:, :, 1:] - mj[:, :, :-1]) + X1ULP + 2 * U32                 # what job j's alpha adds to earlier keys
            later = step[:, :, ::-1].cumsum(axis=2)[:, :, ::-1] - step                                  # sum over jobs after j
            mk = mj[:, :, job]                                                                          # m_J of each key's job
            e = np.exp(S - mk)
            Aexp = U32 * np.abs(mk) + 2 * U32 * (mk - S + 2 * dSmax) + X1ULP
            A = np.expm1(dS) + Aexp + later[:, :, job]
        else:
            A = np.expm1(dS) + 3 * U32 * (M - S + 2 * dSmax) + X1ULP
        C = (1 + U32) ** (npad + 4 * njobs + 8) * (1 + X1ULP) * (1 + U32) - 1
        Abar = (p * A).sum(axis=2, keepdims=True)
        th = (1 + A) * (1 + C) / (1 - Abar) - 1
        if kernel == 2:
            ehi = e * (1 + np.expm1(dS) + Aexp)
            r = np.where(ehi >= N16, H16 * ehi, Z16)
            r = r * np.exp(mk - M) / W * (1 + C) / (1 - Abar) * (1 + A.max(axis=2, keepdims=True))
        else:
            phi = p * (1 + th)
            r = np.where(phi >= N16, H16 * phi, Z16)
        dP = p * th + r
        acc_c = (n * U32) if kernel == 3 else (npad * X1ULP + njobs * U32)
        absV = np.abs(V)
        o = p @ V
        err = dP @ absV + acc_c * ((p + dP) @ absV)
        y = np.abs(o) + err
        err = err + np.where(y >= N16, H16 * y, Z16)
        _store(ref, cu, b, kernel, o)
        _store(bnd, cu, b, kernel, err)
    return ref, bnd


def reference(qkv, cu, heads):
    """fp64 softmax(Q K^T / 8) V per (sequence, head) on the fp16 values widened: float64 [T, hidden]."""
    out = _out(cu, heads, 1, np.float64)
    for b in range(len(cu) - 1):
        Q, K, V = (x.astype(np.float64) for x in split(qkv, cu, heads, b))
        S = Q @ K.transpose(0, 2, 1) / 8.0
        w = np.exp(S - S.max(axis=2, keepdims=True))
        _store(out, cu, b, 1, (w / w.sum(axis=2, keepdims=True)) @ V)
    return out


def bound(qkv, cu, heads, kernel):
    """Elementwise bound on |device - reference| for kernel 1, 2 or 3 (module docstring): float64, shaped like the kernel's output."""
    return reference_and_bound(qkv, cu, heads, kernel)[1]


def cls_rows(x, cu):
    """Rows of a [T, hidden] array that kernel 3 produces: the first query of each sequence."""
    return x[np.asarray(cu[:-1], dtype=np.int64)]


def locator(cu, kernel):
    """index (row, column) of a kernel's output -> "sequence b, len n, head h": the `where` of fp.assert_within"""
    def where(at):
        b = at[0] if kernel == 3 else int(np.searchsorted(cu, at[0], side="right") - 1)
        return f"sequence {b}, len {int(cu[b + 1] - cu[b])}, head {at[1] // 64}"
    return where


def emulate(qkv, cu, heads, kernel, mutation=None, mut_job=1):
    """The kernels' dataflow in numpy: fp32 scores, raw exp2 of the scaled difference, fp16 p at the kernel's rounding point (normalised for
    kernels 1 and 3, unnormalised per job of 96 keys with the running (max, sum) rescale for kernel 2, whose ragged last pair-tile holds clamped
    copies of the last row behind a -inf patch), fp32 P.V, fp16 output. float16, shaped like the kernel's output.

    mutation (None: the correct dataflow) switches ONE defect on, for the tests that prove the bound notices it:
    a_extra_key: the key just past len counted (kernel 2: the clamped copy of the last row, unmasked; kernels 1, 3: a zero row);
    b_drop_last: the last key dropped; c_swap_v: V rows of keys 32 t + 1 and 32 t + 17 swapped in the last pair-tile that holds both;
    d_skip_o_rescale / e_skip_l_rescale: o *= alpha / l *= alpha skipped at job mut_job (kernel 2); f_patch_prev: the -inf patch of a ragged job
    applied one pair-tile early (valid keys lost, clamped copies counted); f_patch_none: no patch; g_next_head_k: head h reads the K of head
    h + 1 (cyclic); h_first_block_q: queries 128..255 computed from the Q rows 0..127; i_job_shift: every job after the first starts 32 keys late.
    """
    assert kernel in (1, 2, 3) and (mutation is None or mutation in MUTATIONS)
    out = _out(cu, heads, kernel, np.float16)
    f32 = np.float32
    for b in range(len(cu) - 1):
        Q, K, V = (x.astype(f32) for x in split(qkv, cu, heads, b))
        n = K.shape[1]
        if mutation == "g_next_head_k":
            K = np.roll(K, -1, axis=0)
        if mutation == "h_first_block_q" and n > 128:
            Q = Q.copy()
            m = min(n, 256) - 128
            Q[:, 128:128 + m] = Q[:, :m]
        if mutation == "c_swap_v" and n > 17:
            t = (n - 18) // PAIR
            V = V.copy()
            V[:, [PAIR * t + 1, PAIR * t + 17]] = V[:, [PAIR * t + 17, PAIR * t + 1]]
        if kernel == 3:
            Q = Q[:, :1]
        nk = n - 1 if (mutation == "b_drop_last" and n > 1) else n       # keys that count
        if kernel in (1, 3):
            Kp, Vp = K[:, :nk], V[:, :nk]
            if mutation == "a_extra_key":                                # the zero row staged behind the sequence, unmasked
                Kp = np.concatenate([Kp, np.zeros_like(K[:, :1])], axis=1)
                Vp = np.concatenate([Vp, np.zeros_like(V[:, :1])], axis=1)
            s = (Q @ Kp.transpose(0, 2, 1)) * f32(0.125)
            mx = s.max(axis=2, keepdims=True)
            e = exp2_32((s - mx) * LOG2E32)
            inv = f32(1) / e.sum(axis=2, keepdims=True, dtype=f32)
            p16 = (e * inv).astype(np.float16)
            o = p16.astype(f32) @ Vp
            _store(out, cu, b, kernel, o.astype(np.float16))
            continue
        nq = Q.shape[1]
        m_run = np.full((heads, nq, 1), -np.inf, f32)
        l_run = np.zeros((heads, nq, 1), f32)
        o = np.zeros((heads, nq, 64), f32)
        for job in range((n + JOB - 1) // JOB):
            kc0 = job * JOB
            npair = (min(JOB, n - kc0) + PAIR - 1) // PAIR
            idx = kc0 + np.arange(npair * PAIR)                          # the keys the lanes believe they hold
            src = idx + (PAIR if (mutation == "i_job_shift" and job > 0) else 0)
            src = np.minimum(src, n - 1)                                 # staging clamps rows past the sequence to its last row
            s = (Q @ K[:, src].transpose(0, 2, 1)) * f32(0.125)
            dead = idx >= nk
            if mutation == "a_extra_key":
                dead = idx >= nk + 1
            elif mutation == "f_patch_none":
                dead = np.zeros_like(dead)
            elif mutation == "f_patch_prev":
                dead = np.zeros_like(dead)
                if npair >= 2 and kc0 + npair * PAIR > n:
                    lo = (npair - 2) * PAIR
                    dead[lo:lo + PAIR] = idx[lo:lo + PAIR] + PAIR >= n
            s[:, :, dead] = -np.inf
            m_new = np.maximum(m_run, s.max(axis=2, keepdims=True))
            with np.errstate(invalid="ignore"):
                alpha = exp2_32((m_run - m_new) * LOG2E32)              # 0 on the first job
            e = exp2_32(fma32(s, LOG2E32, -m_new * LOG2E32))
            csum = e.sum(axis=2, keepdims=True, dtype=f32)
            skip = job == mut_job
            l_run = (l_run if (mutation == "e_skip_l_rescale" and skip) else l_run * alpha) + csum
            if not (mutation == "d_skip_o_rescale" and skip):
                o = o * alpha
            m_run = m_new
            o = o + e.astype(np.float16).astype(f32) @ V[:, src]
        _store(out, cu, b, kernel, (o * (f32(1) / l_run)).astype(np.float16))
    return out


# ---- designed inputs (tests/test_attention_oracle.py, tests/test_attention_gpu.py) ------------------------------------------------------
def pack(seqs, heads):
    """[(Q, K, V) as [heads, n, 64] each] -> (qkv float16 [T, 3 * hidden], cu int32 [B + 1]); asserts that every value is fp16-exact."""
    rows = []
    for Q, K, V in seqs:
        n = Q.shape[1]
        rows.append(np.concatenate([x.transpose(1, 0, 2).reshape(n, 64 * heads) for x in (Q, K, V)], axis=1))
    qkv64 = np.concatenate(rows)
    qkv = qkv64.astype(np.float16)
    assert np.array_equal(qkv.astype(np.float64), qkv64.astype(np.float64)) or qkv64.dtype == np.float16
    cu = np.concatenate([[0], np.cumsum([s[0].shape[1] for s in seqs])]).astype(np.int32)
    return qkv, cu


def _grid_v(rng, heads, n):
    return rng.integers(-16, 17, size=(heads, n, 64)) / 8.0               # multiples of 1/8 in [-2, 2]


def _codes(heads, n, seed):
    """[heads, n, 64]: key j's +-10 code (the 10 bits of j xor a per-head mask) on 10 dimensions chosen per head; 0 elsewhere."""
    out = np.zeros((heads, n, 64))
    for h in range(heads):
        rng = np.random.default_rng([seed, h, 77])
        dims = rng.permutation(64)[:10]
        j = np.arange(n) ^ int(rng.integers(0, 1024))
        out[h][:, dims] = 20.0 * ((j[:, None] >> np.arange(10)) & 1) - 10.0
    return out


def onehot(lens, heads, seed):
    """One-hot permutation family: q_i = code(pi(i)), k_j = code(j): the winner scores 1000 / 8 = 125, every other key at most 100, so every other
    probability is <= e^-25 < 2^-36 and rounds to fp16 zero, and the fp32 sum is exactly 1. v_j: distinct rows of non-zero multiples of 1/8
    (columns 0, 1 spell j), so that the <= 10 e^-25 |v| that an earlier ring job leaves in o stays below half an fp32 ulp of every entry.
    Returns (qkv, cu, expected float16 [T, hidden]): the output must EQUAL expected."""
    seqs, exp = [], []
    for bi, n in enumerate(lens):
        rng = np.random.default_rng([seed, bi, n])
        K = _codes(heads, n, seed)
        pi = np.stack([rng.permutation(n) for _ in range(heads)])
        Q = np.stack([K[h][pi[h]] for h in range(heads)])
        V = rng.integers(1, 33, size=(heads, n, 64)) / 8.0 * rng.choice([-1.0, 1.0], size=(heads, n, 64))
        V[:, :, 0] = (np.arange(n) % 32 + 1) / 8.0
        V[:, :, 1] = -(np.arange(n) // 32 + 1) / 8.0
        seqs.append((Q, K, V))
        exp.append(np.stack([V[h][pi[h]] for h in range(heads)]).transpose(1, 0, 2).reshape(n, 64 * heads))
    qkv, cu = pack(seqs, heads)
    return qkv, cu, np.concatenate(exp).astype(np.float16)


def uniform_ones(lens, heads, seed):
    """q = 0 (every score 0), v = 1, K seeded grid values."""
    seqs = []
    for bi, n in enumerate(lens):
        rng = np.random.default_rng([seed, bi, n, 1])
        seqs.append((np.zeros((heads, n, 64)), _grid_v(rng, heads, n), np.ones((heads, n, 64))))
    return pack(seqs, heads)


def uniform_ones_expected(n, kernel):
    """The bit-known output for q = 0, v = 1 and n keys. Kernel 2 sums the unnormalised p = 1: o = l = n and fp16(fl32(n fl32(1 / n))) = 1.
    Kernels 1 and 3 round the normalised p first: every partial sum of n copies of fp16(fl32(1 / n)) is exact in fp32 (11 bits times at most
    10), so the output is fp16(n * fp16(fl32(1 / n))) in any order -- 1 for many n, one fp16 step away for others."""
    if kernel == 2:
        return np.float16(1.0)
    p = np.float16(np.float32(1.0) / np.float32(n))
    return np.float16(np.float32(n) * np.float32(p))


def indicator_positions(n):
    """Key 0, the last key, and the first and last key of every job of 96 and every pair-tile of 32, inside a sequence of n keys: <= 64 of them."""
    pos = {0, n - 1}
    for k in range(0, 512, PAIR):
        pos |= {k, k + PAIR - 1}
    for k in range(0, 512, JOB):
        pos |= {k, k + JOB - 1}
    return sorted(x for x in pos if x < n)


def uniform_indicators(lens, heads, seed):
    """q = 0, v[j, c] = [j == pos_c]: column c of the output is 1 / len for each designed position pos_c (indicator_positions), 0 beyond them."""
    seqs = []
    for bi, n in enumerate(lens):
        rng = np.random.default_rng([seed, bi, n, 2])
        V = np.zeros((heads, n, 64))
        for c, j in enumerate(indicator_positions(n)):
            V[:, j, c] = 1.0
        seqs.append((np.zeros((heads, n, 64)), _grid_v(rng, heads, n), V))
    return pack(seqs, heads)


def staircase(lens, heads, seed, slope):
    """Scores slope * j for every query (slope = +-0.25): q = (8 slope) e_0, k_j = j e_0 + seeded grid values on the dimensions q does not touch.
    Rising: every ring job lifts the running maximum by 24 (alpha ~ e^-24). Falling: the maximum is key 0 and later jobs are fp16-subnormal / 0."""
    seqs = []
    for bi, n in enumerate(lens):
        rng = np.random.default_rng([seed, bi, n, 3])
        Q = np.zeros((heads, n, 64))
        Q[:, :, 0] = 8.0 * slope
        K = _grid_v(rng, heads, n)
        K[:, :, 0] = np.arange(n)
        seqs.append((Q, K, _grid_v(rng, heads, n)))
    return pack(seqs, heads)


def spike_positions(n):
    """The first, middle and last key of every job of 96 (clipped to the sequence: the ragged last pair-tile's last key included)."""
    pos = {n - 1}
    for k in range(0, n, JOB):
        pos |= {k, min(k + JOB // 2, n - 1), min(k + JOB - 1, n - 1)}
    return sorted(pos)


def spike(lens, heads, seed, height):
    """Query i scores `height` on key pos[i % len(pos)] (spike_positions) and 0 on every other key: k_pos[c] = e_c, every other k = e_63,
    q_i = 8 height e_(i % len(pos)). height 8: old jobs survive a rescale by e^-8; 16: e^-16 is fp16-subnormal."""
    seqs = []
    for bi, n in enumerate(lens):
        rng = np.random.default_rng([seed, bi, n, 4])
        pos = spike_positions(n)
        K = np.zeros((heads, n, 64))
        K[:, :, 63] = 1.0
        for c, j in enumerate(pos):
            K[:, j, 63] = 0.0
            K[:, j, c] = 1.0
        Q = np.zeros((heads, n, 64))
        Q[:, np.arange(n), np.arange(n) % len(pos)] = 8.0 * height
        seqs.append((Q, K, _grid_v(rng, heads, n)))
    return pack(seqs, heads)


def realistic(lens, heads, seed, scale):
    """Seeded N(0, 1) Q, K, V rounded to fp16, Q times `scale`: scores of standard deviation `scale` (sqrt(64) / 8 = 1)."""
    seqs = []
    for bi, n in enumerate(lens):
        rng = np.random.default_rng([seed, bi, n, 5])
        Q, K, V = (rng.standard_normal((heads, n, 64)).astype(np.float16) for _ in range(3))
        seqs.append(((Q.astype(np.float32) * scale).astype(np.float16), K, V))
    return pack(seqs, heads)


# name -> builder(lens, heads, seed) of (qkv, cu); the bound-compared families
FAMILIES = {
    "uniform_indicators": uniform_indicators,
    "stair_up": lambda lens, heads, seed: staircase(lens, heads, seed, 0.25),
    "stair_down": lambda lens, heads, seed: staircase(lens, heads, seed, -0.25),
    "spike8": lambda lens, heads, seed: spike(lens, heads, seed, 8.0),
    "spike16": lambda lens, heads, seed: spike(lens, heads, seed, 16.0),
    "realistic1": lambda lens, heads, seed: realistic(lens, heads, seed, 1.0),
    "realistic4": lambda lens, heads, seed: realistic(lens, heads, seed, 4.0),
}
