"""Host restatement of ONE attention backward call (mdr_attention_backward, include/mdr_attention_grad.h): the six formulas in fp64, a
derived elementwise error bound, an fp32 / fp16 emulation of the kernels' dataflow (with switchable mutations) and makers for dctx. numpy,
except that the bound's float64 arithmetic goes through torch's CPU kernels, which use every core (the [heads, n, n] terms of a hundred
sequences at twelve heads take half a minute in numpy); nothing here is measured from a kernel. Test helper (tests/test_attention_grad_host.py, tests/test_attention_grad_gpu.py); the input
families for qkv are those of oracle/attention_oracle.py.

Layout: qkv float16 [T, 3 * hidden], a row is Q | K | V, head h in columns 64 h .. 64 h + 63 of each part; cu int [B + 1]; dctx float16
[T, hidden] (mode 0) or [B, hidden] (mode 3: the gradient of each sequence's first query alone). Outputs are [T, 3 * hidden], dQ | dK | dV.

Formulas, per (sequence, head), dO = the head's columns of dctx:
    s = Q K^T / 8    p = softmax(s)    dV = p^T dO    dP = dO V^T    delta_i = sum_j p_ij dP_ij    dS = p o (dP - delta)
    dQ = dS K / 8    dK = dS^T Q / 8

The bound
---------
Derived from the rounding points listed at the top of csrc/mdr_attention_grad.hip. u = 2^-24 (fp32 half ulp), X = 2^-23 (one fp32 ulp: the
rounding of an MFMA's internal adds is not documented as nearest-even, and the ISA documents v_exp_f32 / v_rcp_f32 / v_log_f32 as accurate
to 1 ulp), h = 2^-11 (fp16 half ulp of a normal), z = 2^-25 (half the fp16 subnormal spacing: the absolute rounding error of a value below
2^-14). n = keys of the sequence, npad = n rounded up to whole chunks of 64 (the kernels add zeros for the rows behind the sequence),
c = npad / 64 chunks. Everything below is per query i and key j, in fp64, and each line bounds the absolute error of the device's value.

1. Operands are fp16: exact. A product of two fp16 is exact in fp32.
2. Scores and dP: 64 products added in fp32 in some order, at most one ulp lost per addition:
   ds_ij = 64 X sum_k |q_ik k_jk| / 8,  ddP_ij = 64 X sum_k |dO_ik v_jk|. The factor 1/8 is exact.
3. The row statistics. e_j = v_exp_f32(fma(s_j, log2 e, -m log2 e)) against a running maximum m (|m| <= max_j |s_ij| =: Mabs), rescaled
   by alpha = exp2((m_old - m_new) log2 e) at every later chunk. The argument errs by u |m| log2 e (the rounded product) + 2 u |arg|
   (the constant and the fma), the exp by X; the alphas of the later chunks multiply to exp(m - M) up to 3 u (M - m) + c (X + 2 u). With
   the score error the relative error of key j's weight in the sums is at most
       A_ij = ds_ij + u Mabs + 3 u (M - s_ij + 2 max_j ds_ij) + (c + 1)(X + 2 u).
   The sum of npad terms with c rescales: relative (npad + 4 c + 8) u =: G. So lse = m + logf(sum) errs by
       el_i = 1.01 sum_j p_ij A_ij + G + 4 u (|lse_i| + Mabs + 1)        (first order in A, 1 % for the rest; logf and the addition)
   and delta = (sum of e dP) / sum by
       dd_i = 1.01 [sum_j p_ij ddP_ij + sum_j p_ij |dP_ij| A_ij + (sum_j p_ij |dP_ij|) (sum_j p_ij A_ij + 2 G + 4 u)].
   Mode 3 computes p = e / sum against the true maximum and delta from the same e: every term above covers it (M - s <= lse - s, one
   reciprocal X and one product u against the 4 u above).
4. p_ij = v_exp_f32((s_ij - lse_i) log2 e): relative rp_ij = ds_ij + el_i + 3 u |s_ij - lse_i| + 2 u + X, absolute
   dp_ij = 1.01 p_ij rp_ij + 2^-126 (v_exp_f32 flushes subnormal results).
   dS_ij = p (dP - delta) in fp32: d32_ij = 1.01 [dp_ij |dP_ij - delta_i| + (p_ij + dp_ij)(ddP_ij + dd_i)] + 3 u |dS_ij|.
5. The fp16 roundings of the MFMA operands: r(y) = max(h y, z) for a value of magnitude at most y.
   dp16_ij = dp_ij + r(p_ij + dp_ij),  dS16_ij = d32_ij + r(|dS_ij| + d32_ij).
6. The three contractions accumulate products that are exact in fp32, at most one ulp lost per addition over npad terms (a = npad X):
   dQ_ic: [sum_j dS16_ij |k_jc| + a sum_j (|dS_ij| + dS16_ij) |k_jc|] / 8,    dK_jc: the same over i with |q_ic|,
   dV_jc: sum_i dp16_ij |dO_ic| + a sum_i (p_ij + dp16_ij) |dO_ic|.
7. The output's fp16 rounding: r(|ref| + everything above).

Every constant is a format's, a count, or the ISA's 1 ulp; no term was read off a device or off an fp32 CPU run. The emulation below is a
second implementation of the dataflow: the host test shows that it stays inside the bound and that each mutation leaves it.
"""
import numpy as np
import torch

from oracle.fp import F16_MAX, H16, LOG2E32, U32, X1ULP, Z16, exp2_32, fma32

CHUNK = 64       # swept rows per step of the MFMA kernels, and owners per workgroup
TILE = 16        # rows of an MFMA tile

MUTATIONS = ("extra_key", "drop_last_key", "no_delta", "no_scale_dq", "no_scale_dk", "dk_next_head", "dv_unnormalised", "first_block_do",
             "cls_dq_next_row")


# The lengths the GPU tests pack into one ragged call (the host test runs the emulation over the same ones). One head: every length from 1 to
# twice the block of 64 plus one. Twelve heads, L = 512: -1, 0, +1 around every multiple of the MFMA tile of 16 (the blocks of 64 owners and
# the chunks of 64 swept rows are multiples of it), and the lengths of the reference's training command.
LENS_SWEEP = list(range(1, 2 * CHUNK + 2))
LENS_EDGES = sorted({n for m in range(TILE, 513, TILE) for n in (m - 1, m, m + 1) if n <= 512} | {1, 2, 70, 300, 350, 511, 512})
FAMILY_NAMES = ("realistic1", "realistic4", "spike16", "stair_up", "stair_down")


def split(qkv, cu, heads, b):
    """Q, K, V of sequence b as [heads, n, 64] (dtype of qkv)."""
    hidden = 64 * heads
    rows = qkv[int(cu[b]):int(cu[b + 1])]
    n = rows.shape[0]
    return tuple(rows[:, i * hidden:(i + 1) * hidden].reshape(n, heads, 64).transpose(1, 0, 2) for i in range(3))


def split_do(dctx, cu, heads, b, mode):
    """dO of sequence b as [heads, n, 64] (mode 3: [heads, 1, 64])."""
    rows = dctx[b:b + 1] if mode == 3 else dctx[int(cu[b]):int(cu[b + 1])]
    return rows.reshape(rows.shape[0], heads, 64).transpose(1, 0, 2)


def _store(out, cu, b, heads, dQ, dK, dV):
    n, hidden = dK.shape[1], 64 * heads
    rows = out[int(cu[b]):int(cu[b + 1])]
    for i, x in enumerate((dQ, dK, dV)):
        rows[:x.shape[1], i * hidden:(i + 1) * hidden] = x.transpose(1, 0, 2).reshape(x.shape[1], hidden)
    return n


def _T(x):
    return x.transpose(0, 2, 1)


def reference_and_bound(qkv, dctx, cu, heads, mode=0):
    """(reference, bound): float64 [T, 3 * hidden] each. Mode 3: dQ rows behind a sequence's first are 0 with bound 0 (the kernel writes zeros).
    Asserts that no dS leaves the fp16 range (the bound has no term for an overflow)."""
    assert mode in (0, 3)
    T = int(cu[-1])
    ref, bnd = np.zeros((T, 3 * 64 * heads)), np.zeros((T, 3 * 64 * heads))

    for b in range(len(cu) - 1):
        if cu[b + 1] == cu[b]:
            continue
        Qs, Ks, Vs = (torch.from_numpy(x.astype(np.float64)) for x in split(qkv, cu, heads, b))
        dOs = torch.from_numpy(split_do(dctx, cu, heads, b, mode).astype(np.float64))
        if mode == 3:
            Qs = Qs[:, :1]
        out, err = _one_sequence(Qs, Ks, Vs, dOs)
        _store(ref, cu, b, heads, *out)
        _store(bnd, cu, b, heads, *err)
    return ref, bnd


def _one_sequence(Q, K, V, dO, feed=False):
    """(the three gradients, their three bounds) of one sequence: torch float64 [heads, n, 64] in, numpy out."""
    def amax(x):
        return x.amax(dim=2, keepdim=True)

    def rsum(x):
        return x.sum(dim=2, keepdim=True)

    def r16(y):
        return torch.clamp(H16 * y, min=Z16)

    n = K.shape[1]
    npad = (n + CHUNK - 1) // CHUNK * CHUNK
    c = npad // CHUNK
    aQ, aK, aV, aO = Q.abs(), K.abs(), V.abs(), dO.abs()
    Kt, Vt = K.transpose(1, 2), V.transpose(1, 2)
    S = Q @ Kt / 8.0                                          # [h, nq, n]
    dP = dO @ Vt
    ds = (aQ @ aK.transpose(1, 2)) * (64 * X1ULP / 8.0)
    ddP = (aO @ aV.transpose(1, 2)) * (64 * X1ULP)
    M = amax(S)
    Mabs = amax(S.abs())
    w = torch.exp(S - M)
    W = rsum(w)
    p = w / W
    lse = M + torch.log(W)
    delta = rsum(p * dP)
    dS = p * (dP - delta)
    A = ds + U32 * Mabs + 3 * U32 * (M - S + 2 * amax(ds)) + (c + 1) * (X1ULP + 2 * U32)
    G = (npad + 4 * c + 8) * U32
    pA = rsum(p * A)
    el = 1.01 * pA + G + 4 * U32 * (lse.abs() + Mabs + 1)
    padP = p * dP.abs()
    dd = 1.01 * (rsum(p * ddP) + rsum(padP * A) + rsum(padP) * (pA + 2 * G + 4 * U32))
    rp = ds + el + 3 * U32 * (S - lse).abs() + (2 * U32 + X1ULP)
    dp = 1.01 * p * rp + 2.0 ** -126
    adS = dS.abs()
    d32 = 1.01 * (dp * (dP - delta).abs() + (p + dp) * (ddP + dd)) + 3 * U32 * adS
    assert float((adS + d32).max()) < F16_MAX / 2, "dS leaves the fp16 range: scale dctx down"
    dp16 = dp + r16(p + dp)
    dS16 = d32 + r16(adS + d32)
    a = npad * X1ULP
    out, err = [], []
    for val, e in ((dS @ K / 8.0, (dS16 + a * (adS + dS16)) @ aK / 8.0),
                   (dS.transpose(1, 2) @ Q / 8.0, (dS16 + a * (adS + dS16)).transpose(1, 2) @ aQ / 8.0),
                   (p.transpose(1, 2) @ dO, (dp16 + a * (p + dp16)).transpose(1, 2) @ aO)):
        out.append(val.numpy())
        err.append((e + r16(val.abs() + e)).numpy())
    if feed:  # the fp16 rounding point of dS: the least and the largest magnitude the device's fp32 dS_ij can have in front of it
        return out, err, [[x.amax(dim=2, keepdim=True).expand(-1, -1, 64).numpy(), x.amax(dim=1).unsqueeze(2).expand(-1, -1, 64).numpy(),
                           torch.zeros_like(K).numpy()] for x in (adS - d32, adS + d32)]
    return out, err


def ds_feed(qkv, dctx, cu, heads, mode=0):
    """(lo, hi): float64 [T, 3 * hidden] each, in the outputs' layout. For every dQ | dK element the largest |dS_ij| among the dS that feed it (dQ
    row i: over the keys j; dK row j: over the queries i), less (lo) and plus (hi) the bound d32 of the fp32 dS: with dctx multiplied by a power
    of two s, the fp16 rounding of a dS that feeds the element CERTAINLY overflows if s lo >= 65520 and POSSIBLY if s hi >= 65520. dV is fed
    by p and dO alone and p <= 1 never leaves fp16: 0 there. (tests/overflow_ref.py)"""
    T = int(cu[-1])
    lo, hi = np.zeros((T, 3 * 64 * heads)), np.zeros((T, 3 * 64 * heads))
    for b in range(len(cu) - 1):
        if cu[b + 1] == cu[b]:
            continue
        Qs, Ks, Vs = (torch.from_numpy(x.astype(np.float64)) for x in split(qkv, cu, heads, b))
        dOs = torch.from_numpy(split_do(dctx, cu, heads, b, mode).astype(np.float64))
        _, _, (l, h) = _one_sequence(Qs[:, :1] if mode == 3 else Qs, Ks, Vs, dOs, feed=True)
        _store(lo, cu, b, heads, *l)
        _store(hi, cu, b, heads, *h)
    return lo, hi


def reference(qkv, dctx, cu, heads, mode=0):
    """The six formulas in fp64 on the fp16 values widened: float64 [T, 3 * hidden]."""
    T = int(cu[-1])
    ref = np.zeros((T, 3 * 64 * heads))
    for b in range(len(cu) - 1):
        if cu[b + 1] == cu[b]:
            continue
        Q, K, V = (x.astype(np.float64) for x in split(qkv, cu, heads, b))
        dO = split_do(dctx, cu, heads, b, mode).astype(np.float64)
        if mode == 3:
            Q = Q[:, :1]
        S = Q @ _T(K) / 8.0
        w = np.exp(S - S.max(axis=2, keepdims=True))
        p = w / w.sum(axis=2, keepdims=True)
        dP = dO @ _T(V)
        dS = p * (dP - (p * dP).sum(axis=2, keepdims=True))
        _store(ref, cu, b, heads, dS @ K / 8.0, _T(dS) @ Q / 8.0, _T(p) @ dO)
    return ref


def emulate(qkv, dctx, cu, heads, mode=0, mutation=None):
    """The kernels' dataflow in numpy: fp32 scores and dP, the running (max, sum, sum of e dP) over chunks of 64 keys (mode 3: one pass against the
    true maximum), lse and delta in fp32, p = exp2((s - lse) log2 e), dS = p (dP - delta), fp16 p and dS as contraction operands, fp32
    contractions, the 1/8 on the fp32 sums, fp16 outputs. float16 [T, 3 * hidden].

    mutation (None: the correct dataflow) switches ONE defect on, for the tests that prove the bound notices it:
    extra_key: the zero row staged behind the sequence counted as a key (only where the sequence does not end at a tile edge);
    drop_last_key: the last key left out of the softmax and its dK / dV rows never written; no_delta: dS = p dP;
    no_scale_dq / no_scale_dk: the 1/8 missing; dk_next_head: head h gets the dK of head h + 1 (cyclic);
    dv_unnormalised: dV from e = exp(s - max) instead of p; first_block_do: queries 64 .. 127 contracted with the dO rows of queries 0 .. 63;
    cls_dq_next_row: mode 3 writes dQ at row cu[b] + 1.
    """
    assert mode in (0, 3) and (mutation is None or mutation in MUTATIONS)
    f32 = np.float32
    T = int(cu[-1])
    out = np.zeros((T, 3 * 64 * heads), np.float16)
    for b in range(len(cu) - 1):
        if cu[b + 1] == cu[b]:
            continue
        Q, K, V = (x.astype(f32) for x in split(qkv, cu, heads, b))
        dO = split_do(dctx, cu, heads, b, mode).astype(f32)
        n = K.shape[1]
        if mode == 3:
            Q = Q[:, :1]
        elif mutation == "first_block_do" and n > CHUNK:
            dO = dO.copy()
            m = min(n, 2 * CHUNK) - CHUNK
            dO[:, CHUNK:CHUNK + m] = dO[:, :m]
        nk = n
        Kp, Vp = K, V
        if mutation == "extra_key" and n % TILE:
            Kp = np.concatenate([K, np.zeros_like(K[:, :1])], axis=1)
            Vp = np.concatenate([V, np.zeros_like(V[:, :1])], axis=1)
            nk = n + 1
        elif mutation == "drop_last_key" and n > 1:
            Kp, Vp, nk = K[:, :n - 1], V[:, :n - 1], n - 1
        s = (Q @ _T(Kp)) * f32(0.125)
        dP = dO @ _T(Vp)
        nq = Q.shape[1]
        with np.errstate(invalid="ignore", under="ignore"):
            if mode == 3:
                mx = s.max(axis=2, keepdims=True)
                e = exp2_32((s - mx) * LOG2E32)
                inv = f32(1) / e.sum(axis=2, keepdims=True, dtype=f32)
                delta = (e * dP).sum(axis=2, keepdims=True, dtype=f32) * inv
                p = e * inv
                m_run = mx
            else:
                m_run = np.full((heads, nq, 1), -np.inf, f32)
                l_run = np.zeros((heads, nq, 1), f32)
                d_run = np.zeros((heads, nq, 1), f32)
                for c0 in range(0, nk, CHUNK):
                    sc, dc = s[:, :, c0:c0 + CHUNK], dP[:, :, c0:c0 + CHUNK]
                    m_new = np.maximum(m_run, sc.max(axis=2, keepdims=True))
                    alpha = exp2_32((m_run - m_new) * LOG2E32)
                    e = exp2_32(fma32(sc, LOG2E32, -m_new * LOG2E32))
                    l_run = l_run * alpha + e.sum(axis=2, keepdims=True, dtype=f32)
                    d_run = d_run * alpha + (e * dc).sum(axis=2, keepdims=True, dtype=f32)
                    m_run = m_new
                lse = m_run + np.log(l_run).astype(f32)
                delta = d_run / l_run
                p = exp2_32((s - lse) * LOG2E32)
            if mutation == "no_delta":
                delta = np.zeros_like(delta)
            dS16 = (p * (dP - delta)).astype(np.float16).astype(f32)
            pv = exp2_32((s - m_run) * LOG2E32) if mutation == "dv_unnormalised" else p
            p16 = pv.astype(np.float16).astype(f32)
        dQ = (dS16 @ Kp) * f32(8.0 if mutation == "no_scale_dq" else 0.125)
        dK = (_T(dS16) @ Q) * f32(8.0 if mutation == "no_scale_dk" else 0.125)
        dV = _T(p16) @ dO
        if mutation == "dk_next_head":
            dK = np.roll(dK, -1, axis=0)
        dK, dV = dK[:, :n], dV[:, :n]  # (extra_key: the row behind the sequence is not an output)
        with np.errstate(over="ignore"):
            dQ, dK, dV = (x.astype(np.float16) for x in (dQ, dK, dV))
        if mode == 3 and mutation == "cls_dq_next_row" and n > 1:
            dQ = np.concatenate([np.zeros_like(dQ), dQ], axis=1)
        _store(out, cu, b, heads, dQ, dK, dV)
    return out


# ---- makers for dctx -----------------------------------------------------------------------------------------------------------------------
def dctx_grid(rows, hidden, seed, scale=1.0):
    """float16 [rows, hidden]: seeded multiples of 1/8 in [-2, 2], times `scale` (a power of two: a loss scale riding in the gradient)."""
    rng = np.random.default_rng([seed, rows, hidden, 9])
    return (rng.integers(-16, 17, size=(rows, hidden)) / 8.0 * scale).astype(np.float16)


def dctx_first_rows(dctx_cls, cu, hidden):
    """Mode 3's [B, hidden] gradient spread into mode 0's [T, hidden]: zero except at rows cu[b]."""
    out = np.zeros((int(cu[-1]), hidden), np.float16)
    out[np.asarray(cu[:-1], np.int64)] = dctx_cls
    return out
