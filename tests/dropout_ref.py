"""Host restatement of dropout (include/mdr_dropout.h): a numpy replica of Philox4x32-10, the two site mappings as mask builders, the fp64
model of the dropout attention forward and backward under an explicit mask, a derived elementwise error bound, and an fp32 / fp16 emulation
of the kernels' dataflow with switchable mutations. Test helper (tests/test_dropout_host.py, tests/test_dropout_gpu.py); nothing here is
measured from a kernel. Layouts are those of tests/attention_grad_ref.py; ctx is [T, hidden] (mode 0) or [B, hidden] (mode 3).

The mask
--------
key = (seed & 0xffffffff, seed >> 32); one generator call yields four words = 16 bytes, byte k = (word[k >> 2] >> (8 (k & 3))) & 0xff. An
element is kept iff its byte >= T = floor(256 p + 0.5); a kept element is multiplied by fp32(256 / (256 - T)).
hidden site: element (row, col) <- byte col & 15 of counter (col >> 4, row, 0, site).
attention site: query i, key j, head h, sequence b <- byte 4 (i & 3) + (j & 3) of counter (i >> 2, j >> 2, b * heads + h, site).

The model, per (sequence, head), m the mask factors, dO the head's columns of dctx:
    s = Q K^T / 8    p = softmax(s)    Pd = p o m    ctx = Pd V    dV = Pd^T dO    dP = (dO V^T) o m    delta_i = sum_j p_ij dP_ij
    dS = p o (dP - delta)    dQ = dS K / 8    dK = dS^T Q / 8

The bound
---------
attention_grad_ref's derivation (its points 1 - 7, from the rounding points at the top of csrc/mdr_attention_grad.hip) with the two rounding
points the dropout kernels add (points 7 and 8 of the list in front of attn_drop_fwd_kernel). m is exact: the model multiplies by the same
fp32 scale. u, X, h, z, npad, a = npad X as there.
  a. dP o m is an fp32 product of the fp32 dP and m: ddPm_ij = m_ij ddP_ij + u |dPm_ij|. delta, dS and their bounds dd, d32 are
     attention_grad_ref's with dPm and ddPm in the place of dP and ddP (p itself does not see the mask: lse is the softmax's).
  b. Pd = p o m in fp32: dPd_ij = m_ij dp_ij + u Pd_ij; rounded to fp16 only as an operand: dPd16_ij = dPd_ij + r(Pd_ij + dPd_ij). Pd <= 256
     never leaves fp16.
  c. ctx_ic: sum_j dPd16_ij |v_jc| + a sum_j (Pd_ij + dPd16_ij) |v_jc|; dV_jc: the same over i with |dO_ic|; then the output's fp16 rounding.
     The forward computes lse by the instructions the backward's sweep 0 uses: el_i bounds it in both.
Mode 3 computes p = e / sum against the true maximum and p * m as two fp32 products: covered as in attention_grad_ref's point 3.
"""
import numpy as np
import torch

import attention_grad_ref as agr
from oracle.fp import F16_MAX, H16, LOG2E32, U32, X1ULP, Z16, exp2_32, fma32

CHUNK = agr.CHUNK
M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xffffffff)

MUTATIONS = ("mask_transposed", "mask_next_head", "mask_next_sequence", "no_mask_sweep0", "no_scale_dv", "byte_swapped", "cls_row1", "bh_stride_2",
             "fwd_no_rescale")
# the defects that change the mask itself (attn_masks); the others change what emulate() does with the correct one
MASK_MUTATIONS = ("mask_transposed", "mask_next_head", "mask_next_sequence", "byte_swapped", "cls_row1", "bh_stride_2")
# the defects written for the training geometry (more than two heads, more than three chunks), with host cases of their own in
# tests/test_dropout_host.py: bh_stride_2 is the correct mask at two heads
GEOMETRY_MUTATIONS = ("bh_stride_2", "fwd_no_rescale")

# the lengths the bound tests pack into one call, and those of the mask read-out (4-blocks, 16-row tiles, 64-row chunks and owner blocks, the top of
# the counter range at L = 512)
LENS_BOUND = [1, 17, 64, 65, 130]
LENS_READOUT = [1, 3, 5, 63, 64, 65, 129, 130, 512]


# ---- the generator -------------------------------------------------------------------------------------------------------------------------
def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on broadcastable integer arrays: uint32 [..., 4]."""
    c = [np.asarray(v, dtype=np.uint64) & MASK32 for v in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = int(k0) & 0xffffffff, int(k1) & 0xffffffff
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK32]
        k0, k1 = (k0 + W0) & 0xffffffff, (k1 + W1) & 0xffffffff
    return np.stack(c, axis=-1).astype(np.uint32)


def key_of(seed):
    return int(seed) & 0xffffffff, (int(seed) >> 32) & 0xffffffff


def call_bytes(seed, c0, c1, c2, site):
    """uint8 [..., 16]: the 16 bytes of counter (c0, c1, c2, site)."""
    w = philox(c0, c1, c2, site, *key_of(seed))
    return np.stack([(w[..., k >> 2] >> np.uint32(8 * (k & 3))) & np.uint32(0xff) for k in range(16)], axis=-1).astype(np.uint8)


def byte_of(seed, c0, c1, c2, site, k):
    """uint8: byte k (an array, broadcast with the counters) of counter (c0, c1, c2, site)."""
    c0, c1, c2, k = np.broadcast_arrays(c0, c1, c2, k)
    return np.take_along_axis(call_bytes(seed, c0, c1, c2, site), np.asarray(k, np.int64)[..., None], axis=-1)[..., 0]


def threshold(p):
    """T = floor(256 p + 0.5) on the fp32 p the C ABI receives; -1 for an invalid p."""
    p = float(np.float32(p))
    if not (0.0 <= p < 1.0):
        return -1
    T = int(np.floor(256.0 * p + 0.5))
    return -1 if T >= 256 else T


def scale(T):
    return np.float32(256.0 / (256.0 - T))


# ---- the two sites ---------------------------------------------------------------------------------------------------------------------------
def hidden_keep(M, N, T, seed, site):
    """bool [M, N]: element (row, col) kept."""
    assert N % 16 == 0
    b = call_bytes(seed, np.arange(N // 16)[None, :], np.arange(M)[:, None], 0, site)  # [M, N / 16, 16]
    return b.reshape(M, N) >= T


def attn_keep(i, j, bh, T, seed, site, swapped=False):
    """bool, broadcast of i and j: the probability of query i, key j of (sequence, head) number bh kept. swapped: the byte index
    4 (j & 3) + (i & 3), a mutation."""
    i, j = np.broadcast_arrays(np.asarray(i, np.int64), np.asarray(j, np.int64))
    k = 4 * (j & 3) + (i & 3) if swapped else 4 * (i & 3) + (j & 3)
    return byte_of(seed, i >> 2, j >> 2, bh, site, k) >= T


def attn_keep_blocks(i0, ni, j0, nj, bh, T, seed, site, swapped=False):
    """bool [len(bh), ni, nj]: attn_keep(i0 + a, j0 + c, bh[k]) at [k, a, c], from ONE generator call per 4 x 4 block of (query, key) and all
    the (sequence, head) numbers bh at once: the 16 bytes of counter (i >> 2, j >> 2, bh, site) are the block's, byte 4 (i & 3) + (j & 3)."""
    bh = np.asarray(bh, np.int64)
    ib, jb = np.arange(i0 >> 2, ((i0 + ni - 1) >> 2) + 1), np.arange(j0 >> 2, ((j0 + nj - 1) >> 2) + 1)
    by = call_bytes(seed, ib[None, :, None], jb[None, None, :], bh[:, None, None], site)   # [bh, i >> 2, j >> 2, 16]
    by = by.reshape(len(bh), len(ib), len(jb), 4, 4)                                       # [..., i & 3, j & 3] (swapped: [..., j & 3, i & 3])
    by = by.transpose(0, 1, 4, 2, 3) if swapped else by.transpose(0, 1, 3, 2, 4)
    by = by.reshape(len(bh), 4 * len(ib), 4 * len(jb))
    return by[:, i0 - 4 * int(ib[0]):i0 - 4 * int(ib[0]) + ni, j0 - 4 * int(jb[0]):j0 - 4 * int(jb[0]) + nj] >= T


def mask_counter(b, heads, mutation=None):
    """int64 [heads]: the (sequence, head) numbers b * heads + h of sequence b, the counter's third word; mutation: the defects of MUTATIONS that
    sit in this word."""
    h = np.arange(heads, dtype=np.int64)
    if mutation == "bh_stride_2":
        return b * 2 + h
    return b * heads + h + {"mask_next_head": 1, "mask_next_sequence": heads}.get(mutation, 0)


def attn_masks(cu, heads, mode, T, seed, site, mutation=None):
    """per sequence (None for an empty one) the factors m as float64 [heads, nq, n], nq = 1 in mode 3. mutation: the mask-side defects of
    MUTATIONS (every other name: the correct mask). One generator call per 4 x 4 block (attn_keep_blocks); attn_keep is the per-element
    statement of the same mapping, and tests/test_dropout_host.py shows the two equal."""
    out = []
    for b in range(len(cu) - 1):
        n = int(cu[b + 1] - cu[b])
        if n == 0:
            out.append(None)
            continue
        q0, nq = (1 if mutation == "cls_row1" else 0, 1) if mode == 3 else (0, n)
        bh = mask_counter(b, heads, mutation)
        if mutation == "mask_transposed":   # m_ij read at (j, i)
            keep = attn_keep_blocks(0, n, q0, nq, bh, T, seed, site).transpose(0, 2, 1)
        else:
            keep = attn_keep_blocks(q0, nq, 0, n, bh, T, seed, site, mutation == "byte_swapped")
        out.append(keep.astype(np.float64) * float(scale(T)))
    return out


def onehot_pattern(expected, dctx, cu, heads, mode, keep):
    """The bit-known outputs under oracle.attention_oracle.onehot(lens, heads, seed) = (qkv, cu, expected) and T = 128: the fp16-rounded p is
    a permutation matrix pi and the factor is exactly 2, so ctx[i] = fp16(2 V[pi(i)]) where (i, pi(i)) is kept and +0 where it is dropped, and
    dV[pi(i)] = fp16(2 dO[i]) or 0 likewise (mode 3: i = 0 alone; every other dV row is 0). keep: per sequence bool [heads, nq, n] (None for an
    empty one). (ctx float16, dV float16 [T, hidden], pairs kept, pairs): columns 0 and 1 of a head's V rows spell the key, which gives pi
    from `expected`."""
    hidden = 64 * heads
    ctx = np.zeros(((len(cu) - 1) if mode == 3 else int(cu[-1]), hidden), np.float16)
    dV = np.zeros((int(cu[-1]), hidden), np.float16)
    e = expected.astype(np.float64)
    kept, pairs = 0, 0
    for b in range(len(cu) - 1):
        lo, n = int(cu[b]), int(cu[b + 1] - cu[b])
        if n == 0:
            continue
        q = np.arange(1 if mode == 3 else n)
        for h in range(heads):
            cols = slice(64 * h, 64 * h + 64)
            pi = np.rint((-e[lo:lo + n, 64 * h + 1] * 8 - 1) * 32 + e[lo:lo + n, 64 * h] * 8 - 1).astype(np.int64)
            assert sorted(pi) == list(range(n))
            k = keep[b][h, q, pi[q]][:, None]
            dO = (dctx[b:b + 1] if mode == 3 else dctx[lo:lo + n])[:, cols]
            (ctx[b:b + 1] if mode == 3 else ctx[lo:lo + n])[:, cols] = np.where(k, np.float16(2) * expected[lo + q, cols], np.float16(0))
            dV[lo + pi[q], cols] = np.where(k, np.float16(2) * dO, np.float16(0))
            kept, pairs = kept + int(k.sum()), pairs + len(q)
    return ctx, dV, kept, pairs


# ---- the fp64 model and the bound ----------------------------------------------------------------------------------------------------------
def _store_ctx(out, cu, b, heads, mode, ctx):
    rows = out[b:b + 1] if mode == 3 else out[int(cu[b]):int(cu[b + 1])]
    rows[:] = ctx.transpose(1, 0, 2).reshape(ctx.shape[1], 64 * heads)


def _outputs(cu, heads, mode):
    T, hidden = int(cu[-1]), 64 * heads
    return np.zeros(((len(cu) - 1) if mode == 3 else T, hidden)), np.zeros((T, 3 * hidden))


def model(qkv, dctx, cu, heads, mode, masks):
    """(ctx, dqkv) in fp64 on the fp16 values widened, under the explicit masks of attn_masks. dctx None: ctx alone (dqkv zeros)."""
    ctx, dqkv = _outputs(cu, heads, mode)
    for b in range(len(cu) - 1):
        if cu[b + 1] == cu[b]:
            continue
        Q, K, V = (x.astype(np.float64) for x in agr.split(qkv, cu, heads, b))
        m = masks[b]
        if mode == 3:
            Q = Q[:, :1]
        S = Q @ agr._T(K) / 8.0
        w = np.exp(S - S.max(axis=2, keepdims=True))
        p = w / w.sum(axis=2, keepdims=True)
        Pd = p * m
        _store_ctx(ctx, cu, b, heads, mode, Pd @ V)
        if dctx is None:
            continue
        dO = agr.split_do(dctx, cu, heads, b, mode).astype(np.float64)
        dP = (dO @ agr._T(V)) * m
        dS = p * (dP - (p * dP).sum(axis=2, keepdims=True))
        agr._store(dqkv, cu, b, heads, dS @ K / 8.0, agr._T(dS) @ Q / 8.0, agr._T(Pd) @ dO)
    return ctx, dqkv


def reference_and_bound(qkv, dctx, cu, heads, mode, masks):
    """(ctx reference, ctx bound, dqkv reference, dqkv bound), float64. Mode 3: dQ rows behind a sequence's first are 0 with bound 0."""
    assert mode in (0, 3)
    ctx, dqkv = _outputs(cu, heads, mode)
    ctx_b, dqkv_b = _outputs(cu, heads, mode)
    for b in range(len(cu) - 1):
        if cu[b + 1] == cu[b]:
            continue
        Qs, Ks, Vs = (torch.from_numpy(x.astype(np.float64)) for x in agr.split(qkv, cu, heads, b))
        dOs = torch.from_numpy(agr.split_do(dctx, cu, heads, b, mode).astype(np.float64))
        if mode == 3:
            Qs = Qs[:, :1]
        out, err = _one_sequence(Qs, Ks, Vs, dOs, torch.from_numpy(masks[b]))
        _store_ctx(ctx, cu, b, heads, mode, out[0])
        _store_ctx(ctx_b, cu, b, heads, mode, err[0])
        agr._store(dqkv, cu, b, heads, *out[1:])
        agr._store(dqkv_b, cu, b, heads, *err[1:])
    return ctx, ctx_b, dqkv, dqkv_b


def _one_sequence(Q, K, V, dO, m):
    """((ctx, dQ, dK, dV), their bounds) of one sequence: torch float64 [heads, n, 64] in, numpy out. attention_grad_ref._one_sequence with the
    mask factors m [heads, nq, n] (module docstring, a - c)."""
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
    S = Q @ Kt / 8.0
    ds = (aQ @ aK.transpose(1, 2)) * (64 * X1ULP / 8.0)
    dP = (dO @ Vt) * m
    ddP = (aO @ aV.transpose(1, 2)) * (64 * X1ULP) * m + U32 * dP.abs()          # a.
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
    Pd = p * m
    dPd = m * dp + U32 * Pd                                                      # b.
    dPd16 = dPd + r16(Pd + dPd)
    dS16 = d32 + r16(adS + d32)
    a = npad * X1ULP
    out, err = [], []
    for val, e in ((Pd @ V, (dPd16 + a * (Pd + dPd16)) @ aV),                    # c.
                   (dS @ K / 8.0, (dS16 + a * (adS + dS16)) @ aK / 8.0),
                   (dS.transpose(1, 2) @ Q / 8.0, (dS16 + a * (adS + dS16)).transpose(1, 2) @ aQ / 8.0),
                   (Pd.transpose(1, 2) @ dO, (dPd16 + a * (Pd + dPd16)).transpose(1, 2) @ aO)):
        out.append(val.numpy())
        err.append((e + r16(val.abs() + e)).numpy())
    return out, err


# ---- the emulation -----------------------------------------------------------------------------------------------------------------------------
def emulate(qkv, dctx, cu, heads, mode, T, seed, site, mutation=None):
    """The kernels' dataflow in numpy (attention_grad_ref.emulate with the mask): fp32 scores and dP, dP * m in fp32, the running (max, sum, sum of
    e dP) over chunks of 64 keys (mode 3: one pass against the true maximum), p = exp2((s - lse) log2 e), Pd = p * m in fp32 and fp16 as the
    operand of ctx and dV, dS = p (dP - delta) in fp16 as the operand of dQ and dK, fp32 contractions, fp16 outputs.
    (ctx float16, dqkv float16).

    mutation (None: the correct dataflow) switches ONE defect on: mask_transposed: m_ij read at (j, i); mask_next_head / mask_next_sequence: the
    mask of head h + 1 / of sequence b + 1; no_mask_sweep0: delta from the unmasked dP; no_scale_dv: dV from p o keep without the scale;
    byte_swapped: the byte index 4 (j & 3) + (i & 3); cls_row1: mode 3 reads the mask of query 1; bh_stride_2: the counter's third word is
    b * 2 + h (the correct mask at two heads, by construction); fwd_no_rescale: the FORWARD's running sum is l_run + csum without the alpha,
    so its lse, and with it ctx, is wrong wherever a later chunk raises the maximum (mode 0; the backward keeps its own, correct sweep 0)."""
    assert mode in (0, 3) and (mutation is None or mutation in MUTATIONS)
    f32 = np.float32
    masks = attn_masks(cu, heads, mode, T, seed, site, mutation)
    ctx, dqkv = _outputs(cu, heads, mode)
    ctx, dqkv = ctx.astype(np.float16), dqkv.astype(np.float16)
    for b in range(len(cu) - 1):
        if cu[b + 1] == cu[b]:
            continue
        Q, K, V = (x.astype(f32) for x in agr.split(qkv, cu, heads, b))
        dO = agr.split_do(dctx, cu, heads, b, mode).astype(f32)
        m = masks[b].astype(f32)
        n = K.shape[1]
        if mode == 3:
            Q = Q[:, :1]
        s = (Q @ agr._T(K)) * f32(0.125)
        dPr = dO @ agr._T(V)
        dP = dPr * m
        dP0 = dPr if mutation == "no_mask_sweep0" else dP
        nq = Q.shape[1]
        with np.errstate(invalid="ignore", under="ignore"):
            if mode == 3:
                mx = s.max(axis=2, keepdims=True)
                e = exp2_32((s - mx) * LOG2E32)
                inv = f32(1) / e.sum(axis=2, keepdims=True, dtype=f32)
                delta = (e * dP0).sum(axis=2, keepdims=True, dtype=f32) * inv
                p = e * inv
            else:
                m_run = np.full((heads, nq, 1), -np.inf, f32)
                l_run = np.zeros((heads, nq, 1), f32)
                d_run = np.zeros((heads, nq, 1), f32)
                l_fwd = np.zeros((heads, nq, 1), f32)   # the forward's own running sum: l_run, but for fwd_no_rescale
                for c0 in range(0, n, CHUNK):
                    sc, dc = s[:, :, c0:c0 + CHUNK], dP0[:, :, c0:c0 + CHUNK]
                    m_new = np.maximum(m_run, sc.max(axis=2, keepdims=True))
                    alpha = exp2_32((m_run - m_new) * LOG2E32)
                    e = exp2_32(fma32(sc, LOG2E32, -m_new * LOG2E32))
                    csum = e.sum(axis=2, keepdims=True, dtype=f32)
                    l_run = l_run * alpha + csum
                    l_fwd = (l_fwd if mutation == "fwd_no_rescale" else l_fwd * alpha) + csum
                    d_run = d_run * alpha + (e * dc).sum(axis=2, keepdims=True, dtype=f32)
                    m_run = m_new
                lse = m_run + np.log(l_run).astype(f32)
                delta = d_run / l_run
                p = exp2_32((s - lse) * LOG2E32)
                p_fwd = exp2_32((s - (m_run + np.log(l_fwd).astype(f32))) * LOG2E32)
            dS16 = (p * (dP - delta)).astype(np.float16).astype(f32)
            Pd16 = (p * m).astype(np.float16).astype(f32)
            Pc16 = Pd16 if mode == 3 else (p_fwd * m).astype(np.float16).astype(f32)   # the forward's operand of ctx
            Pv16 = (p * (m != 0)).astype(np.float16).astype(f32) if mutation == "no_scale_dv" else Pd16
        with np.errstate(over="ignore"):
            c, dQ, dK, dV = (x.astype(np.float16) for x in (Pc16 @ V, (dS16 @ K) * f32(0.125), (agr._T(dS16) @ Q) * f32(0.125), agr._T(Pv16) @ dO))
        _store_ctx(ctx, cu, b, heads, mode, c)
        agr._store(dqkv, cu, b, heads, dQ, dK, dV)
    return ctx, dqkv
