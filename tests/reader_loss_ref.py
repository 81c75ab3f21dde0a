"""The answer reader's training loss (mdr/qa/qa_model.py:73-102 of the reference), its three heads and every gradient, stated in numpy fp64
with the rounding points of csrc/mdr_reader_loss.inl, and an elementwise DERIVED error bound for an fp32 evaluation of the same formula.
Test helper (tests/test_reader_loss_host.py, tests/test_reader_loss_gpu.py, tests/test_reader_heads_gpu.py). Nothing here is measured on
any code under test.

The loss. Per row b and candidate a:  ls = lse_s - start[s_a] if s_a != -1 else 0,  le likewise,  log_prob = -(ls + le),  masked iff the FP32
log_prob is exactly 0;  M_b = sum of exp(log_prob) over the unmasked;  span = -sum_{M_b != 0} log M_b;  rank = sum_b bce(rank_b, label_b);
sp = sum_bj bce(sp_bj, sent_labels_bj) * offset_bj * label_b;  loss = rank + span + sp_weight * sp.
    d_start[b, l] = g0 / M_b * (softmax_s[l] * P_s - hit_s[l]),  P_s = sum of p_a over s_a != -1,  hit_s[l] = sum of p_a over s_a = l
    d_rank = g0 (sigmoid - label)      d_sp = g0 sp_weight offset label (sigmoid - sent_label)
Mode O1 (`o1=True`; apex O1 as remembered, not captured): every gradient is rounded to fp16 once.

Error bound (u = 2^-24; n = finite entries of a row; A candidates). Steps, each a worst case over summation orders:
  1. lse: the inputs are exact fp16 values, so el = (n + 8) u + u |lse| (n - 1 additions in any order, exp and log a few ulp each, the final add);
  2. ls = lse - x: el + u |ls|;  log_prob: the two sides' errors + u |log_prob|;  p = exp(log_prob) relative rp = e_lp + 4 u, 1 % added for
     second order;
  3. M, P_s, hit_s[l]: sum of p rp over their candidates + (A + 2) u times the sum;  -log M: eM / M + 4 u |log M|;
  4. softmax_s[l] relative el + u |x - lse| + 4 u;  the inner difference, the quotient g0 / M and the product: the terms' errors + 4 u each;
  5. bce(x, y): 6 u (|x| + 1) (three terms of at most |x|, |x| and log 2);  sigmoid: 4 u;
  6. fp16 rounding of a gradient of value v and fp32 error e: the result lies between fp16(v - e) and fp16(v + e), so the bound is
     fp16(v + e) - fp16(v - e): 0 wherever no rounding boundary lies inside the fp32 error, one fp16 step where one does.
  7. The mask decision. The fp32 log_prob is 0 iff on every valid side fp32(lse) == x[s], and fp32(lse) depends on the summation order where the
     true lse lies within el of the midpoint between x[s] and its fp32 successor. A candidate for which fp32(lse - el) and fp32(lse + el) decide
     differently is AMBIGUOUS: the row is evaluated under every decision of its ambiguous candidates (those with the same (s, e) decide alike),
     the reference is the decision of fp32(lse) itself and the bound is widened by the largest difference to any other decision (of the order
     of 1e-7 g0 when the candidate is the row's only one).
The heads' bounds are derived alongside their functions below.
"""
import itertools

import numpy as np

from oracle.fp import U32

MUTATIONS = ("offsets_as_mask", "no_zero_mask", "one_sided_coef_1", "no_label_on_sp")
NEG = -np.inf


def h16(x):
    """Round to fp16 (nearest even, subnormals kept, overflow to inf), returned as fp64."""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(x, np.float64).astype(np.float16).astype(np.float64)


def win16(v, e, o1=True):
    """(the fp16 rounding of v, the width of what an fp32 evaluation off by at most e can round to); mode fp32: (v, e + u |v|)"""
    v, e = np.asarray(v, np.float64), np.asarray(e, np.float64)
    if not o1:
        return v, e + U32 * np.abs(v)
    with np.errstate(invalid="ignore"):
        w = h16(v + e) - h16(v - e)
    return h16(v), np.where(np.isfinite(w), np.maximum(w, 0.0), 0.0)


def f32(x):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


def _lse(x):
    fin = x != NEG
    if not fin.any():
        return NEG, 0.0, 0
    m = x[fin].max()
    lse = m + np.log(np.exp(x[fin] - m).sum())
    n = int(fin.sum())
    return lse, (n + 8) * U32 + U32 * abs(lse), n


def _lse_in(x, ex):
    """_lse of logits that are themselves off by at most ex: the lse moves by at most the largest of them"""
    lse, el, n = _lse(x)
    return lse, el + (float(np.max(ex[x != NEG])) if n else 0.0), n


def _bce(x, y):
    return np.maximum(x, 0.0) - x * y + np.log1p(np.exp(-np.abs(x)))


def _sigmoid(x):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-x))


def _row(xs, xe, starts, ends, masked, mutate, ex=(0.0, 0.0)):
    """one row under the mask decision `masked` [A]: (row loss, its error, counted, ds [L], e_ds, de, e_de) with g0 = 1, before any rounding"""
    L, A = xs.shape[0], starts.shape[0]
    out = []
    x2, idx = [xs, xe], [starts, ends]
    ex = [np.broadcast_to(np.asarray(e, np.float64), (L,)) for e in ex]  # what the logits themselves may be off by (0: exact inputs)
    lse = [_lse_in(x2[k], ex[k]) for k in (0, 1)]
    valid = [(i >= 0) & (i < L) for i in idx]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        lp, e_lp = np.zeros(A), np.zeros(A)
        for k in (0, 1):
            pos = np.where(valid[k], idx[k], 0)
            ls = np.where(valid[k], lse[k][0] - x2[k][pos], 0.0)
            e_ls = np.where(valid[k], lse[k][1] + ex[k][pos] + U32 * np.abs(ls), 0.0)
            lp, e_lp = lp - ls, e_lp + e_ls
        e_lp = e_lp + U32 * np.abs(lp)
        p = np.where(masked, 0.0, np.exp(lp))
        rp = 1.01 * (e_lp + 4 * U32)
        ep = np.where(np.isfinite(p * rp), p * rp, 0.0)
        M = p.sum()
        eM = ep.sum() + (A + 2) * U32 * M
        if np.isnan(M):
            nan = np.full(L, np.nan)
            return np.nan, 0.0, True, nan, np.zeros(L), nan, np.zeros(L)
        if M == 0:
            return 0.0, 0.0, False, np.zeros(L), np.zeros(L), np.zeros(L), np.zeros(L)
        loss = -np.log(M)
        e_loss = 1.01 * eM / M + 4 * U32 * abs(loss)
        for k in (0, 1):
            x, (l_, el, _) = x2[k], lse[k]
            v = valid[k]
            P = p[v].sum()
            eP = ep[v].sum() + (A + 2) * U32 * P
            hit, e_hit = np.zeros(L), np.zeros(L)
            np.add.at(hit, idx[k][v], p[v])
            np.add.at(e_hit, idx[k][v], ep[v])
            e_hit = e_hit + (A + 2) * U32 * hit
            sm = np.where(x == NEG, 0.0, np.exp(x - l_))
            r_sm = el + ex[k] + U32 * np.abs(np.where(x == NEG, 0.0, x - l_)) + 4 * U32
            coefP = M if mutate == "one_sided_coef_1" else P
            inner = sm * coefP - hit
            e_in = 1.01 * (sm * coefP * (r_sm + 2 * U32) + sm * eP + e_hit) + 2 * U32 * (sm * coefP + hit)
            d = np.where(x == NEG, 0.0, inner / M)
            e_d = np.where(x == NEG, 0.0, 1.01 * (e_in / M + np.abs(d) * (eM / M + 4 * U32)))
            out += [d, e_d]
    return float(loss), float(e_loss), True, out[0], out[1], out[2], out[3]


def _decisions(xs, xe, starts, ends, mutate, ex=(0.0, 0.0)):
    """(the reference decision [A], the alternative decisions of the ambiguous candidates): step 7 of the header"""
    L, A = xs.shape[0], starts.shape[0]
    lo, mid, hi = np.ones(A, bool), np.ones(A, bool), np.ones(A, bool)  # "this side's fp32 ls is 0" under lse - el, lse, lse + el
    for x, idx, e_x in ((xs, starts, ex[0]), (xe, ends, ex[1])):
        lse, el, _ = _lse_in(x, np.broadcast_to(np.asarray(e_x, np.float64), (L,)))
        v = (idx >= 0) & (idx < L)
        xv = x[np.where(v, idx, 0)]
        with np.errstate(invalid="ignore"):
            fin = np.isfinite(xv)  # (-inf) - (-inf) is NaN, not 0: a side at a -inf logit never gives an fp32 ls of 0
            lo &= np.where(v, (f32(np.maximum(lse - el, xv)) == xv) & fin, True)  # (an evaluated lse is never below its row's maximum)
            mid &= np.where(v, (f32(lse) == xv) & fin, True)
            hi &= np.where(v, (f32(lse + el) == xv) & fin, True)
    if mutate == "no_zero_mask":
        return np.zeros(A, bool), []
    amb = (lo != mid) | (hi != mid)
    groups = sorted({(int(starts[a]), int(ends[a])) for a in np.nonzero(amb)[0]})
    assert len(groups) <= 4, "more than four ambiguous candidate groups in one row"
    alts = []
    for flips in itertools.product((False, True), repeat=len(groups)):
        if not any(flips):
            continue
        d = mid.copy()
        for g, f in zip(groups, flips):
            if f:
                sel = (starts == g[0]) & (ends == g[1])
                d[sel] = ~mid[sel]
        alts.append(d)
    return mid, alts


def loss_and_grads(inp, g0=1.0, sp_weight=1.0, o1=True, mutate=None, e_in=None):
    """inp: start, end [B, L] (fp16 values, -inf allowed), rank [B], sp [B, NS] or None, starts, ends [B, A], label [B], sent_offsets, sent_labels
    [B, NS]. Returns {"loss", "loss_bound", "grads": {start, end, rank, sp}, "bounds": {...}, "counted": [B]}. `mutate` (one of MUTATIONS) states a
    WRONG formula: what the bound must reject. e_in: None, or {"start", "end", "rank", "sp"}: what the scores themselves may be off by (an fp32
    forward in front of the loss); it is propagated with |d lse / d x| <= 1, |d bce / d x| <= 1 and |d sigmoid / d x| <= 1 / 4."""
    assert mutate is None or mutate in MUTATIONS, mutate
    e_in = e_in or {}
    S, E = np.asarray(inp["start"], np.float64), np.asarray(inp["end"], np.float64)
    B, L = S.shape
    starts, ends = np.asarray(inp["starts"], np.int64), np.asarray(inp["ends"], np.int64)
    label = np.asarray(inp["label"], np.float64).reshape(B)
    g0 = float(g0)
    span, e_span, abs_span = 0.0, 0.0, 0.0
    dS, eS, dE, eE, wS, wE = (np.zeros((B, L)) for _ in range(6))
    counted = np.zeros(B, bool)
    for b in range(B):
        ex = tuple(np.asarray(e_in[k], np.float64)[b] if k in e_in else 0.0 for k in ("start", "end"))
        ref_dec, alts = _decisions(S[b], E[b], starts[b], ends[b], mutate, ex)
        lo_, e_, counted[b], dS[b], eS[b], dE[b], eE[b] = _row(S[b], E[b], starts[b], ends[b], ref_dec, mutate, ex)
        widen = 0.0
        for d in alts:
            alt = _row(S[b], E[b], starts[b], ends[b], d, mutate, ex)
            widen = max(widen, abs(alt[0] - lo_) + alt[1])
            wS[b] = np.maximum(wS[b], np.abs(alt[3] - dS[b]) + alt[4])
            wE[b] = np.maximum(wE[b], np.abs(alt[5] - dE[b]) + alt[6])
        span += lo_
        e_span += max(e_, widen)
        abs_span += abs(lo_)
    eS, eE = np.maximum(eS, wS), np.maximum(eE, wE)
    R = np.asarray(inp["rank"], np.float64).reshape(B)
    rank_terms = _bce(R, label)
    rank = rank_terms.sum()
    exr = np.asarray(e_in.get("rank", np.zeros(B)), np.float64).reshape(B)
    e_rank = (6 * U32 * (np.abs(R) + 1) + exr).sum() + (B + 2) * U32 * np.abs(rank_terms).sum()
    loss = rank + span
    bound = e_rank + e_span + (B + 2) * U32 * abs_span + 4 * U32 * (abs(rank) + abs(span))
    grads = {"start": g0 * dS, "end": g0 * dE, "rank": g0 * (_sigmoid(R) - label)}
    ebs = {"start": abs(g0) * eS + 2 * U32 * np.abs(grads["start"]), "end": abs(g0) * eE + 2 * U32 * np.abs(grads["end"]), "rank": abs(g0) * (8 * U32 + 0.25 * exr)}
    if inp.get("sp") is not None:
        SP = np.asarray(inp["sp"], np.float64)
        off = np.asarray(inp["sent_offsets"], np.float64)
        if mutate == "offsets_as_mask":
            off = (off != 0).astype(np.float64)
        lab = np.ones(B) if mutate == "no_label_on_sp" else label
        sl = np.asarray(inp["sent_labels"], np.float64)
        wgt = off * lab[:, None]
        with np.errstate(invalid="ignore"):
            terms = _bce(SP, sl) * wgt
            sp = terms.sum()
            exs = np.asarray(e_in.get("sp", np.zeros(SP.shape)), np.float64)
            e_sp = ((6 * U32 * (np.abs(SP) + 1) + exs) * wgt).sum() + (SP.size + 4) * U32 * np.abs(terms).sum()
            loss = loss + sp_weight * sp
            bound = bound + abs(sp_weight) * e_sp + 4 * U32 * (abs(sp_weight * sp) + abs(loss))
            grads["sp"] = g0 * sp_weight * wgt * (_sigmoid(SP) - sl)
            ebs["sp"] = np.abs(g0 * sp_weight * wgt) * (8 * U32 + 0.25 * exs) + 4 * U32 * np.abs(grads["sp"])
    out_g, out_b = {}, {}
    for k in grads:
        out_g[k], out_b[k] = win16(grads[k], ebs[k], o1)
    return {"loss": float(loss), "loss_bound": float(bound), "grads": out_g, "bounds": out_b, "counted": counted}


# ------------------------------------------------------------------------------------------------------------------------------ the heads
# Forward (rounding points at the top of csrc/mdr_reader.inl): a logit is fp16(fp32 dot of fp16 operands + the fp16-rounded bias). A dot of H
# terms accumulated in fp32 in any order is off by at most (H + 2) u sum |x||w| (+ u |v| for the bias add), so the fp16 result lies in the
# window of step 6. tanh is taken as 4 u relative in fp32; where pooled16 can round either way the width enters the rank dot through |w|.
# Backward: d_h = fp16(g_s W0 + g_e W1 + g_sp W3) is three fp32 operations on exact operands: 3 u of the terms' magnitudes, plus the error of
# g_sp's own sum ((n + 1) u sum |g_sp_j|) times |W3|. The dw sums over n token rows in any order: (n + 2) u sum |g||h|. An error bound of an
# incoming gradient (eg: what the loss's fp16 window leaves open) is propagated linearly: sum |coefficient| eg.
def heads_params16(P, o1=True):
    r = h16 if o1 else (lambda x: np.asarray(x, np.float64))
    has_sp = P.get("sp.weight") is not None
    H = np.asarray(P["qa_outputs.weight"]).shape[1]
    W = np.concatenate([r(P["qa_outputs.weight"]).reshape(2, H), r(P["rank.weight"]).reshape(1, H),
                        r(P["sp.weight"]).reshape(1, H) if has_sp else np.zeros((1, H))])
    b = np.concatenate([r(P["qa_outputs.bias"]).reshape(2), r(P["rank.bias"]).reshape(1), r(P["sp.bias"]).reshape(1) if has_sp else np.zeros(1)])
    return W, b


def heads_forward(seq, dense, lens, pmask, offs, P, o1=True, e_dense=0.0):
    """seq [B, L, H] (fp16 values in mode O1; rows at or behind lens[b] are not read), dense [B, H]. Returns values and windows:
    {"start", "end" [B, L], "rank" [B], "sp" [B, NS] or None} twice."""
    seq, dense = np.asarray(seq, np.float64), np.asarray(dense, np.float64)
    B, L, H = seq.shape
    W, bias = heads_params16(P, o1)
    inside = (np.arange(L)[None, :] < np.asarray(lens)[:, None]) & (np.asarray(pmask) == 1)
    val, win = {}, {}
    for k, name in ((0, "start"), (1, "end")):
        v = seq @ W[k] + bias[k]
        e = (H + 2) * U32 * (np.abs(seq) @ np.abs(W[k])) + U32 * np.abs(v)
        v, w = win16(v, e, o1)
        val[name], win[name] = np.where(inside, v, NEG), np.where(inside, w, 0.0)
    t = np.tanh(dense)
    pooled, wp = win16(t, 4 * U32 * np.abs(t) + e_dense, o1)  # e_dense: what dense itself may be off by (|tanh'| <= 1)
    v = pooled @ W[2] + bias[2]
    e = (H + 2) * U32 * (np.abs(pooled) @ np.abs(W[2])) + wp @ np.abs(W[2]) + U32 * np.abs(v)
    val["rank"], win["rank"] = win16(v, e, o1)
    val["sp"] = win["sp"] = None
    if offs is not None and P.get("sp.weight") is not None:
        offs = np.asarray(offs, np.int64)
        ok = (offs >= 0) & (offs < np.asarray(lens)[:, None])
        rows = seq[np.arange(B)[:, None], np.where(ok, offs, 0)]
        v = rows @ W[3] + bias[3]
        e = (H + 2) * U32 * (np.abs(rows) @ np.abs(W[3])) + U32 * np.abs(v)
        v, w = win16(v, e, o1)
        val["sp"], win["sp"] = np.where(ok, v, NEG), np.where(ok, w, 0.0)
    return val, win


def heads_backward(seq, dense, lens, pmask, offs, P, g, eg=None, o1=True, e_dense=0.0):
    """g: {"start", "end" [B, L], "rank" [B], "sp" [B, NS] or None}: the score gradients (fp16 values in mode O1); eg: their error bounds or
    None. Returns (grads, bounds) with d_h [B, L, H] (padded layout: row (b, p) is packed row cu[b] + p; 0 at p >= lens[b]), d_dense [B, H],
    dw_qa [2, H], db_qa [2], dw_rank [H], db_rank [1] and, with g["sp"], dw_sp [H], db_sp [1]."""
    seq, dense = np.asarray(seq, np.float64), np.asarray(dense, np.float64)
    B, L, H = seq.shape
    lens = np.asarray(lens)
    W, _ = heads_params16(P, o1)
    live = np.arange(L)[None, :] < lens[:, None]
    inside = live & (np.asarray(pmask) == 1)
    z = lambda a: np.zeros_like(np.asarray(a, np.float64))  # noqa: E731
    eg = eg or {}
    gs, ge = (np.where(inside, np.asarray(g[k], np.float64), 0.0) for k in ("start", "end"))
    egs, ege = (np.where(inside, eg.get(k, z(g[k])), 0.0) for k in ("start", "end"))
    gp, egp, agp = np.zeros((B, L)), np.zeros((B, L)), np.zeros((B, L))
    has_sp = g.get("sp") is not None and np.asarray(g["sp"]).shape[1] > 0
    if has_sp:
        offs = np.asarray(offs, np.int64)
        gsp, egsp = np.asarray(g["sp"], np.float64), np.asarray(eg.get("sp", z(g["sp"])), np.float64)
        ok = (offs >= 0) & (offs < lens[:, None])
        bi = np.broadcast_to(np.arange(B)[:, None], offs.shape)
        np.add.at(gp, (bi[ok], offs[ok]), gsp[ok])
        np.add.at(agp, (bi[ok], offs[ok]), np.abs(gsp[ok]))
        np.add.at(egp, (bi[ok], offs[ok]), egsp[ok])
        egp = egp + (offs.shape[1] + 1) * U32 * agp
    seqz = np.where(live[:, :, None], seq, 0.0)
    aseq = np.abs(seqz)
    grads, bounds = {}, {}
    v = gs[:, :, None] * W[0] + ge[:, :, None] * W[1] + gp[:, :, None] * W[3]
    mag = np.abs(gs)[:, :, None] * np.abs(W[0]) + np.abs(ge)[:, :, None] * np.abs(W[1]) + np.abs(gp)[:, :, None] * np.abs(W[3])
    e = 3 * U32 * mag + egs[:, :, None] * np.abs(W[0]) + ege[:, :, None] * np.abs(W[1]) + egp[:, :, None] * np.abs(W[3])
    grads["d_h"], bounds["d_h"] = win16(v, e, o1)
    n = B * L
    rows = [(gs, egs), (ge, ege)] + ([(gp, egp)] if has_sp else [])
    dw = [(np.einsum("bl,blh->h", a, seqz), np.einsum("bl,blh->h", ea, aseq) + (n + 2) * U32 * np.einsum("bl,blh->h", np.abs(a), aseq)) for a, ea in rows]
    grads["dw_qa"], bounds["dw_qa"] = np.stack([dw[0][0], dw[1][0]]), np.stack([dw[0][1], dw[1][1]])
    grads["db_qa"] = np.array([gs.sum(), ge.sum()])
    bounds["db_qa"] = np.array([egs.sum() + (n + 2) * U32 * np.abs(gs).sum(), ege.sum() + (n + 2) * U32 * np.abs(ge).sum()])
    if has_sp:
        grads["dw_sp"], bounds["dw_sp"] = dw[2]
        grads["db_sp"] = np.array([gsp[ok].sum()])
        bounds["db_sp"] = np.array([egsp[ok].sum() + (gsp.size + 2) * U32 * np.abs(gsp[ok]).sum()])
    # rank, behind the pooler's tanh
    gr = np.asarray(g["rank"], np.float64).reshape(B)
    egr = np.asarray(eg.get("rank", np.zeros(B)), np.float64).reshape(B)
    t = np.tanh(dense)
    pooled, wp = win16(t, 4 * U32 * np.abs(t) + e_dense, o1)  # e_dense: what dense itself may be off by (|tanh'| <= 1)
    gw = gr[:, None] * W[2]  # exact in fp32 in mode O1: 11 x 11 bits
    dp, wdp = win16(gw, egr[:, None] * np.abs(W[2]), o1)
    f = 1.0 - pooled * pooled
    v = dp * f
    e = 3 * U32 * np.abs(v) + 1.01 * np.abs(dp) * 2 * np.abs(pooled) * wp + wdp * np.abs(f)
    grads["d_dense"], bounds["d_dense"] = win16(v, e, o1)
    grads["dw_rank"] = gr @ pooled
    bounds["dw_rank"] = (B + 2) * U32 * (np.abs(gr) @ np.abs(pooled)) + np.abs(gr) @ wp + egr @ np.abs(pooled)
    grads["db_rank"] = np.array([gr.sum()])
    bounds["db_rank"] = np.array([egr.sum() + (B + 2) * U32 * np.abs(gr).sum()])
    return grads, bounds


def pooler_forward(cls, Wp, bp, o1=True):
    """dense = cls Wp^T + bp as linear.packed_linear computes it: fp16 operands, fp32 accumulation, the fp32 bias, one rounding to fp16"""
    r = h16 if o1 else (lambda x: np.asarray(x, np.float64))
    cls, W = np.asarray(cls, np.float64), r(Wp)
    v = cls @ W.T + np.asarray(bp, np.float64)
    e = (cls.shape[1] + 2) * U32 * (np.abs(cls) @ np.abs(W).T) + U32 * np.abs(v)
    return win16(v, e, o1)


def pooler_backward(cls, Wp, d_dense, e_dense, o1=True):
    """(grads, bounds) of d_cls [B, H] (fp16 in mode O1), dW [H, H], db [H] for the fp16 gradient d_dense with error bound e_dense"""
    r = h16 if o1 else (lambda x: np.asarray(x, np.float64))
    cls, W, d = np.asarray(cls, np.float64), r(Wp), np.asarray(d_dense, np.float64)
    B, H = cls.shape
    grads, bounds = {}, {}
    grads["d_cls"], bounds["d_cls"] = win16(d @ W, (H + 2) * U32 * (np.abs(d) @ np.abs(W)) + e_dense @ np.abs(W), o1)
    grads["dW"] = d.T @ cls
    bounds["dW"] = (B + 2) * U32 * (np.abs(d).T @ np.abs(cls)) + e_dense.T @ np.abs(cls)
    grads["db"] = d.sum(0)
    bounds["db"] = (B + 2) * U32 * np.abs(d).sum(0) + e_dense.sum(0)
    return grads, bounds


def chain(seq, lens, batch, P, g0=1.0, sp_weight=1.0, o1=True, forward=None, mutate=None):
    """The whole brick on one padded batch: CLS row -> pooler dense -> heads -> loss -> every gradient, with propagated bounds. seq [B, L, H]
    (rounded to fp16 in mode O1). `forward`: None, or the forward values another evaluation produced ({"dense", "start", "end", "rank", "sp"}),
    used in place of this function's own so that the backward is compared on the same activations. Returns {"forward": (values, windows),
    "loss", "loss_bound", "grads", "bounds"}; grads: seq [B, L, H] and one entry per parameter name of P."""
    r = h16 if o1 else (lambda x: np.asarray(x, np.float64))
    seq = r(seq)
    B, L, H = seq.shape
    has_sp = P.get("sp.weight") is not None
    offs = np.asarray(batch["sent_offsets"]) if has_sp else None
    cls = seq[:, 0]
    dense, w_dense = pooler_forward(cls, P["pooler.dense.weight"], P["pooler.dense.bias"], o1)
    if forward is not None:
        dense = np.asarray(forward["dense"], np.float64)
    # mode fp32 carries the forward's error into the backward; mode O1 with `forward` given evaluates the backward on those very activations
    e_dense = 0.0 if o1 else w_dense
    fv, fw = heads_forward(seq, dense, lens, batch["paragraph_mask"], offs, P, o1, e_dense)
    fw["dense"] = w_dense
    if forward is not None:
        for k in ("start", "end", "rank", "sp"):
            if fv[k] is not None:
                fv[k] = np.asarray(forward[k], np.float64).reshape(fv[k].shape)
    fv["dense"] = dense
    inp = {"start": fv["start"], "end": fv["end"], "rank": fv["rank"], "sp": fv["sp"], "starts": batch["starts"], "ends": batch["ends"],
           "label": batch["label"], "sent_offsets": offs, "sent_labels": batch.get("sent_labels")}
    lg = loss_and_grads(inp, g0, sp_weight, o1, mutate, e_in=None if o1 else {k: fw[k] for k in ("start", "end", "rank", "sp") if fw[k] is not None})
    g = dict(lg["grads"], sp=lg["grads"].get("sp"))
    hg, hb = heads_backward(seq, dense, lens, batch["paragraph_mask"], offs, P, g, lg["bounds"], o1, e_dense)
    pg, pb = pooler_backward(cls, P["pooler.dense.weight"], hg["d_dense"], hb["d_dense"], o1)
    d_seq, b_seq = hg["d_h"].copy(), hb["d_h"].copy()
    v = d_seq[:, 0] + pg["d_cls"]  # the gather's backward: an fp16 add of the two gradients of the CLS rows
    if o1:
        d_seq[:, 0], b_seq[:, 0] = win16(v, b_seq[:, 0] + pb["d_cls"], True)
    else:
        d_seq[:, 0], b_seq[:, 0] = v, b_seq[:, 0] + pb["d_cls"] + U32 * np.abs(v)
    grads = {"seq": d_seq, "pooler.dense.weight": pg["dW"], "pooler.dense.bias": pg["db"], "qa_outputs.weight": hg["dw_qa"], "qa_outputs.bias": hg["db_qa"],
             "rank.weight": hg["dw_rank"].reshape(1, H), "rank.bias": hg["db_rank"]}
    bounds = {"seq": b_seq, "pooler.dense.weight": pb["dW"], "pooler.dense.bias": pb["db"], "qa_outputs.weight": hb["dw_qa"], "qa_outputs.bias": hb["db_qa"],
              "rank.weight": hb["dw_rank"].reshape(1, H), "rank.bias": hb["db_rank"]}
    if has_sp:
        grads.update({"sp.weight": hg["dw_sp"].reshape(1, H), "sp.bias": hg["db_sp"]})
        bounds.update({"sp.weight": hb["dw_sp"].reshape(1, H), "sp.bias": hb["db_sp"]})
    return {"forward": (fv, fw), "loss": lg["loss"], "loss_bound": lg["loss_bound"], "grads": grads, "bounds": bounds}


# ------------------------------------------------------------------------------------------------------------------------------ inputs
def make_loss_case(B, L, A, NS, seed, spread=2.0):
    """A loss batch with every candidate kind: per row a paragraph offset, logits -inf outside [off, hi), candidates cycling through
    (yes/no at off, at off + 1, a real span, one-sided start, one-sided end, all -1); labels 0 and 1; offsets padded with 0 and as large as the row
    allows. Row 4 of every seven has a single real span and padding, row 5 of every seven ignores every candidate."""
    rng = np.random.default_rng([seed, B, L, A, NS])
    start, end = (np.full((B, L), NEG) for _ in range(2))
    starts, ends = (np.full((B, A), -1, np.int64) for _ in range(2))
    label = (np.arange(B) + seed) % 2
    offs, slab = np.zeros((B, NS), np.int64), np.zeros((B, NS), np.int64)
    for b in range(B):
        length = L if b == 0 else int(rng.integers(max(1, L // 2), L + 1))
        off = min(int(rng.integers(1, 6)), length - 1) if length > 1 else 0
        hi = max(off + 1, length - 1)
        start[b, off:hi] = h16(spread * rng.standard_normal(hi - off))
        end[b, off:hi] = h16(spread * rng.standard_normal(hi - off))
        for a in range(A):
            k = (b + a) % 6 if a < 4 else int(rng.integers(0, 6))
            s = int(rng.integers(off, hi))
            e = int(rng.integers(s, hi))
            pairs = [(off, off), (min(off + 1, hi - 1), min(off + 1, hi - 1)), (s, e), (s, -1), (-1, e), (-1, -1)]
            starts[b, a], ends[b, a] = pairs[k]
        if b % 7 == 4:
            starts[b], ends[b] = -1, -1
            starts[b, 0], ends[b, 0] = off, hi - 1
        if b % 7 == 5:
            starts[b], ends[b] = -1, -1
        ns = NS if b == 0 else (int(rng.integers(0, NS + 1)) if NS else 0)
        offs[b, :ns] = np.sort(rng.integers(1, max(2, length), size=ns))
        if ns and b == 0:
            offs[b, ns - 1] = length - 1
        slab[b, :ns] = rng.integers(0, 2, size=ns)
    rank = h16(3.0 * rng.standard_normal(B))
    sp = h16(3.0 * rng.standard_normal((B, NS))) if NS else None
    return {"start": start, "end": end, "rank": rank, "sp": sp, "starts": starts, "ends": ends, "label": label.astype(np.int64), "sent_offsets": offs,
            "sent_labels": slab}


def make_heads_case(B, L, NS, H, seed, lens=None, exact=False):
    """h rows, the pooler dense output, the head parameters and a batch for the heads' tests: ragged rows (lens), a paragraph mask that starts
    inside the row, sentence offsets with a duplicate and a padded 0 (the CLS row). exact: inputs on the grid of oracle/fp.grid."""
    from oracle import fp
    rng = np.random.default_rng([seed, B, L, NS, H])
    lens = np.asarray(lens if lens is not None else [L] + [int(rng.integers(max(2, L // 3), L + 1)) for _ in range(B - 1)])
    if exact:
        seq = fp.grid((B, L, H), seed, dtype=np.float64)
        dense = fp.grid((B, H), seed + 1, 16.0, dtype=np.float64)
        P = {"qa_outputs.weight": fp.grid((2, H), seed + 2), "qa_outputs.bias": fp.grid((2,), seed + 3), "rank.weight": fp.grid((1, H), seed + 4),
             "rank.bias": fp.grid((1,), seed + 5), "sp.weight": fp.grid((1, H), seed + 6), "sp.bias": fp.grid((1,), seed + 7)}
    else:
        seq = h16(rng.standard_normal((B, L, H)))
        dense = h16(1.5 * rng.standard_normal((B, H)))
        s = 1.5 / np.sqrt(H)
        P = {"qa_outputs.weight": (s * rng.standard_normal((2, H))).astype(np.float32), "qa_outputs.bias": (0.1 * rng.standard_normal(2)).astype(np.float32),
             "rank.weight": (s * rng.standard_normal((1, H))).astype(np.float32), "rank.bias": (0.1 * rng.standard_normal(1)).astype(np.float32),
             "sp.weight": (s * rng.standard_normal((1, H))).astype(np.float32), "sp.bias": (0.1 * rng.standard_normal(1)).astype(np.float32)}
    pmask = np.zeros((B, L), np.int64)
    offs = np.zeros((B, NS), np.int64)
    for b in range(B):
        po = min(2, int(lens[b]) - 1)
        pmask[b, po:max(po + 1, int(lens[b]) - 1)] = 1
        ns = min(NS, max(0, NS - (b % 3)))
        if ns:
            offs[b, :ns] = np.sort(rng.integers(1, max(2, int(lens[b])), size=ns))
            if ns >= 2:
                offs[b, 1] = offs[b, 0]  # two markers on one row
    if NS == 0:
        P["sp.weight"] = P["sp.bias"] = None
    return {"seq": seq, "dense": dense, "lens": lens, "pmask": pmask, "offs": offs if NS else None, "P": P}


def pack(seq, lens):
    """(packed rows [T, H], cu int32 [B + 1]) of a padded [B, L, H] array"""
    lens = np.asarray(lens)
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    return np.concatenate([seq[b, :lens[b]] for b in range(len(lens))]), cu


def unpack(rows, lens, L):
    lens = np.asarray(lens)
    cu = np.concatenate([[0], np.cumsum(lens)])
    out = np.zeros((len(lens), L) + rows.shape[1:], rows.dtype)
    for b in range(len(lens)):
        out[b, :lens[b]] = rows[cu[b]:cu[b + 1]]
    return out
