"""The in-batch retrieval loss over 2B + 2 + K columns and its six gradients, stated in numpy fp64, with an elementwise error bound
for an fp32 (or apex-O1) evaluation of the same formula. Test helper (tests/test_mhop_loss_host.py, tests/test_inbatch_grad_gpu.py).

Formula (mdr/retrieval/criterions.py:114-151 of the reference). Row i of hop h scores x_i (q or q_sp) against the columns
[c1; c2] (2B), its own two negatives (2) and the K queue rows; hop 1 masks column B + i; the target is column i (hop 1) or B + i (hop 2).
    lse_i = logsumexp of the unmasked scores      loss = mean(lse1 - s1[t]) + mean(lse2 - s2[t])
    g_ij = (exp(s_ij - lse_i) - [j = t_i]) * g0 / B, 0 at the masked column
    dx_i = sum_j g_ij col_j     dctx_j = sum_h sum_i g^h_ij x^h_i     dneg_i,m = sum_h g^h_i,(2B+m) x^h_i     (no gradient for the queue)

Mode O1 (`o1=True`; apex O1 as remembered, not captured -- the rounding points listed in csrc/mdr_inbatch_grad.hip): operands rounded to
fp16, score = fp16(sum), lse and p in fp32, g rounded to fp16, every mm / bmm backward result rounded to fp16 (per call: the [c1; c2] mm, the
queue mm, the bmm of the negatives, per hop), the terms of one leaf added in fp32.

Error bound, derived (u = 2^-24, the unit roundoff of fp32; N = number of columns; nothing here is measured on any code under test):
  1. a dot product of d terms accumulated in fp32 IN ANY ORDER is off by at most (d + 2) u |x||y| (Higham 3.5 with Cauchy-Schwarz), so a
     score is off by ds_ij = (d + 2) u |x_i||col_j| + u |s_ij| (its final rounding). In mode O1 the score is the fp16 rounding of that sum: the
     rounded value can differ from the helper's only if a rounding boundary lies within the accumulation error, so by monotonicity of rounding
     ds_ij = fp16(s + e) - fp16(s - e), which is 0 for most scores and one fp16 step for the few near a boundary;
  2. lse_i is off by at most el_i = sum_j p_ij ds_ij (a weighted mean of the score errors) + (N + 8) u (N - 1 additions in any order plus
     exp and log, a few ulp each) + u |lse_i|;
  3. p_ij = exp(s_ij - lse_i) is off relatively by rp_ij = ds_ij + el_i + u (|s_ij - lse_i| + 4) (argument error, the subtraction's rounding
     scaled by the argument, exp); 1 % is added for the second-order terms;
  4. g_ij is off by dg_ij = scale (p_ij rp_ij + 4 u |p_ij - onehot|) (subtraction, g0 / B, product). Mode O1: fp16(g + dg) - fp16(g - dg);
  5. a contraction sum_j g_ij y_jk over n terms is off by sum_j dg_ij |y_jk| + (n + 2) u sum_j |g_ij||y_jk|; its result is rounded once
     (fp32: u |t|; mode O1: fp16(t + e) - fp16(t - e)), and the terms of a leaf are added in fp32 (2 u per addition).
The same steps give the bound of the loss. The bound is a worst case over summation orders, so it holds for torch on the CPU, for the device
kernels and for any other correct fp32 evaluation, and it is far below what any of the mutations of `MUTATIONS` changes.
"""
import numpy as np

from oracle.fp import U32

KEYS = ("q", "q_sp1", "c1", "c2", "neg_1", "neg_2")
MUTATIONS = ("no_mask", "no_onehot", "no_inv_b", "no_queue_in_lse", "swap_dneg", "hop2_target_i", "dctx_no_hop2")


def h16(x):
    """Round to fp16 (nearest even, subnormals kept, overflow to inf), returned as fp64."""
    with np.errstate(over="ignore"):
        return np.asarray(x, np.float64).astype(np.float16).astype(np.float64)


def loss_and_grads(inp, queue=None, g0=1.0, o1=False, mutate=None, record=None):
    """inp: the six [B, d] matrices by name; queue [K, d] or None. Returns {"loss", "grads": {name: [B, d]}, "loss_bound", "bounds": {name: [B, d]}}.
    `mutate` (one of MUTATIONS) states a WRONG formula: what the bound must reject.
    `record` (a dict, mode O1; tests/overflow_ref.py): filled with what the gradient's fp16 rounding points are HANDED, value and error in front
    of the rounding: "g" -> per hop (g [B, N], dg), and per leaf name the list of (t [B, d], e) of the contraction results added into it."""
    assert mutate is None or mutate in MUTATIONS, mutate
    r = h16 if o1 else (lambda x: np.asarray(x, np.float64))
    X = [r(inp["q"]), r(inp["q_sp1"])]
    B, d = X[0].shape
    C = np.concatenate([r(inp["c1"]), r(inp["c2"])])
    NG = np.stack([r(inp["neg_1"]), r(inp["neg_2"])], axis=1)
    QU = r(queue) if queue is not None and len(queue) else np.zeros((0, d))
    K = QU.shape[0]
    N = 2 * B + 2 + K
    scale = float(g0) * (1.0 if mutate == "no_inv_b" else 1.0 / B)
    rows = np.arange(B)

    def rt(t, e, leaves=()):  # the rounding of one contraction's result, and what it does to the error
        if record is not None:
            for name, pick in leaves:
                record.setdefault(name, []).append((t[pick], e[pick]))
        return (h16(t), np.maximum(h16(t + e) - h16(t - e), 0.0)) if o1 else (t, e + U32 * np.abs(t))

    loss, loss_bound = 0.0, 0.0
    dx, bx = [], []
    dctx, bctx = np.zeros((2 * B, d)), np.zeros((2 * B, d))
    dneg, bneg = np.zeros((B, 2, d)), np.zeros((B, 2, d))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for h in (0, 1):
            x = X[h]
            sx = np.concatenate([x @ C.T, np.einsum("bd,bnd->bn", x, NG), x @ QU.T], axis=1)
            ncol = np.concatenate([np.broadcast_to(np.linalg.norm(C, axis=1), (B, 2 * B)), np.linalg.norm(NG, axis=2),
                                   np.broadcast_to(np.linalg.norm(QU, axis=1), (B, K))], axis=1)
            es = (d + 2) * U32 * np.linalg.norm(x, axis=1)[:, None] * ncol
            if o1:
                s, ds = h16(sx), np.maximum(h16(sx + es) - h16(sx - es), 0.0)
            else:
                s, ds = sx, es + U32 * np.abs(sx)
            mask = np.zeros((B, N), bool)
            if h == 0 and mutate != "no_mask":
                mask[rows, B + rows] = True
            sm = np.where(mask, -np.inf, s)
            in_lse = sm.copy()
            if mutate == "no_queue_in_lse":
                in_lse[:, 2 * B + 2:] = -np.inf
            mx = in_lse.max(axis=1)
            lse = mx + np.log(np.exp(in_lse - mx[:, None]).sum(axis=1))
            t = rows + (B if h == 1 and mutate != "hop2_target_i" else 0)
            onehot = np.zeros((B, N))
            if mutate != "no_onehot":
                onehot[rows, t] = 1.0
            p = np.where(mask, 0.0, np.exp(sm - lse[:, None]))
            ds = np.where(mask, 0.0, ds)
            el = 1.01 * (p * ds).sum(axis=1) + (N + 8) * U32 + U32 * np.abs(lse)
            rp = ds + el[:, None] + U32 * (np.abs(np.where(mask, 0.0, sm - lse[:, None])) + 4.0)
            g = np.where(mask, 0.0, (p - onehot) * scale)
            dg = abs(scale) * (1.01 * p * rp + 4 * U32 * np.abs(p - onehot))
            dg = np.where(mask, 0.0, dg)
            if record is not None:
                record.setdefault("g", []).append((g, dg))
            if o1:
                g, dg = h16(g), np.maximum(h16(g + dg) - h16(g - dg), 0.0)
            tgt = s[rows, t]
            loss += (lse - tgt).mean()
            loss_bound += (el + ds[rows, t]).mean() + (B + 4) * U32 * np.abs(lse - tgt).mean() + 2 * U32 * (np.abs(lse) + np.abs(tgt)).mean()

            ag = np.abs(g)
            gc, gn, gq = g[:, :2 * B], g[:, 2 * B:2 * B + 2], g[:, 2 * B + 2:]
            ec, en, eq = dg[:, :2 * B], dg[:, 2 * B:2 * B + 2], dg[:, 2 * B + 2:]
            own = [(("q", "q_sp1")[h], slice(None))]
            terms = [rt(gc @ C, ec @ np.abs(C) + (2 * B + 2) * U32 * (ag[:, :2 * B] @ np.abs(C)), own),
                     rt(np.einsum("bn,bnd->bd", gn, NG), np.einsum("bn,bnd->bd", en + 4 * U32 * np.abs(gn), np.abs(NG)), own)]
            if K:
                terms.append(rt(gq @ QU, eq @ np.abs(QU) + (K + 2) * U32 * (ag[:, 2 * B + 2:] @ np.abs(QU)), own))
            dx.append(sum(t_ for t_, _ in terms))
            bx.append(sum(e_ for _, e_ in terms) + 4 * U32 * sum(np.abs(t_) for t_, _ in terms))
            if not (h == 1 and mutate == "dctx_no_hop2"):
                t_, e_ = rt(gc.T @ x, ec.T @ np.abs(x) + (B + 2) * U32 * (ag[:, :2 * B].T @ np.abs(x)), [("c1", slice(0, B)), ("c2", slice(B, 2 * B))])
                dctx += t_
                bctx += e_ + 4 * U32 * np.abs(t_)
            t_, e_ = rt(gn[:, :, None] * x[:, None, :], (en + 4 * U32 * np.abs(gn))[:, :, None] * np.abs(x)[:, None, :],
                        [("neg_1", (slice(None), 0)), ("neg_2", (slice(None), 1))])
            dneg += t_
            bneg += e_ + 4 * U32 * np.abs(t_)
    if mutate == "swap_dneg":
        dneg = dneg[:, ::-1]
    grads = {"q": dx[0], "q_sp1": dx[1], "c1": dctx[:B], "c2": dctx[B:], "neg_1": dneg[:, 0], "neg_2": dneg[:, 1]}
    bounds = {"q": bx[0], "q_sp1": bx[1], "c1": bctx[:B], "c2": bctx[B:], "neg_1": bneg[:, 0], "neg_2": bneg[:, 1]}
    return {"loss": float(loss), "loss_bound": float(loss_bound), "grads": grads, "bounds": bounds}


def violations(ref, loss, grads):
    """Names of the results that leave the bound of `ref` (a loss_and_grads result) anywhere: [] means `loss` and `grads` are accepted. A non-finite
    value where the reference is finite is a violation."""
    bad = []
    if loss is not None and not abs(float(loss) - ref["loss"]) <= ref["loss_bound"]:
        bad.append("loss")
    for k in KEYS:
        err = np.abs(np.asarray(grads[k], np.float64) - ref["grads"][k])
        if not np.all(err <= ref["bounds"][k]):
            bad.append(k)
    return bad


def worst(ref, loss, grads):
    """{name: (largest |error|, the bound there, largest error / bound)} for a report line."""
    out = {"loss": (abs(float(loss) - ref["loss"]), ref["loss_bound"], abs(float(loss) - ref["loss"]) / ref["loss_bound"])}
    for k in KEYS:
        err = np.abs(np.asarray(grads[k], np.float64) - ref["grads"][k])
        ratio = np.where(err > 0, err / np.maximum(ref["bounds"][k], 1e-300), 0.0)
        i = np.unravel_index(np.argmax(ratio), ratio.shape)
        out[k] = (float(err.max()), float(ref["bounds"][k][i]), float(ratio[i]))
    return out


def layernorm_like(rng, n, d, score_scale=3.0):
    """n rows of norm sqrt(d) (what a LayerNorm without affine leaves), scaled by a with a^2 sqrt(d) = score_scale, so that the dot product of
    two unrelated rows (cosine ~ 1 / sqrt(d)) is of the order score_scale."""
    x = rng.standard_normal((n, d))
    x *= np.sqrt(d) / np.linalg.norm(x, axis=1, keepdims=True)
    return (x * np.sqrt(score_scale / np.sqrt(d))).astype(np.float32)


def make_inputs(B, d, K, seed):
    """A batch as the retriever produces: c1 leans towards q, c2 towards q_sp (the targets tend to win, not always), scores O(1-10)."""
    rng = np.random.default_rng(seed)
    q, qsp, n1, n2 = (layernorm_like(rng, B, d) for _ in range(4))
    mix = lambda a: (0.35 * a + 0.94 * layernorm_like(rng, B, d)).astype(np.float32)  # noqa: E731
    inp = {"q": q, "q_sp1": qsp, "c1": mix(q), "c2": mix(qsp), "neg_1": n1, "neg_2": n2}
    return inp, (layernorm_like(rng, K, d) if K else None)
