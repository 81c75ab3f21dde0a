"""Host statements for the overflow contract: an fp16 overflow anywhere in the backward reaches a parameter gradient as a
non-finite fp32 value, where the optimizer's norm kernel finds it. CPU only, numpy and torch; nothing here imports the product and nothing
here was measured on a kernel. Used by tests/test_overflow_host.py (the caps, on the references alone), tests/test_overflow_gpu.py (the bricks)
and tests/test_overflow_chain_gpu.py (the chain under FusedAdam).

classify   what an fp16 output element must be, from the fp64 reference value r and the element's DERIVED bound b (the brick's own
           *_grad_ref.py bound at unit scale, both multiplied by the power of two the gradient was multiplied by: the scaling is exact and
           commutes with every rounding but the last while nothing is subnormal):
             FINITE   |r| + b <  65520 and no intermediate fp16 rounding point that feeds the element overflows: finite and inside the bound
             INF      |r| - b >= 65520 and no such intermediate overflows: +Inf or -Inf, with the sign of r
             POISON   an intermediate fp16 rounding point that feeds the element certainly overflows: Inf of any sign, or NaN
             LEFT_OUT everything else (the element, or an intermediate, is within its bound of the edge)
           65520 is where round-to-nearest-even leaves the fp16 range: 65504 + half a last-place unit of 32.
ladder     the loss scaler on the chain: G1 is the largest magnitude any gradient-rounding point of the regime (tests/encoder_chain_ref.py) is
           handed at scale 1. A power-of-two scale s is SAFE if s G1 <= 65504 / 2, MUST overflow if s G1 >= 2 * 65520, and is UNDECIDED in
           between (at most two powers of two). The factor 2: the device's fp16 gradients differ from the regime's by per cent (DESIGN.md §18:
           0.82 to 1.17 of a 1.2e-2 regime error), and ten steps at lr = 2e-5 move no parameter by more than 2e-4; both are far inside a factor
           of 2, which costs one rung of the ladder.
"""
import numpy as np

import layernorm_grad_ref as nref
import linear_grad_ref as lref
import optim_ref
from oracle.fp import F16_EDGE, F16_MAX

LEFT_OUT, FINITE, INF, POISON = 0, 1, 2, 3
NAMES = {LEFT_OUT: "left out", FINITE: "finite", INF: "inf", POISON: "poison"}
MAX_LEFT_OUT, MIN_CLASS = 0.02, 0.05   # the caps: share of the live elements of one output


# ---- the classification ----------------------------------------------------------------------------------------------------------------------
def classify(r, b, poisoned=None, doubtful=None):
    """int8 array of the shape of r. poisoned / doubtful: bool arrays (broadcast against r) of the elements an intermediate rounding point that
    certainly / possibly overflows feeds."""
    r, b = np.asarray(r, np.float64), np.asarray(b, np.float64)
    assert r.shape == b.shape and (b >= 0).all() and np.isfinite(r).all() and np.isfinite(b).all()
    cls = np.full(r.shape, LEFT_OUT, np.int8)
    cls[np.abs(r) + b < F16_EDGE] = FINITE
    cls[np.abs(r) - b >= F16_EDGE] = INF
    if doubtful is not None:
        cls[np.broadcast_to(doubtful, r.shape)] = LEFT_OUT
    if poisoned is not None:
        cls[np.broadcast_to(poisoned, r.shape)] = POISON
    return cls


def shares(cls):
    """{class name: share of the elements}"""
    return {NAMES[c]: float((cls == c).mean()) for c in NAMES}


def cap_failures(cls, need_poison=False):
    """what of the caps a classification misses: [] = a case the device test may use"""
    s, bad = shares(cls), []
    if s["left out"] > MAX_LEFT_OUT:
        bad.append(f"{s['left out']:.3%} of the elements are left out (at most {MAX_LEFT_OUT:.0%})")
    for k in ("finite", "inf"):
        if s[k] < MIN_CLASS:
            bad.append(f"class {k} holds {s[k]:.3%} of the elements (at least {MIN_CLASS:.0%})")
    if need_poison and not (cls == POISON).any():
        bad.append("no element is fed by an overflowed intermediate")
    return bad


def verdicts(got, r, b, cls, label="", final_rounding_in_b=True):
    """the elements of an fp16 output that are not what their class says: a list of strings, [] = accepted. No tolerance but b.
    final_rounding_in_b: b covers the output's own rounding to fp16 (linear_grad_ref's does); False: b bounds the fp32 value in front of that
    rounding (layernorm_grad_ref's), and a finite element must lie between fp16(r - b) and fp16(r + b), the monotonic rule of
    oracle/trunk_rows_oracle.assert_f16."""
    got = np.asarray(got).astype(np.float64)
    r, b = np.asarray(r, np.float64), np.asarray(b, np.float64)
    assert got.shape == r.shape == cls.shape
    fin = np.isfinite(got)
    with np.errstate(invalid="ignore", over="ignore"):
        if final_rounding_in_b:
            inside = np.abs(np.where(fin, got, 0.0) - r) <= b
        else:
            inside = (got >= (r - b).astype(np.float16).astype(np.float64)) & (got <= (r + b).astype(np.float16).astype(np.float64))
        wrong = {"finite": (cls == FINITE) & ~(fin & inside),
                 "inf": (cls == INF) & ~(np.isinf(got) & (np.sign(got) == np.sign(r))),
                 "poison": (cls == POISON) & fin}
    out = []
    for k, w in wrong.items():
        if w.any():
            i = tuple(int(j) for j in np.argwhere(w)[0])
            out.append(f"{label} class {k}: {int(w.sum())} of {int((cls == {'finite': FINITE, 'inf': INF, 'poison': POISON}[k]).sum())} elements wrong; first at {i}: "
                       f"got {got[i]!r}, reference {r[i]!r}, bound {b[i]:.3e}")
    return out


def largest_power(limit, value):
    """the largest power of two s with s * value <= limit"""
    return 2.0 ** int(np.floor(np.log2(limit / value)))


# ---- the Linear's dX -------------------------------------------------------------------------------------------------------------------------
# linear_grad_ref.realistic: N(0, 1) gradients and weights x 0.02. dy is an fp16 INPUT, so the power it can carry ends where its own largest
# element leaves fp16 (2^13 for N(0, 1)), and dX = dZ W stays below 65520 for every N the kernel has (0.02 sqrt(N) 2^13 ~ 1e3 sqrt(N / 64)).
# The rest of the way is a second power of two on w, which is as exact: dX scales by s_dy s_w, dW and db by s_dy alone.
LINEAR_SHAPES = [(70, 67, 64, 64), (200, 197, 128, 192)]   # (M, rows, N, K): the shapes of part A
# the seed of each (M, gelu). With GELU a dZ must overflow while dy, an fp16 input at the largest power it can carry, does not: that takes an
# element with |dy| within 13 % of the largest at a u where gelu' > 1, which a few seeds in a hundred have (found on the host, from the reference
# alone: tests/test_overflow_host.py holds the caps)
LINEAR_SEEDS = {(70, False): 11, (70, True): 12, (200, False): 11, (200, True): 10}
LINEAR_CASES = [(M, rows, N, K, gelu) for M, rows, N, K in LINEAR_SHAPES for gelu in (False, True)]


def linear_case(M, rows, N, K, gelu, seed=None):
    """dict(x, w, dy, pre, rows, s_dy, s_w, ref = {"dx": (r, b), "dw": .., "db": .., "dz": ..} at the scaled inputs, cls = classes of dx
    [rows, K]). With GELU the pre-activation is the forward's of the SCALED weight (x w^T + b in fp64, rounded once), so that gelu' covers its
    whole range, 1.13 at the top: dZ = fp16(dy gelu'(u)) can then leave fp16 where dy itself does not."""
    seed = LINEAR_SEEDS[(M, gelu)] if seed is None else seed
    x, w, dy = lref.realistic(M, N, K, seed)
    s_dy = largest_power(F16_MAX, np.abs(dy.astype(np.float64)).max())
    best = None
    for e in range(0, 12):  # the power on w: the one whose INF share is nearest 30 %
        pre = poisoned = doubtful = None
        if gelu:
            pre = (x.astype(np.float64) @ (w.astype(np.float64) * 2.0 ** e).T + lref.bias(N, seed)).astype(np.float16)
        rb = lref.reference_and_bound(x, w, dy, pre, rows)
        if gelu:
            dz, edz = rb["dz"]
            over = (np.abs(dz) - edz) * s_dy >= F16_EDGE
            maybe = ((np.abs(dz) + edz) * s_dy >= F16_EDGE) & ~over
            poisoned, doubtful = over.any(axis=1, keepdims=True), (maybe.any(axis=1) & ~over.any(axis=1))[:, None]
        cls = classify(rb["dx"][0] * s_dy * 2.0 ** e, rb["dx"][1] * s_dy * 2.0 ** e, poisoned, doubtful)
        miss = abs(shares(cls)["inf"] - 0.30)
        if best is None or miss < best[0]:
            best = (miss, 2.0 ** e, cls, pre, rb, poisoned, doubtful)
    _, s_w, cls, pre, rb, poisoned, doubtful = best
    ws, dys = (w.astype(np.float64) * s_w).astype(np.float16), (dy.astype(np.float64) * s_dy).astype(np.float16)
    assert np.isfinite(dys).all() and np.isfinite(ws).all() and np.array_equal(ws.astype(np.float64), w.astype(np.float64) * s_w)
    ref = {"dx": tuple(a * s_dy * s_w for a in rb["dx"]), "dw": tuple(a * s_dy for a in rb["dw"]), "db": tuple(a * s_dy for a in rb["db"]),
           "dz": tuple(a * s_dy for a in rb["dz"])}
    return dict(x=x, w=ws, dy=dys, pre=pre, rows=rows, s_dy=s_dy, s_w=s_w, ref=ref, cls=cls, poisoned=poisoned, doubtful=doubtful)


# ---- the LayerNorm's dx16 --------------------------------------------------------------------------------------------------------------------
# layernorm_grad_ref's family small_1e-3 (rstd ~ 300): the one family whose dx leaves fp16 under a power that its fp16 dy survives.
LN_FORMS = {"dy16": ("f32", "none", True, None), "dy16+dy2": ("f32", "res32", True, "f32")}
LN_SHAPES = [(70, 67, 64), (70, 67, 768)]   # (M, rows, H): the scalar and the vector path


def layernorm_case(M, rows, H, form, seed=11):
    """dict(args = the scaled inputs of layernorm_grad_ref.reference_and_bound, rows, s, ref = {"dx", "dg", "db"} scaled, cls of dx [rows, H])"""
    case = nref.make_case("small_1e-3", LN_FORMS[form], M, H, seed)
    rb = nref.reference_and_bound(**case, m=rows)
    r0, b0 = rb["dx"]
    top = max(np.abs(case[k].astype(np.float64)).max() for k in ("dy16", "dy2") if case[k] is not None and case[k].dtype == np.float16)
    best = None
    for e in range(0, int(np.log2(largest_power(F16_MAX, top))) + 1):
        cls = classify(r0 * 2.0 ** e, b0 * 2.0 ** e)
        miss = abs(shares(cls)["inf"] - 0.30)
        if best is None or miss < best[0]:
            best = (miss, 2.0 ** e, cls)
    _, s, cls = best
    args = dict(case)
    for k in ("dy16", "dy2"):
        if case[k] is not None:
            args[k] = (case[k].astype(np.float64) * s).astype(case[k].dtype)
            assert np.isfinite(args[k]).all()
    return dict(args=args, rows=rows, s=s, ref={k: (v[0] * s, v[1] * s) for k, v in rb.items()}, cls=cls)


# ---- the attention's dQ | dK | dV ------------------------------------------------------------------------------------------------------------
# oracle/attention_oracle's family realistic1 and attention_grad_ref.dctx_grid (multiples of 1/8 up to 2), part A's geometry. dctx is an fp16
# INPUT and carries 2^14 at most, which leaves every output of that family finite. The rest of the way is three more powers of two on qkv, each
# applied before the fp16 cast, so the reference and the bound are simply those of the qkv the device is given:
#   V x 2^v       dP = dO V^T, and with it dS, dQ and dK, scale by 2^v; the softmax and dV do not change;
#   Q x 2^a, K / 2^a   the scores do not change; dK = dS^T Q / 8 gains 2^a over dS and can leave fp16 where no dS that feeds it does (the INF
#                 class: in mode 3 a dK element is ONE product dS_0j q_0c / 8, so without this every Inf in dK would be a poisoned one), dQ loses 2^a.
# The reference and the bound are taken at unit dctx and multiplied by 2^e, the power dctx carries: that scaling is exact.
# The listed intermediates: dS16 = fp16(p (dP - delta)) feeds dQ row i (over the keys) and dK row j (over the queries) of its head; the fp16
# p operand is at most 1 and never leaves fp16, so dV is fed by no overflow, and in mode 3 |dV_jc| = p_0j |dO_c| <= 65504 can never be Inf.
# The caps are therefore held by dQ | dK | dV as ONE output, the kernel's one buffer; its live elements are all of it in mode 0, and in mode 3
# all but the dQ rows behind a sequence's first, which are zeros with bound 0 (still classified, FINITE, and checked). (a, v, e) per mode were
# found on the host from the reference alone; tests/test_overflow_host.py holds the caps.
ATTN_HEADS, ATTN_LENS, ATTN_FAMILY, ATTN_SEED = 2, (1, 64, 65, 130), "realistic1", 11
ATTN_POWERS = {0: (5, 2, 14), 3: (5, 5, 14)}   # mode: (a, v, e)


def attention_case(mode):
    """dict(qkv, dctx, cu, heads, L, mode, ref = (r, b) of dQ | dK | dV at the scaled dctx, cls [T, 3 * hidden], live bool [T, 3 * hidden])"""
    import attention_grad_ref as aref
    from oracle import attention_oracle as ao
    a, v, e = ATTN_POWERS[mode]
    heads, hidden = ATTN_HEADS, 64 * ATTN_HEADS
    qkv, cu = ao.FAMILIES[ATTN_FAMILY](list(ATTN_LENS), heads, ATTN_SEED)
    wide = qkv.astype(np.float64)
    wide[:, :hidden] *= 2.0 ** a
    wide[:, hidden:2 * hidden] /= 2.0 ** a
    wide[:, 2 * hidden:] *= 2.0 ** v
    qkv = wide.astype(np.float16)
    assert np.isfinite(qkv).all()
    rows = (len(cu) - 1) if mode == 3 else int(cu[-1])
    unit, s = aref.dctx_grid(rows, hidden, 2, 1.0), 2.0 ** e
    dctx = aref.dctx_grid(rows, hidden, 2, s)
    assert np.isfinite(dctx).all() and np.array_equal(dctx.astype(np.float64), unit.astype(np.float64) * s)
    r, b = aref.reference_and_bound(qkv, unit, cu, heads, mode)
    lo, hi = aref.ds_feed(qkv, unit, cu, heads, mode)
    poisoned = lo * s >= F16_EDGE
    cls = classify(r * s, b * s, poisoned, (hi * s >= F16_EDGE) & ~poisoned)
    live = np.ones(r.shape, bool)
    if mode == 3:
        live[:, :hidden] = False
        live[np.asarray(cu[:-1], np.int64), :hidden] = True
    return dict(qkv=qkv, dctx=dctx, cu=cu, heads=heads, L=max(ATTN_LENS), mode=mode, ref=(r * s, b * s), cls=cls, live=live, poisoned=poisoned)


# ---- the O1 loss's gradients -----------------------------------------------------------------------------------------------------------------
# The six gradients are fp32, but each is the fp32 sum of two or three values that were rounded to fp16 (csrc/mdr_inbatch_grad.hip, rounding
# points 2 and 3: g once, then the result of every mm / bmm backward call). Those are the listed points, and mhop_loss_ref's recorder gives what
# each is handed, value t and error e in front of the rounding, so the classes are, per element:
#   POISON   a g that feeds it certainly overflows (|g| - dg >= 65520), or two of its terms certainly overflow with opposite signs (Inf - Inf)
#   INF      no g that feeds it can overflow, at least one term certainly does (|t| - e >= 65520), every term that can has that one's sign, and no
#            term is in doubt: Inf plus finite values, or plus Infs of the same sign, is that Inf
#   FINITE   nothing that feeds it can overflow (|.| + error < 65520 throughout): inside mhop_loss_ref's O1 bound, taken at the g0 itself (the O1
#            bound is a difference of fp16 roundings and not linear in the scale, so it is computed at the scale, not multiplied up to it)
#   LEFT_OUT the rest: something that feeds it is within its error of 65520
# g0 is the power of two the incoming gradient carries. With make_inputs' rows (elements ~ 0.3) a term |sum_j g_ij y_j| stays below the largest
# g that feeds it, so every Inf would be a poisoned one. As for the attention, q and q_sp1 are multiplied by 2^a and the contexts, negatives
# and queue divided by it: the scores do not change, dctx and dneg gain 2^a over g and dq loses it. (B, d, K) = (17, 64, 17): at d = 768
# make_inputs is a solved batch (p - onehot ~ 1e-7, a loss of 1e-7) whose gradients no fp32 g0 below 2^38 lifts out of fp16; at d = 64 the softmax
# is mixed. dq and dq_sp1 then hold no INF element at all (they lose 2^a), so the caps are held by the six gradients TOGETHER, one call's
# output; (a, g0) were found on the host from the reference alone, and tests/test_overflow_host.py holds the caps.
LOSS_SHAPE, LOSS_A, LOSS_G0 = (17, 64, 17), 3, 2.0 ** 21


def loss_case(shape=LOSS_SHAPE, a=LOSS_A, g0=LOSS_G0):
    """dict(inp, queue, g0, ref = {leaf: (r, b)}, cls = {leaf: [B, d]}): mhop_loss_ref.loss_and_grads(o1=True) at g0 and the classes above"""
    import mhop_loss_ref
    B, d, K = shape
    inp, queue = mhop_loss_ref.make_inputs(B, d, K, seed=7 * B + d + K)
    up = 2.0 ** a
    inp = {k: (v * up if k in ("q", "q_sp1") else v / up).astype(np.float32) for k, v in inp.items()}
    queue = (queue / up).astype(np.float32) if queue is not None else None
    rec = {}
    out = mhop_loss_ref.loss_and_grads(inp, queue, g0=g0, o1=True, record=rec)
    with np.errstate(invalid="ignore"):
        g_over = [np.abs(g) - dg >= F16_EDGE for g, dg in rec["g"]]              # per hop [B, N]
        g_maybe = [np.abs(g) + dg >= F16_EDGE for g, dg in rec["g"]]
    rows = np.arange(B)

    def fed(flags):  # per leaf, [B]: does a flagged g feed the row
        f0, f1 = flags
        return {"q": f0.any(axis=1), "q_sp1": f1.any(axis=1), "c1": (f0[:, :B] | f1[:, :B]).any(axis=0), "c2": (f0[:, B:2 * B] | f1[:, B:2 * B]).any(axis=0),
                "neg_1": f0[rows, 2 * B] | f1[rows, 2 * B], "neg_2": f0[rows, 2 * B + 1] | f1[rows, 2 * B + 1]}

    over, maybe = fed(g_over), fed(g_maybe)
    ref, cls = {}, {}
    for k in mhop_loss_ref.KEYS:
        sure_p, sure_n, can_p, can_n = (np.zeros((B, d), bool) for _ in range(4))
        for t, e in rec[k]:
            t, e = np.nan_to_num(t, nan=0.0, posinf=0.0, neginf=0.0), np.nan_to_num(e, nan=0.0, posinf=0.0, neginf=0.0)  # (rows a poisoned g feeds)
            sure_p |= t - e >= F16_EDGE
            sure_n |= -t - e >= F16_EDGE
            can_p |= t + e >= F16_EDGE
            can_n |= -t + e >= F16_EDGE
        c = np.full((B, d), LEFT_OUT, np.int8)
        c[~can_p & ~can_n] = FINITE
        c[(sure_p & ~can_n & (can_p == sure_p)) | (sure_n & ~can_p & (can_n == sure_n))] = INF
        c[sure_p & sure_n] = POISON
        c[maybe[k]] = LEFT_OUT
        c[over[k]] = POISON
        sign = np.where(sure_p, 1.0, -1.0)
        r = np.where(c == FINITE, np.nan_to_num(out["grads"][k], nan=0.0, posinf=0.0, neginf=0.0), sign)   # (INF: only the sign of r is used)
        b = np.where(c == FINITE, np.nan_to_num(out["bounds"][k], nan=0.0, posinf=0.0, neginf=0.0), 0.0)
        ref[k], cls[k] = (r, b), c
    return dict(inp=inp, queue=queue, g0=g0, ref=ref, cls=cls, rec=rec)


# ---- the ladder ------------------------------------------------------------------------------------------------------------------------------
SAFE, UNDECIDED, MUST = "safe", "undecided", "must overflow"


def scale_class(s, G1):
    if s * G1 <= F16_MAX / 2:
        return SAFE
    if s * G1 >= 2 * F16_EDGE:
        return MUST
    return UNDECIDED


def ladder(G1):
    """(the last safe power of two, the first that must overflow, the undecided powers in between)"""
    safe = largest_power(F16_MAX / 2, G1)
    must = 2.0 ** int(np.ceil(np.log2(2 * F16_EDGE / G1)))
    between = []
    s = 2 * safe
    while s < must:
        between.append(s)
        s *= 2
    assert scale_class(safe, G1) == SAFE and scale_class(2 * safe, G1) != SAFE and scale_class(must, G1) == MUST and scale_class(must / 2, G1) != MUST
    assert len(between) <= 2 and all(scale_class(s, G1) == UNDECIDED for s in between)
    return safe, must, between


def simulate(G1, start, steps, scale_window, undecided_overflow, beta1=0.9, beta2=0.999, max_scale=2.0 ** 24):
    """the scaler's run on a gradient that does not change: [(scale, class, bad)] per step and the final state. An undecided scale overflows or
    not as `undecided_overflow` (a bool, or a function of the scale) says; on the device its own skipped_last takes that place."""
    st, out = optim_ref.initial_state(start), []
    for _ in range(steps):
        s = float(st["loss_scale"])
        c = scale_class(s, G1)
        bad = c == MUST or (c == UNDECIDED and (undecided_overflow(s) if callable(undecided_overflow) else bool(undecided_overflow)))
        out.append((s, c, bad))
        st = optim_ref.advance(st, bad, beta1, beta2, 1, scale_window, max_scale)
    return out, st


def run_summary(events):
    """(skipped steps, clean steps, doublings, distinct undecided scales) of a run [(scale, class, bad)]"""
    doublings = sum(1 for a, b in zip(events, events[1:]) if b[0] == 2 * a[0])
    return sum(1 for e in events if e[2]), sum(1 for e in events if not e[2]), doublings, len({e[0] for e in events if e[1] == UNDECIDED})


# ---- the chain's inputs (parts C and D) ------------------------------------------------------------------------------------------------------
CHAIN = dict(batch="L48", lr=2e-5, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, max_grad_norm=2.0, scale_window=2, steps=10)
NO_DECAY = ("bias", "LayerNorm.weight")   # names of the reference trainer's second (undecayed) group


def chain_batches():
    """six encodes of one batch: {key: (ids, mask)}"""
    import encoder_chain_ref as ch
    ids, mask = ch.batch(CHAIN["batch"])
    return {k: (ids, mask) for k in ch.KEYS}


_G1 = {}


def chain_g1():
    """(G1, {rounding point: the largest |gradient| it is handed}) of the regime at the start parameters, scale 1; made once"""
    if not _G1:
        import encoder_chain_ref as ch
        with ch.record_grad_peaks() as peaks:
            ch.grads_loss("regime", ch.state_dict(), ch.GEOM, chain_batches())
            _G1["peaks"] = dict(peaks)
        _G1["G1"] = max(_G1["peaks"].values())
    return _G1["G1"], _G1["peaks"]
