"""Host restatement of the embedding backward (include/mdr_embedding_grad.h): the plan in numpy, the five gradients in fp64, a derived
elementwise error bound, an fp32 emulation of the kernels' dataflow (plan, pieces, order; with switchable mutations) and makers for the
inputs. numpy (the int sentinel comes from tests/guarded.py); nothing here is measured from a kernel. Test helper (tests/test_embedding_grad_host.py, tests/test_embedding_grad_gpu.py).

A case is a dict: ids int64 (any shape, indexed flat by tok_src), tok_src / tok_pid int32 [cap], total, word fp32 [vocab, H], pos fp32
[max_pos, H], type0, g fp32 [H], dy16 None or fp16 [cap, H], dy2 None or fp16 / fp32 [cap, H], pad_row.

Formulas, over the tokens t < total:
    wid = clamp(ids[tok_src[t]], 0, vocab - 1)      prow = clamp(tok_pid[t], 0, max_pos - 1)      x = (word[wid] + pos[prow]) + type0
    mu = mean(x)   A = mean((x - mu)^2) + eps   r = A^-1/2   xhat = (x - mu) r   dy = dy16 + dy2   a = dy g   c1 = mean(a)   c2 = mean(a xhat)
    d = r (a - c1 - xhat c2)
    dword[v] = sum of d over the tokens with wid = v, dpos[p] the same with prow = p; row pad_row of either is 0 (pad_row = -1: no such row)
    dtype0 = sum of d      dg = sum of dy xhat      db = sum of dy      (each + the old value with accumulate)

The plan (plan()): per table the tokens in np.argsort(kind="stable") order of their row, the segment starts, the segments' rows (-1 - row
for pad_row) and the number of segments.

The bound
---------
Derived from the rounding points listed at the top of csrc/mdr_embedding_grad.hip. u = 2^-24.
1 - 6. d: the derivation of tests/layernorm_grad_ref.py (its lines 1 - 6, restated by ln_terms below and compared with its
   reference_and_bound on the host), started from oracle/trunk_rows_oracle.py's embed_inputs: ex = u |w + p| + u |x|, two rounded adds.
   The statistics add the lane's H / 64 columns l + 64 i in order at every H, then the butterfly: D = H / 64 + 6, as there.
7. A table row with the terms d_1 .. d_n in token order, each known to Ed_i: the device adds them in pieces of P, the pieces in order, the
   old value last, so a term passes through at most Aadd = (P - 1) + ceil(n / P) + 1 additions:
       E = sum(Ed_i) + Aadd u (sum(|d_i| + Ed_i) + |old|).
8. dtype0, dg and db under the chunk split (chunks(): rows_per_chunk / 4 + 4 + S + 1 additions), the same form:
       E = sum(Eterm) + Nadd u (sum(|term| + Eterm) + |old|),  term = d (Ed), dy xhat (the product's Eterm of layernorm_grad_ref) or dy (Edy).
A final factor 1 + 2^-10 covers the neglected products of two error terms. Every constant is a format's, a count or the ISA's 1 ulp of
v_rsq_f32; no term was read off a device.
"""
import numpy as np

import layernorm_grad_ref as lref
from guarded import ISENTINEL
from oracle import fp
from oracle import trunk_rows_oracle as tr
from oracle.fp import U32

P = 16                        # MDR_EMBEDDING_PIECE
PLAN_HEADER = 16
PLAN_MAGIC = 0x4D455031
WAVES = 4
STRANDS = 16
MAX_CHUNKS = 1024
MAX_PARTIAL_BYTES = 4 << 20
EPS = 1e-5
VOCAB, MAX_POS = 97, 40       # small tables: collisions are the rule
OUTPUTS = ("d", "dword", "dpos", "dtype0", "dg", "db")

MUTATIONS = ("pad_not_skipped", "oob_dropped", "last_token_dropped", "first_piece_dropped", "pos_from_src", "dtype0_mean", "accumulate_ignored",
             "extra_token", "stats_without_type0")
FAMILIES = ("unit", "mean30", "const", "outlier40", "small_1e-3")
DY_FORMS = ("dy16", "dy2_f32", "both")
HS = [64, 192, 768, 1024]
# (B, L): token counts 1, 3, 4, 5 and a few hundred; cap = B L > total in every one (make_pack masks at least one position out)
BL_SWEEP = [(1, 2), (2, 2), (1, 5), (2, 3), (7, 50)]
# A batch of 150 sequences, the README's training batch, at 25 positions: cap = 3750 and about 1900 tokens, so that at H = 768 and 1024 a wave
# of emb_ln_grad_kernel walks three tokens with dg, db and dtype0 in registers (rows_per_chunk = 12), hundreds of chunks lie behind `total`,
# and the longest table rows own more than 8 P tokens: emb_scatter_kernel sums 8 pieces per round and goes round again. (kind, pad_row): with
# "random" the longest rows of both tables are the pad id's and the pad position's, which only pad_row = -1 sums; with "equal" one word row
# owns every token. assert_large() states the properties. The host emulation runs over all of it (under a second a case).
BL_LARGE = (150, 25)
HS_LARGE = [768, 1024]
KINDS_LARGE = [("random", -1), ("equal", 1)]
ROUND = 8 * P                 # tokens of one round of emb_scatter_kernel: kEgScatterWaves pieces


def chunks(cap, H):
    """(S, rows_per_chunk) of mdr_embedding_backward_chunks: a function of (cap, H) alone."""
    if cap < 1 or cap > 1 << 20 or H < 64 or H > 1024 or H % 64:
        return 0, 0
    most = min(MAX_CHUNKS, MAX_PARTIAL_BYTES // (12 * H))
    rpc = ((cap + most - 1) // most + 3) // 4 * 4
    return (cap + rpc - 1) // rpc, rpc


def longest_summed_segments(case):
    """(word, pos): the most tokens a table row owns that the scatter sums (pad_row is skipped)"""
    out = []
    for keys in rows(case):
        n = np.bincount(keys)
        if 0 <= case["pad_row"] < len(n):
            n[case["pad_row"]] = 0
        out.append(int(n.max(initial=0)))
    return tuple(out)


def assert_large(case, chunks_of=None):
    """A case at BL_LARGE: rows_per_chunk >= 12, whole chunks behind `total`, and a longest summed segment of more than one round in the
    word table (pad_row = -1: in both tables). Returns (S, rows_per_chunk, longest word segment, longest position segment)."""
    cap, H = len(case["tok_src"]), case["word"].shape[1]
    S, rpc = (chunks_of or chunks)(cap, H)
    lw, lp = longest_summed_segments(case)
    assert rpc >= 3 * WAVES and case["total"] + rpc < (S - 1) * rpc and lw > ROUND and (lp > ROUND or case["pad_row"] >= 0), (cap, H, S, rpc, case["total"], lw, lp)
    return S, rpc, lw, lp


def plan_layout(cap):
    stride = (3 * cap + 1 + 3) // 4 * 4
    out = {"words": PLAN_HEADER + 2 * stride + 2 * cap}
    for i, name in enumerate(("word", "pos")):
        base = PLAN_HEADER + i * stride
        out[name] = {"order": base, "seg_start": base + cap, "seg_row": base + 2 * cap + 1, "key": PLAN_HEADER + 2 * stride + i * cap}
    return out


def rows(case, total=None, mutation=None):
    """(wid, prow) int64 [total]: the table rows of the valid tokens, clamped as the forward reads them"""
    total = case["total"] if total is None else total
    src = case["tok_src"][:total].astype(np.int64)
    wid = np.clip(case["ids"].reshape(-1)[src], 0, case["word"].shape[0] - 1)
    pid = src if mutation == "pos_from_src" else case["tok_pid"][:total].astype(np.int64)
    return wid, np.clip(pid, 0, case["pos"].shape[0] - 1)


def plan_table(keys, pad_row):
    """dict(order, seg_start [nseg + 1], seg_row [nseg], nseg) for the rows `keys` of the valid tokens"""
    keys = np.asarray(keys, np.int64)
    order = np.argsort(keys, kind="stable").astype(np.int32)
    sk = keys[order]
    heads = np.flatnonzero(np.concatenate([[True], sk[1:] != sk[:-1]])) if len(sk) else np.zeros(0, np.int64)
    seg_row = sk[heads]
    seg_row = np.where(seg_row == pad_row, -1 - seg_row, seg_row).astype(np.int32)
    return dict(order=order, seg_start=np.concatenate([heads, [len(sk)]]).astype(np.int32), seg_row=seg_row, nseg=len(heads))


def plan(case):
    wid, prow = rows(case)
    return {"word": plan_table(wid, case["pad_row"]), "pos": plan_table(prow, case["pad_row"])}


def assert_plan(got, case, label=""):
    """got: the device's plan words (int32, filled with ISENTINEL before the call). Header, order, segment tables and keys equal numpy's;
    what lies behind them still holds ISENTINEL."""
    cap, total = len(case["tok_src"]), case["total"]
    lay, exp = plan_layout(cap), plan(case)
    keys = dict(zip(("word", "pos"), rows(case)))
    head = [PLAN_MAGIC, total, exp["word"]["nseg"], exp["pos"]["nseg"], cap, case["word"].shape[0], case["pos"].shape[0], case["pad_row"]] + [0] * 8
    tr.assert_ints(got[:PLAN_HEADER], np.asarray(head, np.int32), "header", label)
    for name in ("word", "pos"):
        o, e = lay[name], exp[name]
        n = e["nseg"]
        for sec, want, room in (("order", e["order"], cap), ("seg_start", e["seg_start"], cap + 1), ("seg_row", e["seg_row"], cap),
                                ("key", keys[name].astype(np.int32), cap)):
            sl = got[o[sec]:o[sec] + room]
            tr.assert_ints(sl[:len(want)], want, f"{name} {sec}", label)
            tr.assert_ints(sl[len(want):], np.full(room - len(want), ISENTINEL, np.int32), f"{name} {sec} behind its end", label)
        assert n <= total


# ---- fp64 statement and bound ----------------------------------------------------------------------------------------------------------
def ln_terms(x, ex, dy16, dy2, g, eps):
    """lines 1 - 6 of tests/layernorm_grad_ref.py's bound for rows x known to ex: dict(d, Ed, dy, Edy, t, Et), float64 [m, H]"""
    m, H = x.shape
    D = H // 64 + 6
    mean = lref._mean
    st = lref.stats(x, ex, eps)
    r, t, Et, rho_r = st["r"], st["t"], st["Et"], st["rho_r"]
    assert np.isfinite(rho_r).all(), "the bound says nothing here (rho_A >= 1): not a family to test with"
    at = np.abs(t)
    G = np.asarray(g, np.float64)
    dy, Edy = lref._dy64(dy16, dy2, m)
    a = dy * G
    Ea = np.abs(G) * Edy + U32 * (np.abs(a) + np.abs(G) * Edy)
    c1 = mean(a)
    Ec1 = mean(Ea) + D * U32 * mean(np.abs(a) + Ea) + 3 * U32 * np.abs(c1)
    p = a * t
    Ep = at * Ea + (np.abs(a) + Ea) * Et
    Ep = Ep + U32 * (np.abs(p) + Ep)
    c2 = mean(p)
    Ec2 = mean(Ep) + D * U32 * mean(np.abs(p) + Ep) + 3 * U32 * np.abs(c2)
    q = t * c2
    Eq = at * Ec2 + (np.abs(c2) + Ec2) * Et
    Eq = Eq + U32 * (np.abs(q) + Eq)
    E1 = Ea + Ec1
    E1 = E1 + U32 * (np.abs(a - c1) + E1)
    w = a - c1 - q
    Ew = E1 + Eq
    Ew = Ew + U32 * (np.abs(w) + Ew)
    d = r * w
    Ed = r * (1 + rho_r) * Ew
    Ed = (Ed + np.abs(d) * (rho_r + U32) + U32 * Ed) * (1 + 2.0 ** -10)
    return dict(d=d, Ed=Ed, dy=dy, Edy=Edy, t=t, Et=Et)


def _sum_bound(term, Eterm, nadd, old):
    """value and bound of a sum of terms (axis 0) that pass through at most nadd additions, the old value last"""
    o = np.zeros(term.shape[1]) if old is None else old.astype(np.float64)
    return term.sum(axis=0) + o, (Eterm.sum(axis=0) + nadd * U32 * ((np.abs(term) + Eterm).sum(axis=0) + np.abs(o))) * (1 + 2.0 ** -10)


def _table(d, Ed, keys, nrows, pad_row, old):
    H = d.shape[1]
    ref = np.zeros((nrows, H)) if old is None else old.astype(np.float64).copy()
    bnd = np.zeros((nrows, H))
    for v in np.unique(keys):
        if v == pad_row:
            continue
        sel = keys == v
        n = int(sel.sum())
        ref[v], bnd[v] = _sum_bound(d[sel], Ed[sel], (P - 1) + (n + P - 1) // P + 1, None if old is None else old[v])
    return ref, bnd


def reference_and_bound(case, eps=EPS, old=None, d_given=None):
    """{"d", "dword", "dpos", "dtype0", "dg", "db"} -> (reference, bound), float64; d has `total` rows. old: None or a dict of the old
    values of the accumulating outputs. d_given: fp32 [cap, H] -- the scatter alone: d is an exact input (Ed = 0) and dg, db are absent."""
    total, cap, H = case["total"], len(case["tok_src"]), case["word"].shape[1]
    old = old or {}
    wid, prow = rows(case)
    out = {}
    if d_given is None:
        x, ex = tr.embed_inputs(case["word"], case["pos"], case["type0"][None, :], wid, prow, np.zeros_like(wid))
        T = ln_terms(x, ex, case["dy16"], case["dy2"], case["g"], eps)
        d, Ed = T["d"], T["Ed"]
    else:
        d, Ed = d_given[:total].astype(np.float64), np.zeros((total, H))
    S, rpc = chunks(cap, H)
    nadd = rpc // WAVES + 4 + S + 1
    out["d"] = (d, Ed)
    out["dword"] = _table(d, Ed, wid, case["word"].shape[0], case["pad_row"], old.get("dword"))
    out["dpos"] = _table(d, Ed, prow, case["pos"].shape[0], case["pad_row"], old.get("dpos"))
    out["dtype0"] = _sum_bound(d, Ed, nadd, old.get("dtype0"))
    if d_given is None:
        dy, Edy, t, Et = T["dy"], T["Edy"], T["t"], T["Et"]
        term = dy * t
        Eterm = np.abs(t) * Edy + (np.abs(dy) + Edy) * Et
        Eterm = Eterm + U32 * (np.abs(term) + Eterm)
        out["dg"] = _sum_bound(term, Eterm, nadd, old.get("dg"))
        out["db"] = _sum_bound(dy, Edy, nadd, old.get("db"))
    return out


# ---- the emulation -------------------------------------------------------------------------------------------------------------------------
def _lanes(a):
    """[rows, H] -> [rows, 64 lanes, H / 64]: lane l holds columns l + 64 i, at every H"""
    R, H = a.shape
    return a.reshape(R, H // 64, 64).transpose(0, 2, 1)


def _split_sum(term, cap, H, old):
    """the chunk / wave / strand sum of csrc/mdr_embedding_grad.hip over the rows of `term` (fp32 [m, H], m <= cap), the old value last"""
    f32 = np.float32
    S, rpc = chunks(cap, H)
    padded = np.concatenate([term, np.zeros((S * rpc - term.shape[0], H), f32)]).reshape(S, rpc // WAVES, WAVES, H)
    w = np.zeros((S, WAVES, H), f32)
    for k in range(rpc // WAVES):
        w = w + padded[:, k]
    part = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
    out = None
    for j in range(min(STRANDS, S)):
        s = np.zeros(H, f32)
        for c in range(j, S, STRANDS):
            s = s + part[c]
        out = s if out is None else out + s
    return out if old is None else out + old.astype(f32)


def emulate_scatter(d32, keys, nrows, pad_row, old=None, accumulate=False, mutation=None):
    """the segmented sum in fp32: pieces of P from 0 in token order, the pieces from 0 in order, the old value last. accumulate False: zeros
    elsewhere; True: `old` elsewhere."""
    f32 = np.float32
    H = d32.shape[1]
    keep_old = accumulate and mutation != "accumulate_ignored"
    out = old.astype(f32).copy() if accumulate else np.zeros((nrows, H), f32)
    pl = plan_table(keys, -1 if mutation == "pad_not_skipped" else pad_row)
    for s in range(pl["nseg"]):
        row = int(pl["seg_row"][s])
        if row < 0:
            continue
        toks = pl["order"][pl["seg_start"][s]:pl["seg_start"][s + 1]]
        if mutation == "last_token_dropped":
            toks = toks[:-1]
        tot = np.zeros(H, f32)
        for k in range(0, len(toks), P):
            acc = np.zeros(H, f32)
            for t in toks[k:k + P]:
                acc = acc + d32[t]
            if not (mutation == "first_piece_dropped" and k == 0 and len(toks) > P):
                tot = tot + acc
        out[row] = tot + out[row] if keep_old else tot
    return out


def emulate(case, eps=EPS, old=None, accumulate=False, mutation=None):
    """The kernels' dataflow in numpy, every operation rounded to fp32 (no fused multiply-add): dict of d [total, H], dword, dpos, dtype0,
    dg, db (float32). `old`: dict of the old values (all five) when accumulate.

    mutation (None: the correct dataflow) switches ONE defect on: pad_not_skipped: pad_row gets its sums; oob_dropped: a token whose id or
    position is out of range adds nothing to the tables instead of joining the clamped row; last_token_dropped: of every segment;
    first_piece_dropped: of every segment longer than P; pos_from_src: the position row taken from tok_src; dtype0_mean: divided by the
    token count; accumulate_ignored: the old values not added; extra_token: the token at `total` taken as valid; stats_without_type0: mu and
    rstd from word + pos alone."""
    assert mutation is None or mutation in MUTATIONS
    f32 = np.float32
    cap, H = len(case["tok_src"]), case["word"].shape[1]
    total = case["total"] + (1 if mutation == "extra_token" else 0)
    assert total <= cap
    wid, prow = rows(case, total, mutation)
    with np.errstate(all="ignore"):
        wp = case["word"][wid] + case["pos"][prow]
        x = wp + case["type0"]
        xs = wp if mutation == "stats_without_type0" else x
        dy = None
        for part in (case["dy16"], case["dy2"]):
            if part is not None:
                dy = part[:total].astype(f32) if dy is None else dy + part[:total].astype(f32)
        Hf = f32(H)
        xl = _lanes(xs)
        mu = lref._row_sum(xl, False, False) / Hf
        dl = xl - mu[:, :, None]
        var = lref._row_sum(dl * dl, False, False) / Hf
        rstd = (f32(1) / np.sqrt((var + f32(eps)).astype(np.float64))).astype(f32)
        xh = (xs - mu) * rstd
        a = dy * case["g"]
        c1 = lref._row_sum(_lanes(a), False, False) / Hf
        c2 = lref._row_sum(_lanes(a * xh), False, False) / Hf
        d = (rstd * ((a - c1) - xh * c2)).astype(f32)
        old = old or {}
        kw, kp = wid.copy(), prow.copy()
        dt = d
        if mutation == "oob_dropped":
            raw_id = case["ids"].reshape(-1)[case["tok_src"][:total].astype(np.int64)]
            raw_pid = case["tok_pid"][:total].astype(np.int64)
            keep_w = (raw_id >= 0) & (raw_id < case["word"].shape[0])
            keep_p = (raw_pid >= 0) & (raw_pid < case["pos"].shape[0])
            dword = emulate_scatter(np.where(keep_w[:, None], d, f32(0)), kw, case["word"].shape[0], case["pad_row"], old.get("dword"), accumulate)
            dpos = emulate_scatter(np.where(keep_p[:, None], d, f32(0)), kp, case["pos"].shape[0], case["pad_row"], old.get("dpos"), accumulate)
        else:
            dword = emulate_scatter(dt, kw, case["word"].shape[0], case["pad_row"], old.get("dword"), accumulate, mutation)
            dpos = emulate_scatter(dt, kp, case["pos"].shape[0], case["pad_row"], old.get("dpos"), accumulate, mutation)
        keep_old = accumulate and mutation != "accumulate_ignored"
        sums = {}
        for name, term in (("dtype0", d), ("dg", dy * xh), ("db", dy)):
            sums[name] = _split_sum(term.astype(f32), cap, H, old.get(name) if keep_old else None)
        if mutation == "dtype0_mean":
            sums["dtype0"] = (sums["dtype0"] / f32(max(total, 1))).astype(f32)
    return dict(d=d[:case["total"]], dword=dword, dpos=dpos, **sums)


def worst_shares(got, rb, keys=None):
    """{output: largest |got - ref| / bound} (oracle/fp.py, worst_ratio, per output)"""
    return {k: fp.worst_ratio(got[k], *rb[k])[0] for k in (keys or rb) if k in got}


# ---- makers --------------------------------------------------------------------------------------------------------------------------------
def make_pack(kind, B, L, seed, pad_id=1, vocab=VOCAB):
    """ids, mask int64 [B, L] and the packing of oracle/trunk_rows_oracle.py: dict(ids, tok_src, tok_pid [B L, ISENTINEL from total on], total).
    Masks are NOT prefixes (a random subset of every row, at least one position of the batch masked out, so cap > total); kind: random ids
    in 0 .. vocab - 1 with pad ids inside; equal: one id; distinct: no id twice (B L <= vocab); range: -5, 0, vocab - 1 and vocab + 7 mixed
    in; empty: random with sequences of length 0 first, last and in between; none: total = 0. L > MAX_POS - 2 makes tok_pid pass max_pos."""
    rng = np.random.default_rng([seed, B, L, sum(map(ord, kind))])
    n = np.full(B, L) if B * L <= 8 else rng.integers(1, L + 1, B)  # (the tiny batches are full but for one position: 1, 3, 4, 5 tokens)
    if kind == "empty":
        n[::3] = 0
        n[-1] = 0
    if kind == "none":
        n[:] = 0
    if n.sum() == B * L:
        n[0] -= 1
    mask = np.zeros((B, L), np.int64)
    for b in range(B):
        mask[b, rng.permutation(L)[:n[b]]] = rng.choice(np.asarray([1, 2, -1]))
    ids = rng.integers(0, vocab, (B, L)).astype(np.int64)
    if kind == "equal":
        ids[:] = 5
    elif kind == "distinct":
        assert B * L <= vocab
        ids = rng.permutation(vocab)[:B * L].reshape(B, L).astype(np.int64)
    elif kind == "range":
        ids[rng.random((B, L)) < 0.4] = 0
        sel = rng.random((B, L))
        ids[sel < 0.15] = -5
        ids[(sel >= 0.15) & (sel < 0.3)] = vocab + 7
        ids[(sel >= 0.3) & (sel < 0.45)] = vocab - 1
    if kind not in ("equal", "distinct"):
        ids[rng.random((B, L)) < 0.1] = pad_id
    pk = tr.pack(ids, mask, pad_id)
    total, cap = int(pk["total"][0]), B * L
    assert total < cap
    src, pid = np.full(cap, ISENTINEL, np.int32), np.full(cap, ISENTINEL, np.int32)
    src[:total], pid[:total] = pk["tok_src"], pk["tok_pid"]
    return dict(ids=ids, tok_src=src, tok_pid=pid, total=total)


def make_tables(family, H, seed, vocab=VOCAB, max_pos=MAX_POS):
    """word, pos, type0, g: x = (word + pos) + type0 keeps the family's character (pos and type0 are small N(0, 1) / 16 perturbations in
    the family's scale, except for the constant rows, where they are the constants 1 and 0.5)"""
    rng = np.random.default_rng([seed, H, sum(map(ord, family))])
    word = lref._rows(family, rng, vocab, H).astype(np.float32)
    scale = (1e-3 if family == "small_1e-3" else 1.0) * 0.0625
    pos = (np.ones((max_pos, H)) if family == "const" else scale * rng.standard_normal((max_pos, H))).astype(np.float32)
    type0 = (np.full(H, 0.5) if family == "const" else scale * rng.standard_normal(H)).astype(np.float32)
    g = (1.0 + 0.3 * rng.standard_normal(H)).astype(np.float32)
    return dict(word=word, pos=pos, type0=type0, g=g)


def make_dy(form, cap, H, seed):
    rng = np.random.default_rng([seed, cap, H, sum(map(ord, form))])
    d = rng.standard_normal((cap, H))
    if form == "dy16":
        return dict(dy16=d.astype(np.float16), dy2=None)
    if form == "dy2_f32":
        return dict(dy16=None, dy2=d.astype(np.float32))
    return dict(dy16=(0.5 * d).astype(np.float16), dy2=(0.5 * d).astype(np.float32))


def make_case(family, H, B, L, seed, kind="random", form="both", pad_row=1):
    return dict(**make_pack(kind, B, L, seed), **make_tables(family, H, seed), **make_dy(form, B * L, H, seed), pad_row=pad_row)


def make_flat(counts, seed, cap_extra=3, vocab=VOCAB, max_pos=MAX_POS):
    """A packing given directly: counts = {id: number of tokens}; the tokens are shuffled, tok_src is the identity on a flat ids array and
    tok_pid a seeded draw in 0 .. max_pos - 1. cap = total + cap_extra."""
    rng = np.random.default_rng([seed, len(counts), sum(counts.values())])
    flat = rng.permutation(np.concatenate([np.full(n, v, np.int64) for v, n in counts.items()]))
    total, cap = len(flat), len(flat) + cap_extra
    ids = np.concatenate([flat, np.full(cap_extra, 3, np.int64)])
    src, pid = np.full(cap, ISENTINEL, np.int32), np.full(cap, ISENTINEL, np.int32)
    src[:total], pid[:total] = np.arange(total), rng.integers(0, max_pos, total)
    return dict(ids=ids, tok_src=src, tok_pid=pid, total=total)


def exact_tables(case, d32, old=None):
    """the integer sums of a d on the grid of multiples of 1/8: dict(dword, dpos, dtype0) float32, exact in any order"""
    total = case["total"]
    wid, prow = rows(case)
    d = d32[:total].astype(np.float64)
    old = old or {}
    out = {}
    for name, keys, n in (("dword", wid, case["word"].shape[0]), ("dpos", prow, case["pos"].shape[0])):
        t = np.zeros((n, d.shape[1]))
        sel = keys != case["pad_row"]
        np.add.at(t, keys[sel], d[sel])
        if name in old:
            touched = np.zeros(n, bool)
            touched[keys[sel]] = True
            t = np.where(touched[:, None], t + old[name].astype(np.float64), old[name].astype(np.float64))
        out[name] = t
    out["dtype0"] = d.sum(axis=0) + (old["dtype0"].astype(np.float64) if "dtype0" in old else 0.0)
    for k, v in out.items():
        assert (v * 8 == np.round(v * 8)).all() and np.abs(v).max(initial=0) * 8 < 2 ** 24, k
        out[k] = v.astype(np.float32)
    return out
