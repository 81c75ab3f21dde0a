"""Host restatement of the READER's embedding backward (include/mdr_reader_embedding_grad.h), built on tests/embedding_grad_ref.py: the
plan in numpy, the gradients in fp64 with a derived elementwise bound, an fp32 emulation of the kernels' dataflow with switchable mutations,
and makers for the inputs. numpy; nothing here is measured from a kernel. Test helper (tests/test_reader_embedding_grad_host.py,
tests/test_reader_embedding_grad_gpu.py).

A case is a dict: ids int64 [B, L], types None or int64 [B, L], tok_src int32 [cap = B L] (ISENTINEL from total on), total, L, word fp32
[vocab, H], pos fp32 [max_pos, H], type fp32 [TV, H], g fp32 [H], dy16 None or fp16 [cap, H], dy2 None or fp16 / fp32 [cap, H], pad_row.

Formulas, over the tokens t < total (the rest as tests/embedding_grad_ref.py states them):
    wid = clamp(ids[tok_src[t]], 0, vocab - 1)      prow = tok_src[t] % L      ty = clamp(types[tok_src[t]], 0, TV - 1), 0 without types
    x = (word[wid] + pos[prow]) + type[ty]          d = the LayerNorm backward of x
    dword[v] = sum of d over wid = v, row pad_row is 0;   dpos[p] = sum of d over prow = p, EVERY row (the position table has no pad row)
    dtype[k] = sum of d over ty = k      dg = sum of dy xhat      db = sum of dy      (each + the old value with accumulate)

The bound is that helper's, line for line: d by ln_terms from embed_inputs' two rounded adds (lines 1 - 6), a table row by _table (line 7),
dg, db and each dtype[k] by _sum_bound under the chunk split of (cap, H) (line 8; a row of dtype passes through no more additions than
dtype0 does: the tokens of other types add nothing to it). No term was read off a device.
"""
import numpy as np

import embedding_grad_ref as ref
import layernorm_grad_ref as lref
from guarded import ISENTINEL
from oracle import trunk_rows_oracle as tr

P = ref.P
PLAN_HEADER = ref.PLAN_HEADER
READER_PLAN_MAGIC = 0x4D455032
MAX_TYPES = 4
EPS = 1e-12                    # ELECTRA's layer_norm_eps
VOCAB, MAX_POS = 97, 40
OUTPUTS = ("d", "dword", "dpos", "dtype", "dg", "db")
HS = [64, 128, 1024]
MUTATIONS = ("pos_pad_skipped", "pos_row0_dropped", "type_all_to_row0", "type_unclamped_dropped", "pos_from_count", "word_pad_not_skipped",
             "stats_with_type0", "accumulate_ignored", "extra_token")


def rows(case, total=None, mutation=None):
    """(wid, prow, ty) int64 [total]: the table rows of the valid tokens, as the forward reads them"""
    total = case["total"] if total is None else total
    src = case["tok_src"][:total].astype(np.int64)
    wid, prow, ty = tr.embed_rows(case["ids"].reshape(-1), src, None, case["word"], case["pos"], case["type"], case["types"], case["L"])
    if mutation == "pos_from_count":  # RoBERTa-style: 1-based counts of the non-pad tokens, offset by the pad id
        pid = tr.position_ids_full(case["ids"], max(case["pad_row"], 0)).reshape(-1)[src]
        prow = np.clip(pid, 0, case["pos"].shape[0] - 1)
    return wid, prow, ty


def plan(case):
    wid, prow, _ = rows(case)
    return {"word": ref.plan_table(wid, case["pad_row"]), "pos": ref.plan_table(prow, -1)}


def plan_header(case):
    cap, pl = len(case["tok_src"]), plan(case)
    return np.asarray([READER_PLAN_MAGIC, case["total"], pl["word"]["nseg"], pl["pos"]["nseg"], cap, case["word"].shape[0], case["pos"].shape[0],
                       case["pad_row"], -1, case["L"]] + [0] * 6, np.int32)


def assert_plan(got, case, label=""):
    """got: the device's plan words (int32, ISENTINEL before the call): header, order, segment tables and keys equal numpy's; what lies
    behind them still holds ISENTINEL."""
    cap = len(case["tok_src"])
    lay, exp = ref.plan_layout(cap), plan(case)
    wid, prow, _ = rows(case)
    tr.assert_ints(got[:PLAN_HEADER], plan_header(case), "header", label)
    for name, keys in (("word", wid), ("pos", prow)):
        o, e = lay[name], exp[name]
        for sec, want, room in (("order", e["order"], cap), ("seg_start", e["seg_start"], cap + 1), ("seg_row", e["seg_row"], cap),
                                ("key", keys.astype(np.int32), cap)):
            sl = got[o[sec]:o[sec] + room]
            tr.assert_ints(sl[:len(want)], want, f"{name} {sec}", label)
            tr.assert_ints(sl[len(want):], np.full(room - len(want), ISENTINEL, np.int32), f"{name} {sec} behind its end", label)
    assert (exp["pos"]["seg_row"] >= 0).all(), "the position table has no pad row"


# ---- fp64 statement and bound ----------------------------------------------------------------------------------------------------------
def reference_and_bound(case, eps=EPS, old=None):
    """{"d", "dword", "dpos", "dtype", "dg", "db"} -> (reference, bound), float64; d has `total` rows, dtype [TV, H]."""
    total, cap, H = case["total"], len(case["tok_src"]), case["word"].shape[1]
    old = old or {}
    wid, prow, ty = rows(case)
    x, ex = tr.embed_inputs(case["word"], case["pos"], case["type"], wid, prow, ty)
    T = ref.ln_terms(x, ex, case["dy16"], case["dy2"], case["g"], eps)
    d, Ed = T["d"], T["Ed"]
    S, rpc = ref.chunks(cap, H)
    nadd = rpc // ref.WAVES + 4 + S + 1
    out = {"d": (d, Ed)}
    out["dword"] = ref._table(d, Ed, wid, case["word"].shape[0], case["pad_row"], old.get("dword"))
    out["dpos"] = ref._table(d, Ed, prow, case["pos"].shape[0], -1, old.get("dpos"))
    TV = case["type"].shape[0]
    tref, tbnd = np.zeros((TV, H)), np.zeros((TV, H))
    for k in range(TV):
        sel = ty == k
        tref[k], tbnd[k] = ref._sum_bound(d[sel], Ed[sel], nadd, None if "dtype" not in old else old["dtype"][k])
    out["dtype"] = (tref, tbnd)
    dy, Edy, t, Et = T["dy"], T["Edy"], T["t"], T["Et"]
    term = dy * t
    Eterm = np.abs(t) * Edy + (np.abs(dy) + Edy) * Et
    Eterm = Eterm + ref.U32 * (np.abs(term) + Eterm)
    out["dg"] = ref._sum_bound(term, Eterm, nadd, old.get("dg"))
    out["db"] = ref._sum_bound(dy, Edy, nadd, old.get("db"))
    return out


# ---- the emulation -------------------------------------------------------------------------------------------------------------------------
def emulate(case, eps=EPS, old=None, accumulate=False, mutation=None):
    """The kernels' dataflow in numpy, every operation rounded to fp32 (no fused multiply-add): dict of d [total, H], dword, dpos, dtype,
    dg, db (float32). `old`: dict of the old values when accumulate.

    mutation (None: the correct dataflow) switches ONE defect on. pos_pad_skipped: the retriever's rule, row pad_row of the position table
    gets nothing; pos_row0_dropped: position row 0 gets nothing; type_all_to_row0: every token's d joins dtype[0]; type_unclamped_dropped: a
    type id outside 0 .. TV - 1 adds to no row; pos_from_count: the position rows RoBERTa's way; word_pad_not_skipped; stats_with_type0: x
    built with type[0] for every token; accumulate_ignored; extra_token: the token at `total` taken as valid."""
    assert mutation is None or mutation in MUTATIONS
    f32 = np.float32
    cap, H, TV = len(case["tok_src"]), case["word"].shape[1], case["type"].shape[0]
    total = case["total"] + (1 if mutation == "extra_token" else 0)
    assert total <= cap
    wid, prow, ty = rows(case, total, mutation)
    with np.errstate(all="ignore"):
        x = (case["word"][wid] + case["pos"][prow]) + case["type"][np.zeros_like(ty) if mutation == "stats_with_type0" else ty]
        dy = None
        for part in (case["dy16"], case["dy2"]):
            if part is not None:
                dy = part[:total].astype(f32) if dy is None else dy + part[:total].astype(f32)
        Hf = f32(H)
        xl = ref._lanes(x)
        mu = lref._row_sum(xl, False, False) / Hf
        dl = xl - mu[:, :, None]
        var = lref._row_sum(dl * dl, False, False) / Hf
        rstd = (f32(1) / np.sqrt((var + f32(eps)).astype(np.float64))).astype(f32)
        xh = (x - mu) * rstd
        a = dy * case["g"]
        c1 = lref._row_sum(ref._lanes(a), False, False) / Hf
        c2 = lref._row_sum(ref._lanes(a * xh), False, False) / Hf
        d = (rstd * ((a - c1) - xh * c2)).astype(f32)
        old = old or {}
        scatter_mut = "accumulate_ignored" if mutation == "accumulate_ignored" else None
        dword = ref.emulate_scatter(d, wid, case["word"].shape[0], -1 if mutation == "word_pad_not_skipped" else case["pad_row"], old.get("dword"), accumulate,
                                    scatter_mut)
        pos_pad = {"pos_pad_skipped": case["pad_row"], "pos_row0_dropped": 0}.get(mutation, -1)
        dpos = ref.emulate_scatter(d, prow, case["pos"].shape[0], pos_pad, old.get("dpos"), accumulate, scatter_mut)
        keep_old = accumulate and mutation != "accumulate_ignored"
        sums = {name: ref._split_sum(term.astype(f32), cap, H, old.get(name) if keep_old else None) for name, term in (("dg", dy * xh), ("db", dy))}
        tk = ty
        if mutation == "type_all_to_row0":
            tk = np.zeros_like(ty)
        if mutation == "type_unclamped_dropped":
            raw = np.zeros_like(ty) if case["types"] is None else case["types"].reshape(-1)[case["tok_src"][:total].astype(np.int64)]
            tk = np.where((raw >= 0) & (raw < TV), ty, -1)
        # a token adds to its own row only; the others' zeros change no sum (x + 0 = x in fp32)
        sums["dtype"] = np.stack([ref._split_sum(np.where((tk == k)[:, None], d, f32(0)).astype(f32), cap, H, old["dtype"][k] if keep_old and "dtype" in old else None)
                                  for k in range(TV)])
    return dict(d=d[:case["total"]], dword=dword, dpos=dpos, **sums)


worst_shares = ref.worst_shares


# ---- makers --------------------------------------------------------------------------------------------------------------------------------
def make_pack(lengths, L, ids, types):
    """The packing of right-padded rows (qa_collate's masks): tok_src = b L + p for p < lengths[b], ISENTINEL from total on."""
    B = len(lengths)
    assert ids.shape == (B, L) and (types is None or types.shape == (B, L)) and all(0 <= n <= L for n in lengths)
    src = np.concatenate([b * L + np.arange(n) for b, n in enumerate(lengths)] + [np.zeros(0, np.int64)]).astype(np.int32)
    full = np.full(B * L, ISENTINEL, np.int32)
    full[:len(src)] = src
    return dict(ids=ids.astype(np.int64), types=None if types is None else types.astype(np.int64), tok_src=full, total=len(src), L=L)


def make_tables(family, H, seed, TV=2, vocab=VOCAB, max_pos=MAX_POS):
    t = ref.make_tables(family, H, seed, vocab, max_pos)
    rng = np.random.default_rng([seed, H, TV, 99])
    scale = (1e-3 if family == "small_1e-3" else 1.0) * 0.0625
    typ = (np.full((TV, H), 0.5) + np.arange(TV)[:, None] * 0.25 if family == "const" else scale * rng.standard_normal((TV, H))).astype(np.float32)
    return dict(word=t["word"], pos=t["pos"], type=typ, g=t["g"])


def make_case(name, H, seed=3, family="unit", form="both", pad_row=0, TV=2):
    """The named cases of the GPU test. pad_row 0 is ELECTRA's pad_token_id. Every case but "full512" holds the pad id inside the mask, a
    type id of 7 and one of -2 (the clamp), and one sequence entirely of type 0."""
    rng = np.random.default_rng([seed, H, sum(map(ord, name))])
    max_pos = MAX_POS
    if name == "b3":            # B = 3, L = 16, lengths 16, 1, 7
        lengths, L = [16, 1, 7], 16
    elif name == "repeat40":    # one id more than 40 times: a word segment that crosses two piece boundaries
        lengths, L = [16, 16, 14], 16
    elif name == "b20":         # 20 short sequences: position row 0 owns 20 tokens, two pieces
        lengths, L = [8] + list(rng.integers(1, 6, 19)), 16
    elif name == "full512":     # B = 1, L = 512 = max_pos
        lengths, L, max_pos = [512], 512, 512
    elif name == "notypes":
        lengths, L = [16, 1, 7], 16
    else:
        raise ValueError(name)
    B = len(lengths)
    ids = rng.integers(1, VOCAB, (B, L))
    types = rng.integers(0, TV, (B, L))
    if name == "repeat40":
        ids[:] = 5  # (three of them are overwritten below: 43 remain, pieces of 16, 16 and 11)
    if name != "full512":
        ids[0, 3] = pad_row if pad_row >= 0 else 0   # the pad id inside the mask
        ids[0, 5], ids[0, 6] = -4, VOCAB + 9          # clamped ids
        types[0, 1], types[0, 2] = 7, -2              # clamped type ids
        types[B - 1, :] = 0                           # one sequence entirely type 0
    pk = make_pack(lengths, L, ids, None if name == "notypes" else types)
    return dict(pk, **make_tables(family, H, seed, TV, VOCAB, max_pos), **ref.make_dy(form, B * L, H, seed), pad_row=pad_row, lengths=lengths)
