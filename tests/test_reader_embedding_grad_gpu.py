"""GPU (-m gpu): the reader's embedding backward in isolation (include/mdr_reader_embedding_grad.h) against
tests/reader_embedding_grad_ref.py: the plan against numpy's stable argsort, the whole call against the fp64 statement and its derived bound
(no tolerance here was read off a device; tests/test_reader_embedding_grad_host.py shows the bound to hold a second implementation and to
throw out each defect), and embedding.packed_reader_embedding_layer_norm on top of it. EVERY element is compared.

Shapes: H in {64, 128, 1024}; B = 3, L = 16 with lengths 16, 1, 7; B = 1, L = 512 = max_pos; one id repeated more than 40 times (a word
segment over two piece boundaries); 20 short sequences (position row 0 owns 20 tokens, over a piece boundary); a sequence entirely of type 0
and types = None; type ids 7 and -2 (the clamp); the pad id inside the mask. Every float output starts as a finite sentinel (or the old
values) with guard rows behind it, the plan as ISENTINEL; tok_src holds ISENTINEL from `total` on, which no kernel may dereference.
"""
import numpy as np
import pytest
import torch

import embedding_grad_ref as eref
import reader_embedding_grad_ref as ref
from guarded import ISENTINEL, SENTINEL, Guarded, assert_untouched, dev
from multihop_dense_retrieval_amd._lib import ptr
from oracle import fp
from oracle.fp import bits

pytestmark = pytest.mark.gpu

GUARD = 8
CASES = ("b3", "repeat40", "b20", "notypes", "full512")
SUMS = ("dtype", "dg", "db")


def emb():
    from multihop_dense_retrieval_amd import embedding
    return embedding


def stream():
    from multihop_dense_retrieval_amd import _lib
    return _lib.current_stream_ptr()


def check(rc):
    from multihop_dense_retrieval_amd import _lib
    _lib.check(rc)


def pack_dev(case):
    return dict(ids=dev(case["ids"]), types=dev(case["types"]), src=dev(case["tok_src"]), total=torch.tensor([case["total"]], dtype=torch.int32, device="cuda"))


def build_plan(case, pk=None):
    """mdr_reader_embedding_plan into a buffer of ISENTINEL -> (device plan, its words on the host)"""
    pk = pk or pack_dev(case)
    cap = len(case["tok_src"])
    nbytes = int(emb().lib().mdr_embedding_plan_bytes(cap))
    plan = torch.full((nbytes // 4 + GUARD,), ISENTINEL, dtype=torch.int32, device="cuda")
    check(emb().lib().mdr_reader_embedding_plan(ptr(pk["ids"]), ptr(pk["src"]), ptr(pk["total"]), cap, case["L"], case["word"].shape[0], case["pos"].shape[0],
                                                case["pad_row"], -1, ptr(plan), nbytes, 0, stream()))
    torch.cuda.synchronize()
    words = plan.cpu().numpy()
    assert (words[eref.plan_layout(cap)["words"]:] == ISENTINEL).all(), "the plan wrote behind its layout"
    return plan, words


class Outs:
    """the float outputs of one call, each SENTINEL (or the old value) with GUARD rows / elements of SENTINEL behind it"""

    def __init__(self, case, which, old=None):
        H = case["word"].shape[1]
        shapes = {"dword": (case["word"].shape[0], H), "dpos": (case["pos"].shape[0], H), "dtype": (case["type"].shape[0], H), "dg": (H,), "db": (H,),
                  "d": (len(case["tok_src"]), H)}
        self.out = {k: Guarded(shapes[k][0], shapes[k][1:], torch.float32, 0, GUARD, (old or {}).get(k), outside=f"{k}: the guard behind the output was written")
                    for k in which}

    def ptr(self, k):
        return self.out[k].ptr() if k in self.out else None

    def host(self):
        torch.cuda.synchronize()
        return {k: g.checked() for k, g in self.out.items()}


def run_backward(case, plan=None, which=ref.OUTPUTS, old=None, accumulate=False, eps=ref.EPS, pk=None):
    """mdr_reader_embedding_backward on a numpy case -> {output: float32 array}; d rows at or behind total must keep the sentinel"""
    pk = pk or pack_dev(case)
    if plan is None and ("dword" in which or "dpos" in which):
        plan = build_plan(case, pk)[0]
    cap, H, TV = len(case["tok_src"]), case["word"].shape[1], case["type"].shape[0]
    o = Outs(case, which, old)
    need = int(emb().lib().mdr_reader_embedding_backward_workspace_bytes(cap, H, TV))
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    held = [dev(case[k]) for k in ("word", "pos", "type", "g", "dy16", "dy2")]
    check(emb().lib().mdr_reader_embedding_backward(ptr(pk["ids"]), ptr(pk["types"]), ptr(pk["src"]), ptr(pk["total"]), cap, case["L"], ptr(held[0]), ptr(held[1]),
                                                    ptr(held[2]), TV, ptr(held[3]), H, case["word"].shape[0], case["pos"].shape[0], eps, ptr(held[4]), ptr(held[5]),
                                                    1 if case["dy2"] is not None and case["dy2"].dtype == np.float32 else 0, ptr(plan), o.ptr("dword"), o.ptr("dpos"),
                                                    o.ptr("dtype"), o.ptr("dg"), o.ptr("db"), o.ptr("d"), 1 if accumulate else 0, ptr(ws), need, 0, stream()))
    got = o.host()
    if "d" in got:
        assert_untouched(got["d"][case["total"]:], "d rows at or behind total were written")
        got["d"] = got["d"][:case["total"]]
    return got


def old_values(case, seed):
    H = case["word"].shape[1]
    return {"dword": fp.grid(case["word"].shape, seed, 4.0), "dpos": fp.grid(case["pos"].shape, seed + 1, 4.0), "dtype": fp.grid(case["type"].shape, seed + 2, 4.0),
            "dg": fp.grid((H,), seed + 3, 4.0), "db": fp.grid((H,), seed + 4, 4.0)}


@pytest.mark.parametrize("name", CASES)
def test_plan_equals_numpy_stable_argsort(name):
    """header (its own magic, pad_row, -1, L), order, segment starts, segment rows and keys, bit for bit; the position table skips no row"""
    case = ref.make_case(name, 64)
    ref.assert_plan(build_plan(case)[1], case, f"plan {name}")
    if name == "b3":
        case = ref.make_case(name, 64, pad_row=-1)
        ref.assert_plan(build_plan(case)[1], case, f"plan {name} without a pad row")


@pytest.mark.parametrize("H", ref.HS)
@pytest.mark.parametrize("name", CASES)
def test_backward_is_inside_the_bound_accumulates_by_one_add_and_repeats(name, H):
    case = ref.make_case(name, H)
    pk = pack_dev(case)
    plan, _ = build_plan(case, pk)
    got = run_backward(case, plan, pk=pk)
    rb = ref.reference_and_bound(case)
    shares = ref.worst_shares(got, rb)
    print(f"SHARE {name} H={H} " + " ".join(f"{k}={v:.4f}" for k, v in shares.items()))
    assert all(v <= 1.0 for v in shares.values()), shares
    wid, prow, ty = ref.rows(case)
    # position row 0 is every sequence's [CLS] and receives its gradient; the word table's pad row receives +0
    assert got["dpos"][0].any() and np.abs(rb["dpos"][0][0]).max() > 0
    assert (wid == case["pad_row"]).any() or name == "full512"
    assert not bits(got["dword"][case["pad_row"]]).any(), "the word table's pad row is not +0"
    for k, keys in (("dword", wid), ("dpos", prow), ("dtype", ty)):  # rows that own no token: +0
        empty = np.ones(len(got[k]), bool)
        empty[keys] = False
        assert not bits(got[k][empty]).any(), (k, "a row without tokens is not +0")
    # two runs give equal bits
    again = run_backward(case, plan, pk=pk)
    for k in got:
        assert np.array_equal(bits(got[k]), bits(again[k])), (k, "two runs differ")
    # accumulate: exactly one fp32 add per element, new = sum + old; rows without a (counted) segment keep their bits
    old = old_values(case, 31)
    acc = run_backward(case, plan, which=("dword", "dpos") + SUMS, old=old, accumulate=True, pk=pk)
    for k in SUMS:
        assert np.array_equal(bits(acc[k]), bits((got[k] + old[k]).astype(np.float32))), (k, "accumulate is not one add onto the old value")
    for k, keys, pad in (("dword", wid, case["pad_row"]), ("dpos", prow, -1)):
        touched = np.zeros(len(got[k]), bool)
        touched[keys[keys != pad]] = True
        assert np.array_equal(bits(acc[k][touched]), bits((got[k][touched] + old[k][touched]).astype(np.float32))), (k, "accumulate is not one add")
        assert np.array_equal(bits(acc[k][~touched]), bits(old[k][~touched])), (k, "a row without a segment was written under accumulate")
    acc_b = fp.worst_ratio(acc["dpos"], *ref.reference_and_bound(case, old=old)["dpos"])[0]
    assert acc_b <= 1.0
    # each output alone gives the same bits
    for k in ("dtype", "dpos", "dg"):
        assert np.array_equal(bits(run_backward(case, plan, which=(k,), pk=pk)[k]), bits(got[k])), (k, "alone")


@pytest.mark.parametrize("H", [64, 1024])
def test_without_types_every_token_is_type_zero(H):
    """types = NULL gives the bits of an all-zero types tensor, and dtype rows 1 .. TV - 1 are +0"""
    case = ref.make_case("notypes", H)
    assert case["types"] is None
    got = run_backward(case)
    zeros = dict(case, types=np.zeros_like(case["ids"]))
    want = run_backward(zeros)
    for k in got:
        assert np.array_equal(bits(got[k]), bits(want[k])), k
    assert got["dtype"][0].any() and not bits(got["dtype"][1:]).any()
    # and dtype[0] is then the sum of every d: the retriever's dtype0 split over the same rows
    want0 = eref._split_sum(got["d"], len(case["tok_src"]), H, None)
    assert np.array_equal(bits(got["dtype"][0]), bits(want0))


def test_type_vocab_one_to_four():
    """TV = 1, 3, 4: every row inside the bound; ids beyond TV - 1 join the last row"""
    for TV in (1, 3, 4):
        case = ref.make_case("b20", 128, TV=TV)
        got = run_backward(case)
        shares = ref.worst_shares(got, ref.reference_and_bound(case))
        print(f"SHARE TV={TV} " + " ".join(f"{k}={v:.4f}" for k, v in shares.items()))
        assert all(v <= 1.0 for v in shares.values()), (TV, shares)
        assert got["dtype"].shape[0] == TV and got["dtype"][TV - 1].any()


def test_a_sequences_d_does_not_depend_on_its_place_in_the_batch():
    """the sequences of a batch in another order, their dy rows with them: every token's d keeps its bits"""
    H = 128
    case = ref.make_case("b20", H)
    B, L = case["ids"].shape
    lengths = np.asarray(case["lengths"])
    cu = np.concatenate([[0], np.cumsum(lengths)])
    got = run_backward(case, which=("d",))["d"]
    perm = np.random.default_rng(4).permutation(B)
    assert (perm != np.arange(B)).any()
    moved = dict(case, **ref.make_pack(list(lengths[perm]), L, case["ids"][perm], case["types"][perm]))
    cu2 = np.concatenate([[0], np.cumsum(lengths[perm])])
    for key in ("dy16", "dy2"):
        buf = np.zeros_like(case[key])
        for j, b in enumerate(perm):
            buf[cu2[j]:cu2[j + 1]] = case[key][cu[b]:cu[b + 1]]
        moved[key] = buf
    got2 = run_backward(moved, which=("d",))["d"]
    for j, b in enumerate(perm):
        assert np.array_equal(bits(got2[cu2[j]:cu2[j + 1]]), bits(got[cu[b]:cu[b + 1]])), (j, b)


def test_a_plan_of_the_other_kind_makes_the_table_kernels_do_nothing():
    """the reader's plan under mdr_embedding_backward and mdr_embedding_scatter, and the retriever's plan (and a reader plan built with
    another L) under mdr_reader_embedding_backward: dword and dpos keep their old bits under accumulate"""
    H = 64
    case = ref.make_case("b3", H)
    pk = pack_dev(case)
    cap, vocab, max_pos = len(case["tok_src"]), case["word"].shape[0], case["pos"].shape[0]
    rplan, _ = build_plan(case, pk)
    pid = dev(np.where(case["tok_src"] >= 0, case["tok_src"] % case["L"], ISENTINEL).astype(np.int32))
    nbytes = int(emb().lib().mdr_embedding_plan_bytes(cap))
    eplan = torch.full((nbytes // 4,), ISENTINEL, dtype=torch.int32, device="cuda")
    check(emb().lib().mdr_embedding_plan(ptr(pk["ids"]), ptr(pk["src"]), ptr(pid), ptr(pk["total"]), cap, vocab, max_pos, case["pad_row"], ptr(eplan), nbytes, 0, stream()))
    other_L = dict(case, **ref.make_pack([8, 1, 7], 8, case["ids"][:, :8], case["types"][:, :8]))
    lplan, _ = build_plan(dict(other_L, tok_src=np.concatenate([other_L["tok_src"], np.full(cap - 24, ISENTINEL, np.int32)])))
    old = {"dword": np.full((vocab, H), SENTINEL, np.float32), "dpos": np.full((max_pos, H), SENTINEL, np.float32)}
    for label, plan in (("the retriever's plan", eplan), ("a reader plan of another L", lplan)):
        got = run_backward(case, plan, which=("dword", "dpos"), old=old, accumulate=True, pk=pk)
        assert (got["dword"] == SENTINEL).all() and (got["dpos"] == SENTINEL).all(), label
    got = run_backward(case, rplan, which=("dword", "dpos"), old=old, accumulate=True, pk=pk)
    assert (got["dword"] != SENTINEL).any() and (got["dpos"] != SENTINEL).any()
    # the reader's plan under the retriever's entry points
    o = {k: Guarded(n, (H,), torch.float32, 0, GUARD, old[k]) for k, n in (("dword", vocab), ("dpos", max_pos))}
    d32 = dev(fp.grid((cap, H), 3))
    need = int(emb().lib().mdr_embedding_scatter_workspace_bytes(cap, H))
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device="cuda")
    check(emb().lib().mdr_embedding_scatter(ptr(d32), ptr(rplan), cap, H, vocab, max_pos, o["dword"].ptr(), o["dpos"].ptr(), None, 1, ptr(ws), need, 0, stream()))
    torch.cuda.synchronize()
    assert all((g.checked() == SENTINEL).all() for g in o.values()), "mdr_embedding_scatter summed by a reader plan"
    check(emb().lib().mdr_embedding_scatter(ptr(d32), ptr(eplan), cap, H, vocab, max_pos, o["dword"].ptr(), o["dpos"].ptr(), None, 1, ptr(ws), need, 0, stream()))
    torch.cuda.synchronize()
    assert all((g.checked() != SENTINEL).any() for g in o.values()), "mdr_embedding_scatter no longer sums by its own plan"


@pytest.mark.parametrize("name", ["b3", "notypes"])
def test_autograd_function_is_the_readers_forward_and_the_raw_backward(name):
    """packed_reader_embedding_layer_norm: the forward's bits are flavour 1 of mdr_test_embed_ln (the inference reader's kernel), the five
    gradients the raw call's bits for the two output gradients; the word table's pad row gets +0 and position row 0 does not"""
    from multihop_dense_retrieval_amd import _lib
    H = 128
    case = ref.make_case(name, H)
    pk = pack_dev(case)
    cap, L, total = len(case["tok_src"]), case["L"], case["total"]
    src = torch.where(pk["src"] == ISENTINEL, torch.zeros_like(pk["src"]), pk["src"])  # (the forward's launch reads no entry behind total either; keep the buffer tame)
    P = {k: dev(case[k]).requires_grad_(True) for k in ("word", "pos", "type", "g")}
    bias = dev(fp.grid((H,), 5)).requires_grad_(True)
    y16, y32 = emb().packed_reader_embedding_layer_norm(pk["ids"], pk["types"], src, pk["total"], L, P["word"], P["pos"], P["type"], P["g"], bias, ref.EPS, cap,
                                                        case["pad_row"], True)
    w16 = torch.zeros((cap, H), dtype=torch.float16, device="cuda")
    w32 = torch.zeros((cap, H), dtype=torch.float32, device="cuda")
    _lib.call(_lib.lib().mdr_test_embed_ln, 1, ptr(pk["ids"]), ptr(pk["types"]), ptr(src), None, ptr(pk["total"]), cap, L, ptr(P["word"].detach()),
              ptr(P["pos"].detach()), ptr(P["type"].detach()), case["type"].shape[0], ptr(P["g"].detach()), ptr(bias.detach()), H, case["word"].shape[0],
              case["pos"].shape[0], ref.EPS, ptr(w16), ptr(w32), dev=y16.device)
    assert torch.equal(y16.detach().view(torch.int16), w16.view(torch.int16)) and torch.equal(y32.detach().view(torch.int32), w32.view(torch.int32))
    g16, g32 = dev(case["dy16"]), dev(case["dy2"])
    torch.autograd.backward([y16, y32], [g16, g32])
    want = run_backward(dict(case, tok_src=src.cpu().numpy()), which=("dword", "dpos", "dtype", "dg", "db"), pk=dict(pk, src=src))
    for k, t in (("dword", P["word"]), ("dpos", P["pos"]), ("dtype", P["type"]), ("dg", P["g"]), ("db", bias)):
        assert np.array_equal(bits(t.grad.cpu().numpy()), bits(want[k])), k
    assert not bits(P["word"].grad[case["pad_row"]].cpu().numpy()).any() and bool(P["pos"].grad[0].any())
    assert total < cap
