"""CPU: the fp64 statement of the embedding backward (tests/embedding_grad_ref.py) against torch.autograd in float64, the emulation of the
kernels' dataflow (plan, pieces, order) against the derived bound, each mutation against the same bound, and the header / binding / shape
contract of include/mdr_embedding_grad.h. No device and no kernel runs here."""
import os
import re

import numpy as np
import pytest
import torch

import embedding_grad_ref as ref
import layernorm_grad_ref as lref
from oracle import fp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def old_values(case, seed):
    H = case["word"].shape[1]
    return {"dword": fp.grid(case["word"].shape, seed, 4.0), "dpos": fp.grid(case["pos"].shape, seed + 1, 4.0), "dtype0": fp.grid((H,), seed + 2, 4.0),
            "dg": fp.grid((H,), seed + 3, 4.0), "db": fp.grid((H,), seed + 4, 4.0)}


@pytest.mark.parametrize("kind", ["random", "range"])
@pytest.mark.parametrize("pad_row", [1, -1])
def test_fp64_statement_agrees_with_torch_autograd(pad_row, kind):
    """F.layer_norm(F.embedding(ids, word, padding_idx) + F.embedding(pid, pos, padding_idx) + type0) in float64 with the two output
    gradients summed, with and without pad_row, with clamped ids (and positions beyond max_pos: L = 50). Both sides are fp64 and differ
    only in the order of operations: |a - b| <= 1e-9 max|b| per output."""
    H = 192
    case = ref.make_case("unit", H, 7, 50, 1, kind=kind, form="both", pad_row=pad_row)
    total = case["total"]
    wid, prow = ref.rows(case)
    assert kind != "range" or ((case["ids"].reshape(-1)[case["tok_src"][:total]] < 0).any() and (case["tok_pid"][:total] >= ref.MAX_POS).any())
    assert (wid == 1).any() and (prow == 1).any()  # pad_row owns tokens in both tables
    leaves = [torch.from_numpy(case[k].astype(np.float64)).requires_grad_(True) for k in ("word", "pos", "type0", "g")]
    bias = torch.zeros(H, dtype=torch.float64, requires_grad=True)
    F = torch.nn.functional
    pad = None if pad_row < 0 else pad_row
    x = F.embedding(torch.from_numpy(wid), leaves[0], padding_idx=pad) + F.embedding(torch.from_numpy(prow), leaves[1], padding_idx=pad) + leaves[2]
    y = F.layer_norm(x, (H,), leaves[3], bias, ref.EPS)
    outs = [y * 1.0, y * 1.0]  # the output is used twice: autograd sums the two gradients
    grads = [torch.from_numpy(case[k][:total].astype(np.float64)) for k in ("dy16", "dy2")]
    want = torch.autograd.grad(outs, leaves + [bias], grads)
    rb = ref.reference_and_bound(case)
    for k, w in zip(("dword", "dpos", "dtype0", "dg", "db"), want):
        assert np.abs(rb[k][0] - w.numpy()).max() <= 1e-9 * np.abs(w.numpy()).max(), k
    if pad_row >= 0:
        assert not rb["dword"][0][pad_row].any() and not rb["dpos"][0][pad_row].any()


def test_ln_terms_restate_the_layernorm_bound():
    """ln_terms repeats lines 1 - 6 of tests/layernorm_grad_ref.py: on a materialised fp32 x without a residual (ex = 0) it gives that
    helper's dx and bound."""
    for family in ref.FAMILIES:
        case = lref.make_case(family, ("f32", "none", True, "f32"), 9, 192, 3)
        rb = lref.reference_and_bound(**case)
        x = case["inp"].astype(np.float64)
        T = ref.ln_terms(x, np.zeros_like(x), case["dy16"], case["dy2"], case["g"], lref.EPS)
        assert np.array_equal(T["d"], rb["dx"][0]) and np.allclose(T["Ed"], rb["dx"][1], rtol=1e-12, atol=0), family


def test_plan_is_a_stable_counting_sort():
    """plan_table against the definition the device uses: the rank of t is the number of t' whose (row, t') is smaller"""
    rng = np.random.default_rng(5)
    keys = rng.integers(0, 9, 200)
    pl = ref.plan_table(keys, 4)
    rank = np.asarray([((keys < keys[t]) | ((keys == keys[t]) & (np.arange(200) < t))).sum() for t in range(200)])
    assert np.array_equal(pl["order"][rank], np.arange(200))
    assert pl["nseg"] == len(np.unique(keys)) and pl["seg_start"][-1] == 200
    assert sorted(int(-1 - r if r < 0 else r) for r in pl["seg_row"]) == sorted(np.unique(keys).tolist()) and (pl["seg_row"] < 0).sum() == 1


@pytest.mark.parametrize("family", ref.FAMILIES)
@pytest.mark.parametrize("H", ref.HS)
def test_emulation_stays_inside_the_bound(H, family):
    """A second implementation of the listed dataflow, on every family and shape the GPU test uses, every gradient form, with and without
    old values."""
    worst = dict.fromkeys(ref.OUTPUTS, 0.0)
    for B, L in ref.BL_SWEEP:
        for form in (ref.DY_FORMS if (B, L) == (7, 50) else ref.DY_FORMS[2:]):
            for kind in (("random", "range") if (B, L) == (7, 50) else ("random",)):
                case = ref.make_case(family, H, B, L, 11, kind=kind, form=form)
                for old in (None, old_values(case, 12)):
                    rb = ref.reference_and_bound(case, old=old)
                    for k, w in ref.worst_shares(ref.emulate(case, old=old, accumulate=old is not None), rb).items():
                        assert w <= 1.0, (B, L, H, family, form, kind, old is not None, k, w)
                        worst[k] = max(worst[k], w)
    print(f"RATIO emulation H={H} {family}: worst |err| / bound " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))


@pytest.mark.parametrize("family", ref.FAMILIES)
@pytest.mark.parametrize("kind,pad_row", ref.KINDS_LARGE)
@pytest.mark.parametrize("H", ref.HS_LARGE)
def test_emulation_stays_inside_the_bound_at_training_token_counts(H, kind, pad_row, family):
    """The same at BL_LARGE (the GPU test's cases): three tokens per wave and chunk, chunks behind total, segments of more than one round of
    eight pieces; with and without old values. The split of the case is the LIBRARY's."""
    from multihop_dense_retrieval_amd import embedding
    case = ref.make_case(family, H, *ref.BL_LARGE, 11, kind=kind, pad_row=pad_row)
    assert ref.assert_large(case, embedding.backward_chunks) == ref.assert_large(case)
    rb = ref.reference_and_bound(case)
    for old in (None, old_values(case, 12)):
        if old is not None:
            rb = ref.reference_and_bound(case, old=old)
        shares = ref.worst_shares(ref.emulate(case, old=old, accumulate=old is not None), rb)
        assert max(shares.values()) <= 1.0, (H, kind, family, old is not None, shares)
    print(f"RATIO emulation H={H} {kind} {family}: worst |err| / bound " + ", ".join(f"{k} {v:.3g}" for k, v in shares.items()))


def test_emulated_scatter_on_the_grid_is_exact():
    """segments of 1, P - 1, P, P + 1, 2 P + 1 tokens: the emulated pieces give the integer sums"""
    P = ref.P
    pk = ref.make_flat({3: 1, 5: P - 1, 7: P, 9: P + 1, 11: 2 * P + 1, 1: 4}, 7)
    case = dict(pk, **ref.make_tables("unit", 64, 7), pad_row=1)
    d32 = fp.grid((len(pk["tok_src"]), 64), 8)
    wid, prow = ref.rows(case)
    exact = ref.exact_tables(case, d32)
    assert np.array_equal(ref.emulate_scatter(d32, wid, ref.VOCAB, 1), exact["dword"])
    assert np.array_equal(ref.emulate_scatter(d32, prow, ref.MAX_POS, 1), exact["dpos"])
    assert not exact["dword"][1].any() and exact["dword"][11].any()
    # and over several rounds of eight pieces (the GPU test's "rounds" case)
    pk = ref.make_flat({3: 8 * P, 5: 8 * P + 1, 7: 16 * P - 1, 9: 16 * P + 1, 11: 40 * P + 5, 1: 4, 0: 2}, 15)
    case = dict(pk, **ref.make_tables("unit", 64, 7), pad_row=-1)
    d32 = fp.grid((len(pk["tok_src"]), 64), 14)
    wid, prow = ref.rows(case)
    exact = ref.exact_tables(case, d32)
    assert np.array_equal(ref.emulate_scatter(d32, wid, ref.VOCAB, -1), exact["dword"]) and np.array_equal(ref.emulate_scatter(d32, prow, ref.MAX_POS, -1), exact["dpos"])
    assert ref.longest_summed_segments(case)[0] == 40 * P + 5 > 5 * ref.ROUND


@pytest.mark.parametrize("mutation", ref.MUTATIONS)
def test_each_mutation_leaves_the_bound(mutation):
    """The bound is worth something: every plan, piece, clamp, operand, count and accumulate defect is thrown out."""
    H = 192
    case = ref.make_case("unit", H, 7, 50, 21, kind="range")
    total = case["total"]
    case["tok_src"][total], case["tok_pid"][total] = 0, 3  # (the mutation that takes the token at `total` needs one to take)
    assert max(np.bincount(ref.rows(case)[0])) > ref.P and (ref.rows(case)[0] == 1).any()
    old = old_values(case, 22)
    rb = ref.reference_and_bound(case, old=old)
    assert max(ref.worst_shares(ref.emulate(case, old=old, accumulate=True), rb).values()) <= 1.0
    r = ref.worst_shares(ref.emulate(case, old=old, accumulate=True, mutation=mutation), rb)
    print(f"mutation {mutation}: worst |err| / bound " + ", ".join(f"{k} {v:.3g}" for k, v in r.items()))
    assert max(r.values()) > 1.0, mutation


def test_header_binding_and_library_agree():
    """The constants of include/mdr_embedding_grad.h are the module's and the helper's (its symbol table:
    tests/test_capi_symbols.py::test_header_binding_and_library_agree)."""
    from multihop_dense_retrieval_amd import embedding
    raw = open(os.path.join(ROOT, "include", "mdr_embedding_grad.h")).read()
    defines = {k: int(v, 0) for k, v in re.findall(r"#define (MDR_EMBEDDING_[A-Z_]+) (\w+)", raw)}
    assert defines == {"MDR_EMBEDDING_PIECE": ref.P == embedding.PIECE and ref.P, "MDR_EMBEDDING_PLAN_HEADER": ref.PLAN_HEADER,
                       "MDR_EMBEDDING_PLAN_MAGIC": ref.PLAN_MAGIC}
    assert (embedding.PLAN_HEADER, embedding.PLAN_MAGIC) == (ref.PLAN_HEADER, ref.PLAN_MAGIC)


def test_bytes_and_split_are_functions_of_the_shape():
    """the *_bytes queries and the split equal the helper's restatement, cover the documented layout, and are 0 outside the limits"""
    from multihop_dense_retrieval_amd import embedding
    lib = embedding.lib()
    up = lambda n: (n + 255) // 256 * 256  # noqa: E731
    some_split = False
    for cap in (1, 2, 3, 4, 5, 10, 350, 1023, 1024, 1025, 8608, 11400, 38400, 2 ** 20):
        assert embedding.plan_layout(cap) == ref.plan_layout(cap)
        assert lib.mdr_embedding_plan_bytes(cap) == up(4 * ref.plan_layout(cap)["words"])
        for H in range(64, 1025, 64):
            S, rpc = embedding.backward_chunks(cap, H)
            assert (S, rpc) == ref.chunks(cap, H) and S >= 1 and rpc % 4 == 0 and (S - 1) * rpc < cap <= S * rpc, (cap, H, S, rpc)
            assert S * 3 * H * 4 <= ref.MAX_PARTIAL_BYTES
            some_split |= S > 1
            assert lib.mdr_embedding_scatter_workspace_bytes(cap, H) == up(S * H * 4)
            assert lib.mdr_embedding_backward_workspace_bytes(cap, H) == up(cap * H * 4) + up(S * 3 * H * 4)
    assert some_split
    for cap in (0, -1, 2 ** 20 + 1):
        assert lib.mdr_embedding_plan_bytes(cap) == 0 and lib.mdr_embedding_scatter_workspace_bytes(cap, 64) == 0
        assert lib.mdr_embedding_backward_workspace_bytes(cap, 64) == 0 and embedding.backward_chunks(cap, 64) == (0, 0) == ref.chunks(cap, 64)
    for H in (0, 32, 96, 1088, -64):
        assert lib.mdr_embedding_scatter_workspace_bytes(5, H) == 0 and lib.mdr_embedding_backward_workspace_bytes(5, H) == 0
        assert embedding.backward_chunks(5, H) == (0, 0) == ref.chunks(5, H)


def test_module_fails_loudly_without_a_device():
    from multihop_dense_retrieval_amd import embedding
    ids, src, pid, total = torch.zeros(8, dtype=torch.int64), torch.zeros(8, dtype=torch.int32), torch.zeros(8, dtype=torch.int32), torch.ones(1, dtype=torch.int32)
    word, pos, vec = torch.zeros(10, 64), torch.zeros(6, 64), torch.zeros(64)
    with pytest.raises(RuntimeError):
        embedding.packed_embedding_layer_norm(ids, src, pid, total, word, pos, vec, vec, vec, 1e-5, 8, 1)
    with pytest.raises(RuntimeError):
        embedding.embedding_plan(ids, src, pid, total, 8, 10, 6, 1)
    with pytest.raises(RuntimeError):
        embedding.embedding_scatter(torch.zeros(8, 64), torch.zeros(200, dtype=torch.int32), 10, 6, dword=torch.zeros(10, 64))
    with pytest.raises(RuntimeError):
        embedding.embedding_backward(ids, src, pid, total, 8, word, pos, vec, vec, 1e-5, torch.zeros(8, 64, dtype=torch.float16), None, None, dg=vec.clone())
