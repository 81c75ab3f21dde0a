"""CPU: the fp64 statement of the reader's embedding backward (tests/reader_embedding_grad_ref.py) against torch.autograd in float64, the
emulation of the kernels' dataflow against the derived bound on every case the GPU test runs, each mutation against the same bound, and the
header / binding / validation contract of include/mdr_reader_embedding_grad.h. No device and no kernel runs here."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import embedding_grad_ref as eref
import reader_embedding_grad_ref as ref
from guarded import E_INVALID
from oracle import fp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("b3", "repeat40", "b20", "notypes", "full512")


def old_values(case, seed):
    H = case["word"].shape[1]
    return {"dword": fp.grid(case["word"].shape, seed, 4.0), "dpos": fp.grid(case["pos"].shape, seed + 1, 4.0), "dtype": fp.grid(case["type"].shape, seed + 2, 4.0),
            "dg": fp.grid((H,), seed + 3, 4.0), "db": fp.grid((H,), seed + 4, 4.0)}


@pytest.mark.parametrize("name", ["b3", "notypes", "b20"])
def test_fp64_statement_agrees_with_torch_autograd(name):
    """Hugging Face's ElectraEmbeddings in float64: word_embeddings with padding_idx = pad_row, position_embeddings and
    token_type_embeddings without one, absolute positions 0 .. len - 1, LayerNorm; the output used twice. Both sides are fp64 and differ only
    in the order of operations."""
    H = 128
    case = ref.make_case(name, H)
    total = case["total"]
    wid, prow, ty = ref.rows(case)
    assert (wid == case["pad_row"]).any() and (prow == 0).sum() == len(case["lengths"])
    leaves = [torch.from_numpy(case[k].astype(np.float64)).requires_grad_(True) for k in ("word", "pos", "type", "g")]
    bias = torch.zeros(H, dtype=torch.float64, requires_grad=True)
    F = torch.nn.functional
    x = F.embedding(torch.from_numpy(wid), leaves[0], padding_idx=case["pad_row"]) + F.embedding(torch.from_numpy(prow), leaves[1]) + \
        F.embedding(torch.from_numpy(ty), leaves[2])
    y = F.layer_norm(x, (H,), leaves[3], bias, ref.EPS)
    grads = [torch.from_numpy(case[k][:total].astype(np.float64)) for k in ("dy16", "dy2")]
    want = torch.autograd.grad([y * 1.0, y * 1.0], leaves + [bias], grads)
    rb = ref.reference_and_bound(case)
    for k, w in zip(("dword", "dpos", "dtype", "dg", "db"), want):
        assert np.abs(rb[k][0] - w.numpy()).max() <= 1e-9 * np.abs(w.numpy()).max(), k
    assert not rb["dword"][0][case["pad_row"]].any() and rb["dpos"][0][0].any()


@pytest.mark.parametrize("H", ref.HS)
@pytest.mark.parametrize("name", CASES)
def test_emulation_stays_inside_the_bound(name, H):
    """A second implementation of the listed dataflow on every case and H of the GPU test, with and without old values; and the properties
    the cases are there for."""
    case = ref.make_case(name, H)
    wid, prow, ty = ref.rows(case)
    if name == "repeat40":
        assert (wid == 5).sum() >= 40 > 2 * ref.P
    if name == "b20":
        assert (prow == 0).sum() == 20 > ref.P
    if name == "full512":
        assert case["total"] == 512 == case["pos"].shape[0] == case["L"]
    else:
        raw = case["ids"].reshape(-1)[case["tok_src"][:case["total"]]]
        assert (raw == case["pad_row"]).any() and (raw < 0).any() and (raw >= ref.VOCAB).any()
    if case["types"] is not None and name != "full512":
        rawt = case["types"].reshape(-1)[case["tok_src"][:case["total"]]]
        assert (rawt == 7).any() and (rawt < 0).any() and (ty == 1).any()
    for old in (None, old_values(case, 12)):
        rb = ref.reference_and_bound(case, old=old)
        shares = ref.worst_shares(ref.emulate(case, old=old, accumulate=old is not None), rb)
        assert max(shares.values()) <= 1.0, (name, H, old is not None, shares)
    print(f"RATIO emulation {name} H={H}: worst |err| / bound " + ", ".join(f"{k} {v:.3g}" for k, v in shares.items()))


@pytest.mark.parametrize("mutation", ref.MUTATIONS)
def test_each_mutation_leaves_the_bound(mutation):
    """The bound is worth something: every position, type, pad, count and accumulate defect is thrown out."""
    case = ref.make_case("b3", 128, pad_row=0)
    case["tok_src"][case["total"]] = 16 + 3  # (the mutation that takes the token at `total` needs one to take)
    old = old_values(case, 22)
    rb = ref.reference_and_bound(case, old=old)
    assert max(ref.worst_shares(ref.emulate(case, old=old, accumulate=True), rb).values()) <= 1.0
    r = ref.worst_shares(ref.emulate(case, old=old, accumulate=True, mutation=mutation), rb)
    print(f"mutation {mutation}: worst |err| / bound " + ", ".join(f"{k} {v:.3g}" for k, v in r.items()))
    assert max(r.values()) > 1.0, mutation


def test_plan_header_and_layout():
    """The reader's plan has the retriever's layout and size, its own magic, a pad row per table and L in the header; its position table
    skips no row."""
    from multihop_dense_retrieval_amd import embedding
    case = ref.make_case("b3", 64)
    head = ref.plan_header(case)
    assert head[0] == embedding.READER_PLAN_MAGIC != embedding.PLAN_MAGIC and list(head[7:10]) == [case["pad_row"], -1, 16] and not head[10:].any()
    pl = ref.plan(case)
    assert (pl["pos"]["seg_row"] >= 0).all() and pl["pos"]["seg_row"][0] == 0 and (pl["word"]["seg_row"] < 0).sum() == 1
    assert pl["pos"]["nseg"] == max(case["lengths"])  # row p owns one token of every sequence longer than p
    first = pl["pos"]["order"][pl["pos"]["seg_start"][0]:pl["pos"]["seg_start"][1]]
    assert list(first) == [0, 16, 17]  # the [CLS] tokens: the packed row cu[b] of every sequence, ascending
    for cap in (1, 48, 512, 49152):
        assert embedding.plan_layout(cap) == eref.plan_layout(cap)


def test_header_binding_and_library_agree():
    """include/mdr_reader_embedding_grad.h declares exactly what embedding.READER_SIGNATURES binds and the library exports; the constants are
    the module's and the helper's."""
    from multihop_dense_retrieval_amd import _lib, build, embedding
    raw = open(os.path.join(ROOT, "include", "mdr_reader_embedding_grad.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = sorted(set(re.findall(r"\b(mdr_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(embedding.READER_SIGNATURES) == sorted(embedding.READER_EXPORTED_SYMBOLS)
    assert declared == ["mdr_reader_embedding_backward", "mdr_reader_embedding_backward_workspace_bytes", "mdr_reader_embedding_plan"]
    assert not set(declared) & (set(embedding.SIGNATURES) | set(_lib.EXPORTED_SYMBOLS))
    for name, (_, args) in embedding.READER_SIGNATURES.items():
        proto = re.search(r"\b" + name + r"\s*\(([^)]*)\)", text).group(1)
        assert len(args) == proto.count(",") + 1, name
    lib = ctypes.CDLL(build.build_lib())
    for name in declared:
        assert hasattr(lib, name), name
    defines = {k: int(v, 0) for k, v in re.findall(r"#define (MDR_READER_EMBEDDING_[A-Z_]+) (\w+)", raw)}
    assert defines == {"MDR_READER_EMBEDDING_PLAN_MAGIC": ref.READER_PLAN_MAGIC, "MDR_READER_EMBEDDING_MAX_TYPES": ref.MAX_TYPES}
    assert (embedding.READER_PLAN_MAGIC, embedding.READER_MAX_TYPES) == (ref.READER_PLAN_MAGIC, ref.MAX_TYPES)


def test_workspace_bytes_are_a_function_of_the_shape():
    from multihop_dense_retrieval_amd import embedding
    lib = embedding.lib()
    up = lambda n: (n + 255) // 256 * 256  # noqa: E731
    for cap in (1, 48, 512, 8608, 49152):
        for H in (64, 128, 1024):
            S, _ = embedding.backward_chunks(cap, H)  # the split is the retriever's: a function of (cap, H) alone
            for tv in (1, 2, 4):
                assert lib.mdr_reader_embedding_backward_workspace_bytes(cap, H, tv) == up(cap * H * 4) + up(S * 2 * H * 4) + up(S * tv * H * 4)
    for cap, H, tv in ((0, 64, 2), (48, 96, 2), (48, 64, 0), (48, 64, 5), (2 ** 20 + 1, 64, 1)):
        assert lib.mdr_reader_embedding_backward_workspace_bytes(cap, H, tv) == 0


def test_validation_errors_come_without_a_launch():
    """type_vocab 0 or 5, L > max_pos, L < 1, a short plan buffer: MDR_E_INVALID (or MDR_E_WORKSPACE) with a message, decided on the host
    before any device call -- the pointers here are never dereferenced."""
    from multihop_dense_retrieval_amd import _lib, embedding
    lib = embedding.lib()
    fake = 0x10000  # non-NULL, 16-byte aligned, never read
    err = lambda: _lib.lib().mdr_last_error().decode()  # noqa: E731

    def backward(L=16, max_pos=40, tv=2, cap=48, H=64):
        return lib.mdr_reader_embedding_backward(fake, fake, fake, fake, cap, L, fake, fake, fake, tv, fake, H, 97, max_pos, 1e-12, fake, None, 0, fake, fake, fake, fake,
                                                 fake, fake, None, 0, fake, 1 << 30, 0, None)
    for tv in (0, 5, -1):
        assert backward(tv=tv) == E_INVALID and "type_vocab" in err()
    assert backward(L=41) == E_INVALID and "L=41" in err()
    assert backward(L=0) == E_INVALID and "L=0" in err()
    assert backward(H=96) == E_INVALID and "H=96" in err()
    plan = lambda L=16, max_pos=40, nbytes=1 << 20, pad_pos=-1: lib.mdr_reader_embedding_plan(fake, fake, fake, 48, L, 97, max_pos, 0, pad_pos, fake, nbytes, 0, None)  # noqa: E731
    assert plan(L=41) == E_INVALID and "L=41" in err()
    assert plan(L=513, max_pos=512) == E_INVALID
    assert plan(pad_pos=-2) == E_INVALID and "pad_pos" in err()
    assert plan(nbytes=64) == -4 and "mdr_embedding_plan_bytes" in err()


def test_module_validates_before_a_launch_and_fails_loudly_without_a_device():
    from multihop_dense_retrieval_amd import embedding
    ids, src, total = torch.zeros(2, 4, dtype=torch.int64), torch.zeros(8, dtype=torch.int32), torch.ones(1, dtype=torch.int32)
    word, pos, typ, vec = torch.zeros(10, 64), torch.zeros(6, 64), torch.zeros(2, 64), torch.zeros(64)
    with pytest.raises(RuntimeError):
        embedding.packed_reader_embedding_layer_norm(ids, None, src, total, 4, word, pos, typ, vec, vec, 1e-12, 8, 0)
    with pytest.raises(RuntimeError):
        embedding.reader_embedding_plan(ids, src, total, 8, 4, 10, 6, 0)
    # the size rules, which need no device
    for tv in (0, 5):
        with pytest.raises(ValueError, match="type_vocab"):
            embedding._check_reader_sizes(10, 6, 4, tv, 0)
    with pytest.raises(ValueError, match="exceeds max_pos"):
        embedding._check_reader_sizes(10, 6, 7, 2, 0)
    embedding._check_reader_sizes(10, 6, 6, 4, -1)
    # a plan of the wrong kind: a tensor of the right size that reader_embedding_plan did not return
    words = embedding.plan_layout(8)["words"]
    other = torch.zeros(words, dtype=torch.int32)
    with pytest.raises(ValueError, match="reader_embedding_plan"):
        embedding._check_reader_plan(other, 8, other.device)
    other.mdr_plan_kind = "reader"
    embedding._check_reader_plan(other, 8, other.device)
