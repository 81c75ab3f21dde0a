"""CPU: the fp64 statement of the reader's loss, heads and gradients (tests/reader_loss_ref.py) and reader_loss.host_loss against the golden
that the reference's own QAModel.forward produced (tests/golden/reader_loss_ref.npz, scripts/gen_reader_loss_golden.py); the mutants of the
helper against the same golden; and the header / binding / validation contract of include/mdr_reader_loss.h. No device and no kernel runs
here: every refusal below returns before the entry point selects a device.

Tolerance. The golden is an fp32 evaluation by torch on the CPU, so it must lie inside the helper's bound for ANY fp32 evaluation of the
formula around the fp64 value (mode fp32 of the helper: every accumulation in any order, the forward's error carried into the backward); the
bound is derived in the helper's header, nothing is chosen here."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest
import torch

import reader_loss_ref as ref
from guarded import E_INVALID, E_WORKSPACE
from oracle import fp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "reader_loss_ref.npz")
CASES = ("B1_sp", "B1_nosp", "B5_sp", "B5_nosp")
BATCH_KEYS = ("paragraph_mask", "starts", "ends", "label", "sent_offsets", "sent_labels")


def load_case(case):
    """(seq [B, L, H], params, batch, sp_weight, golden {"loss", "grads"}) of one golden case; lens = L: the reference saw padded rows"""
    z = np.load(GOLD)
    P = {k[6:]: z[k] for k in z.files if k.startswith("param.")}
    if case.endswith("nosp"):
        P["sp.weight"] = P["sp.bias"] = None
    batch = {k: z[f"{case}.{k}"] for k in BATCH_KEYS}
    grads = {}
    for k in ["seq"] + [n for n, v in P.items() if v is not None]:
        key = f"{case}.grad.{k}"
        grads[k] = z[key] if key in z.files else z[f"{case.replace('nosp', 'sp')}.grad.{k}"]  # stored once where the two cases agree bit for bit
    return z["seq"][z[f"{case}.rows"]], P, batch, float(z[f"{case}.sp_weight"].reshape(-1)[0]), {"loss": float(z[f"{case}.loss"][0]), "grads": grads, "lens": z[f"{case}.lens"]}


def outside(r, gold):
    """names of the golden results that leave the bound of the helper result r"""
    bad = [] if abs(gold["loss"] - r["loss"]) <= r["loss_bound"] else ["loss"]
    return bad + [k for k in r["grads"] if not fp.worst_ratio(gold["grads"][k], r["grads"][k], r["bounds"][k])[0] <= 1.0]


@pytest.mark.parametrize("case", CASES)
def test_fp64_statement_agrees_with_the_reference(case):
    seq, P, batch, spw, gold = load_case(case)
    r = ref.chain(seq, np.full(seq.shape[0], seq.shape[1]), batch, P, 1.0, spw, o1=False)
    assert outside(r, gold) == []
    assert set(r["grads"]) == set(gold["grads"])
    # the ragged packing the device tests use sees the same numbers: nothing behind lens[b] carries a gradient or is read
    r2 = ref.chain(seq, gold["lens"], batch, P, 1.0, spw, o1=False)
    assert outside(r2, gold) == []
    assert all(np.all(gold["grads"]["seq"][b, n:] == 0) for b, n in enumerate(gold["lens"]))


def test_the_golden_covers_every_candidate_kind():
    _, _, batch, _, _ = load_case("B5_sp")
    s, e, pm = batch["starts"], batch["ends"], batch["paragraph_mask"]
    off = pm.argmax(1)
    assert s[0, 0] == off[0] == e[0, 0] and s[1, 0] == off[1] + 1                      # yes / no at para_offset and para_offset + 1
    assert ((s[2] >= 0) & (e[2] >= 0)).sum() >= 3 and (s[3] == -1).all() and (e[3] == -1).all()  # several spans; all ignored
    assert ((s[4] >= 0) != (e[4] >= 0)).sum() == 2                                     # one-sided, each side once
    assert set(batch["label"].reshape(-1)) == {0, 1} and (batch["sent_offsets"] == 0).any() and batch["sent_offsets"].max() > 1


@pytest.mark.parametrize("mutant", ref.MUTATIONS)
def test_the_golden_rejects_every_mutant(mutant):
    seq, P, batch, spw, gold = load_case("B5_sp")
    r = ref.chain(seq, np.full(5, seq.shape[1]), batch, P, 1.0, spw, o1=False, mutate=mutant)
    assert outside(r, gold) != [], mutant


@pytest.mark.parametrize("case", CASES)
def test_host_loss_is_the_reference_formula(case):
    """reader_loss.host_loss on the fp32 logits of the golden's own parameters: the golden's loss, and torch autograd's score gradients equal
    the helper's closed form"""
    from multihop_dense_retrieval_amd import reader_loss
    seq, P, batch, spw, gold = load_case(case)
    B, L, _ = seq.shape
    fv, fw = ref.heads_forward(seq, seq[:, 0] @ P["pooler.dense.weight"].T.astype(np.float64) + P["pooler.dense.bias"], np.full(B, L), batch["paragraph_mask"],
                               batch["sent_offsets"], P, o1=False)
    t = {k: torch.from_numpy(np.asarray(fv[k], np.float32)).requires_grad_(True) for k in ("start", "end", "rank", "sp") if fv[k] is not None}
    tb = {k: torch.from_numpy(v) for k, v in batch.items()}
    loss = reader_loss.host_loss(t["start"], t["end"], t["rank"], t.get("sp"), tb, spw)
    assert tuple(loss.shape) == (1,) and loss.dtype == torch.float32
    r = ref.chain(seq, np.full(B, L), batch, P, 1.0, spw, o1=False)
    assert abs(float(loss.detach()) - gold["loss"]) <= r["loss_bound"]
    loss.sum().backward()
    inp = dict({k: np.asarray(v.detach().numpy(), np.float64) for k, v in t.items()}, sp=t["sp"].detach().numpy() if "sp" in t else None, **batch)
    lg = ref.loss_and_grads(inp, 1.0, spw, o1=False)
    for k, v in t.items():
        fp.assert_within(v.grad.numpy().reshape(lg["grads"][k].shape), lg["grads"][k], lg["bounds"][k], f"{case} d_{k}")


def test_closed_form_agrees_with_autograd_in_fp64():
    """the helper's gradients against torch autograd on an fp64 restatement of the reference's call sequence: mixed -1 sides, an all-ignored row,
    padded offsets"""
    inp = ref.make_loss_case(6, 19, 5, 3, 4)
    F = torch.nn.functional
    s, e, rk, sp = (torch.from_numpy(np.asarray(inp[k], np.float64)).requires_grad_(True) for k in ("start", "end", "rank", "sp"))
    ce = torch.nn.CrossEntropyLoss(ignore_index=-1, reduction="none")
    lt = torch.stack([ce(s, a) for a in torch.from_numpy(inp["starts"]).unbind(1)], 1) + torch.stack([ce(e, a) for a in torch.from_numpy(inp["ends"]).unbind(1)], 1)
    lp = (-lt).masked_fill(-lt == 0, float("-inf"))
    m = torch.exp(lp).sum(1)
    label = torch.from_numpy(inp["label"]).double()
    loss = -torch.log(m[m != 0]).sum() + F.binary_cross_entropy_with_logits(rk, label, reduction="sum")
    loss = loss + 0.7 * ((F.binary_cross_entropy_with_logits(sp, torch.from_numpy(inp["sent_labels"]).double(), reduction="none")
                          * torch.from_numpy(inp["sent_offsets"])) * label[:, None]).sum()
    loss.backward()
    r = ref.loss_and_grads(inp, 1.0, 0.7, o1=False)
    assert abs(float(loss.detach()) - r["loss"]) < 1e-12 * abs(r["loss"])
    assert (~r["counted"]).any() and r["counted"].any()
    for k, t in (("start", s), ("end", e), ("rank", rk), ("sp", sp)):
        assert np.abs(t.grad.numpy() - r["grads"][k]).max() < 1e-12, k
        assert not np.isnan(r["grads"][k]).any()


def test_header_binding_and_library_agree():
    """as tests/test_capi_symbols.py::test_header_binding_and_library_agree does for the other headers: the header declares exactly what
    reader_loss.SIGNATURES binds and the library exports, the table shares no name with any other, and every signature has the prototype's
    number of arguments"""
    from multihop_dense_retrieval_amd import _lib, build, reader_loss
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mdr_reader_loss.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(mdr_[a-z0-9_]+)\s*\(", text)))
    assert sorted(reader_loss.SIGNATURES) == declared == [
        "mdr_reader_heads_backward", "mdr_reader_heads_backward_workspace_bytes", "mdr_reader_heads_forward", "mdr_reader_loss_backward",
        "mdr_reader_loss_forward", "mdr_reader_loss_workspace_bytes"]
    assert sorted(reader_loss.EXPORTED_SYMBOLS) == declared
    assert not set(reader_loss.SIGNATURES) & set(_lib.EXPORTED_SYMBOLS)
    others = [("attention", "SIGNATURES"), ("linear", "SIGNATURES"), ("layernorm", "SIGNATURES"), ("embedding", "SIGNATURES"), ("optim", "SIGNATURES"),
              ("dropout", "SIGNATURES"), ("criterions", "SIGNATURES"), ("criterions", "LOSS_SIGNATURES"), ("reader", "SIGNATURES"), ("head", "SIGNATURES")]
    for m, a in others:
        assert not set(reader_loss.SIGNATURES) & set(getattr(importlib.import_module("multihop_dense_retrieval_amd." + m), a)), m
    for name, (_, args) in reader_loss.SIGNATURES.items():
        proto = re.search(r"\b" + name + r"\s*\(([^)]*)\)", text).group(1)
        assert len(args) == proto.count(",") + 1, name
    lib = ctypes.CDLL(build.build_lib())
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in include/mdr_reader_loss.h but not exported"
    reader_loss.lib()


def _host_buffers(sizes):
    bufs = [np.zeros(n + 32, np.uint8) for n in sizes]
    return bufs, [b.ctypes.data + (-b.ctypes.data) % 16 for b in bufs]


def _refused(L, rc, code, word):
    from multihop_dense_retrieval_amd import _lib
    assert rc == code, (rc, _lib.lib().mdr_last_error())
    assert word in _lib.lib().mdr_last_error().decode(), _lib.lib().mdr_last_error()


def test_loss_entry_points_refuse_bad_arguments_without_a_launch():
    """MDR_E_INVALID / MDR_E_WORKSPACE with a message, on HOST pointers that are never dereferenced (a machine without a GPU runs this)"""
    from multihop_dense_retrieval_amd import reader_loss
    L = reader_loss.lib()
    B, SL, A, NS = 3, 40, 4, 5
    keep, p = _host_buffers([B * SL * 2] * 2 + [B * 2, B * NS * 2, B * A * 8, B * A * 8, B * 8, B * NS * 8, B * NS * 8, 4, 4096, 4] + [B * SL * 2] * 2 + [B * 2, B * NS * 2])
    need = int(L.mdr_reader_loss_workspace_bytes(B, SL, A, NS))
    assert need == 256 and L.mdr_reader_loss_workspace_bytes(97, 512, 65, 30) == 1280
    for bad in ((0, SL, A, NS), (B, 0, A, NS), (B, 513, A, NS), (B, SL, 0, NS), (B, SL, A, -1)):
        assert L.mdr_reader_loss_workspace_bytes(*bad) == 0

    def fwd(ptrs=None, shape=(B, SL, A, NS), ws=p[10], nbytes=need, loss=p[9]):
        q = list(p[:9]) if ptrs is None else ptrs
        return L.mdr_reader_loss_forward(*q, *shape, 0.5, loss, ws, nbytes, 0, None)

    def bwd(ptrs=None, shape=(B, SL, A, NS), outs=None, g0=p[11]):
        q = list(p[:9]) if ptrs is None else ptrs
        return L.mdr_reader_loss_backward(*q, *shape, 0.5, g0, *(p[12:16] if outs is None else outs), 0, None)

    for f in (fwd, bwd):
        for i in (0, 1, 2, 4, 5, 6):
            q = list(p[:9])
            q[i] = None
            _refused(L, f(ptrs=q), E_INVALID, "NULL")
        for i in (7, 8):
            q = list(p[:9])
            q[i] = None
            _refused(L, f(ptrs=q), E_INVALID, "sent_offsets")
        for bad in ((0, SL, A, NS), (B, 0, A, NS), (B, 513, A, NS), (B, SL, 0, NS), (B, SL, A, -1)):
            _refused(L, f(shape=bad), E_INVALID, "bad shape")
    _refused(L, fwd(loss=None), E_INVALID, "NULL")
    _refused(L, fwd(nbytes=need - 1), E_WORKSPACE, "mdr_reader_loss_workspace_bytes")
    _refused(L, fwd(ws=None), E_WORKSPACE, "mdr_reader_loss_workspace_bytes")
    _refused(L, fwd(ws=p[10] + 4), E_INVALID, "aligned")
    _refused(L, bwd(g0=None), E_INVALID, "NULL")
    for i in range(3):
        outs = list(p[12:16])
        outs[i] = None
        _refused(L, bwd(outs=outs), E_INVALID, "NULL")
    _refused(L, bwd(outs=list(p[12:15]) + [None]), E_INVALID, "d_sp")


def test_heads_entry_points_refuse_bad_arguments_without_a_launch():
    from multihop_dense_retrieval_amd import reader_loss
    L = reader_loss.lib()
    B, SL, NS, H, T = 3, 40, 5, 128, 100
    sizes = [T * H * 2, (B + 1) * 4, B * H * 2, B * SL * 8, B * NS * 8, 4 * H * 2, 16] + [B * SL * 2] * 2 + [B * 2, B * NS * 2]
    keep, p = _host_buffers(sizes + [T * H * 2, B * H * 2, 2 * H * 4, 8, H * 4, 4, H * 4, 4, 1 << 20])
    h, cu, dense, pm, offs, w, bias, s, e, r, sp, dh, dd, dwqa, dbqa, dwsp, dbsp, dwr, dbr, ws = p
    need = int(L.mdr_reader_heads_backward_workspace_bytes(B, SL, H))
    assert 0 < need <= 1 << 20
    for bad in ((0, SL, H), (B, 0, H), (B, SL, 64), (B, SL, 192), (B, SL, 1152), (1 << 16, 1 << 15, H)):
        assert L.mdr_reader_heads_backward_workspace_bytes(*bad) == 0

    def fwd(**kw):
        a = dict(h=h, cu=cu, dense=dense, pm=pm, offs=offs, B=B, L=SL, NS=NS, H=H, w=w, bias=bias, s=s, e=e, r=r, sp=sp)
        a.update(kw)
        return L.mdr_reader_heads_forward(a["h"], a["cu"], a["dense"], a["pm"], a["offs"], a["B"], a["L"], a["NS"], a["H"], a["w"], a["bias"], a["s"], a["e"],
                                          a["r"], a["sp"], 0, None)

    def bwd(**kw):
        a = dict(h=h, cu=cu, dense=dense, pm=pm, offs=offs, B=B, L=SL, NS=NS, H=H, T=T, w=w, s=s, e=e, r=r, sp=sp, dh=dh, dd=dd, dwqa=dwqa, dbqa=dbqa,
                 dwsp=dwsp, dbsp=dbsp, dwr=dwr, dbr=dbr, acc=0, ws=ws, nbytes=need)
        a.update(kw)
        return L.mdr_reader_heads_backward(a["h"], a["cu"], a["dense"], a["pm"], a["offs"], a["B"], a["L"], a["NS"], a["H"], a["T"], a["w"], a["s"], a["e"], a["r"],
                                           a["sp"], a["dh"], a["dd"], a["dwqa"], a["dbqa"], a["dwsp"], a["dbsp"], a["dwr"], a["dbr"], a["acc"], a["ws"],
                                           a["nbytes"], 0, None)

    for f in (fwd, bwd):
        for name in ("h", "cu", "dense", "pm", "w", "s", "e", "r"):
            _refused(L, f(**{name: None}), E_INVALID, "NULL")
        for kw in ({"B": 0}, {"L": 0}, {"NS": -1}, {"H": 64}, {"H": 192}, {"H": 1152}):
            _refused(L, f(**kw), E_INVALID, "bad shape")
        for name, q in (("h", h), ("dense", dense), ("w", w)):
            _refused(L, f(**{name: q + 4}), E_INVALID, "aligned")
        _refused(L, f(offs=None), E_INVALID, "sent_offsets")
    _refused(L, fwd(bias=None), E_INVALID, "NULL")
    for name in ("dh", "dd", "dwqa", "dbqa", "dwr", "dbr"):
        _refused(L, bwd(**{name: None}), E_INVALID, "NULL")
    _refused(L, bwd(dwsp=None), E_INVALID, "dw_sp")
    _refused(L, bwd(T=0), E_INVALID, "rows_cap")
    _refused(L, bwd(dh=dh + 8), E_INVALID, "aligned")
    _refused(L, bwd(nbytes=need - 1), E_WORKSPACE, "mdr_reader_heads_backward_workspace_bytes")
    _refused(L, bwd(ws=None), E_WORKSPACE, "mdr_reader_heads_backward_workspace_bytes")


def test_module_fails_loudly_without_a_device():
    from multihop_dense_retrieval_amd import reader_loss
    s = torch.zeros(2, 8, dtype=torch.float16)
    batch = {"starts": torch.zeros(2, 1, dtype=torch.int64), "ends": torch.zeros(2, 1, dtype=torch.int64), "label": torch.zeros(2, dtype=torch.int64),
             "paragraph_mask": torch.ones(2, 8, dtype=torch.int64)}
    with pytest.raises(RuntimeError):
        reader_loss.qa_loss(s, s, torch.zeros(2, dtype=torch.float16), None, batch, 1.0)
    with pytest.raises(RuntimeError):
        reader_loss.reader_heads(torch.zeros(16, 128, dtype=torch.float16), torch.zeros(2, 128, dtype=torch.float16), torch.zeros(3, dtype=torch.int32), batch, {})


def test_reader_training_is_still_refused():
    """this brick changes nothing for reader.QAModel and qa_data.QADataset: training stays out of scope"""
    src = open(os.path.join(ROOT, "multihop_dense_retrieval_amd", "reader.py")).read() + open(os.path.join(ROOT, "multihop_dense_retrieval_amd", "qa_data.py")).read()
    assert src.count("training is not supported: the reader runs inference only") >= 2
