"""CPU: the fp64 statement of the head Linear's backward (tests/head_grad_ref.py) against torch.autograd in float64, the fp32 replica of the
kernels' dataflow against the derived bound, and the header / binding / validation contract of include/mdr_head_grad.h. No device and no
kernel runs here: every refusal below returns before the entry point selects a device."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest
import torch

import head_grad_ref as ref
from guarded import E_INVALID, E_WORKSPACE
from oracle import fp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTPUTS = ("dx", "dw", "db")


def test_fp64_statement_agrees_with_torch_autograd():
    M, N, K = 37, 128, 64
    x, w, dy = ref.realistic(M, N, K, 1)
    tx, tw = (torch.from_numpy(a.astype(np.float64)).requires_grad_(True) for a in (x, w))
    tb = torch.zeros(N, dtype=torch.float64, requires_grad=True)
    want = [g.numpy() for g in torch.autograd.grad(torch.nn.functional.linear(tx, tw, tb), (tx, tw, tb), torch.from_numpy(dy.astype(np.float64)))]
    rb = ref.reference_and_bound(x, w, dy)
    for k, wnt in zip(OUTPUTS, want):
        assert np.abs(rb[k][0] - wnt).max() <= 1e-10 * np.abs(wnt).max(), k


@pytest.mark.parametrize("N,K", ref.NK, ids=[f"{n}-{k}" for n, k in ref.NK])
def test_replica_stays_inside_its_bound(N, K):
    """the fused fp32 dataflow on every shape of the GPU test, overwrite and accumulate, unit and loss scale; and a plain (unfused, numpy's own
    order) fp32 product too: the bound does not pin the order"""
    for M in ref.M_SWEEP:
        for scale in (1.0, 256.0):
            x, w, dy = ref.realistic(M, N, K, 11, scale)
            for old in ((None, None), ref.old_values(N, K, 12)):
                rb = ref.reference_and_bound(x, w, dy, *old)
                for k, g in zip(OUTPUTS, ref.emulate(x, w, dy, *old)):
                    worst, at = fp.worst_ratio(g, *rb[k])
                    assert worst <= 1.0, (M, N, K, scale, k, worst, at)
            rb = ref.reference_and_bound(x, w, dy)
            f = np.float32
            plain = ((dy @ w.astype(f)).astype(np.float16), dy.T @ x.astype(f), dy.sum(axis=0, dtype=f))
            for k, g in zip(OUTPUTS, plain):
                assert fp.worst_ratio(g, *rb[k])[0] <= 1.0, (M, N, K, scale, k)


def test_the_bound_notices_a_dy_rounded_to_fp16_and_a_dropped_row():
    """the bound is worth something: the defect this brick exists to remove (dY through fp16) and a missing last row leave it"""
    M, N, K = 150, 128, 128
    x, w, dy = ref.realistic(M, N, K, 21)
    rb = ref.reference_and_bound(x, w, dy)
    rounded = ref.emulate(x, w, dy.astype(np.float16).astype(np.float32))
    short = ref.emulate(x[:-1], w, dy[:-1])
    for k, g in zip(OUTPUTS, rounded):
        assert fp.worst_ratio(g, *rb[k])[0] > 1.0, k
    for k, g in zip(OUTPUTS[1:], short[1:]):
        assert fp.worst_ratio(g, *rb[k])[0] > 1.0, k


def test_header_binding_and_library_agree():
    """as tests/test_capi_symbols.py::test_header_binding_and_library_agree does for the other headers: the header declares exactly what
    head.SIGNATURES binds and the library exports, the table shares no name with any other, and every signature has the prototype's number
    of arguments"""
    from multihop_dense_retrieval_amd import _lib, build, head
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mdr_head_grad.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(mdr_[a-z0-9_]+)\s*\(", text)))
    assert sorted(head.SIGNATURES) == declared == ["mdr_head_backward", "mdr_head_backward_workspace_bytes"]
    assert sorted(head.EXPORTED_SYMBOLS) == declared
    assert not set(head.SIGNATURES) & set(_lib.EXPORTED_SYMBOLS)
    others = [("attention", "SIGNATURES"), ("linear", "SIGNATURES"), ("layernorm", "SIGNATURES"), ("embedding", "SIGNATURES"), ("optim", "SIGNATURES"),
              ("dropout", "SIGNATURES"), ("criterions", "SIGNATURES"), ("criterions", "LOSS_SIGNATURES"), ("reader", "SIGNATURES")]
    for m, a in others:
        assert not set(head.SIGNATURES) & set(getattr(importlib.import_module("multihop_dense_retrieval_amd." + m), a)), m
    for name, (_, args) in head.SIGNATURES.items():
        proto = re.search(r"\b" + name + r"\s*\(([^)]*)\)", text).group(1)
        assert len(args) == proto.count(",") + 1, name
    lib = ctypes.CDLL(build.build_lib())
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in include/mdr_head_grad.h but not exported"
    head.lib()


def test_workspace_is_a_function_of_the_shape():
    from multihop_dense_retrieval_amd import head
    L = head.lib()
    assert head.CHUNK == ref.CHUNK
    up = lambda b: (b + 255) // 256 * 256  # noqa: E731
    for N, K in ref.NK:
        for M in ref.M_SWEEP + [128, 129, 300]:
            S = ref.chunks(M)
            assert L.mdr_head_backward_workspace_bytes(M, N, K, 1) == 0
            assert L.mdr_head_backward_workspace_bytes(M, N, K, 2) == (up(S * N * K * 4) if S > 1 else 0)
            assert L.mdr_head_backward_workspace_bytes(M, N, K, 4) == (up(S * N * 4) if S > 1 else 0)
            assert L.mdr_head_backward_workspace_bytes(M, N, K, 7) == (up(S * N * K * 4) + up(S * N * 4) if S > 1 else 0)
    assert any(ref.chunks(M) > 1 for M in ref.M_SWEEP)  # the GPU test's own sweep reaches the chunked path
    for M, N, K in ((0, 64, 64), (-1, 64, 64), (5, 0, 64), (5, 64, 0), (5, 96, 64), (5, 64, 100), (5, -64, 64)):
        assert L.mdr_head_backward_workspace_bytes(M, N, K, 7) == 0


def test_entry_point_refuses_bad_arguments_without_a_launch():
    """MDR_E_INVALID / MDR_E_WORKSPACE with a message, on HOST pointers that are never dereferenced: every refusal comes before the device is
    selected and before any launch (a machine without a GPU runs this)."""
    from multihop_dense_retrieval_amd import _lib, head
    L = head.lib()
    M, N, K = 150, 128, 64
    bufs = [np.zeros(n + 32, np.uint8) for n in (M * K * 2, N * K * 2, M * N * 4, M * K * 2, N * K * 4, N * 4, 1 << 20)]
    x, w, dy, dx, dw, db, ws = (b.ctypes.data + (-b.ctypes.data) % 16 for b in bufs)
    need = int(L.mdr_head_backward_workspace_bytes(M, N, K, 7))
    assert 0 < need <= 1 << 20

    def call(x=x, w=w, dy=dy, M=M, N=N, K=K, dx=dx, dw=dw, db=db, acc=0, ws=ws, nbytes=need):
        return L.mdr_head_backward(x, w, dy, M, N, K, dx, dw, db, acc, ws, nbytes, 0, None)

    def refused(code, word, **kw):
        assert call(**kw) == code, kw
        assert word in _lib.lib().mdr_last_error().decode(), (kw, _lib.lib().mdr_last_error())

    for name in ("x", "w", "dy"):
        refused(E_INVALID, "NULL", **{name: None})
    refused(E_INVALID, "nothing to compute", dx=None, dw=None, db=None)
    for bad in (0, -3):
        refused(E_INVALID, "M=", M=bad)
    for kw in ({"N": 0}, {"N": 96}, {"N": -64}, {"K": 0}, {"K": 100}, {"K": 32}):
        refused(E_INVALID, "multiples of 64", **kw)
    for name, p in (("x", x), ("w", w), ("dy", dy), ("dx", dx), ("dw", dw), ("db", db), ("ws", ws)):
        refused(E_INVALID, "aligned", **{name: p + 4})
    refused(E_WORKSPACE, "mdr_head_backward_workspace_bytes", nbytes=need - 1)
    refused(E_WORKSPACE, "mdr_head_backward_workspace_bytes", ws=None)
    refused(E_WORKSPACE, "mdr_head_backward_workspace_bytes", dx=None, db=None, nbytes=int(L.mdr_head_backward_workspace_bytes(M, N, K, 2)) - 1)


def test_module_fails_loudly_without_a_device():
    from multihop_dense_retrieval_amd import head
    x, w, b = torch.zeros(4, 64, dtype=torch.float16), torch.zeros(64, 64), torch.zeros(64)
    with pytest.raises(RuntimeError):
        head.packed_head_linear(x, w, b)
    with pytest.raises(RuntimeError):
        head.head_backward(x, w.half(), torch.zeros(4, 64))
