"""CPU: the fp64 statement of the attention backward (tests/attention_grad_ref.py) against torch.autograd in float64, the emulation of the
kernels' dataflow against the derived bound, each mutation against the same bound, and the header / binding / workspace contract of
include/mdr_attention_grad.h. No device and no kernel runs here."""

import numpy as np
import pytest
import torch

import attention_grad_ref as ref
from oracle import attention_oracle as ao
from oracle import fp


def test_fp64_statement_agrees_with_torch_autograd():
    """Both sides are fp64 and differ only in summation order: |a - b| <= 1e-10 max|b| per output matrix, on ragged batches, both modes."""
    heads, lens = 3, [1, 2, 17, 64, 65, 130, 33]
    hidden = 64 * heads
    qkv, cu = ao.realistic(lens, heads, 5, 1.0)
    for mode in (0, 3):
        dctx = ref.dctx_grid(len(lens) if mode == 3 else int(cu[-1]), hidden, 1)
        mine = ref.reference(qkv, dctx, cu, heads, mode)
        want = np.zeros_like(mine)
        for b in range(len(lens)):
            Q, K, V = (torch.from_numpy(np.ascontiguousarray(x).astype(np.float64)).requires_grad_(True) for x in ao.split(qkv, cu, heads, b))
            dO = torch.from_numpy(np.ascontiguousarray(ref.split_do(dctx, cu, heads, b, mode)).astype(np.float64))
            out = torch.softmax(Q @ K.transpose(1, 2) / 8.0, dim=2) @ V
            if mode == 3:
                out = out[:, :1]
            grads = torch.autograd.grad(out, (Q, K, V), dO)
            ref._store(want, cu, b, heads, *(g.numpy() for g in grads))
        for part, name in enumerate(("dQ", "dK", "dV")):
            a, w = mine[:, part * hidden:(part + 1) * hidden], want[:, part * hidden:(part + 1) * hidden]
            assert np.abs(a - w).max() <= 1e-10 * np.abs(w).max(), (mode, name, np.abs(a - w).max(), np.abs(w).max())


@pytest.mark.parametrize("scale", [1.0, 256.0])
@pytest.mark.parametrize("family", ref.FAMILY_NAMES)
@pytest.mark.parametrize("heads,lens", [pytest.param(1, ref.LENS_SWEEP, id="sweep"), pytest.param(1, ref.LENS_EDGES, id="edges")])
def test_emulation_stays_inside_the_bound(heads, lens, family, scale):
    """A second implementation of the listed dataflow, on every family and every length the GPU tests use, both modes."""
    qkv, cu = ao.FAMILIES[family](lens, heads, 11)
    for mode in (0, 3):
        dctx = ref.dctx_grid(len(lens) if mode == 3 else int(cu[-1]), 64 * heads, 2, scale)
        r, bnd = ref.reference_and_bound(qkv, dctx, cu, heads, mode)
        worst, at = fp.worst_ratio(ref.emulate(qkv, dctx, cu, heads, mode), r, bnd)
        print(f"RATIO emulation mode={mode} family={family} scale={scale} worst |err| / bound = {worst:.4f}")
        assert worst <= 1.0, (mode, worst, at)


@pytest.mark.parametrize("mutation", ref.MUTATIONS)
def test_each_mutation_leaves_the_bound(mutation):
    """The bound is worth something: every index, mask, scale and normalisation defect is thrown out on at least one family."""
    heads, lens = 2, [1, 2, 17, 63, 64, 65, 100, 129, 200]
    mode = 3 if mutation.startswith("cls_") else 0
    caught = []
    for family in ref.FAMILY_NAMES:
        qkv, cu = ao.FAMILIES[family](lens, heads, 11)
        dctx = ref.dctx_grid(len(lens) if mode == 3 else int(cu[-1]), 64 * heads, 2)
        r, bnd = ref.reference_and_bound(qkv, dctx, cu, heads, mode)
        assert fp.worst_ratio(ref.emulate(qkv, dctx, cu, heads, mode), r, bnd)[0] <= 1.0
        worst, _ = fp.worst_ratio(ref.emulate(qkv, dctx, cu, heads, mode, mutation), r, bnd)
        if not worst <= 1.0:
            caught.append(family)
    print(f"mutation {mutation}: outside the bound on {caught}")
    assert caught, mutation


def test_workspace_cap_and_unsupported_shapes():
    """At most 16 B L heads + 4096 bytes, enough for one (lse, delta) fp32 pair per (token, head) in mode 0; 0 for what the call rejects."""
    from multihop_dense_retrieval_amd import attention
    lib = attention.lib()
    for B in (1, 2, 19, 38, 1000):
        for L in (1, 64, 70, 300, 350, 512):
            for heads in (1, 12, 16):
                for mode in (0, 3):
                    need = lib.mdr_attention_backward_workspace_bytes(B, L, heads, mode)
                    assert need <= 16 * B * L * heads + 4096, (B, L, heads, mode, need)
                    if mode == 0:
                        assert need >= 8 * B * L * heads
    for B, L, heads, mode in ((0, 64, 12, 0), (1, 0, 12, 0), (1, 513, 12, 0), (1, 64, 0, 0), (1, 64, 12, 1), (1, 64, 12, 2), (-1, 64, 12, 3)):
        assert lib.mdr_attention_backward_workspace_bytes(B, L, heads, mode) == 0


def test_module_fails_loudly_without_a_device():
    from multihop_dense_retrieval_amd import attention
    with pytest.raises(RuntimeError):
        attention.packed_self_attention(torch.zeros(4, 192, dtype=torch.float16), torch.tensor([0, 4], dtype=torch.int32), 1, 4)
