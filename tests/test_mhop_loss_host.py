"""CPU: the fp64 statement of the in-batch loss and its gradients (tests/mhop_loss_ref.py) against what the REFERENCE's own mhop_loss and
dequeue_and_enqueue computed in fp32 (tests/golden/mhop_loss_grad_ref.npz, written by scripts/gen_mhop_loss_grad_golden.py), the derived error
bound against wrong formulas, and MemoryBank against the reference's queue. No device."""
import os
import types

import numpy as np
import pytest
import torch

import mhop_loss_ref as ref

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mhop_loss_grad_ref.npz")
CASES = [(B, K) for B in (1, 3, 17) for K in (0, 5, 40)]


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLD) as z:
        return {k: z[k] for k in z.files}


def case(gold, B, K):
    pre = f"B{B}_K{K}."
    inp = {k: gold[pre + k] for k in ref.KEYS}
    grads = {k: gold[pre + "grad." + k] for k in ref.KEYS}
    return inp, (gold[pre + "queue_before"] if K else None), float(gold[pre + "loss"]), grads


@pytest.mark.parametrize("B,K", CASES)
def test_fp64_statement_reproduces_the_reference(gold, B, K):
    inp, queue, loss, grads = case(gold, B, K)
    r = ref.loss_and_grads(inp, queue)
    print({k: f"{v[0]:.2e} (bound {v[1]:.2e})" for k, v in ref.worst(r, loss, grads).items()})
    assert ref.violations(r, loss, grads) == []
    # the bound is not vacuous: a gradient element is (p - onehot) / B times an input element, summed; the bound stays below 1 % of one such term
    top = max(np.abs(v).max() for v in inp.values()) / B
    for k in ref.KEYS:
        assert r["bounds"][k].max() <= 0.01 * top, (k, r["bounds"][k].max(), top)


def torch_autograd(inp, queue):
    """The formula by torch autograd in fp32 on the CPU (cross_entropy over the concatenated scores)."""
    t = {k: torch.from_numpy(v.copy()).requires_grad_(True) for k, v in inp.items()}
    B = t["q"].shape[0]
    ctx = torch.cat([t["c1"], t["c2"]])
    neg = torch.stack([t["neg_1"], t["neg_2"]], dim=1)
    loss = 0.0
    for h, x in enumerate((t["q"], t["q_sp1"])):
        s = x @ ctx.t()
        if h == 0:
            s = s.masked_fill(torch.cat([torch.zeros(B, B), torch.eye(B)], dim=1).bool(), float("-inf"))
        cols = [s, torch.einsum("bd,bnd->bn", x, neg)] + ([x @ torch.from_numpy(queue).t()] if queue is not None else [])
        loss = loss + torch.nn.functional.cross_entropy(torch.cat(cols, dim=1), torch.arange(B) + h * B)
    loss.backward()
    return float(loss), {k: v.grad.numpy() for k, v in t.items()}


@pytest.mark.parametrize("B,K", CASES)
def test_unmutated_torch_fp32_gradients_sit_inside_the_bound(gold, B, K):
    inp, queue, _, _ = case(gold, B, K)
    loss, grads = torch_autograd(inp, queue)
    assert ref.violations(ref.loss_and_grads(inp, queue), loss, grads) == []


# mutation -> the matrices it must move out of the bound, and the fixture cases it can show on
REJECT = {"no_mask": (("q",), [(3, 0), (17, 5)]), "no_onehot": (("q", "q_sp1", "c1", "c2"), [(1, 0), (3, 5), (17, 40)]),
          "no_inv_b": (("q", "q_sp1", "c1", "c2", "neg_1", "neg_2"), [(3, 0), (17, 40)]), "no_queue_in_lse": (("q", "q_sp1"), [(1, 5), (17, 40)]),
          "swap_dneg": (("neg_1", "neg_2"), [(1, 0), (17, 5)]), "hop2_target_i": (("q_sp1", "c1", "c2"), [(3, 0), (17, 40)]),
          "dctx_no_hop2": (("c1", "c2"), [(1, 0), (17, 5)])}


@pytest.mark.parametrize("mutation", ref.MUTATIONS)
def test_the_bound_rejects_a_wrong_formula(gold, mutation):
    names, cases = REJECT[mutation]
    for B, K in cases:
        inp, queue, loss, _ = case(gold, B, K)
        good = ref.loss_and_grads(inp, queue)
        wrong = ref.loss_and_grads(inp, queue, mutate=mutation)
        bad = ref.violations(good, None, wrong["grads"])
        assert set(names) <= set(bad), (mutation, B, K, bad)


def test_the_bound_rejects_a_single_wrong_element_and_a_nan(gold):
    inp, queue, loss, grads = case(gold, 17, 40)
    r = ref.loss_and_grads(inp, queue)
    g = {k: v.copy() for k, v in grads.items()}
    g["c2"][16, 31] += 10 * r["bounds"]["c2"][16, 31] + 1e-6
    assert ref.violations(r, loss, g) == ["c2"]
    g = {k: v.copy() for k, v in grads.items()}
    g["neg_1"][0, 0] = np.nan
    assert ref.violations(r, loss, g) == ["neg_1"]
    assert ref.violations(r, loss + 1e-3, grads) == ["loss"]


@pytest.mark.parametrize("B,K", [c for c in CASES if c[1]])
def test_memory_bank_reproduces_the_reference_queue(gold, B, K):
    from multihop_dense_retrieval_amd import criterions
    pre = f"B{B}_K{K}."
    bank = criterions.MemoryBank(K, 32, "cpu")
    assert bank.queue.shape == (K, 32) and bank.queue.dtype == torch.float32 and int(bank.queue_ptr) == 0
    assert 0.5 < float(bank.queue.std()) < 1.5  # torch.randn
    bank.queue.copy_(torch.from_numpy(gold[pre + "queue_before"]))
    bank.queue_ptr[0] = int(gold[pre + "ptr_before"])
    bank.dequeue_and_enqueue(torch.from_numpy(np.concatenate([gold[pre + "c1"], gold[pre + "c2"]])))
    assert np.array_equal(bank.queue.numpy(), gold[pre + "queue_after"])
    assert int(bank.queue_ptr) == int(gold[pre + "ptr_after"])


def test_a_truncated_enqueue_is_in_the_fixture(gold):
    """2B = 34 rows at pointer 20 of 40: 20 rows are written, 14 dropped (not wrapped to the front), and the pointer returns to 0."""
    pre = "B17_K40."
    before, after = gold[pre + "queue_before"], gold[pre + "queue_after"]
    emb = np.concatenate([gold[pre + "c1"], gold[pre + "c2"]])
    assert int(gold[pre + "ptr_before"]) == 20 and int(gold[pre + "ptr_after"]) == 0
    assert np.array_equal(after[:20], before[:20]) and np.array_equal(after[20:], emb[:20])


def test_train_args_accept_the_momentum_flags():
    from multihop_dense_retrieval_amd import config
    a = config.train_args(["--momentum", "--k", "76800", "--m", "0.999", "--temperature", "1", "--init-retriever", "x.pt"])
    assert a.momentum and a.k == 76800 and a.m == 0.999 and a.temperature == 1 and a.init_retriever == "x.pt"


def test_the_loss_refuses_cpu_tensors():
    from multihop_dense_retrieval_amd import criterions
    o = {k: torch.zeros(2, 32) for k in ref.KEYS}
    with pytest.raises(RuntimeError, match="HIP device only"):
        criterions.mhop_loss_outputs(o, types.SimpleNamespace(fp16=False))
