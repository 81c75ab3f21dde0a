"""Generate tests/golden/mhop_loss_grad_ref.npz by EXECUTING the reference's own mhop_loss (mdr/retrieval/criterions.py:114-151) and
RobertaMomentumRetriever.dequeue_and_enqueue (mdr/retrieval/models/mhop_retriever.py:85-106) on the CPU in fp32 (run once, where the
reference checkout is present):

    PYTHONDONTWRITEBYTECODE=1 python scripts/gen_mhop_loss_grad_golden.py [--ref /path/to/multihop_dense_retrieval]

Both are imported under the library stubs of oracle/gen_cli_golden.py (apex / tqdm / faiss no-ops). The model is a stub that returns six leaf
tensors with requires_grad (the inputs of tests/mhop_loss_ref.make_inputs, d = 32); with --momentum it also carries `queue`, `queue_ptr` and `k`,
and the reference's dequeue_and_enqueue is bound to it, so the queue after the step and the pointer are the reference's. Cases: B in {1, 3, 17},
K in {0, 5, 40}; K = 0 runs without args.momentum. The starting pointer of every K > 0 case is listed in START_PTR: four of the six enqueues pass
the end of the queue and are truncated. Stored per case `B<B>_K<K>.`: the six inputs, queue_before, ptr_before, loss, the six grads,
queue_after, ptr_after. Only data is written (apex does not exist here: no O1 run can be captured).
"""
import argparse
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

D = 32
SIZES_B, SIZES_K = (1, 3, 17), (0, 5, 40)
# (B, K) -> queue_ptr before the step. 2B rows are enqueued: (1, 5) and (1, 40) fit; the other four are truncated at the end of the queue.
START_PTR = {(1, 5): 2, (3, 5): 0, (17, 5): 3, (1, 40): 10, (3, 40): 36, (17, 40): 20}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("MDR_REFERENCE", "/root/reference"))
    ref_root = ap.parse_args().ref
    import warnings
    warnings.simplefilter("ignore")
    import torch
    import mhop_loss_ref as ref
    from oracle import gen_cli_golden as cli
    cli.REF = ref_root
    arrays = {}
    with cli.stubbed(cli.Capture()):
        sys.modules["transformers"].AdamW = torch.optim.AdamW
        import mdr.retrieval.criterions as ref_crit
        import mdr.retrieval.models.mhop_retriever as ref_model

        class StubModel:
            def __init__(self, leaves, queue, ptr):
                self.leaves, self.module = leaves, self
                if queue is not None:
                    self.k = queue.shape[0]
                    self.queue = torch.from_numpy(queue.copy())
                    self.queue_ptr = torch.tensor([ptr], dtype=torch.long)

            def __call__(self, batch):
                return self.leaves

            def dequeue_and_enqueue(self, embeddings):
                return ref_model.RobertaMomentumRetriever.dequeue_and_enqueue(self, embeddings)

        for B in SIZES_B:
            for K in SIZES_K:
                inp, queue = ref.make_inputs(B, D, K, seed=1000 * B + K)
                leaves = {k: torch.from_numpy(v.copy()).requires_grad_(True) for k, v in inp.items()}
                model = StubModel(leaves, queue, START_PTR.get((B, K), 0))
                loss = ref_crit.mhop_loss(model, None, types.SimpleNamespace(momentum=K > 0))
                loss.backward()
                pre = f"B{B}_K{K}."
                for k, v in inp.items():
                    arrays[pre + k] = v
                    arrays[pre + "grad." + k] = leaves[k].grad.numpy().copy()
                arrays[pre + "loss"] = np.float32(loss.item())
                if K:
                    arrays[pre + "queue_before"] = queue
                    arrays[pre + "ptr_before"] = np.int64(START_PTR[(B, K)])
                    arrays[pre + "queue_after"] = model.queue.numpy().copy()
                    arrays[pre + "ptr_after"] = np.int64(int(model.queue_ptr))
                    n_written = min(2 * B, K - START_PTR[(B, K)])
                    print(pre, "loss", float(loss.item()), "enqueued", n_written, "of", 2 * B, "ptr", START_PTR[(B, K)], "->", int(model.queue_ptr))
                else:
                    print(pre, "loss", float(loss.item()))
    assert sum(2 * B > K - p for (B, K), p in START_PTR.items()) >= 1, "no enqueue is truncated"
    out = os.path.join(GOLD, "mhop_loss_grad_ref.npz")
    np.savez_compressed(out, **arrays)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
