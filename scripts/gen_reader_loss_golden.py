"""Generate tests/golden/reader_loss_ref.npz by EXECUTING the training branch of the reference's QAModel.forward (mdr/qa/qa_model.py:49-102) on the
CPU in fp32 (run once, where the reference checkout is present):

    PYTHONDONTWRITEBYTECODE=1 python scripts/gen_reader_loss_golden.py [--ref /path/to/multihop_dense_retrieval]

QAModel is imported under the library stubs of oracle/gen_cli_golden.py. Its encoder is a stub that returns a given `sequence_output` leaf
[B, L, H] with requires_grad, so the reference's own pooler, qa_outputs, rank and sp modules, its masking, its loss and torch autograd produce
every number. Cases: H = 128, L = 24, B in {1, 5}, each with and without --sp-pred (`B<B>_sp.` / `B<B>_nosp.`); the rows (tests/reader_loss_ref.py
has no part in them) cover a yes / no answer at para_offset and at para_offset + 1, several matched spans, a row whose candidates are all -1, a
one-sided candidate, labels 0 and 1 and sent_offsets padded with 0. Stored once: the head and pooler parameters (`param.<name>`) and the B = 5
sequence_output (B = 1 is its row 2); per case the batch tensors, lens, sp_weight, the loss and autograd's gradients of sequence_output and of
every parameter (`grad.<name>`; a `nosp` gradient that equals the `sp` case's bit for bit is stored there alone). Only data is written (apex does not exist here: no O1 run can be captured). The archive is written with fixed
member dates, so a second run gives the same bytes.
"""
import argparse
import io
import os
import sys
import types
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

H, L, NS, A = 128, 24, 4, 4
SP_WEIGHT = 0.5
LENS = [24, 17, 21, 12, 19]
PARA_OFFSET = [6, 5, 7, 4, 6]
# (start, end) candidates per row, -1 = ignore: yes / no at para_offset; at para_offset + 1; several spans (one of them twice); all ignored; one-sided
CANDIDATES = [[(6, 6), (-1, -1), (-1, -1), (-1, -1)],
              [(6, 6), (-1, -1), (-1, -1), (-1, -1)],
              [(9, 11), (14, 14), (9, 11), (-1, -1)],
              [(-1, -1), (-1, -1), (-1, -1), (-1, -1)],
              [(8, -1), (-1, 15), (10, 12), (-1, -1)]]
LABEL = [1, 0, 1, 0, 1]
SENT_OFFSETS = [[7, 12, 18, 22], [6, 11, 0, 0], [8, 8, 15, 0], [5, 0, 0, 0], [7, 13, 17, 0]]
SENT_LABELS = [[1, 0, 1, 0], [0, 1, 0, 0], [1, 1, 0, 0], [0, 0, 0, 0], [0, 1, 1, 0]]


def write_npz(path, arrays):
    """an .npz numpy.load reads, with sorted members and fixed dates: the same arrays give the same bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("MDR_REFERENCE", "/root/reference"))
    ref_root = ap.parse_args().ref
    import warnings
    warnings.simplefilter("ignore")
    import torch
    import transformers
    from oracle import gen_cli_golden as cli
    cli.REF = ref_root
    rng = np.random.default_rng(20)
    seq5 = rng.standard_normal((5, L, H)).astype(np.float32)
    arrays = {"seq": seq5}

    class StubEncoder(torch.nn.Module):
        leaf = None

        def forward(self, input_ids, attention_mask, token_type_ids=None):
            return (StubEncoder.leaf,)

    with cli.stubbed(cli.Capture()):
        saved = transformers.AutoModel.from_pretrained
        transformers.AutoModel.from_pretrained = staticmethod(lambda name: StubEncoder())
        try:
            import mdr.qa.qa_model as ref_model
            cfg = types.SimpleNamespace(hidden_size=H)
            torch.manual_seed(3)
            models = {}
            for sp_pred in (True, False):
                args = types.SimpleNamespace(model_name="electra-stub", sp_weight=SP_WEIGHT, sp_pred=sp_pred)
                m = ref_model.QAModel(cfg, args)
                if sp_pred:
                    with torch.no_grad():
                        for n, p in m.named_parameters():  # spread logits (|logit| of a few units), O(1) pooler outputs
                            p.copy_((1.5 / p.shape[-1] ** 0.5) * torch.randn_like(p) if p.dim() == 2 else 0.1 * torch.randn_like(p))
                    sd = m.state_dict()
                    for n, v in sd.items():
                        arrays["param." + n] = v.numpy().copy()
                else:
                    m.load_state_dict({k: v for k, v in sd.items() if not k.startswith("sp.")})
                m.train()
                models[sp_pred] = m
            for B, rows in ((1, [2]), (5, [0, 1, 2, 3, 4])):
                pmask = np.zeros((B, L), np.int64)
                for i, r in enumerate(rows):
                    pmask[i, PARA_OFFSET[r]:LENS[r] - 1] = 1
                batch = {"input_ids": torch.zeros((B, L), dtype=torch.long), "attention_mask": torch.ones((B, L), dtype=torch.long),
                         "paragraph_mask": torch.from_numpy(pmask),
                         "starts": torch.tensor([[c[0] for c in CANDIDATES[r]] for r in rows]), "ends": torch.tensor([[c[1] for c in CANDIDATES[r]] for r in rows]),
                         "label": torch.tensor([[LABEL[r]] for r in rows]), "sent_offsets": torch.tensor([SENT_OFFSETS[r] for r in rows]),
                         "sent_labels": torch.tensor([SENT_LABELS[r] for r in rows])}
                for sp_pred in (True, False):
                    m = models[sp_pred]
                    m.zero_grad()
                    StubEncoder.leaf = torch.from_numpy(seq5[rows].copy()).requires_grad_(True)
                    loss = m(batch)
                    assert tuple(loss.shape) == (1,)
                    loss.sum().backward()
                    pre = f"B{B}_{'sp' if sp_pred else 'nosp'}."
                    for k in ("paragraph_mask", "starts", "ends", "label", "sent_offsets", "sent_labels"):
                        arrays[pre + k] = batch[k].numpy().copy()
                    arrays[pre + "rows"] = np.array(rows, np.int64)
                    arrays[pre + "lens"] = np.array([LENS[r] for r in rows], np.int64)
                    arrays[pre + "sp_weight"] = np.float32(SP_WEIGHT)
                    arrays[pre + "loss"] = loss.detach().numpy().copy()
                    arrays[pre + "grad.seq"] = StubEncoder.leaf.grad.numpy().copy()
                    for n, p in m.named_parameters():
                        g = p.grad.numpy().copy()
                        twin = arrays.get(f"B{B}_sp.grad." + n)  # the pooler and rank gradients do not depend on the sp head: stored once
                        if sp_pred or not np.array_equal(twin, g):
                            arrays[pre + "grad." + n] = g
                    print(pre, "loss", float(loss.item()))
        finally:
            transformers.AutoModel.from_pretrained = saved
    out = os.path.join(GOLD, "reader_loss_ref.npz")
    write_npz(out, arrays)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
