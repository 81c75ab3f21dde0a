"""CPU: what multihop_dense_retrieval_amd/reader_train.py decides without a device (the parameter order, the two weight-decay groups, the
fp16 copies), the internal consistency of tests/golden/reader_train_ref.npz, and the three mutants of a CPU fp32 restatement of the golden's
computation against the GPU test's threshold (tests/reader_train_ref.py). No kernel runs here."""
import numpy as np
import pytest
import torch

import reader_train_ref as ref


def model_of(sp_pred):
    from multihop_dense_retrieval_amd import reader_train
    return reader_train.TrainableReader(ref.tiny_config(), ref.make_args(sp_pred))


@pytest.mark.parametrize("sp_pred", [True, False])
def test_parameters_are_the_references_in_its_order(sp_pred):
    from multihop_dense_retrieval_amd import reader
    m = model_of(sp_pred)
    shapes = reader.expected_state_dict_shapes(ref.tiny_config(), "electra", sp_pred)
    got = [(k, tuple(v.shape)) for k, v in m.named_parameters()]
    assert got == [(k, tuple(s)) for k, s in shapes.items()] and list(m.state_dict()) == list(shapes)
    assert all(v.requires_grad and v.dtype == torch.float32 for _, v in m.named_parameters())
    p = "encoder.encoder.layer.0.attention.self."
    assert {p + "query.weight", p + "key.weight", p + "value.weight", "pooler.dense.weight"} <= set(shapes) and ("sp.weight" in shapes) == sp_pred
    m.load_state_dict(ref.checkpoint(sp_pred))  # the committed checkpoint loads strictly


def test_decay_groups_and_fp16_copies_on_the_tiny_config():
    from multihop_dense_retrieval_amd import reader_train, train
    names = [k for k, _ in model_of(True).named_parameters()]
    decay, no_decay = reader_train.decay_groups(names)
    assert sorted(decay + no_decay) == sorted(names) and not set(decay) & set(no_decay)
    assert all(("bias" in n or "LayerNorm.weight" in n) for n in no_decay) and not any(("bias" in n or "LayerNorm.weight" in n) for n in decay)
    assert decay == [n for n in names if n in decay] and no_decay == [n for n in names if n in no_decay]  # each in the given order
    E = "encoder.embeddings."
    assert {E + "word_embeddings.weight", E + "position_embeddings.weight", E + "token_type_embeddings.weight", "pooler.dense.weight", "qa_outputs.weight",
            "rank.weight", "sp.weight"} <= set(decay)
    assert {E + "LayerNorm.weight", "pooler.dense.bias", "sp.bias", "encoder.encoder.layer.0.output.LayerNorm.weight"} <= set(no_decay)
    assert reader_train.NO_DECAY is train.NO_DECAY
    half = reader_train.fp16_copy_names(names)
    p = "encoder.encoder.layer.0."
    assert half == [p + "attention.self.query.weight", p + "attention.self.key.weight", p + "attention.self.value.weight", p + "attention.output.dense.weight",
                    p + "intermediate.dense.weight", p + "output.dense.weight", "pooler.dense.weight"]


def test_refusals():
    from multihop_dense_retrieval_amd import reader_train
    cfg = ref.tiny_config()
    for name in ("roberta-base", "spanbert-large", "bert-base-uncased"):
        with pytest.raises(NotImplementedError):
            reader_train.TrainableReader(cfg, ref.make_args(True, model_name=name))
    small = ref.tiny_config()
    small.embedding_size = 64
    with pytest.raises(NotImplementedError):
        reader_train.TrainableReader(small, ref.make_args(True))
    m = model_of(True)
    with pytest.raises(RuntimeError):  # no CPU fallback
        m.eval()(ref.batch_of(ref.golden(), "sp.b0"))


@pytest.mark.parametrize("tag,sp_pred", ref.SETS)
def test_golden_is_consistent_with_itself(tag, sp_pred):
    """the loss recomputed by reader_loss.host_loss from the golden's own scores; the training fields are there; position row 0 has a
    gradient and the word table's pad row none; rows behind the longest sequence are zero"""
    from multihop_dense_retrieval_amd import reader_loss
    z = ref.golden()
    batch = ref.batch_of(z, tag)
    assert {"starts", "ends", "label", "sent_labels", "token_type_ids"} <= set(batch) and batch["input_ids"].shape[0] <= 5 and batch["input_ids"].shape[1] <= 128
    s = {k: torch.from_numpy(z[f"{tag}.out.{k}"]) for k in ("start_logits", "end_logits", "rank_score")}
    sp = torch.from_numpy(z[f"{tag}.out.sp_score"]) if sp_pred else None
    assert (f"{tag}.out.sp_score" in z.files) == sp_pred
    loss = reader_loss.host_loss(s["start_logits"], s["end_logits"], s["rank_score"], sp, batch, float(z["meta.sp_weight"]))
    want = z[f"{tag}.loss"]
    assert loss.shape == (1,) and abs(float(loss[0]) - float(want[0])) <= 1e-5 * abs(float(want[0])), (float(loss[0]), float(want[0]))
    gpos, rows = z[f"{tag}.g.{ref.POS}"], z[f"{tag}.rows.{ref.WORD}"]
    longest = int(batch["attention_mask"].sum(1).max())
    assert np.abs(gpos[0]).max() > 0 and not gpos[longest:].any() and gpos[:longest].any(axis=1).all()
    assert rows[0] == 0 and not z[f"{tag}.g.{ref.WORD}"][0].any() and z[f"{tag}.g.{ref.WORD}"][1:].any(axis=1).all()
    assert (batch["starts"] >= 0).any() and (batch["starts"] == -1).any()


@pytest.fixture(scope="module")
def restated():
    z = ref.golden()
    out = {}
    for tag, sp_pred in ref.SETS:
        for mutant in (None,) + ref.MUTANTS:
            out[tag, mutant] = ref.restate(ref.checkpoint(sp_pred), ref.batch_of(z, tag), sp_pred, float(z["meta.sp_weight"]), mutant)
    return z, out


@pytest.mark.parametrize("tag,sp_pred", ref.SETS)
def test_restatement_reproduces_the_golden(restated, tag, sp_pred):
    """The CPU fp32 restatement is the reference's computation: loss and every stored gradient within fp32 rounding of the golden -- 2^-12,
    sixty-four times below THRESHOLD -- so a mutant's miss is the defect's and not the restatement's."""
    z, out = restated
    loss, grads, scores = out[tag, None]
    assert abs(float(loss[0]) - float(z[f"{tag}.loss"][0])) <= 1e-5 * abs(float(z[f"{tag}.loss"][0]))
    e = ref.errors(grads, z, tag)
    worst = max(e, key=e.get)
    print(f"{tag}: restatement against the golden, worst e = {e[worst]:.3g} ({worst})")
    assert e[worst] <= 2.0 ** -12 <= ref.THRESHOLD / 64, (worst, e[worst])
    assert set(e) == set(ref.checkpoint(sp_pred))


@pytest.mark.parametrize("mutant", ref.MUTANTS)
@pytest.mark.parametrize("tag,sp_pred", ref.SETS)
def test_each_mutant_misses_the_golden_by_ten_thresholds(restated, tag, sp_pred, mutant):
    z, out = restated
    e = ref.errors(out[tag, mutant][1], z, tag)
    worst = max(e, key=e.get)
    print(f"{tag} {mutant}: worst e = {e[worst]:.3g} ({worst}) = {e[worst] / ref.THRESHOLD:.1f} thresholds")
    assert e[worst] > 10 * ref.THRESHOLD, (mutant, worst, e[worst])
    if mutant != "pos_roberta":  # the two gradient defects touch their own table alone
        assert worst == {"pos_row0_dropped": ref.POS, "type_all_to_row0": ref.TYPE}[mutant]
        assert all(v <= 2.0 ** -12 for k, v in e.items() if k != worst)
