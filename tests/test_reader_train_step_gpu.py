"""GPU (-m gpu): multihop_dense_retrieval_amd/reader_train.py -- TrainableReader, optimizer_for and train_step -- on the committed tiny
ELECTRA (tests/golden/reader_electra_tiny) and the two batches of tests/golden/reader_train_ref.npz (B = 4, L = 48), with and without the
sp head.

1  the eval() forward's four tensors ARE reader.QAModel's, bit for bit, and a train() forward with dropout off gives the same scores
2  gradients against the reference's (the golden: QAModel in training mode on the CPU in fp32): e = ||g / scale - g_gold|| / ||g_gold|| per
   parameter on the stored entries, every e printed, asserted at reader_train_ref.THRESHOLD (four times the largest e measured on an
   MI355X, rounded up to a power of two; every mutant of tests/test_reader_train_host.py misses by more than ten times that)
3  wiring: loss and every gradient equal a hand-composed chain of the same bricks on copies of the leaves, bit for bit
4  three train_step + opt.step() on one batch at a constant lr lower the loss each time, dropout off
5  dropout 0.1: one seed gives the same bits in every gradient twice, another seed other bits
6  a non-finite gradient skips the step, halves the scale and leaves the masters' bits
7  after steps, inference() equals the module's eval forward
"""
import numpy as np
import pytest
import torch

import reader_train_ref as ref

pytestmark = pytest.mark.gpu

SCALE = 256.0


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def make_model(sp_pred, p=0.0, **kw):
    from multihop_dense_retrieval_amd import reader_train
    m = reader_train.TrainableReader(ref.tiny_config(p, p), ref.make_args(sp_pred, **kw))
    m.load_state_dict(ref.checkpoint(sp_pred))
    return m.cuda()


def grads_of(model):
    return {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}


@pytest.fixture(scope="module")
def z():
    return ref.golden()


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,sp_pred", ref.SETS)
def test_eval_forward_is_the_inference_readers(z, tag, sp_pred):
    from multihop_dense_retrieval_amd import reader
    model = make_model(sp_pred).eval()
    batch = ref.batch_of(z, tag, "cuda")
    served = reader.QAModel(ref.tiny_config(), ref.make_args(sp_pred))
    served.load_state_dict(ref.checkpoint(sp_pred))
    served.to("cuda")
    want = served(batch)
    with torch.no_grad():
        got = model(batch)
    assert list(got) == ["start_logits", "end_logits", "rank_score", "sp_score"]
    for k in got:
        if k == "sp_score" and not sp_pred:
            assert got[k] is None and want[k] is None
            continue
        assert same_bits(got[k], want[k]), (k, "the eval() forward is not reader.QAModel's")
    # the scores are the reference's up to fp16: within 2^-6 of the golden's fp32 scores, relative to the largest finite one
    for k in ("start_logits", "end_logits", "rank_score") + (("sp_score",) if sp_pred else ()):
        a, b = got[k].float().cpu().numpy().reshape(-1), z[f"{tag}.out.{k}"].reshape(-1)
        fin = np.isfinite(b)
        assert (np.isfinite(a) == fin).all() and np.abs(a[fin] - b[fin]).max() <= 2.0 ** -6 * np.abs(b[fin]).max(), k
    # a train() forward with both probabilities 0 makes no dropout call: the loss is qa_loss of the same scores
    from multihop_dense_retrieval_amd import reader_loss
    model.train()
    loss = model(batch, seed=None)
    want_loss = reader_loss.qa_loss(got["start_logits"], got["end_logits"], got["rank_score"], got["sp_score"], batch, float(z["meta.sp_weight"]))
    assert loss.shape == (1,) and loss.dtype == torch.float32 and same_bits(loss.detach(), want_loss)
    gold = float(z[f"{tag}.loss"][0])
    print(f"{tag}: loss {float(loss):.4f}, reference {gold:.4f}")
    assert abs(float(loss) - gold) <= 2.0 ** -6 * abs(gold)


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,sp_pred", ref.SETS)
def test_gradients_against_the_references(z, tag, sp_pred):
    from multihop_dense_retrieval_amd import reader_train
    args = ref.make_args(sp_pred)
    model = make_model(sp_pred).train()
    opt = reader_train.optimizer_for(model, args, loss_scale=SCALE)
    reader_train.train_step(model, ref.batch_of(z, tag, "cuda"), args, opt, seed=0)
    g = {k: (v / SCALE).cpu().numpy() for k, v in grads_of(model).items()}
    assert set(g) == set(ref.checkpoint(sp_pred)) and all(np.isfinite(v).all() for v in g.values())
    e = ref.errors(g, z, tag)
    for k, v in e.items():
        print(f"E {tag} {k} {v:.3e}")
    worst = max(e, key=e.get)
    print(f"E {tag} worst {e[worst]:.3e} ({worst}); threshold {ref.THRESHOLD:.3e}")
    assert e[worst] <= ref.THRESHOLD, (worst, e[worst])
    assert g[ref.POS][0].any() and not g[ref.WORD][0].any()  # position row 0 has its gradient, the word table's pad row none


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------------------
def hand_composed(P, batch, cfg, sp_weight, half):
    """the chain of reader_train.TrainableReader.scores + qa_loss written out once more on the leaves P, brick by brick, one layer"""
    from multihop_dense_retrieval_amd import _lib, reader_loss
    from multihop_dense_retrieval_amd._lib import ptr
    from multihop_dense_retrieval_amd.attention import packed_self_attention
    from multihop_dense_retrieval_amd.embedding import packed_reader_embedding_layer_norm
    from multihop_dense_retrieval_amd.layernorm import packed_layer_norm
    from multihop_dense_retrieval_amd.linear import packed_linear
    ids, mask, tt = (batch[k].contiguous() for k in ("input_ids", "attention_mask", "token_type_ids"))
    B, L = ids.shape
    i32 = lambda n: torch.zeros(n, dtype=torch.int32, device="cuda")  # noqa: E731
    lens, cu, total, order, src, pid = i32(B), i32(B + 1), i32(1), i32(B), i32(B * L), i32(B * L)
    _lib.call(_lib.lib().mdr_test_pack, ptr(ids), ptr(mask), B, L, 0, ptr(lens), ptr(cu), ptr(total), ptr(order), ptr(src), ptr(pid), dev=ids.device)
    E, p, eps = "encoder.embeddings.", "encoder.encoder.layer.0.", cfg.layer_norm_eps
    h16, h32 = packed_reader_embedding_layer_norm(ids, tt, src, total, L, P[E + "word_embeddings.weight"], P[E + "position_embeddings.weight"],
                                                  P[E + "token_type_embeddings.weight"], P[E + "LayerNorm.weight"], P[E + "LayerNorm.bias"], eps, B * L, 0, True)
    qkv_names = [p + "attention.self." + n for n in ("query", "key", "value")]
    qkv = packed_linear(h16, torch.cat([P[n + ".weight"] for n in qkv_names]), torch.cat([P[n + ".bias"] for n in qkv_names]), False, total,
                        torch.cat([half(P[n + ".weight"]) for n in qkv_names]))
    ctx = packed_self_attention(qkv, cu, cfg.num_attention_heads, L, False)
    lin = lambda x, n, gelu=False, rows=total: packed_linear(x, P[n + ".weight"], P[n + ".bias"], gelu, rows, half(P[n + ".weight"]))  # noqa: E731
    a16, a32 = packed_layer_norm(lin(ctx, p + "attention.output.dense"), h32, P[p + "attention.output.LayerNorm.weight"], P[p + "attention.output.LayerNorm.bias"],
                                 eps, total, True)
    f2 = lin(lin(a16, p + "intermediate.dense", True), p + "output.dense")
    o16, _ = packed_layer_norm(f2, a32, P[p + "output.LayerNorm.weight"], P[p + "output.LayerNorm.bias"], eps, total, True)
    dense16 = lin(o16[cu[:-1].to(torch.int64)].contiguous(), "pooler.dense", False, None)
    s = reader_loss.reader_heads(o16, dense16, cu, batch, {k: P[k] for k in reader_loss.HEAD_KEYS if k in P})
    return reader_loss.qa_loss(s["start_logits"], s["end_logits"], s["rank_score"], s["sp_score"], batch, sp_weight)


@pytest.mark.parametrize("tag,sp_pred", ref.SETS)
def test_wiring_is_the_hand_composed_chain(z, tag, sp_pred):
    from multihop_dense_retrieval_amd import optim, reader_train
    args = ref.make_args(sp_pred)
    batch = ref.batch_of(z, tag, "cuda")
    model = make_model(sp_pred).train()
    opt = reader_train.optimizer_for(model, args, loss_scale=SCALE)
    names = [k for k, _ in model.named_parameters()]
    P = {k: v.detach().clone().requires_grad_(True) for k, v in model.named_parameters()}
    decay, no_decay = reader_train.decay_groups(names)
    ref_opt = optim.FusedAdam([{"params": [P[k] for k in decay], "weight_decay": args.weight_decay}, {"params": [P[k] for k in no_decay], "weight_decay": 0.0}],
                              lr=args.learning_rate, eps=args.adam_epsilon, max_grad_norm=args.max_grad_norm, loss_scale=SCALE,
                              fp16_copies=[P[k] for k in reader_train.fp16_copy_names(names)], decoupled_weight_decay=True)
    assert opt.decoupled_weight_decay and [g["weight_decay"] for g in opt.param_groups] == [args.weight_decay, 0.0]
    mine = dict(model.named_parameters())
    for step in range(2):
        loss = reader_train.train_step(model, batch, args, opt, seed=step)
        ref_loss = hand_composed(P, batch, ref.tiny_config(), args.sp_weight, ref_opt.half)
        ref_opt.scale_loss(ref_loss).backward()
        assert same_bits(loss, ref_loss.detach()), step
        for k in names:
            assert same_bits(mine[k].grad, P[k].grad), (step, k, "gradient")
        opt.step()
        ref_opt.step()
        for k in names:
            assert same_bits(mine[k].detach(), P[k].detach()), (step, k, "parameter")
        for k in reader_train.fp16_copy_names(names):
            assert same_bits(opt.half(mine[k]), ref_opt.half(P[k])), (step, k, "fp16 copy")
    st = opt.read_state()
    assert st["skipped_total"] == 0 and st["adam_step"] == 2, st
    assert not opt_is_adam(make_model(sp_pred), ref.make_args(sp_pred)) and opt_is_adam(make_model(sp_pred), ref.make_args(sp_pred, use_adam=True))


def opt_is_adam(model, args):
    from multihop_dense_retrieval_amd import reader_train
    return not reader_train.optimizer_for(model, args).decoupled_weight_decay


# ---- 4, 7 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,sp_pred", ref.SETS)
def test_three_steps_lower_the_loss_and_inference_follows(z, tag, sp_pred):
    from multihop_dense_retrieval_amd import reader_train
    args = ref.make_args(sp_pred, learning_rate=1e-3, weight_decay=0.0)
    batch = ref.batch_of(z, tag, "cuda")
    model = make_model(sp_pred).train()
    opt = reader_train.optimizer_for(model, args, loss_scale=SCALE)
    losses = []
    for step in range(3):
        losses.append(float(reader_train.train_step(model, batch, args, opt, seed=step)))
        opt.step()
    with torch.no_grad():
        losses.append(float(model(batch, half=opt.half)))
    print(f"{tag}: losses " + " -> ".join(f"{x:.3f}" for x in losses))
    assert opt.read_state()["skipped_total"] == 0 and all(b < a for a, b in zip(losses, losses[1:])), losses
    model.eval()
    with torch.no_grad():
        mine = model(batch)
    served = model.inference()(batch)
    for k in mine:
        assert (mine[k] is None and served[k] is None) or same_bits(mine[k], served[k]), (k, "inference() after steps is not the module's eval forward")


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------------------
def test_dropout_is_replayable_by_its_seed(z):
    from multihop_dense_retrieval_amd import reader_train
    tag, sp_pred = ref.SETS[0]
    args = ref.make_args(sp_pred)
    batch = ref.batch_of(z, tag, "cuda")
    runs = []
    for seed in (11, 11, 12):
        model = make_model(sp_pred, p=0.1).train()
        opt = reader_train.optimizer_for(model, args, loss_scale=SCALE)
        loss = reader_train.train_step(model, batch, args, opt, seed=seed)
        runs.append((loss, grads_of(model)))
    plain = make_model(sp_pred).train()
    plain_loss = reader_train.train_step(plain, batch, args, reader_train.optimizer_for(plain, args, loss_scale=SCALE), seed=11)
    assert same_bits(runs[0][0], runs[1][0]) and not same_bits(runs[0][0], runs[2][0]) and not same_bits(runs[0][0], plain_loss)
    assert set(runs[0][1]) == set(ref.checkpoint(sp_pred))
    for k in runs[0][1]:
        assert bool(torch.isfinite(runs[0][1][k]).all()) and same_bits(runs[0][1][k], runs[1][1][k]), (k, "one seed, two gradients")
    differ = [k for k in runs[0][1] if not same_bits(runs[0][1][k], runs[2][1][k])]
    assert len(differ) >= len(runs[0][1]) - 2, "another seed left most gradients alone"
    with pytest.raises(ValueError):
        make_model(sp_pred, p=0.1).train()(batch)  # dropout without a seed


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------------------
def test_a_non_finite_gradient_skips_the_step_and_leaves_the_masters(z):
    from multihop_dense_retrieval_amd import reader_train
    tag, sp_pred = ref.SETS[0]
    args = ref.make_args(sp_pred)
    batch = ref.batch_of(z, tag, "cuda")
    model = make_model(sp_pred).train()
    opt = reader_train.optimizer_for(model, args)  # the dynamic scale, 2^16
    before = {k: v.detach().clone() for k, v in model.named_parameters()}
    half_before = {k: opt.half(p).clone() for k, p in model.named_parameters() if k in reader_train.fp16_copy_names(list(before))}
    reader_train.train_step(model, batch, args, opt, seed=0)
    g = grads_of(model)
    if all(bool(torch.isfinite(v).all()) for v in g.values()):  # nothing overflowed at 2^16 on this batch: inject the infinity
        model.rank.bias.grad[0] = float("inf")
    opt.step()
    st = opt.read_state()
    assert st["skipped_last"] == 1 and st["adam_step"] == 0 and st["loss_scale"] == 2.0 ** 15, st
    for k, v in model.named_parameters():
        assert same_bits(v.detach(), before[k]), (k, "a skipped step changed a master")
        assert not bool(v.grad.any()), (k, "a skipped step left a gradient behind")
    for k, h in half_before.items():
        assert same_bits(opt.half(dict(model.named_parameters())[k]), h), (k, "a skipped step changed an fp16 copy")
    loss = reader_train.train_step(model, batch, args, opt, seed=0)
    opt.step()
    st = opt.read_state()
    assert bool(torch.isfinite(loss).all()) and st["adam_step"] + st["skipped_total"] == 2
