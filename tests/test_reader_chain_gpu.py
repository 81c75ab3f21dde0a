"""GPU (-m gpu): the answer reader's training chain -- reader_train.TrainableReader, optimizer_for and train_step -- as ONE chain at READER3
(tests/reader_chain_ref.py: ELECTRA, 3 layers, hidden 256, 4 heads, FFN 384), on the batches R160 (the ring attention kernel) and R48 (the
one-shot kernel), with and without the sp head. Every earlier value test of this composition ran at one layer, where the loop over the layers
runs once: a residual taken from the wrong layer's stream, an fp16 copy from the wrong layer, a dropped hand-over between two full layers or
a dropout site that ignores the layer index changes no bit there (tests/test_reader_chain_host.py shows it element for element).

A  forward. eval() gives reader.QAModel's four score tensors bit for bit (the C++ trunk against the Python chain at 3 layers, 4 heads, both
   attention kernels); the scores pass the forward criterion against the fp64 model; the train-mode loss with dropout off is within 2^-6,
   relative, of the fp64 model's (tests/test_reader_train_step_gpu.py's own bar).
E  backward. One train_step at loss scale 256: every gradient divided by the scale passes criterion E against the fp64 model, the yardstick
   being the host regime's own error; the rows that own nothing are exactly zero, the biases that are zero by symmetry are held against their
   sibling's norm (tests/reader_chain_ref.py). Then the same with dropout 0.1 at every site under encoder_chain_ref.DROP_SEED, the fp64 model
   and the regime under the replica's masks: the first value check of the reader's dropout.
R  replay and unwritten rows. Two whole runs give the same bits; with the caching allocator seeded with NaN blocks before the forward and again
   before the backward (encoder_chain_dev.poison) every gradient stays finite and keeps its bits. tests/guarded.py's buffers do not apply: the
   chain hands no kernel a caller-owned output buffer, every output is allocated inside the differentiable functions, whose own tests guard
   them; what a row behind the valid count could leak is what the poisoned allocator shows.
Every check prints its figures (`FWD`, `E ...`, the worst share of the bar, the worst e_dev / e_reg) before it asserts;
profiles/reader_grad_chain.md holds them. The host references are built once per module."""
import time

import numpy as np
import pytest
import torch

import reader_chain_ref as rc
from encoder_chain_dev import poison, same_bits

pytestmark = pytest.mark.gpu

SCALE = 256.0
GEOM = rc.READER3
CASES = [pytest.param(name, sp, id=f"{name}-{'sp' if sp else 'nosp'}") for name in rc.BATCHES for sp in (True, False)]
DROP_CASES = [pytest.param(name, sp, drop, id=f"{name}-{'sp' if sp else 'nosp'}-{'drop' if drop else 'plain'}")
              for name in rc.BATCHES for sp in (True, False) for drop in (False, True)]

_HOST, _RUNS = {}, {}


def host(name, sp, drop):
    """the batch, the weights, model64 and the regime at the device's loss scale on the CPU, once per configuration"""
    if (name, sp, drop) not in _HOST:
        t0 = time.time()
        sd, batch = rc.state_dict(GEOM, sp), rc.make_batch(name, GEOM)
        d = rc.DROP if drop else None
        _HOST[name, sp, drop] = dict(sd=sd, batch=batch, m64=rc.run("model64", sd, GEOM, batch, drop=d), reg=rc.run("regime", sd, GEOM, batch, SCALE, drop=d))
        print(f"WALL host references {name} sp {sp} dropout {drop} {time.time() - t0:.2f} s")
    return _HOST[name, sp, drop]


def make_model(sp, p=0.0):
    from multihop_dense_retrieval_amd import reader_train
    m = reader_train.TrainableReader(rc.config(GEOM, p, p), rc.make_args(sp))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in rc.state_dict(GEOM, sp).items()})
    return m.cuda()


def step(name, sp, drop, with_poison=False):
    """one train_step at loss scale 256 -> (loss, {name: gradient}). with_poison: the same forward and backward as train_step's two lines, the
    allocator seeded with NaN blocks in front of each"""
    from multihop_dense_retrieval_amd import reader_train
    args = rc.make_args(sp)
    model = make_model(sp, rc.DROP[0] if drop else 0.0).train()
    opt = reader_train.optimizer_for(model, args, loss_scale=SCALE)
    batch = rc.torch_batch(rc.make_batch(name, GEOM), "cuda")
    if not with_poison:
        loss = reader_train.train_step(model, batch, args, opt, seed=rc.DROP[1])
    else:
        poison(geom=GEOM)
        out = model(batch, seed=rc.DROP[1], half=opt.half)
        poison(geom=GEOM)
        opt.scale_loss(out).backward()
        loss = out.detach()
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
    assert list(grads) == list(rc.state_dict_shapes(GEOM, sp))
    return loss, grads


def run(name, sp, drop):
    if (name, sp, drop) not in _RUNS:
        _RUNS[name, sp, drop] = step(name, sp, drop)
    return _RUNS[name, sp, drop]


def check_e(g_dev, h, title):
    rows, e_pool = rc.criterion_e(g_dev, h["reg"]["grads"], h["m64"]["grads"])
    print(rc.table(rows, e_pool, "E " + title))
    print(f"E {title}: worst share of the bar {max(r[4] for r in rows):.3f}, worst e_dev / e_reg "
          f"{max(r[1] / r[2] for r in rows if r[2] > 0 and not rc.zero_by_symmetry(r[0])):.3f}")
    for k, e_dev, e_reg, bar, _ in rows:
        if rc.zero_by_symmetry(k):
            print(f"E {title}: {k} |g_dev| / |g64({rc.zero_by_symmetry(k)})| {e_dev:.3e} (zero by symmetry; the regime's {e_reg:.3e}, the bar {bar:.3e})")
    assert len(rows) == len(h["sd"]) and all(np.isfinite(v).all() for v in g_dev.values())
    assert rc.exact_zeros_hold(g_dev, h["batch"], GEOM) and rc.exact_zeros_hold(h["m64"]["grads"], h["batch"], GEOM), \
        "a table row that owns no token (a word row, the pad row, a position at or behind L, a type) has a gradient"
    assert not rc.failures(rows), [(r[0], round(r[4], 3)) for r in rc.failures(rows)]


# ---- A ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,sp", CASES)
def test_a_forward_is_the_inference_readers_and_the_fp64_models(name, sp):
    from multihop_dense_retrieval_amd import reader
    t0 = time.time()
    h = host(name, sp, False)
    batch = rc.torch_batch(h["batch"], "cuda")
    model = make_model(sp).eval()
    served = reader.QAModel(rc.config(GEOM), rc.make_args(sp))
    served.load_state_dict({k: torch.from_numpy(v) for k, v in h["sd"].items()})
    served.to("cuda")
    assert GEOM["layers"] == 3 and GEOM["heads"] == 4 and int(served.residual_fp32) == 2
    want = served(batch)
    with torch.no_grad():
        got = model(batch)
    assert list(got) == list(rc.SCORES)
    for k in got:
        if k == "sp_score" and not sp:
            assert got[k] is None and want[k] is None
            continue
        assert same_bits(got[k], want[k]), (k, "the eval() forward is not reader.QAModel's")
    dev = {k: None if v is None else v.float().cpu().numpy().astype(np.float64).reshape(len(h["batch"]["label"]), -1) for k, v in got.items()}
    rows, e_pool, same_inf = rc.criterion_fwd(dev, h["reg"]["scores"], h["m64"]["scores"])
    print(rc.table(rows, e_pool, f"FWD {name} sp {sp}"))
    print(f"FWD {name} sp {sp}: worst share of the bar {max(r[4] for r in rows):.3f}; the -inf positions are the fp64 model's: {same_inf}")
    model.train()
    loss = model(batch, seed=None)
    l64, ldev = h["m64"]["loss"], float(loss.detach())
    print(f"FWD {name} sp {sp}: train-mode loss, dropout off: device {ldev:.5f} regime {h['reg']['loss']:.5f} model64 {l64:.5f}, "
          f"|device - model64| / |model64| {abs(ldev - l64) / abs(l64):.3e} (bar {2.0 ** -6:.3e})")
    assert same_inf and not rc.failures(rows), [(r[0], round(r[4], 3)) for r in rc.failures(rows)]
    assert loss.shape == (1,) and loss.dtype == torch.float32 and abs(ldev - l64) <= 2.0 ** -6 * abs(l64)
    print(f"WALL a {name} sp {sp} {time.time() - t0:.2f} s")


# ---- E ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,sp", CASES)
def test_e_gradients_against_the_fp64_model(name, sp):
    t0 = time.time()
    h = host(name, sp, False)
    loss, grads = run(name, sp, False)
    print(f"E {name} sp {sp}: loss device {float(loss):.5f} regime {h['reg']['loss']:.5f} model64 {h['m64']['loss']:.5f}")
    check_e({k: v.cpu().numpy().astype(np.float64) / SCALE for k, v in grads.items()}, h, f"{name} sp {sp} scale {SCALE:g}")
    print(f"WALL e {name} sp {sp} {time.time() - t0:.2f} s")


@pytest.mark.parametrize("name,sp", CASES)
def test_e_gradients_with_dropout_against_the_masked_fp64_model(name, sp):
    t0 = time.time()
    h = host(name, sp, True)
    loss, grads = run(name, sp, True)
    plain = host(name, sp, False)["m64"]["loss"]
    print(f"E {name} sp {sp} dropout {rc.DROP[0]}: loss device {float(loss):.5f} regime {h['reg']['loss']:.5f} model64 {h['m64']['loss']:.5f} (without dropout {plain:.5f})")
    assert abs(h["m64"]["loss"] - plain) > 1e-2  # the masks do something
    check_e({k: v.cpu().numpy().astype(np.float64) / SCALE for k, v in grads.items()}, h, f"{name} sp {sp} dropout {rc.DROP[0]} scale {SCALE:g}")
    print(f"WALL e dropout {name} sp {sp} {time.time() - t0:.2f} s")


# ---- R ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,sp,drop", DROP_CASES)
def test_r_two_whole_runs_give_the_same_bits(name, sp, drop):
    t0 = time.time()
    (loss_a, a), (loss_b, b) = run(name, sp, drop), step(name, sp, drop)
    assert same_bits(loss_a, loss_b)
    for k in a:
        assert same_bits(a[k], b[k]), k
    print(f"WALL r replay {name} sp {sp} dropout {drop} {time.time() - t0:.2f} s")


@pytest.mark.parametrize("drop", [False, True], ids=["plain", "drop"])
def test_r_unwritten_rows_are_never_read(drop):
    t0 = time.time()
    H = GEOM["hidden"]
    run("R160", True, drop)
    poison(geom=GEOM)  # the premise: what torch.empty hands out after the seeding is NaN, in the chain's own sizes
    probe = [torch.empty(s, dtype=d, device="cuda") for s, d in (((1280, H), torch.float16), ((1280, 3 * H), torch.float16), ((8, H), torch.float32))]
    print(f"R dropout {drop}: share of NaN in the probes {[round(float(torch.isnan(t).float().mean()), 4) for t in probe]}; reserved "
          f"{torch.cuda.memory_reserved() >> 20} MiB, allocated {torch.cuda.memory_allocated() >> 20} MiB")
    assert all(bool(torch.isnan(t).all()) for t in probe), "the allocator did not hand the seeded blocks out: this test would show nothing"
    del probe
    for name in rc.BATCHES:
        (loss_a, a), (loss_b, b) = run(name, True, drop), step(name, True, drop, with_poison=True)
        assert bool(torch.isfinite(loss_b).all()) and same_bits(loss_a, loss_b), name
        for k in a:
            assert bool(torch.isfinite(b[k]).all()), (name, k)
            assert same_bits(a[k], b[k]), (name, k)
    print(f"WALL r poison dropout {drop} {time.time() - t0:.2f} s")
