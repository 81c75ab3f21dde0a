"""CPU: the fp32 restatement of the optimizer's decoupled mode (tests/adamw_ref.py) against its fp64 version within the derived running
bound over 5 steps, against torch.optim.AdamW where the two formulas coincide, what tells it from the L2 form, and the header / binding
contract of include/mdr_optim_adamw.h. No device and no kernel runs here."""
import ctypes
import os
import re

import numpy as np
import torch

import adamw_ref as ref
import optim_ref as oref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
HYPER = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8)


def gradient(rng, n):
    return (np.ldexp(1.0, rng.integers(-12, 3, n)) * rng.uniform(1, 2, n) * rng.choice([-1.0, 1.0], n)).astype(F)


def test_replay_stays_inside_the_fp64_bound_over_five_steps():
    """p, m and v of the fp32 replay against update64's values and running bounds, with and without decay, under a moving lr; mult and the
    bias corrections are the state machine's fp32 numbers in both (tests/test_optim_host.py holds those against torch)."""
    rng = np.random.default_rng(3)
    n = 5000
    worst = {}
    for wd in (0.0, 0.1):
        p = rng.normal(0, 0.05, n).astype(F)
        m, v = np.zeros(n, F), np.zeros(n, F)
        P, M, V = [(a.astype(np.float64), np.zeros(n)) for a in (p, m, v)]
        st = oref.initial_state(1.0)
        for k in range(5):
            g = gradient(rng, n)
            g[::97] = 0  # elements that see no gradient: v stays 0 until one comes, denom = eps
            st = oref.advance(st, False, HYPER["beta1"], HYPER["beta2"], 0, 2000, 2.0 ** 24)
            lr = HYPER["lr"] * (1 - 0.1 * k)
            args = (wd, F(0.5), st["bias1"], st["bias2"], lr, HYPER["beta1"], HYPER["beta2"], HYPER["eps"])
            p, m, v, _ = ref.replay_update(p, g, m, v, *args)
            P, M, V = ref.update64(P, M, V, g, *args)
            for name, got, (want, bnd) in (("p", p, P), ("m", m, M), ("v", v, V)):
                err = np.abs(got.astype(np.float64) - want)
                assert (err <= bnd).all(), (wd, k, name, float((err / np.maximum(bnd, 1e-300)).max()))
                worst[name] = max(worst.get(name, 0.0), float((err / np.maximum(bnd, 1e-300)).max()))
        # the bound is tight enough to mean something: p is known to a few ulps of the step
        assert float((P[1] / (np.abs(P[0]) + HYPER["lr"])).max()) < 1e-4
    print("RATIO replay against fp64, worst |err| / bound: " + ", ".join(f"{k} {w:.3g}" for k, w in worst.items()))


def test_decay_never_reaches_the_moments():
    """What tells AdamW from Adam's L2 form: with weight_decay = 0.1, m and v after a step are those with weight_decay = 0, bit for bit, and p
    differs; under the L2 form (tests/optim_ref.py) m and v differ."""
    rng = np.random.default_rng(5)
    n = 4097
    p, g = rng.normal(0, 0.05, n).astype(F), gradient(rng, n)
    m, v = rng.normal(0, 1e-3, n).astype(F), (rng.normal(0, 1e-3, n) ** 2).astype(F)
    st = oref.advance(oref.initial_state(1.0), False, HYPER["beta1"], HYPER["beta2"], 0, 2000, 2.0 ** 24)
    tail = (F(1), st["bias1"], st["bias2"], HYPER["lr"], HYPER["beta1"], HYPER["beta2"], HYPER["eps"])
    p0, m0, v0, _ = ref.replay_update(p, g, m, v, 0.0, *tail)
    p1, m1, v1, _ = ref.replay_update(p, g, m, v, 0.1, *tail)
    assert np.array_equal(m0.view(np.uint32), m1.view(np.uint32)) and np.array_equal(v0.view(np.uint32), v1.view(np.uint32))
    assert not np.array_equal(p0, p1)
    # the decay is a shrink of the UPDATED p by lr * wd, one multiply and one subtraction
    w = F(HYPER["lr"]) * F(0.1)
    assert np.array_equal(p1.view(np.uint32), (p0 - w * p0).astype(F).view(np.uint32))
    _, m2, v2, _ = oref.replay_update(p, g, m, v, 0.1, *tail)
    assert not np.array_equal(m2, m0) and not np.array_equal(v2, v0)


def test_agrees_with_torch_adamw_up_to_the_place_of_eps():
    """torch.optim.AdamW decays before the Adam step and divides by sqrt(v) / sqrt(bias2) + eps. With |g| >= 1/8 (sqrt(v) >= 0.0039 after the
    first step, against eps / sqrt(bias2) <= 3.2e-7: 8e-5 of the step) and lr * wd = 1e-4 (the order of the decay: 1e-4 of the step), a step
    of the two differs by less than 1e-3 of its size, at most lr: five steps stay within 5e-3 lr. A check that no term of the formula is
    missing or misplaced, not a rounding bound."""
    rng = np.random.default_rng(7)
    n = 2000
    p = rng.normal(0, 0.05, n).astype(F)
    tp = torch.nn.Parameter(torch.from_numpy(p.astype(np.float64)))
    opt = torch.optim.AdamW([tp], lr=HYPER["lr"], betas=(HYPER["beta1"], HYPER["beta2"]), eps=HYPER["eps"], weight_decay=0.1)
    m, v = np.zeros(n, F), np.zeros(n, F)
    st = oref.initial_state(1.0)
    for _ in range(5):
        g = (np.ldexp(1.0, rng.integers(-3, 3, n)) * rng.uniform(1, 2, n) * rng.choice([-1.0, 1.0], n)).astype(F)
        tp.grad = torch.from_numpy(g.astype(np.float64))
        opt.step()
        st = oref.advance(st, False, HYPER["beta1"], HYPER["beta2"], 0, 2000, 2.0 ** 24)
        p, m, v, _ = ref.replay_update(p, g, m, v, 0.1, F(1), st["bias1"], st["bias2"], HYPER["lr"], HYPER["beta1"], HYPER["beta2"], HYPER["eps"])
    want = tp.detach().numpy()
    assert np.abs(p - want).max() <= 5e-3 * HYPER["lr"], float(np.abs(p - want).max())


def test_header_binding_and_library_agree():
    from multihop_dense_retrieval_amd import _lib, build, optim
    raw = open(os.path.join(ROOT, "include", "mdr_optim_adamw.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = sorted(set(re.findall(r"\b(mdr_[a-z0-9_]+)\s*\(", text)))
    assert declared == ["mdr_optim_step_ex"] == sorted(optim.ADAMW_SIGNATURES) == sorted(optim.ADAMW_EXPORTED_SYMBOLS)
    assert not set(declared) & (set(optim.SIGNATURES) | set(_lib.EXPORTED_SYMBOLS))
    args = optim.ADAMW_SIGNATURES["mdr_optim_step_ex"][1]
    proto = re.search(r"\bmdr_optim_step_ex\s*\(([^)]*)\)", text).group(1)
    assert len(args) == proto.count(",") + 1 == len(optim.SIGNATURES["mdr_optim_step"][1]) + 1
    assert [a.strip().split()[-1] for a in proto.split(",")][13] == "decay_mode" and args[13] is ctypes.c_int
    assert hasattr(ctypes.CDLL(build.build_lib()), "mdr_optim_step_ex")
    defines = {k: int(v, 0) for k, v in re.findall(r"#define (MDR_OPTIM_DECAY_[A-Z0-9_]+) (\w+)", raw)}
    assert defines == {"MDR_OPTIM_DECAY_L2": optim.DECAY_L2, "MDR_OPTIM_DECAY_DECOUPLED": optim.DECAY_DECOUPLED} and (optim.DECAY_L2, optim.DECAY_DECOUPLED) == (0, 1)


def test_an_unknown_decay_mode_is_refused_without_a_launch():
    from multihop_dense_retrieval_amd import _lib, optim
    fake = 0x10000
    for mode in (2, -1):
        rc = optim.lib().mdr_optim_step_ex(fake, 1, 1, fake, 1e-3, 0.9, 0.999, 1e-8, 2.0, 1, 2000, 2.0 ** 24, 1, mode, fake, 1 << 20, 0, None)
        assert rc == -1 and "decay_mode" in _lib.lib().mdr_last_error().decode()
