"""GPU (-m gpu): the optimizer step's decoupled mode (include/mdr_optim_adamw.h: mdr_optim_step_ex with decay_mode 1, transformers.AdamW)
against its host replay (tests/adamw_ref.py), and optim.FusedAdam(decoupled_weight_decay=True) on top of it.

Tensor sizes 1, 4095, 4096, 4097 (a chunk is 4096 elements), two decay groups (0.1 on every second tensor), fp16 copies on two of three,
three steps under a moving lr. p, m, v, p16 and the state are held bit for bit against the numpy-float32 replay fed the device's own mult
(the norm's bound is tests/test_optim_gpu.py's business: the norm and finalize kernels are shared and unchanged). Mode 0 through the new
entry point is mdr_optim_step, bit for bit. NaN lies behind every tensor's n and in the workspace.
"""
import numpy as np
import pytest
import torch

import adamw_ref as ref
import optim_ref as oref
from multihop_dense_retrieval_amd._lib import ptr
from oracle.fp import bits, same_bits

pytestmark = pytest.mark.gpu

F = np.float32
SIZES = [1, 4095, 4096, 4097]
HYPER = dict(beta1=0.9, beta2=0.999, eps=1e-8, max_grad_norm=2.0)
LRS = (1e-3, 7e-4, 2.5e-4)  # a moving lr: the step and lr * weight_decay are formed from the lr of the call
SLACK = 8
WD = 0.1


def slack_tensor(values, fill, dtype=torch.float32):
    t = torch.full((len(values) + SLACK,), fill, dtype=dtype, device="cuda")
    t[:len(values)] = torch.from_numpy(values).to("cuda")
    return t


def gradient(rng, n):
    """magnitudes from 2^-30 to 2^10 (the scaled gradient, at loss scale 2^16), both signs"""
    return (np.ldexp(1.0, rng.integers(-30, 10, n)) * rng.uniform(1, 2, n) * rng.choice([-1.0, 1.0], n)).astype(F)


class Table:
    """SIZES plus one tensor without a gradient, on the device with a host mirror: decay WD on every second descriptor, p16 on two of three"""

    def __init__(self, seed, fill, with16=True, scale=2.0 ** 16, dynamic=1):
        from multihop_dense_retrieval_amd import _lib, optim
        self.optim, self._lib = optim, _lib
        rng = np.random.default_rng(seed)
        self.sizes, self.frozen, self.dynamic = SIZES + [70], len(SIZES), dynamic
        n_t = len(self.sizes)
        self.decay = [WD if i % 2 == 0 else 0.0 for i in range(n_t)]
        self.has16 = [with16 and i % 3 != 2 for i in range(n_t)]
        self.p = [rng.normal(0, 0.05, n).astype(F) for n in self.sizes]
        self.m = [rng.normal(0, 1e-3, n).astype(F) for n in self.sizes]
        self.v = [(rng.normal(0, 1e-3, n) ** 2).astype(F) for n in self.sizes]
        self.p16 = [p.astype(np.float16) if h else None for p, h in zip(self.p, self.has16)]
        self.dp, self.dm, self.dv = ([slack_tensor(a, fill) for a in arrs] for arrs in (self.p, self.m, self.v))
        self.dg = [None if i == self.frozen else slack_tensor(np.zeros(n, F), fill) for i, n in enumerate(self.sizes)]
        self.d16 = [slack_tensor(a, fill, torch.float16) if a is not None else None for a in self.p16]
        rows = [(self.dp[i].data_ptr(), 0 if self.dg[i] is None else self.dg[i].data_ptr(), self.dm[i].data_ptr(), self.dv[i].data_ptr(),
                 0 if self.d16[i] is None else self.d16[i].data_ptr(), n, self.decay[i]) for i, n in enumerate(self.sizes)]
        host, self.n_chunks = optim.build_table(rows)
        self.table = torch.from_numpy(host).to("cuda")
        self.ws = torch.full((optim.workspace_bytes(self.sizes) // 4,), fill, dtype=torch.float32, device="cuda")
        self.state = torch.zeros(16, dtype=torch.int32, device="cuda")
        _lib.check(optim.lib().mdr_optim_state_init(ptr(self.state), scale, 0, _lib.current_stream_ptr()))

    def set_grads(self, grads):
        for d, g in zip(self.dg, grads):
            if d is not None:
                d[:len(g)] = torch.from_numpy(g).to("cuda")

    def step(self, lr, mode):
        """mode 0, 1: mdr_optim_step_ex; None: mdr_optim_step"""
        L = self.optim.lib()
        head = (ptr(self.table), len(self.sizes), self.n_chunks, ptr(self.state), lr, HYPER["beta1"], HYPER["beta2"], HYPER["eps"], HYPER["max_grad_norm"],
                self.dynamic, 2000, 2.0 ** 24, 1)
        tail = (ptr(self.ws), self.ws.numel() * 4, 0, self._lib.current_stream_ptr())
        self._lib.check(L.mdr_optim_step(*head, *tail) if mode is None else L.mdr_optim_step_ex(*head, mode, *tail))

    def read_state(self):
        raw = self.state.cpu().numpy().view(np.uint8)[:self.optim.STATE_DTYPE.itemsize].view(self.optim.STATE_DTYPE)[0]
        return {k: raw[k] for k in self.optim.STATE_DTYPE.names}

    def read(self):
        cp = lambda ts: [None if t is None else t.cpu().numpy() for t in ts]  # noqa: E731
        return cp(self.dp), cp(self.dm), cp(self.dv), cp(self.d16), cp(self.dg)


def run_three_steps(mode, fill, with16=True, seed=11):
    t = Table(seed, fill, with16)
    rng = np.random.default_rng(12)
    out = []
    for lr in LRS:
        grads = [gradient(rng, n) for n in t.sizes]
        t.set_grads(grads)
        t.step(lr, mode)
        out.append(dict(state=t.read_state(), grads=grads, read=t.read(), lr=lr))
    return t, out


@pytest.fixture(scope="module")
def adamw_steps():
    return run_three_steps(1, float("nan"))


COUNTERS = ("loss_scale", "unskipped", "adam_step", "b1_pow", "b2_pow", "skipped_last", "skipped_total", "bias1", "bias2")


@pytest.mark.parametrize("with16", [True, False], ids=["p16", "nop16"])
def test_update_and_state_equal_the_replay_bit_for_bit(adamw_steps, with16):
    """p, m, v, p16 after each of three steps under a moving lr, and the state machine's counters; the tensor without a gradient keeps its
    bits; g is +0; nothing behind n moved"""
    t, out = adamw_steps if with16 else run_three_steps(1, float("nan"), with16=False)
    p, m, v = [a.copy() for a in t.p], [a.copy() for a in t.m], [a.copy() for a in t.v]
    model = oref.initial_state(2.0 ** 16)
    for s, rec in enumerate(out):
        st = rec["state"]
        model = oref.advance(model, False, HYPER["beta1"], HYPER["beta2"], 1, 2000, 2.0 ** 24)
        for k in COUNTERS:
            assert bits(np.asarray(st[k])) == bits(np.asarray(model[k]).astype(st[k].dtype)), (s, k, st[k], model[k])
        coef, mult = oref.clip_and_mult(st["grad_norm"], HYPER["max_grad_norm"], 2.0 ** 16)
        assert same_bits(st["clip_coef"], coef) and same_bits(st["mult"], mult)
        dp, dm, dv, d16, dg = rec["read"]
        for i, n in enumerate(t.sizes):
            if i == t.frozen:
                assert same_bits(dp[i][:n], t.p[i]) and same_bits(dm[i][:n], t.m[i]) and same_bits(dv[i][:n], t.v[i]), "a tensor without a gradient moved"
                assert d16[i] is None or same_bits(d16[i][:n], t.p16[i])
                continue
            p[i], m[i], v[i], h = ref.replay_update(p[i], rec["grads"][i], m[i], v[i], t.decay[i], st["mult"], st["bias1"], st["bias2"], rec["lr"],
                                                    HYPER["beta1"], HYPER["beta2"], HYPER["eps"])
            for name, got, want in (("p", dp[i], p[i]), ("m", dm[i], m[i]), ("v", dv[i], v[i])):
                diff = np.flatnonzero(bits(got[:n]) != bits(want))
                assert diff.size == 0, (s, i, n, name, diff[:5], got[diff[:5]], want[diff[:5]])
                assert np.isnan(got[n:]).all(), (s, i, name, "the slack behind n was written")
            assert (d16[i] is not None) == t.has16[i]
            if d16[i] is not None:
                assert same_bits(d16[i][:n], h), (s, i)
                assert np.isnan(d16[i][n:]).all()
            assert not bits(dg[i][:n]).any() and np.isnan(dg[i][n:]).all(), (s, i)
    assert np.isfinite(np.concatenate([a for i, a in enumerate(p) if i != t.frozen])).all()
    # the decay reached p and not the moments: the replay without decay gives the same m and v and another p on the decayed tensors
    g0 = out[0]["grads"][2]
    st0 = out[0]["state"]
    tail = (st0["mult"], st0["bias1"], st0["bias2"], LRS[0], HYPER["beta1"], HYPER["beta2"], HYPER["eps"])
    pn, mn, vn, _ = ref.replay_update(t.p[2], g0, t.m[2], t.v[2], 0.0, *tail)
    d = out[0]["read"]
    assert same_bits(d[1][2][:SIZES[2]], mn) and same_bits(d[2][2][:SIZES[2]], vn) and not same_bits(d[0][2][:SIZES[2]], pn)
    # and it is not the L2 form
    pl, ml, _, _ = oref.replay_update(t.p[2], g0, t.m[2], t.v[2], WD, *tail)
    assert not same_bits(d[1][2][:SIZES[2]], ml) and not same_bits(d[0][2][:SIZES[2]], pl)


def test_mode_zero_through_the_new_entry_point_is_mdr_optim_step():
    _, a = run_three_steps(None, 0.0)
    _, b = run_three_steps(0, 0.0)
    t, c = run_three_steps(1, 0.0)
    differs = False
    for ra, rb, rc in zip(a, b, c):
        for k in ra["state"]:
            assert same_bits(ra["state"][k], rb["state"][k]), k
        for xa, xb, xc in zip(ra["read"], rb["read"], rc["read"]):
            for i in range(len(t.sizes)):
                if xa[i] is not None:
                    assert same_bits(xa[i], xb[i]), i
                    differs |= not same_bits(xa[i], xc[i])
    assert differs, "mode 1 gives mode 0's bits: this test shows nothing"


def test_two_runs_give_the_same_bits_whatever_lies_in_the_slack_and_the_workspace(adamw_steps):
    (t, a), (_, b) = adamw_steps, run_three_steps(1, 0.0)
    for s, (ra, rb) in enumerate(zip(a, b)):
        for k in ra["state"]:
            assert same_bits(ra["state"][k], rb["state"][k]), (s, k)
        for xa, xb in zip(ra["read"], rb["read"]):
            for i, n in enumerate(t.sizes):
                if xa[i] is not None:
                    assert same_bits(xa[i][:n], xb[i][:n]), (s, i)


def test_an_infinite_gradient_skips_the_step_and_halves_the_scale():
    t = Table(21, 0.0)
    rng = np.random.default_rng(22)
    grads = [gradient(rng, n) for n in t.sizes]
    grads[3][-1] = np.inf
    t.set_grads(grads)
    t.step(LRS[0], 1)
    st = t.read_state()
    assert st["skipped_last"] == 1 and st["skipped_total"] == 1 and st["adam_step"] == 0 and st["loss_scale"] == 2.0 ** 15 and st["bias1"] == 0
    dp, dm, dv, d16, dg = t.read()
    for i, n in enumerate(t.sizes):
        assert same_bits(dp[i][:n], t.p[i]) and same_bits(dm[i][:n], t.m[i]) and same_bits(dv[i][:n], t.v[i]), (i, "a skipped step moved p, m or v")
        if d16[i] is not None:
            assert same_bits(d16[i][:n], t.p16[i])
        if dg[i] is not None:
            assert not bits(dg[i][:n]).any(), "zero_grads holds for a skipped step too"
    # the next clean step is the first Adam step, at the halved scale
    grads = [gradient(rng, n) for n in t.sizes]
    t.set_grads(grads)
    t.step(LRS[1], 1)
    st = t.read_state()
    assert st["skipped_last"] == 0 and st["adam_step"] == 1 and st["loss_scale"] == 2.0 ** 15
    want, _, _, _ = ref.replay_update(t.p[1], grads[1], t.m[1], t.v[1], t.decay[1], st["mult"], st["bias1"], st["bias2"], LRS[1], HYPER["beta1"], HYPER["beta2"],
                                      HYPER["eps"])
    assert same_bits(t.read()[0][1][:SIZES[1]], want)


def test_fused_adam_selects_the_mode_and_keeps_the_default():
    """optim.FusedAdam(decoupled_weight_decay=True) is the replay's whole step (two groups, fp16 copies, a parameter without .grad); the
    default is mdr_optim_step's bits as before"""
    from multihop_dense_retrieval_amd import optim
    rng = np.random.default_rng(31)
    host = [rng.normal(0, 0.05, n).astype(F) for n in SIZES + [70]]
    grads = [gradient(rng, n) for n in SIZES] + [None]
    results = {}
    for decoupled in (True, False):
        ps = [torch.nn.Parameter(torch.from_numpy(a.copy()).cuda()) for a in host]
        opt = optim.FusedAdam([{"params": ps[0::2], "weight_decay": WD}, {"params": ps[1::2], "weight_decay": 0.0}], lr=LRS[0], max_grad_norm=HYPER["max_grad_norm"],
                              fp16_copies=[ps[1], ps[2]], decoupled_weight_decay=decoupled)
        for p, g in zip(ps, grads):
            p.grad = None if g is None else torch.from_numpy(g).cuda()
        opt.step()
        st = opt.read_state()
        order = ps[0::2] + ps[1::2]  # the table's order: group by group
        idx = list(range(0, 5, 2)) + list(range(1, 5, 2))
        for p, i in zip(order, idx):
            if grads[i] is None:
                assert same_bits(p.detach().cpu().numpy(), host[i])
                continue
            fn = ref.replay_update if decoupled else oref.replay_update
            want, _, _, h = fn(host[i], grads[i], np.zeros_like(host[i]), np.zeros_like(host[i]), WD if i % 2 == 0 else 0.0, st["mult"], st["bias1"], st["bias2"],
                               LRS[0], 0.9, 0.999, 1e-8)
            assert same_bits(p.detach().cpu().numpy(), want), (decoupled, i)
            if i in (1, 2):
                assert same_bits(opt.half(p).cpu().numpy(), h), (decoupled, i)
        results[decoupled] = [p.detach().cpu().numpy() for p in ps]
    assert not same_bits(results[True][0], results[False][0])
