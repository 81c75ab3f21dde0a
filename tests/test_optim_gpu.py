"""GPU: the optimizer step (include/mdr_optim.h) against its host model (tests/optim_ref.py), and optim.FusedAdam, momentum_update and
packed_linear's weight16 on top of it.

The update is held bit for bit: p, m, v and p16 after each of three consecutive steps equal the numpy-float32 replay fed the device's own
mult, bias1 and bias2 (csrc/mdr_optim.hip lists the operations; none is contracted).

The norm. A term of a chunk sum passes through at most 30 fp32 roundings (1 / loss_scale and the product enter the square twice: 5; the
thread's 16 additions, the butterfly's 6, the waves' 3), every term is >= 0, the chunk sums are added in fp64, the square root halves a
relative error and its rounding to fp32 adds u = 2^-24:
    |grad_norm - norm64| <= (gamma_30 / 2 + 2 u) norm64,     gamma_k = k u / (1 - k u)
(optim_ref.NORM_REL_BOUND; the second u pays for the fp64 steps and the second-order terms). clip_coef and mult are the host's fp32
expressions of the device's grad_norm, bit for bit.

The trajectory's bar is e(ours) <= 2 e(torch fp32), e the largest |p - p64| / (|p64| + 1e-3) over the 12 tensors after 20 steps: two
correct fp32 implementations differ from fp64 by their own roundings (criterion E)."""
import numpy as np
import pytest
import torch

import optim_ref as ref
from multihop_dense_retrieval_amd._lib import ptr
from oracle.fp import bits, same_bits

pytestmark = pytest.mark.gpu

C = ref.CHUNK
F = np.float32
HYPER = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, max_grad_norm=2.0)
SMALL = [1, 3, 63, 64, 65, 4095, 4096, 4097, 3 * C + 1]
BIG = 9_000_001  # 2198 chunks: more than the grid's 2048 workgroups and than the finalize workgroup's 1024 threads
SLACK = 8        # elements allocated behind every tensor's n


def slack_tensor(values, fill, dtype=torch.float32):
    """a device buffer of len(values) + SLACK elements: the values, then `fill`"""
    t = torch.full((len(values) + SLACK,), fill, dtype=dtype, device="cuda")
    t[:len(values)] = torch.from_numpy(values).to("cuda")
    return t


def gradient(rng, n):
    """magnitudes from 2^-30 to 2^10 (the scaled gradient, at loss scale 2^16), both signs"""
    return (np.ldexp(1.0, rng.integers(-30, 10, n)) * rng.uniform(1, 2, n) * rng.choice([-1.0, 1.0], n)).astype(F)


class Table:
    """A tensor table on the device with its host mirror: sizes, decay on every second descriptor, p16 on two of three, `frozen` = the index
    of a descriptor without a gradient (NaNs among its values), `fill` = what lies behind every tensor's n and in the workspace."""

    def __init__(self, sizes, seed, fill, frozen=None, scale=2.0 ** 16, **state_kw):
        from multihop_dense_retrieval_amd import _lib, optim
        self.optim, self._lib = optim, _lib
        rng = np.random.default_rng(seed)
        self.sizes, self.fill, self.frozen = list(sizes), fill, frozen
        self.decay = [0.01 if i % 2 == 0 else 0.0 for i in range(len(sizes))]
        self.has16 = [i % 3 != 2 for i in range(len(sizes))]
        self.p = [rng.normal(0, 0.05, n).astype(F) for n in sizes]
        if frozen is not None:
            self.p[frozen][::3] = np.nan
        self.m = [(rng.normal(0, 1e-3, n)).astype(F) for n in sizes]
        self.v = [(rng.normal(0, 1e-3, n) ** 2).astype(F) for n in sizes]
        self.p16 = [p.astype(np.float16) if h else None for p, h in zip(self.p, self.has16)]
        self.dp = [slack_tensor(a, fill) for a in self.p]
        self.dm = [slack_tensor(a, fill) for a in self.m]
        self.dv = [slack_tensor(a, fill) for a in self.v]
        self.dg = [None if i == frozen else slack_tensor(np.zeros(n, F), fill) for i, n in enumerate(sizes)]
        self.d16 = [slack_tensor(a, fill, torch.float16) if a is not None else None for a in self.p16]
        rows = [(self.dp[i].data_ptr(), 0 if self.dg[i] is None else self.dg[i].data_ptr(), self.dm[i].data_ptr(), self.dv[i].data_ptr(),
                 0 if self.d16[i] is None else self.d16[i].data_ptr(), n, self.decay[i]) for i, n in enumerate(sizes)]
        host, self.n_chunks = optim.build_table(rows)
        assert self.n_chunks == ref.chunks(self.sizes)[0]
        self.table = torch.from_numpy(host).to("cuda")
        self.ws = torch.full((optim.workspace_bytes(sizes) // 4,), fill, dtype=torch.float32, device="cuda")
        self.state = torch.zeros(16, dtype=torch.int32, device="cuda")
        _lib.check(optim.lib().mdr_optim_state_init(ptr(self.state), scale, 0, _lib.current_stream_ptr()))
        self.model = ref.initial_state(scale)
        self.state_kw = dict(dynamic=1, scale_window=2000, max_scale=2.0 ** 24)
        self.state_kw.update(state_kw)

    def set_grads(self, grads):
        for d, g in zip(self.dg, grads):
            if d is not None:
                d[:len(g)] = torch.from_numpy(g).to("cuda")

    def step(self, lr=HYPER["lr"], zero_grads=1):
        k = self.state_kw
        self._lib.check(self.optim.lib().mdr_optim_step(ptr(self.table), len(self.sizes), self.n_chunks, ptr(self.state), lr, HYPER["beta1"], HYPER["beta2"],
                                                         HYPER["eps"], HYPER["max_grad_norm"], k["dynamic"], k["scale_window"], k["max_scale"], zero_grads,
                                                         ptr(self.ws), self.ws.numel() * 4, 0, self._lib.current_stream_ptr()))

    def read_state(self):
        raw = self.state.cpu().numpy().view(np.uint8)[:self.optim.STATE_DTYPE.itemsize].view(self.optim.STATE_DTYPE)[0]
        return {k: raw[k] for k in self.optim.STATE_DTYPE.names}

    def read(self):
        """(p, m, v, p16, g) as lists of whole host arrays, slack included"""
        cp = lambda ts: [None if t is None else t.cpu().numpy() for t in ts]  # noqa: E731
        return cp(self.dp), cp(self.dm), cp(self.dv), cp(self.d16), cp(self.dg)

    def advance_model(self, bad):
        self.model = ref.advance(self.model, bad, HYPER["beta1"], HYPER["beta2"], self.state_kw["dynamic"], self.state_kw["scale_window"],
                                 self.state_kw["max_scale"])
        return self.model


COUNTERS = ("loss_scale", "unskipped", "adam_step", "b1_pow", "b2_pow", "skipped_last", "skipped_total", "bias1", "bias2")


def assert_counters(got, model, label):
    for k in COUNTERS:
        assert bits(np.asarray(got[k])) == bits(np.asarray(model[k]).astype(got[k].dtype)), (label, k, got[k], model[k])


def run_three_steps(fill):
    """three consecutive steps on SMALL + a frozen tensor + BIG; per step the device's state, the gradients used and everything read back"""
    sizes = SMALL + [70, BIG]
    frozen = len(SMALL)
    t = Table(sizes, 11, fill, frozen=frozen)
    rng = np.random.default_rng(12)
    out = []
    for _ in range(3):
        grads = [gradient(rng, n) for n in sizes]
        t.set_grads(grads)
        t.step()
        out.append(dict(state=t.read_state(), grads=grads, read=t.read()))
    return t, out


@pytest.fixture(scope="module")
def three_steps():
    return run_three_steps(float("nan"))  # NaN behind every tensor's n and in the workspace


@pytest.fixture(scope="module")
def three_steps_again():
    return run_three_steps(0.0)


def test_update_equals_the_replay_bit_for_bit(three_steps):
    """p, m, v, p16 after each of three steps; the tensor without a gradient keeps its bits, NaNs included; g is all +0; nothing behind n moved"""
    t, out = three_steps
    p, m, v = [a.copy() for a in t.p], [a.copy() for a in t.m], [a.copy() for a in t.v]
    for s, rec in enumerate(out):
        st = rec["state"]
        assert st["skipped_last"] == 0 and st["adam_step"] == s + 1
        dp, dm, dv, d16, dg = rec["read"]
        for i, n in enumerate(t.sizes):
            if i == t.frozen:
                assert same_bits(dp[i][:n], t.p[i]) and same_bits(dm[i][:n], t.m[i]) and same_bits(dv[i][:n], t.v[i]) and np.isnan(dp[i][:n]).any()
                assert same_bits(d16[i][:n], t.p16[i])
                continue
            p[i], m[i], v[i], h = ref.replay_update(p[i], rec["grads"][i], m[i], v[i], t.decay[i], st["mult"], st["bias1"], st["bias2"], HYPER["lr"],
                                                    HYPER["beta1"], HYPER["beta2"], HYPER["eps"])
            for name, got, want in (("p", dp[i], p[i]), ("m", dm[i], m[i]), ("v", dv[i], v[i])):
                diff = np.flatnonzero(bits(got[:n]) != bits(want))
                assert diff.size == 0, (s, i, n, name, diff[:5], got[diff[:5]], want[diff[:5]])
                assert np.isnan(got[n:]).all(), (s, i, name)
            if d16[i] is not None:
                assert same_bits(d16[i][:n], h), (s, i)
                assert np.isnan(d16[i][n:]).all()
            assert not bits(dg[i][:n]).any(), (s, i)  # +0, not -0
            assert np.isnan(dg[i][n:]).all()
    assert np.isfinite(np.concatenate([a for i, a in enumerate(p) if i != t.frozen])).all()


def test_norm_within_its_bound_and_clip_and_mult_exact(three_steps):
    t, out = three_steps
    model = ref.initial_state(2.0 ** 16)
    for s, rec in enumerate(out):
        st = rec["state"]
        total = sum(float(((g.astype(np.float64) / 2.0 ** 16) ** 2).sum()) for i, g in enumerate(rec["grads"]) if i != t.frozen)
        norm64 = np.sqrt(total)
        err = abs(float(st["grad_norm"]) - norm64)
        print(f"step {s}: grad_norm {st['grad_norm']:.9g}, fp64 {norm64:.12g}, |err| / bound {err / (ref.NORM_REL_BOUND * norm64):.3g}")
        assert err <= ref.NORM_REL_BOUND * norm64
        coef, mult = ref.clip_and_mult(st["grad_norm"], HYPER["max_grad_norm"], 2.0 ** 16)
        assert same_bits(st["clip_coef"], coef) and same_bits(st["mult"], mult)
        model = ref.advance(model, False, HYPER["beta1"], HYPER["beta2"], 1, 2000, 2.0 ** 24)
        assert_counters(st, model, s)
    assert 0 < out[0]["state"]["clip_coef"] < 1  # the clip is active on these gradients


def test_two_runs_give_the_same_bits_whatever_lies_in_the_slack_and_the_workspace(three_steps, three_steps_again):
    (t, a), (t2, b) = three_steps, three_steps_again
    for s, (ra, rb) in enumerate(zip(a, b)):
        for k in t.optim.STATE_DTYPE.names:
            assert same_bits(ra["state"][k], rb["state"][k]), (s, k)
        for xa, xb in zip(ra["read"], rb["read"]):
            for i, n in enumerate(t.sizes):
                if xa[i] is not None:
                    assert same_bits(xa[i][:n], xb[i][:n]), (s, i)
                    assert not xb[i][n:].any()


@pytest.mark.parametrize("where", ["inf_last_of_last", "nan_first_of_first"])
def test_a_non_finite_gradient_skips_the_step(where):
    t = Table(SMALL, 21, 0.0)
    rng = np.random.default_rng(22)
    grads = [gradient(rng, n) for n in SMALL]
    if where == "inf_last_of_last":
        grads[-1][-1] = np.inf
    else:
        grads[0][0] = np.nan
    t.set_grads(grads)
    t.step()
    st = t.read_state()
    assert st["skipped_last"] == 1 and st["skipped_total"] == 1 and st["adam_step"] == 0 and st["loss_scale"] == 2.0 ** 15
    assert_counters(st, t.advance_model(True), where)
    dp, dm, dv, d16, dg = t.read()
    for i, n in enumerate(SMALL):
        assert same_bits(dp[i][:n], t.p[i]) and same_bits(dm[i][:n], t.m[i]) and same_bits(dv[i][:n], t.v[i]), i
        assert d16[i] is None or same_bits(d16[i][:n], t.p16[i])
        assert not bits(dg[i]).any(), i
    # the next clean step updates from the kept values, at the halved scale
    grads = [gradient(rng, n) for n in SMALL]
    t.set_grads(grads)
    t.step()
    st = t.read_state()
    assert_counters(st, t.advance_model(False), where)
    assert same_bits(st["mult"], ref.clip_and_mult(st["grad_norm"], HYPER["max_grad_norm"], 2.0 ** 15)[1])
    dp = t.read()[0]
    for i, n in enumerate(SMALL):
        want = ref.replay_update(t.p[i], grads[i], t.m[i], t.v[i], t.decay[i], st["mult"], st["bias1"], st["bias2"], HYPER["lr"], HYPER["beta1"],
                                 HYPER["beta2"], HYPER["eps"])[0]
        assert same_bits(dp[i][:n], want), i


@pytest.mark.parametrize("case", ["window3", "clamp", "static"])
def test_state_machine_on_the_device_equals_the_model(case):
    """the host test's sequences: clean x 3 (the scale doubles), inf, nan (halves twice, both skipped), clean; the clamp at max_scale; a
    static scale that never moves but still skips"""
    events, kw, scale = {"window3": ((0, 0, 0, "inf", "nan", 0), dict(scale_window=3), 2.0 ** 16),
                         "clamp": ((0, 0, 0, 0), dict(scale_window=1, max_scale=2.0 ** 18), 2.0 ** 16),
                         "static": ((0, "inf", 0, 0, "nan"), dict(dynamic=0, scale_window=1), 128.0)}[case]
    sizes = [65, 4097]
    t = Table(sizes, 31, 0.0, scale=scale, **kw)
    rng = np.random.default_rng(32)
    seen = []
    for s, ev in enumerate(events):
        grads = [gradient(rng, n) for n in sizes]
        if ev:
            grads[1][4096] = np.inf if ev == "inf" else np.nan
        before = t.read()[0]
        t.set_grads(grads)
        t.step()
        st = t.read_state()
        assert_counters(st, t.advance_model(bool(ev)), (case, s))
        seen.append(float(st["loss_scale"]))
        after = t.read()
        assert all(not bits(g).any() for g in after[4])
        moved = any(not same_bits(a, b) for a, b in zip(before, after[0]))
        assert moved == (not ev), (case, s)
    assert seen == {"window3": [2.0 ** 16, 2.0 ** 16, 2.0 ** 17, 2.0 ** 16, 2.0 ** 15, 2.0 ** 15], "clamp": [2.0 ** 17, 2.0 ** 18, 2.0 ** 18, 2.0 ** 18],
                    "static": [128.0] * 5}[case]


def test_zero_grads_off_leaves_the_gradients():
    t = Table([65, 4097], 41, 0.0)
    grads = [gradient(np.random.default_rng(42), n) for n in t.sizes]
    t.set_grads(grads)
    t.step(zero_grads=0)
    for g, got in zip(grads, t.read()[4]):
        assert same_bits(got[:len(g)], g)
    assert t.read_state()["adam_step"] == 1


def test_trajectory_stays_as_close_to_fp64_as_torch_fp32_does():
    """20 steps of g = S * (p - target) on 12 tensors: FusedAdam, torch's fp32 Adam + clip_grad_norm_ on the device and the fp64 model on the CPU
    from the same start. e(ours) <= 2 e(torch fp32)."""
    from multihop_dense_retrieval_amd import optim
    params, targets = ref.trajectory_start()
    want = ref.torch_trajectory(params, targets, 20, torch.float64)
    e_torch = max(ref.traj_errors(ref.torch_trajectory(params, targets, 20, torch.float32, "cuda"), want))
    ps = [torch.nn.Parameter(torch.from_numpy(p.copy()).cuda()) for p in params]
    ts = [torch.from_numpy(t).cuda() for t in targets]
    opt = optim.FusedAdam([{"params": ps[0::2], "weight_decay": ref.TRAJ["weight_decay"]}, {"params": ps[1::2], "weight_decay": 0.0}], lr=ref.TRAJ["lr"],
                          betas=ref.TRAJ["betas"], eps=ref.TRAJ["eps"], max_grad_norm=ref.TRAJ["max_grad_norm"])
    scale = torch.tensor(2.0 ** 16, device="cuda")
    for s in range(20):
        for p, t in zip(ps, ts):
            g = scale * (p.detach() - t)
            if p.grad is None:
                p.grad = g
            else:
                p.grad.copy_(g)
        opt.step()
    st = opt.read_state()
    assert st["adam_step"] == 20 and st["skipped_total"] == 0 and st["loss_scale"] == 2.0 ** 16
    e_ours = max(ref.traj_errors([p.detach().cpu().numpy() for p in ps], want))
    print(f"trajectory: e(ours) {e_ours:.3g}, e(torch fp32) {e_torch:.3g}")
    assert e_torch > 0
    assert e_ours <= 2 * e_torch, (e_ours, e_torch)


def test_ema_equals_torch_expression_bit_for_bit():
    from multihop_dense_retrieval_amd import optim
    g = torch.Generator().manual_seed(5)
    sizes = [(1,), (65,), (64, 64), (4097,), (3 * C + 1,)]
    ks = [torch.randn(s, generator=g).cuda() for s in sizes]
    qs = [torch.randn(s, generator=g).cuda() for s in sizes]
    hs = [torch.zeros(s, dtype=torch.float16, device="cuda") if i % 2 == 0 else None for i, s in enumerate(sizes)]
    m = 0.999
    for _ in range(2):  # the second call takes the cached tables
        want = [k * m + q * (1. - m) for k, q in zip(ks, qs)]
        host = [ref.replay_ema(k.cpu().numpy(), q.cpu().numpy(), m) for k, q in zip(ks, qs)]
        q_before = [q.clone() for q in qs]
        optim.momentum_update(ks, qs, m, fp16_copies=hs)
        for k, w, (hw, h16), h, q, qb in zip(ks, want, host, hs, qs, q_before):
            assert torch.equal(k.view(torch.int32), w.view(torch.int32))
            assert same_bits(k.cpu().numpy(), hw)
            assert torch.equal(q, qb)
            if h is not None:
                assert torch.equal(h.view(torch.int16), k.half().view(torch.int16)) and same_bits(h.cpu().numpy(), h16)


def test_packed_linear_with_weight16_gives_the_same_bits():
    """M = 70 rows with rows = 67, N = K = 64, the smallest shape the GEMM serves: with the fp16 copy FusedAdam keeps, y, dx, dW and db are
    those of the cast inside."""
    from multihop_dense_retrieval_amd import linear, optim
    g = torch.Generator().manual_seed(9)
    M, N, K = 70, 64, 64
    W = torch.nn.Parameter((0.1 * torch.randn(N, K, generator=g)).cuda())
    b = torch.nn.Parameter((0.1 * torch.randn(N, generator=g)).cuda())
    opt = optim.FusedAdam([W, b], lr=1e-2, fp16_copies=True)
    W.grad = (2.0 ** 16 * torch.randn(N, K, generator=g)).cuda()
    b.grad = (2.0 ** 16 * torch.randn(N, generator=g)).cuda()
    W0 = W.detach().clone()
    opt.step()
    assert not torch.equal(W.detach(), W0)
    w16 = opt.half(W)
    assert w16.dtype == torch.float16 and torch.equal(w16.view(torch.int16), W.detach().half().view(torch.int16))
    with pytest.raises(RuntimeError):
        opt.half(b)  # one-dimensional: no copy kept
    x = torch.randn(M, K, generator=g).half().cuda()
    dy = torch.randn(M, N, generator=g).half().cuda()
    rows = torch.tensor([67], dtype=torch.int32, device="cuda")
    for gelu in (False, True):
        outs = []
        for kw in ({}, {"weight16": w16}):
            xx = x.clone().requires_grad_(True)
            W.grad = b.grad = None
            y = linear.packed_linear(xx, W, b, gelu=gelu, rows=rows, **kw)
            y.backward(dy)
            outs.append((y.detach(), xx.grad, W.grad, b.grad))
        for name, a, c in zip(("y", "dx", "dW", "db"), *outs):
            assert a.dtype == c.dtype and torch.equal(a.view(torch.int16 if a.dtype == torch.float16 else torch.int32),
                                                      c.view(torch.int16 if c.dtype == torch.float16 else torch.int32)), (gelu, name)
        assert outs[0][2].abs().max() > 0


def test_lambda_lr_drives_the_lr_the_kernel_uses():
    """The reference's two groups (no decay on bias and LayerNorm.weight) under LambdaLR with the warm-up schedule: after every step the
    parameters equal the replay at the scheduled lr, bit for bit; a parameter without .grad (the pooler) is left alone; the table is
    uploaded once."""
    from multihop_dense_retrieval_amd import optim
    g = torch.Generator().manual_seed(3)
    named = {"encoder.layer.0.dense.weight": (64, 65), "encoder.layer.0.dense.bias": (64,), "encoder.layer.0.LayerNorm.weight": (64,),
             "encoder.layer.0.LayerNorm.bias": (64,), "encoder.pooler.dense.weight": (8, 8), "project.weight": (33, 129)}
    params = {k: torch.nn.Parameter((0.1 * torch.randn(s, generator=g)).cuda()) for k, s in named.items()}
    no_decay = ["bias", "LayerNorm.weight"]
    groups = [{"params": [p for n, p in params.items() if not any(nd in n for nd in no_decay)], "weight_decay": 0.01},
              {"params": [p for n, p in params.items() if any(nd in n for nd in no_decay)], "weight_decay": 0.0}]
    base = 2e-3
    opt = optim.FusedAdam(groups, lr=base, eps=1e-8, loss_scale=128.0)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: optim.linear_schedule_with_warmup(s, 2, 6))
    live = [n for n in named if "pooler" not in n]
    host = {n: params[n].detach().cpu().numpy().copy() for n in named}
    mom = {n: (np.zeros_like(host[n]), np.zeros_like(host[n])) for n in live}
    keys = []
    for s in range(7):
        grads = {n: (128.0 * 0.01 * torch.randn(named[n], generator=g)).numpy() for n in live}
        loss = sum((params[n] * torch.from_numpy(grads[n] / 128.0).cuda()).sum() for n in live)
        opt.scale_loss(loss).backward()  # d/dp = 128 * grads / 128: exact, the scale is a power of two
        for n in live:
            assert same_bits(params[n].grad.cpu().numpy(), grads[n]), n
        opt.step()
        keys.append(opt._key)
        st = opt.read_state()
        lr = base * optim.linear_schedule_with_warmup(s, 2, 6)
        assert opt.last_lr == lr and st["adam_step"] == s + 1
        for n in live:
            wd = 0.0 if any(nd in n for nd in no_decay) else 0.01
            host[n], m, v, _ = ref.replay_update(host[n], grads[n], *mom[n], wd, st["mult"], st["bias1"], st["bias2"], lr, 0.9, 0.999, 1e-8)
            mom[n] = (m, v)
        for n in named:
            assert same_bits(params[n].detach().cpu().numpy(), host[n]), (s, n)
            assert n not in live or not bits(params[n].grad.cpu().numpy()).any()
        sched.step()
    assert params["encoder.pooler.dense.weight"].grad is None
    assert all(k == keys[0] for k in keys)  # every .grad stayed where the first backward put it
    assert [base * optim.linear_schedule_with_warmup(s, 2, 6) for s in range(7)] == pytest.approx([0.0, 1e-3, 2e-3, 1.5e-3, 1e-3, 5e-4, 0.0], rel=1e-12)
