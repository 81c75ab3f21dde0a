"""GPU (-m gpu): mdr_inbatch_rank (include/mdr_inbatch.h) -- the fused contraction, rank count and log-sum-exp of the retriever's
in-batch-negative evaluation -- against integer / fp64 arithmetic done here.

Exact grid. Inputs are multiples of 1/8 in [-4, 4] with d = 768: every product is a multiple of 1/64 and every partial sum is below
768 * 16 = 12288 = 786432 / 64, far inside the 2^24 integers fp32 holds, so the fp32 accumulation is exact in ANY order and the fp16
rounding of mode O1 is a pure function of the exact score. Expected ranks and target scores come from int64 products here, rounded
with numpy's float16 (round to nearest even) for mode O1 and ranked with the stable tie rule; the device must EQUAL them. Mode O1 ties
heavily on these inputs (scores of magnitude 10^2..10^3 on a grid of 1/64 rounded to 11 bits), which is the point.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import fp

pytestmark = pytest.mark.gpu

F32, O1 = 0, 1


def grid_inputs(B, d, seed):
    """q, q_sp, c1, c2 [B, d] and neg [B, 2, d] as int64 multiples of 1/8 in [-4, 4] (i.e. integers in [-32, 32]), with planted rows."""
    rng = np.random.default_rng(seed)
    q, qsp, c1, c2 = (rng.integers(-32, 33, size=(B, d)) for _ in range(4))
    neg = rng.integers(-32, 33, size=(B, 2, d))
    if B >= 2:
        c2[0] = 32 * np.sign(q[0]) + (q[0] == 0)  # row 0: the masked column (its own bridge passage) would otherwise win hop 1
        neg[1, 0] = 32 * np.sign(q[1])            # row 1: a negative wins hop 1
        neg[1, 1] = 32 * np.sign(qsp[1])          #        and hop 2
    if B >= 31:
        c2[5] = c1[5]                             # c1 == c2 duplicates: column 5 and column B + 5 tie in every row
        c1[7] = c1[6]                             # duplicates inside c1: columns 6 and 7 tie, the target of row 7 comes second
        c2[9] = c2[8]
        q[10] = 0                                 # an all-zero query: every finite score is 0, every column ties
        qsp[10] = 0
        q[12] = q[11]                             # two equal questions
    return q, qsp, c1, c2, neg


def expected(q, qsp, c1, c2, neg, mode):
    """(rank1, rank2, tscore1, tscore2, scores1, scores2) from int64 products; scores are what the device compares, as float64."""
    B = q.shape[0]
    ctx = np.concatenate([c1, c2])
    out = []
    for h, Q in enumerate((q, qsp)):
        s = np.concatenate([Q @ ctx.T, np.einsum("bd,bnd->bn", Q, neg)], axis=1).astype(np.float64) / 64.0  # exact
        if mode == O1:
            s = s.astype(np.float16).astype(np.float64)
        if h == 0:
            s[np.arange(B), B + np.arange(B)] = -np.inf
        t = np.arange(B) + h * B
        st = s[np.arange(B), t][:, None]
        before = np.arange(s.shape[1])[None, :] < t[:, None]
        out.append((1 + (s > st).sum(1) + ((s == st) & before).sum(1), st[:, 0], s))
    return out[0][0], out[1][0], out[0][1], out[1][1], out[0][2], out[1][2]


def run(q, qsp, c1, c2, neg, mode):
    from multihop_dense_retrieval_amd import criterions
    f = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()  # noqa: E731
    r = criterions.inbatch_rank(f(q), f(qsp), f(c1), f(c2), f(neg[:, 0]), f(neg[:, 1]), mode)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in r.items()}


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float32))).astype(np.float64)


@pytest.mark.parametrize("mode", [F32, O1])
@pytest.mark.parametrize("B", [1, 2, 31, 64, 257, 1000])
def test_ranks_and_target_scores_are_bit_exact_on_the_grid(B, mode):
    q, qsp, c1, c2, neg = grid_inputs(B, 768, 100 + B)
    r1, r2, t1, t2, s1, s2 = expected(q, qsp, c1, c2, neg, mode)
    got = run(q / 8.0, qsp / 8.0, c1 / 8.0, c2 / 8.0, neg / 8.0, mode)
    assert np.array_equal(got["tscore1"].astype(np.float64), t1)
    assert np.array_equal(got["tscore2"].astype(np.float64), t2)
    assert np.array_equal(got["rank1"], r1), np.nonzero(got["rank1"] != r1)[0][:10]
    assert np.array_equal(got["rank2"], r2), np.nonzero(got["rank2"] != r2)[0][:10]
    if B >= 2:
        assert r1[0] < 2 * B + 2 and s1[0, B] == -np.inf           # the masked column does not count
        assert r1[1] >= 2 and r2[1] >= 2                            # a negative beats the target
    if B >= 31:
        assert r2[5] >= 2 and r1[7] >= 2 and r2[9] >= 2             # duplicates: the later column ranks behind its twin
        assert r1[10] == 1 + 10 and r2[10] == 1 + B + 10            # all-zero query: ties only, rank = 1 + columns before the target
    if mode == O1 and B >= 64:  # the grid really ties under fp16 rounding
        ties = sum(int(((s[i] == s[i, t]).sum() > 1)) for s, off in ((s1, 0), (s2, B)) for i, t in ((i, i + off) for i in range(B)))
        assert ties >= 1, ties  # (rows whose target shares its fp16 score with another column; the planted duplicates tie in both modes)


def check_lse(dev, s, label):
    """Device log-sum-exp against fp64 over the same (bit-known) scores; the bound is derived in test_log_sum_exp_on_the_grid."""
    ref = torch.logsumexp(torch.from_numpy(s), dim=1).numpy()  # fp64 over the same (rounded) scores
    t32 = torch.logsumexp(torch.from_numpy(s.astype(np.float32)), dim=1).numpy().astype(np.float64)
    u = ulp32(ref)
    torch_ulps = np.abs(t32 - ref) / u
    dev_ulps = np.abs(dev.astype(np.float64) - ref) / u
    bound = max(1.0, 4.0 * torch_ulps.max())
    print(f"{label}: device {dev_ulps.max():.3f} ulp, torch fp32 {torch_ulps.max():.3f} ulp, bound {bound:.3f}, "
          f"ratio {dev_ulps.max() / max(torch_ulps.max(), 1e-30):.3f}")
    assert dev_ulps.max() <= bound, (label, dev_ulps.max(), bound)


@pytest.mark.parametrize("mode", [F32, O1])
@pytest.mark.parametrize("B", [2, 64, 1000])
def test_log_sum_exp_on_the_grid(B, mode):
    """The scores are bit-known, so the only error is fp32 exp / log / summation. Bound: the error of torch.logsumexp in fp32 on the same scores,
    measured here in units of the result's fp32 ulp (the worst row), times 4 for a different summation tree over up to 6002 terms; never less
    than one ulp of the result."""
    q, qsp, c1, c2, neg = grid_inputs(B, 768, 100 + B)
    _, _, _, _, s1, s2 = expected(q, qsp, c1, c2, neg, mode)
    got = run(q / 8.0, qsp / 8.0, c1 / 8.0, c2 / 8.0, neg / 8.0, mode)
    for name, s in (("lse1", s1), ("lse2", s2)):
        check_lse(got[name], s, f"B={B} mode={mode} {name}")


def test_realistic_rows_mode_f32():
    """B = 512, d = 768, q, q_sp, neg ~ N(0, 1), c1 = a q + N(0, 1), c2 = a q_sp + N(0, 1) with a = 0.2, seed 0. A rank is accepted inside
    [1 + #{s > t + m}, #{s >= t - m}] from fp64 scores with m = 2 * 768 * 2^-24 * (sum |q||c| + sum |q||c_t|), the accumulation bound of an
    fp32 dot product of 768 terms in any order (the -inf column is excluded before m is formed). At least 95 % of the rows must have a
    one-point interval, so that the interval cannot hide a wrong count."""
    B, d, a = 512, 768, 0.2
    rng = np.random.default_rng(0)
    q, qsp = rng.standard_normal((B, d)).astype(np.float32), rng.standard_normal((B, d)).astype(np.float32)
    neg = rng.standard_normal((B, 2, d)).astype(np.float32)
    c1 = (a * q + rng.standard_normal((B, d))).astype(np.float32)
    c2 = (a * qsp + rng.standard_normal((B, d))).astype(np.float32)
    got = run(q, qsp, c1, c2, neg, F32)
    ctx = np.concatenate([c1, c2]).astype(np.float64)
    for h, (Q, name) in enumerate(((q, "rank1"), (qsp, "rank2"))):
        Q64 = Q.astype(np.float64)
        s = np.concatenate([Q64 @ ctx.T, np.einsum("bd,bnd->bn", Q64, neg.astype(np.float64))], axis=1)
        ab = np.concatenate([np.abs(Q64) @ np.abs(ctx).T, np.einsum("bd,bnd->bn", np.abs(Q64), np.abs(neg.astype(np.float64)))], axis=1)
        t = np.arange(B) + h * B
        keep = np.ones_like(s, bool)
        if h == 0:
            keep[np.arange(B), B + np.arange(B)] = False
        st = s[np.arange(B), t][:, None]
        m = 2 * 768 * fp.U32 * (ab + ab[np.arange(B), t][:, None])
        lo = 1 + ((s > st + m) & keep).sum(1)
        hi = ((s >= st - m) & keep).sum(1)
        decided = (lo == hi).mean()
        print(f"hop {h + 1}: {decided:.4f} of the rows decided by the fp64 reference alone")
        assert decided >= 0.95
        assert ((got[name] >= lo) & (got[name] <= hi)).all(), np.nonzero((got[name] < lo) | (got[name] > hi))[0][:10]
        ts = got["tscore1" if h == 0 else "tscore2"].astype(np.float64)
        assert (np.abs(ts - st[:, 0]) <= 768 * fp.U32 * ab[np.arange(B), t]).all()


@pytest.mark.parametrize("mode", [F32, O1])
def test_small_shapes_b1_and_d64(mode):
    """B = 1: the hop-1 mask hits column B + 0, not the target, so the target score is finite; d = 64 is the tiny test geometry's width."""
    for B, d in ((1, 768), (1, 64), (5, 64), (33, 64), (3, 32)):
        rng = np.random.default_rng(B * 1000 + d)
        q, qsp, c1, c2 = (rng.integers(-32, 33, size=(B, d)) for _ in range(4))
        neg = rng.integers(-32, 33, size=(B, 2, d))
        r1, r2, t1, t2, s1, s2 = expected(q, qsp, c1, c2, neg, mode)
        got = run(q / 8.0, qsp / 8.0, c1 / 8.0, c2 / 8.0, neg / 8.0, mode)
        assert np.isfinite(got["tscore1"]).all()
        for k, e in (("rank1", r1), ("rank2", r2), ("tscore1", t1), ("tscore2", t2)):
            assert np.array_equal(got[k].astype(np.float64), e.astype(np.float64)), (B, d, k)
        for k, s in (("lse1", s1), ("lse2", s2)):
            check_lse(got[k], s, f"B={B} d={d} mode={mode} {k}")


@pytest.mark.parametrize("mode", [F32, O1])
def test_nan_inputs_follow_the_documented_rule(mode):
    """Inputs that are NaN on arrival: a NaN score never counts as greater or equal, a row whose target score is NaN ranks last (2B + 2), the
    other rows' counts are what they are without the NaN columns, and a row's log-sum-exp is NaN exactly when one of its scores is."""
    B, d = 40, 64
    rng = np.random.default_rng(3)
    q, qsp, c1, c2 = (rng.integers(-32, 33, size=(B, d)).astype(np.float64) for _ in range(4))
    neg = rng.integers(-32, 33, size=(B, 2, d)).astype(np.float64)
    q[3, 5] = np.nan    # hop-1 row 3: every score NaN -> rank 2B + 2
    c1[17, 0] = np.nan  # column 17 is NaN in every row of both hops: never counted; it is the hop-1 target of row 17
    neg[20, 1, 2] = np.nan
    got = run(q / 8.0, qsp / 8.0, c1 / 8.0, c2 / 8.0, neg / 8.0, mode)
    ctx = np.concatenate([c1, c2])
    for h, Q in enumerate((q, qsp)):
        s = np.concatenate([Q @ ctx.T, np.einsum("bd,bnd->bn", Q, neg)], axis=1) / 64.0
        if mode == O1:
            s = s.astype(np.float16).astype(np.float64)
        if h == 0:
            s[np.arange(B), B + np.arange(B)] = -np.inf
        t = np.arange(B) + h * B
        st = s[np.arange(B), t][:, None]
        with np.errstate(invalid="ignore"):
            rank = 1 + (s > st).sum(1) + ((s == st) & (np.arange(s.shape[1])[None, :] < t[:, None])).sum(1)
        rank = np.where(np.isnan(st[:, 0]), 2 * B + 2, rank)
        assert np.array_equal(got[f"rank{h + 1}"], rank)
        assert np.array_equal(np.isnan(got[f"lse{h + 1}"]), np.isnan(s).any(1))
        assert np.array_equal(np.isnan(got[f"tscore{h + 1}"]), np.isnan(st[:, 0]))
    assert got["rank1"][3] == 2 * B + 2 and got["rank1"][17] == 2 * B + 2 and got["rank2"][17] < 2 * B + 2


def test_bad_arguments_are_errors_not_undefined_behaviour():
    from multihop_dense_retrieval_amd import _lib, criterions
    L = criterions.lib()
    x = torch.zeros((4, 64), dtype=torch.float32, device="cuda")
    ctx = torch.zeros((8, 64), dtype=torch.float32, device="cuda")
    neg = torch.zeros((4, 2, 64), dtype=torch.float32, device="cuda")
    rk = torch.zeros(4, dtype=torch.int32, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def call(q=p(x), qsp=p(x), c=p(ctx), n=p(neg), B=4, d=64, mode=0, r1=p(rk), r2=p(rk)):
        return L.mdr_inbatch_rank(q, qsp, c, n, B, d, mode, r1, r2, None, None, None, None, None, 0, None)

    assert call() == 0  # the optional outputs and the workspace may be NULL
    torch.cuda.synchronize()
    for kw, word in ((dict(B=0), "B"), (dict(B=-3), "B"), (dict(q=None), "NULL"), (dict(c=None), "NULL"), (dict(n=None), "NULL"), (dict(r1=None), "NULL"),
                     (dict(r2=None), "NULL"), (dict(d=48), "d"), (dict(d=0), "d"), (dict(d=2048), "d"), (dict(mode=2), "mode")):
        assert call(**kw) == -1, kw
        assert word in L.mdr_last_error().decode(), (kw, L.mdr_last_error())
    with pytest.raises(_lib.MdrError):
        _lib.check(call(B=0))
    with pytest.raises(RuntimeError, match="HIP device"):
        criterions.mhop_eval({k: torch.zeros(2, 64) for k in ("q", "q_sp1", "c1", "c2", "neg_1", "neg_2")}, None)


def test_mhop_eval_and_loss_value_match_the_host_formula_on_the_grid():
    """criterions.mhop_eval / mhop_loss_value (device) against mhop_eval_host / the CrossEntropyLoss of the host scores: on the grid the host's
    fp32 matmul is exact too, so the reciprocal ranks are equal in both modes and the loss differs by fp32 round-off of its exp / log / mean."""
    import types
    from multihop_dense_retrieval_amd import criterions
    q, qsp, c1, c2, neg = grid_inputs(64, 768, 5)
    outs = {k: torch.from_numpy((v / 8.0).astype(np.float32)) for k, v in (("q", q), ("q_sp1", qsp), ("c1", c1), ("c2", c2), ("neg_1", neg[:, 0]), ("neg_2", neg[:, 1]))}
    dev = {k: v.cuda() for k, v in outs.items()}
    for fp16 in (False, True):
        got = criterions.mhop_eval(dev, types.SimpleNamespace(fp16=fp16))
        assert got == criterions.mhop_eval_host(outs, fp16)
        assert all(isinstance(x, float) for x in got["rrs_1"] + got["rrs_2"])
        a, b = criterions.mhop_loss_value(dev, fp16), criterions.mhop_loss_value(outs, fp16)
        # both sides hold each row's log-sum-exp to a few fp32 ulps OF THAT VALUE (4 for the device, as above, and as many for torch's own fp32
        # cross entropy); the loss is a mean of lse - t per hop, so it inherits at most that absolute error per hop
        s1, s2 = criterions.host_scores(outs, fp16)
        tol = sum(8 * 2.0 ** -23 * float(torch.logsumexp(s.double(), dim=1).abs().max()) for s in (s1, s2))
        print(f"fp16={fp16}: loss device {a!r} host {b!r} tol {tol:.3e}")
        assert abs(a - b) <= tol, (a, b, tol)
