"""GPU (-m gpu): mdr_reader_select (include/mdr_reader_select.h) against predict()'s literal sorts (qa_eval.select_sweep_host).

About 500 questions per launch, segment sizes mixed and adjacent (empty ones, one wave and one item around it, several strides of a lane),
on a tie-heavy and a low-tie family of fp16 scores; every output sits between tests/guarded.py guard rows and the call is made twice.
Non-finite scores at the first item, the last item and items 63 and 64 of a 129-item question flag that question and no other. n_lambda
0 or 17 is refused and writes nothing; n_q = 0 is a no-op. (Negative or decreasing offsets are the caller's contract:
tests/test_qa_eval_host.py::test_check_offsets_states_the_kernels_contract.)"""
import ctypes

import numpy as np
import pytest
import torch

import select_cases as cases
from guarded import E_INVALID, OK, Guarded, dev

pytestmark = pytest.mark.gpu


def outputs(n_q, K):
    return (Guarded(n_q, (K,), torch.int32, 3, 3, name="winners"), Guarded(n_q, (), torch.int32, 5, 5, name="rank_top", unit="entries"),
            Guarded(n_q, (), torch.int32, 5, 5, name="flags", unit="entries"))


def run(rank, span, q, lambdas):
    """One guarded call: (winners, rank_top, flags) as numpy, the guards checked."""
    from multihop_dense_retrieval_amd import qa_eval
    qa_eval.check_offsets(q, len(rank))
    out = outputs(len(q) - 1, len(lambdas))
    qa_eval.select(dev(rank), dev(span), dev(q), lambdas, out=tuple(g.own for g in out))
    torch.cuda.synchronize()
    return tuple(g.checked() for g in out)


@pytest.fixture(scope="module")
def families():
    """{name: (rank, span, q_offsets, {factor list name: the yardstick})}: computed once, never written."""
    from multihop_dense_retrieval_amd import qa_eval
    out = {}
    for name in ("tie_heavy", "low_tie"):
        rank, span, q = getattr(cases, name)(23, 500)
        out[name] = (rank, span, q, {k: qa_eval.select_sweep_host(rank, span, q, lam) for k, lam in (("sweep", cases.SWEEP), ("one", [0.8]), ("sixteen", cases.SIXTEEN))})
    return out


@pytest.mark.parametrize("name", ["tie_heavy", "low_tie"])
@pytest.mark.parametrize("which,lambdas", [("sweep", cases.SWEEP), ("one", [0.8]), ("sixteen", cases.SIXTEEN)])
def test_kernel_equals_the_literal_sorts(families, name, which, lambdas):
    from multihop_dense_retrieval_amd import qa_eval
    rank, span, q, want = families[name]
    sizes = np.diff(q)
    assert set(cases.BASE_SIZES + cases.EDGE_SIZES) == set(sizes.tolist()) and len(sizes) == 500
    want_w, want_r = want[which]
    w, r, f = run(rank, span, q, lambdas)
    assert not f.any()
    assert np.array_equal(r, want_r), np.nonzero(r != want_r)[0][:10]
    assert np.array_equal(w, want_w), np.argwhere(w != want_w)[:10]
    assert (w[sizes == 0] == -1).all() and (r[sizes == 0] == -1).all()
    w2, r2, f2 = run(rank, span, q, lambdas)  # no atomics: the same bits again
    assert np.array_equal(w, w2) and np.array_equal(r, r2) and np.array_equal(f, f2)
    hw, hr, hf = qa_eval.select_host(rank, span, q, lambdas)  # the numpy statement says the same
    assert np.array_equal(hw, w) and np.array_equal(hr, r) and np.array_equal(hf, f)
    if name == "tie_heavy" and which == "sweep":
        assert (qa_eval.select_host(rank, span, q, lambdas, first_index=True)[0] != want_w).any()  # the inputs tell the rules apart


def test_non_finite_scores_flag_their_question_and_no_other():
    from multihop_dense_retrieval_amd import qa_eval
    rng = np.random.default_rng(4)
    plants = [(pos, val, arr) for pos in (0, 128, 63, 64) for val, arr in ((np.nan, 0), (np.inf, 1), (-np.inf, 0))]
    plants += [(0, np.inf, 0), (128, np.nan, 1), (63, -np.inf, 1), (64, np.nan, 1)]
    sizes, bad = [], []
    for _ in plants:
        sizes += [int(rng.choice(cases.BASE_SIZES)), 129]
        bad.append(len(sizes) - 1)
    sizes.append(7)
    q = cases.offsets_of(sizes)
    grid = np.arange(-2, 2.5, 0.5).astype(np.float16)
    rank, span = rng.choice(grid, q[-1]), rng.choice(grid, q[-1])
    want_w, want_r = qa_eval.select_sweep_host(rank, span, q, cases.SWEEP)  # on the clean scores: the neighbours' yardstick
    for j, (pos, val, arr) in zip(bad, plants):
        (rank, span)[arr][q[j] + pos] = val
    w, r, f = run(rank, span, q, cases.SWEEP)
    assert np.nonzero(f)[0].tolist() == bad and set(f.tolist()) == {0, 1}
    assert (w[bad] == -1).all() and (r[bad] == -1).all()
    rest = np.setdiff1d(np.arange(len(sizes)), bad)
    assert np.array_equal(w[rest], want_w[rest]) and np.array_equal(r[rest], want_r[rest])
    hw, hr, hf = qa_eval.select_host(rank, span, q, cases.SWEEP)
    assert np.array_equal(hw, w) and np.array_equal(hr, r) and np.array_equal(hf, f)


def test_bad_factor_counts_are_refused_and_an_empty_call_is_a_no_op():
    from multihop_dense_retrieval_amd import _lib, qa_eval
    rank, span, q = cases.tie_heavy(2, 40, edge_repeats=1)
    d_rank, d_span, d_q = dev(rank), dev(span), dev(q)
    lam = (ctypes.c_double * 17)(*([0.5] * 17))
    for K in (0, 17, -1):
        out = outputs(40, 17)
        with torch.cuda.device(0):
            code = qa_eval.lib().mdr_reader_select(_lib.ptr(d_rank), _lib.ptr(d_span), _lib.ptr(d_q), 40, lam, lam, K, *(g.ptr() for g in out), 0,
                                                   _lib.current_stream_ptr(torch.device("cuda", 0)))
        torch.cuda.synchronize()
        assert code == E_INVALID and b"n_lambda" in _lib.lib().mdr_last_error()
        for g in out:
            g.checked(asked=False)  # nothing was written
    with pytest.raises(ValueError):
        qa_eval.select(d_rank, d_span, d_q.to(torch.int32), cases.SWEEP)
    with pytest.raises(ValueError):
        qa_eval.select(d_rank.float(), d_span, d_q, cases.SWEEP)
    out = outputs(0, 11)  # n_q = 0
    got = qa_eval.select(d_rank, d_span, dev(np.zeros(1, np.int64)), cases.SWEEP, out=tuple(g.own for g in out))
    torch.cuda.synchronize()
    assert [tuple(t.shape) for t in got] == [(0, 11), (0,), (0,)]
    for g in out:
        g.checked()
    with torch.cuda.device(0):
        assert qa_eval.lib().mdr_reader_select(None, None, None, 0, lam, lam, 11, None, None, None, 0, _lib.current_stream_ptr(torch.device("cuda", 0))) == OK
