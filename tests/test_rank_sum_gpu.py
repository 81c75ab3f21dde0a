"""GPU (-m gpu): mdr_rank_sum (include/mdr_rank_sum.h), the ordered gradient sum of training on several ranks, bit for bit against
dist.rank_sum_host (numpy float32 adding one row after another).

1  n in {1, 3, 4, 5, 255, 256, 257, 3073, 2^20 + 3} x N in {1, 2, 3, 8, 16} x stride in {n rounded up to 4, that plus 1024}: magnitudes span
   2^-20 .. 2^20 so that the order shows, the rows' padding n .. stride is NaN and must not leak, the output sits between guards, and a
   second call gives the same bits
2  designed values: -0.0 everywhere, +inf meeting -inf, a NaN in one rank, one rank as a copy of the bits (a NaN's payload included)
3  every violated constraint returns MDR_E_INVALID and leaves the output untouched

Where the result is a NaN the test asks for a NaN, not for its bits: IEEE 754 leaves the sign and payload of a generated or propagated NaN
to the implementation, and numpy on the host and the device choose differently (inf - inf is 0xFFC00000 on x86). Everything else is compared
as bits.
"""
import numpy as np
import pytest
import torch

from guarded import E_INVALID, OK, Guarded, assert_untouched, dev

pytestmark = pytest.mark.gpu

NS = (1, 3, 4, 5, 255, 256, 257, 3073, 2 ** 20 + 3)
RANKS = (1, 2, 3, 8, 16)
GUARD = 64  # elements: the call's own part stays 16-byte aligned behind it


def wide(seed, shape):
    rng = np.random.RandomState(seed)
    return (rng.standard_normal(shape) * np.exp2(rng.randint(-20, 21, shape))).astype(np.float32)


@pytest.fixture(scope="module")
def pool():
    """16 rows of the longest case, drawn once: every case reads its corner of them and nobody writes them."""
    a = wide(11, (max(RANKS), max(NS)))
    a.setflags(write=False)
    return a


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def call(recv_dev, N, n, stride, out_dev):
    from multihop_dense_retrieval_amd import _lib, dist
    return dist.lib().mdr_rank_sum(_lib.ptr(recv_dev), N, n, stride, _lib.ptr(out_dev), _lib.current_stream_ptr())


def run(rows, stride):
    """rows [N, n] -> the device's out[0 .. n) for recv rows of `stride` floats whose padding is NaN, from a guarded buffer, called twice."""
    N, n = rows.shape
    recv = np.full((N, stride), np.nan, np.float32)
    recv[:, :n] = rows
    recv_dev = dev(recv)
    outs = []
    for _ in range(2):
        g = Guarded(n, (), torch.float32, GUARD, GUARD, name="out", unit="elements")
        assert call(recv_dev, N, n, stride, g.own) == OK
        torch.cuda.synchronize()
        outs.append(g.checked().copy())
    assert np.array_equal(bits(outs[0]), bits(outs[1])), "two calls gave different bits"
    return outs[0]


def same(got, want):
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got)[~nan], bits(want)[~nan])


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", NS)
def test_bit_for_bit_in_rank_order_with_nan_padding_and_guards(pool, n):
    from multihop_dense_retrieval_amd.dist import rank_sum_host
    for N in RANKS:
        rows = pool[:N, :n]
        want = rank_sum_host(rows)
        assert not np.isnan(want).any()
        if N >= 3 and n >= 255:
            assert not np.array_equal(bits(rank_sum_host(rows[::-1].copy())), bits(want)), "the descending order gives the same bits: this input shows nothing"
        for stride in ((n + 3) // 4 * 4, (n + 3) // 4 * 4 + 1024):
            got = run(rows, stride)
            assert not np.isnan(got).any(), (N, stride, "the rows' padding leaked into a result")
            assert np.array_equal(bits(got), bits(want)), (N, stride, int((bits(got) != bits(want)).sum()))


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [5, 3073])
def test_designed_values(pool, n):
    from multihop_dense_retrieval_amd.dist import rank_sum_host
    stride = (n + 3) // 4 * 4
    for N in (2, 3, 16):
        zeros = np.full((N, n), -0.0, np.float32)
        got = run(zeros, stride)
        assert np.array_equal(bits(got), np.full(n, 0x80000000, np.uint32)), (N, "-0.0 in every rank must stay -0.0: the accumulator starts at rank 0, not at +0")
        rows = pool[:N, :n].copy()
        rows[0, 0::7], rows[N - 1, 0::7] = np.inf, -np.inf   # meet: NaN
        rows[N - 1, 1::7] = np.inf                            # alone: +inf
        rows[N // 2, 2::7] = np.nan                           # a NaN in one rank
        got, want = run(rows, stride), rank_sum_host(rows)
        assert np.isnan(want[0::7]).all() and np.isposinf(want[1::7]).all() and np.isnan(want[2::7]).all()
        assert same(got, want), N
    one = pool[:1, :n].copy()
    one[0, 0], one[0, n // 2], one[0, n - 1] = -0.0, np.inf, np.nan
    one.view(np.uint32)[0, 1] = 0x7FC12345  # a quiet NaN with a payload
    one.view(np.uint32)[0, 2] = 0xFF812345  # a signalling one, negative
    assert np.array_equal(bits(run(one, stride)), bits(one[0])), "one rank is a copy of the bits"
    assert np.array_equal(bits(run(one, stride + 1024)), bits(one[0]))


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------------------
def test_every_violated_constraint_is_refused_with_the_output_untouched(pool):
    from multihop_dense_retrieval_amd import _lib
    n, stride = 257, 260
    recv = dev(np.ascontiguousarray(pool[:16, :stride]))
    g = Guarded(n + 3, (), torch.float32, GUARD, GUARD, name="out", unit="elements")
    out = g.own
    assert call(recv, 16, n, stride, out) == OK  # the valid call of the same buffers, so that every refusal below is the one constraint's
    torch.cuda.synchronize()
    g = Guarded(n + 3, (), torch.float32, GUARD, GUARD, name="out", unit="elements")
    out = g.own
    flat = recv.view(-1)
    cases = {
        "n_ranks = 0": (recv, 0, n, stride, out),
        "n_ranks = 17": (recv, 17, n, stride, out),
        "n_ranks < 0": (recv, -1, n, stride, out),
        "n = 0": (recv, 2, 0, stride, out),
        "n < 0": (recv, 2, -4, stride, out),
        "stride < n": (recv, 2, n, 256, out),
        "stride % 4 != 0": (recv, 2, n, 258, out),
        "recv misaligned": (flat[1:], 2, n, stride, out),
        "out misaligned": (recv, 2, n, stride, out[1:]),
        "recv is NULL": (None, 2, n, stride, out),
        "out is NULL": (recv, 2, n, stride, None),
        "out is a row of recv": (recv, 4, n, stride, recv[2]),
        "out ends inside recv": (flat[1024:], 2, n, stride, flat[1024 - 256:]),
        "out starts inside the last row": (recv, 2, n, stride, flat[stride + 256:]),
    }
    before = recv.clone()
    for what, (r, N, n_, s, o) in cases.items():
        assert call(r, N, n_, s, o) == E_INVALID, what
        assert b"mdr_rank_sum" in _lib.lib().mdr_last_error(), what
    torch.cuda.synchronize()
    assert_untouched(g.buf.cpu().numpy(), "a refused call wrote the output")
    assert torch.equal(before.view(torch.int32), recv.view(torch.int32))
    # behind the rows: out directly behind the last column read is no overlap
    assert call(recv, 2, n, stride, flat[stride + 260:]) == OK
    torch.cuda.synchronize()
