"""GPU (-m gpu): the three attention kernels in isolation (mdr_test_attention, include/mdr_hip.h) against the fp64 softmax of
oracle/attention_oracle.py. EVERY output element of EVERY query row is compared; nothing is averaged.

The bar is the oracle's `bound`, derived from the formats and the kernels' documented rounding points (its docstring) and shown on the host
(tests/test_attention_oracle.py) to hold a second implementation of the dataflow and to throw out each index / mask / rescale defect. No
tolerance here was read off a device. The one-hot and v = 1 families assert EQUALITY with bit-known outputs.

Many lengths are packed into one call (ragged cu): kernel 1 at every len in 1..128 (L = 128) and, for its 24- and 32-tile instantiations,
129..384 (L = 384) and 385..512 (L = 512); kernel 2 at every len in 1..512 in batches of L = 129, 300 and 512 (the longer batches also hold
short sequences, whose later query blocks must leave at once); kernel 3 at every len in 1..512. heads = 1 for the full sweeps, 12 and 16 at
the lengths around every tile, pair-tile, job and query-block edge.
"""
import ctypes

import numpy as np
import pytest
import torch

from guarded import Guarded
from oracle import attention_oracle as ao
from oracle import fp
from oracle.fp import bits

pytestmark = pytest.mark.gpu

GUARD = 64        # rows of ctx in front of and behind the call's own, which must keep their bits
EDGES = [1, 2, 15, 16, 17, 31, 32, 33, 64, 95, 96, 97, 127, 128, 129, 160, 191, 192, 193, 255, 256, 257, 288, 289, 300, 383, 384, 385, 480, 511, 512]
SHORT = [1, 31, 100, 128]  # sequences that end before the second query block


def batches(kernel):
    """[(L, lens)]: together every length the kernel serves."""
    if kernel == 1:
        return [(128, list(range(1, 129))), (384, SHORT + list(range(129, 385))), (512, SHORT + [129, 384] + list(range(385, 513)))]
    if kernel == 2:
        return [(129, list(range(1, 130))), (300, SHORT + [129] + list(range(130, 301))), (512, SHORT + [129, 256, 257, 300] + list(range(301, 513)))]
    return [(512, list(range(1, 513)))]


def edge_batches(kernel):
    """[(heads, L, lens)]: the multi-head runs, at the lengths around every tile, pair-tile, job and query-block edge."""
    upto = lambda m: [n for n in EDGES if n <= m]  # noqa: E731
    if kernel == 1:
        return [(12, 128, upto(128)), (12, 384, upto(384)), (16, 512, EDGES)]
    if kernel == 2:
        return [(12, 300, upto(300)), (16, 512, EDGES)]
    return [(12, 512, EDGES), (16, 512, EDGES)]


def cases():
    out = []
    for kernel in (1, 2, 3):
        out += [pytest.param(kernel, 1, L, lens, id=f"k{kernel}-h1-L{L}") for L, lens in batches(kernel)]
        out += [pytest.param(kernel, heads, L, lens, id=f"k{kernel}-h{heads}-L{L}-edges") for heads, L, lens in edge_batches(kernel)]
    return out


def run(qkv, cu, heads, kernel, L, order=None):
    """One hook call. ctx starts as SENTINEL with GUARD rows on both sides of the call's own; returns the call's rows (numpy float16) after
    asserting that the guards kept their bits."""
    from multihop_dense_retrieval_amd import _lib
    lib = _lib.lib()
    assert max(int(b - a) for a, b in zip(cu[:-1], cu[1:])) <= L and min(int(b - a) for a, b in zip(cu[:-1], cu[1:])) >= 1  # the caller's promise
    B, hidden = len(cu) - 1, 64 * heads
    rows = B if kernel == 3 else int(cu[-1])
    q = torch.from_numpy(qkv).cuda()
    c = torch.from_numpy(np.asarray(cu, np.int32)).cuda()
    o = torch.from_numpy(np.asarray(order, np.int32)).cuda() if order is not None else None
    ctx = Guarded(rows, (hidden,), torch.float16, GUARD, GUARD)
    _lib.check(lib.mdr_test_attention(q.data_ptr(), c.data_ptr(), o.data_ptr() if o is not None else None, B, L, hidden, heads, kernel, ctx.own.data_ptr(),
                                      0, _lib.current_stream_ptr()))
    torch.cuda.synchronize()
    return ctx.checked()


def first_mismatch(got, exp, cu, kernel):
    bad = np.argwhere(bits(got) != bits(exp))
    if not len(bad):
        return None
    r, c = (int(x) for x in bad[0])
    b = r if kernel == 3 else int(np.searchsorted(cu, r, side="right") - 1)
    return dict(n_bad=len(bad), row=r, seq=b, len=int(cu[b + 1] - cu[b]), query=0 if kernel == 3 else r - int(cu[b]), col=c, got=float(got[r, c]), exp=float(exp[r, c]))


def check_bound(got, qkv, cu, heads, kernel, label):
    ref, bnd = ao.reference_and_bound(qkv, cu, heads, kernel)
    worst = fp.assert_within(got, ref, bnd, f"{label} kernel {kernel}", ao.locator(cu, kernel))
    print(f"RATIO kernel={kernel} {label} worst |err| / bound = {worst:.4f}")
    return worst


@pytest.mark.parametrize("kernel,heads,L,lens", cases())
def test_onehot_permutation_is_bit_exact(kernel, heads, L, lens):
    """q_i = code(pi(i)): the output must EQUAL v[pi(i)] -- the key-to-V-row map of every tile, pair-tile, lane slot, job and query block."""
    qkv, cu, expected = ao.onehot(lens, heads, 3)
    got = run(qkv, cu, heads, kernel, L)
    exp = ao.cls_rows(expected, cu) if kernel == 3 else expected
    assert first_mismatch(got, exp, cu, kernel) is None, first_mismatch(got, exp, cu, kernel)


@pytest.mark.parametrize("kernel,heads,L,lens", cases())
def test_uniform_scores(kernel, heads, L, lens):
    """q = 0. v = 1: the bit-known value (exactly 1 for the ring kernel and for power-of-two lengths; ao.uniform_ones_expected derives the rest).
    v = indicator of one key, for key 0, the last key and both ends of every pair-tile and job: 1 / len within the bound -- a key counted twice
    or dropped is off by a factor len / (len +- 1)."""
    qkv, cu = ao.uniform_ones(lens, heads, 0)
    got = run(qkv, cu, heads, kernel, L)
    exp = np.empty_like(got)
    for b, n in enumerate(lens):
        exp[b if kernel == 3 else slice(int(cu[b]), int(cu[b + 1]))] = ao.uniform_ones_expected(n, kernel)
    assert first_mismatch(got, exp, cu, kernel) is None, first_mismatch(got, exp, cu, kernel)
    qkv, cu = ao.uniform_indicators(lens, heads, 0)
    check_bound(run(qkv, cu, heads, kernel, L), qkv, cu, heads, kernel, f"family=uniform_indicators heads={heads} L={L}")


@pytest.mark.parametrize("family", ["stair_up", "stair_down", "spike8", "spike16", "realistic1", "realistic4"])
@pytest.mark.parametrize("kernel,heads,L,lens", cases())
def test_family_within_the_derived_bound(kernel, heads, L, lens, family):
    qkv, cu = ao.FAMILIES[family](lens, heads, 11)
    check_bound(run(qkv, cu, heads, kernel, L), qkv, cu, heads, kernel, f"family={family} heads={heads} L={L}")


@pytest.mark.parametrize("L,chosen", [(1, 1), (64, 1), (128, 1), (129, 2), (300, 2), (512, 2)])
def test_kernel_0_is_the_documented_choice(L, chosen):
    """kernel 0 = what mdr_encoder_forward / mdr_reader_forward launch for L: the one-shot kernel up to 128, the ring kernel above. Same bits."""
    lens = sorted({1, L, max(1, L // 2), max(1, L - 1)})
    qkv, cu = ao.realistic(lens, 12, 21, 1.0)
    a, b = run(qkv, cu, 12, 0, L), run(qkv, cu, 12, chosen, L)
    assert np.array_equal(bits(a), bits(b))
    other = run(qkv, cu, 12, 3 - chosen, L)
    check_bound(other, qkv, cu, 12, 3 - chosen, f"family=realistic1 heads=12 L={L} (the kernel not chosen)")


def test_ring_walk_order_does_not_change_the_bits():
    lens = [300, 1, 129, 512, 96, 97, 257, 128, 33, 400]
    qkv, cu = ao.realistic(lens, 12, 22, 1.0)
    base = run(qkv, cu, 12, 2, 512, None)
    check_bound(base, qkv, cu, 12, 2, "family=realistic1 heads=12 L=512 (order test)")
    assert np.array_equal(bits(base), bits(run(qkv, cu, 12, 2, 512, np.arange(len(lens)))))
    perm = np.random.default_rng(5).permutation(len(lens))
    assert np.array_equal(bits(base), bits(run(qkv, cu, 12, 2, 512, perm)))
    by_len = np.argsort(-np.asarray(lens), kind="stable")  # what enc_scan_kernel hands the product: longest first
    assert np.array_equal(bits(base), bits(run(qkv, cu, 12, 2, 512, by_len)))


@pytest.mark.parametrize("kernel,L", [(1, 128), (1, 512), (2, 512), (3, 512)])
def test_heads_and_sequences_do_not_see_each_other(kernel, L):
    """A (sequence, head) pair's output is a function of its own Q / K / V alone: one head of one sequence, cut out and run on its own (heads = 1,
    B = 1) returns the bits it had inside a batch whose other heads and sequences hold large finite sentinels; and rows of ctx outside the call
    keep theirs (run() checks the guards on every call of this file)."""
    heads = 12
    lens = [n for n in (1, 33, 97, 128, 129, 257, 300, 512) if n <= L]
    qkv, cu = ao.realistic(lens, heads, 23, 1.0)
    hidden = 64 * heads
    probes = [(b, h) for b in range(len(lens)) for h in (0, 5, 11)]
    loud = qkv.copy()
    noise = np.random.default_rng(9).choice(np.asarray([-48.0, -6.5, 6.5, 48.0], np.float16), size=qkv.shape)
    keepers = {(b, h) for b, h in probes}
    # every (sequence, head) pair that is not probed gets sentinels; a probed pair keeps its values
    pair_keep = np.zeros(qkv.shape, bool)
    for b in range(len(lens)):
        for h in range(heads):
            if (b, h) in keepers:
                for part in range(3):
                    pair_keep[int(cu[b]):int(cu[b + 1]), part * hidden + 64 * h:part * hidden + 64 * h + 64] = True
    loud[~pair_keep] = noise[~pair_keep]
    quiet, noisy = run(qkv, cu, heads, kernel, L), run(loud, cu, heads, kernel, L)
    assert np.isfinite(noisy.astype(np.float32)).all()
    for b, h in probes:
        rows = slice(b, b + 1) if kernel == 3 else slice(int(cu[b]), int(cu[b + 1]))
        cols = slice(64 * h, 64 * h + 64)
        assert np.array_equal(bits(quiet[rows, cols]), bits(noisy[rows, cols])), (b, h)
        seq = qkv[int(cu[b]):int(cu[b + 1])]
        one = np.ascontiguousarray(np.concatenate([seq[:, part * hidden + 64 * h:part * hidden + 64 * h + 64] for part in range(3)], axis=1))
        alone = run(one, np.asarray([0, lens[b]], np.int32), 1, kernel, L)
        assert np.array_equal(bits(alone), bits(quiet[rows, cols])), (b, h)


def test_bad_arguments_are_errors_not_undefined_behaviour():
    from multihop_dense_retrieval_amd import _lib
    lib = _lib.lib()
    qkv = torch.zeros((8, 3 * 128), dtype=torch.float16, device="cuda")
    cu = torch.tensor([0, 3, 8], dtype=torch.int32, device="cuda")
    ctx = torch.zeros((8, 128), dtype=torch.float16, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def call(q=p(qkv), c=p(cu), o=None, B=2, L=8, hidden=128, heads=2, kernel=0, out=p(ctx)):
        return lib.mdr_test_attention(q, c, o, B, L, hidden, heads, kernel, out, 0, None)

    for k in (0, 1, 2, 3):
        assert call(kernel=k) == 0  # order may be NULL
    torch.cuda.synchronize()
    for kw, word in ((dict(q=None), "NULL"), (dict(c=None), "NULL"), (dict(out=None), "NULL"), (dict(B=0), "B"), (dict(B=-1), "B"), (dict(L=0), "L"),
                     (dict(L=513), "L"), (dict(L=513, kernel=1), "L"), (dict(hidden=96), "head dim"), (dict(heads=3), "head dim"),
                     (dict(hidden=0, heads=0), "head dim"), (dict(kernel=4), "kernel"), (dict(kernel=-1), "kernel")):
        assert call(**kw) == -1, kw
        assert word in lib.mdr_last_error().decode(), (kw, lib.mdr_last_error())
    with pytest.raises(_lib.MdrError):
        _lib.check(call(B=0))
