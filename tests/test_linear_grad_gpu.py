"""GPU (-m gpu): the Linear backward in isolation (mdr_linear_backward, include/mdr_linear_grad.h) against the fp64 statement of
tests/linear_grad_ref.py, and packed_linear (multihop_dense_retrieval_amd/linear.py) on top of it. EVERY element of dX, dW and db is
compared; nothing is averaged.

Two bars. On the grid (x, w, dy multiples of 1/8 of magnitude at most 2: every product is a multiple of 1/64 of magnitude at most 4, and
any fp32 sum of M <= 65536 of them is exact in any order because 4 * 64 * M <= 2^24) dW and db must EQUAL the integer result bit for bit and
dX its correctly rounded fp16: every index map, the zero-fill, the chunk seams and the reduction without a tolerance. On realistic rows the
bar is linear_grad_ref's bound, derived from the formats and the rounding points listed in csrc/mdr_linear_grad.inl and shown on the host
(tests/test_linear_grad_host.py) to hold a second implementation of the dataflow and to throw out each defect. No tolerance here was read
off a device.

Every output starts as a finite sentinel: dx with 64 guard rows on both sides, dw and db with 64 guard elements on both sides, which must
keep their bits in every call of this file. Shapes: a whole 64 x 64 quarter tile, a 64-wide remainder on either side of a 128 x 128 tile,
one whole tile, several tiles with a remainder, each at M = 1 .. 300 around the MFMA k-step, the slab and one and two chunks of 64 rows;
the four Linears of roberta-base at M = 300; and linear_grad_ref.LARGE_MNK, the smallest training row counts at which a chunk of the
weight-gradient kernel holds three slabs or more (its register double buffer in the steady state, S >= 3 partials, a ragged last chunk) and
at which dX of FFN2 leaves the one-tile GEMMs for a persistent kernel with its device-side row count.

The answer reader's geometry (ELECTRA-large: width 1024, FFN 4096), each shape the smallest that reaches its path:
READER_NK        the reader's four Linears at M = 300 beside roberta-base's: 8 dW tile columns (K = 1024) or 32 (K = 4096) where the
                 retriever has 6 or 24, and dX as a forward GEMM of (N, K) = (1024, 3072), (1024, 1024), (1024, 4096), (4096, 1024).
POOLER_MNK       (1024, 1024) at M = 1, 3 and 64 rows without a device-side row count: the pooler runs on the B CLS rows of a batch, and
                 below M = 300 the model widths were never run (one row, a count that is no multiple of 4, one whole slab).
LARGE_MNK        gains the fused QKV (2051, 3072, 1024): S = 3, and the out-projection (2051, 1024, 1024): S = 7, at the list's own smallest M.
TWO_CHUNK_MNK    FFN1 and FFN2 at 2051 rows. Their 256 dW tiles make the split S = 2 at every M, which assert_large (S >= 3) rules out and
                 the small shapes only have with ONE slab per chunk; here a chunk is 17 slabs and the last ends on a slab of 3 rows.
PERSIST_DX_MNK   QKV and FFN1 at 12300 rows: from 12033 rows on (256 compute units) their dX leaves the one-tile GEMMs for a persistent one
                 with N = 1024 and K = 3072 / 4096, and a chunk of FFN1's dW is a chain of 97 slabs. On the exact grid alone (every sum stays
                 exact: exact_grid asserts it), with a device-side row count one row into the last row tile. FFN2's dX (GEMM N = 4096, wider
                 than kPersistBiasMax) stays on the one-tile kernels at every M, which is asserted instead of run.
"""
import numpy as np
import pytest
import torch

import linear_grad_ref as ref
from guarded import E_INVALID, E_WORKSPACE, SENTINEL, Guarded, dev
from multihop_dense_retrieval_amd._lib import ptr
from oracle import fp

pytestmark = pytest.mark.gpu

GUARD = 64        # rows of dx / elements of dw and db in front of and behind the call's own, which must keep their bits
# (M, N, K): M None is the shape's sweep of small row counts (ms_for); LARGE_MNK gives its own M
ALL_NK = [pytest.param(None, N, K, id=f"N{N}-K{K}") for N, K in ref.SMALL_NK + ref.MODEL_NK + ref.READER_NK] + \
         [pytest.param(M, N, K, id=f"M{M}-N{N}-K{K}") for M, N, K in ref.LARGE_MNK + ref.TWO_CHUNK_MNK]
POOLER = [pytest.param(M, N, K, id=f"M{M}-N{N}-K{K}") for M, N, K in ref.POOLER_MNK]
PERSIST_DX = [pytest.param(M, N, K, id=f"M{M}-N{N}-K{K}") for M, N, K in ref.PERSIST_DX_MNK]
FFN2_LARGE = (4099, 768, 3072)  # the shape of LARGE_MNK whose dX takes a persistent GEMM
READER_FFN2 = (1024, 4096)      # (N, K) of the reader Linear whose dX stays on the one-tile GEMMs at every M


def ms_for(N, K, M=None):
    if M is not None:
        return [M]
    return ref.M_SWEEP if (N, K) in ref.SMALL_NK else [300]


def raw_call(x, w, dy, pre, M, m_dev, N, K, dx, dw, db, accumulate, ws, ws_bytes):
    from multihop_dense_retrieval_amd import _lib, linear
    return linear.lib().mdr_linear_backward(ptr(x), ptr(w), ptr(dy), ptr(pre), M, ptr(m_dev), N, K, ptr(dx), ptr(dw), ptr(db), accumulate, ptr(ws), ws_bytes,
                                            0, _lib.current_stream_ptr())


def run(x, w, dy, pre=None, m=None, outs="xwb", old_dw=None, old_db=None, accumulate=False, ws_extra=0):
    """One call on numpy inputs. Outputs start as SENTINEL (dw / db: the old values if given) inside guards; returns {"dx": float16 [M, K] (rows
    at or behind m still SENTINEL), "dw": float32 [N, K], "db": float32 [N]} for the outputs asked for, after asserting MDR_OK and that the
    guards kept their bits."""
    from multihop_dense_retrieval_amd import _lib, linear
    M, K = x.shape
    N = w.shape[0]
    bx = Guarded(M, (K,), torch.float16, GUARD, GUARD, name="dx")
    bw = Guarded(N * K, (), torch.float32, GUARD, GUARD, None if old_dw is None else old_dw.astype(np.float32), "dw", "elements")
    bb = Guarded(N, (), torch.float32, GUARD, GUARD, None if old_db is None else old_db.astype(np.float32), "db", "elements")
    want = (1 if "x" in outs else 0) | (2 if "w" in outs else 0) | (4 if "b" in outs else 0) | (8 if pre is not None else 0)
    need = int(linear.lib().mdr_linear_backward_workspace_bytes(M, N, K, want))
    ws = torch.empty(max(need + ws_extra, 16), dtype=torch.uint8, device="cuda")
    m_dev = None if m is None else torch.tensor([m], dtype=torch.int32, device="cuda")
    _lib.check(raw_call(dev(x), dev(w), dev(dy), dev(pre), M, m_dev, N, K, bx.own if "x" in outs else None, bw.own if "w" in outs else None,
                        bb.own if "b" in outs else None, 1 if accumulate else 0, ws, need + ws_extra))
    torch.cuda.synchronize()
    return {"dx": bx.checked(valid=M if m is None else m, asked="x" in outs), "dw": bw.checked(asked="w" in outs).reshape(N, K),
            "db": bb.checked(asked="b" in outs)}


def forward_hook(x, w, b, epilogue, m=None):
    """mdr_test_gemm_f16 with kernel = 0 on numpy inputs -> float16 [M, N] (rows at or behind m: zero)."""
    from multihop_dense_retrieval_amd import _lib
    M, K = x.shape
    N = w.shape[0]
    out = torch.zeros((M, N), dtype=torch.float16, device="cuda")
    m_dev = None if m is None else torch.tensor([m], dtype=torch.int32, device="cuda")
    tx, tw, tb = dev(x), dev(w), dev(b)  # (held until the synchronise below)
    _lib.check(_lib.lib().mdr_test_gemm_f16(ptr(tx), ptr(tw), ptr(tb), M, ptr(m_dev), N, K, ptr(out), epilogue, 0, 0, _lib.current_stream_ptr()))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def exact_grid(x, w, dz, m=None, old_dw=None, old_db=None):
    """The integer result of a grid call: (dx float16 correctly rounded [m, K], dw float32, db float32), asserting that everything is exact in
    fp32 and that no dX leaves the fp16 range. dz may be dy / 2 (multiples of 1/16 times a power of two)."""
    m = x.shape[0] if m is None else m
    X, W, DZ = x[:m].astype(np.float64), w.astype(np.float64), dz[:m].astype(np.float64)
    for a in (X, W, DZ):
        assert (a * 1024 == np.round(a * 1024)).all()
    dx, dw, db = DZ @ W, DZ.T @ X, DZ.sum(axis=0)
    odw, odb = (np.zeros(1) if o is None else o.astype(np.float64) for o in (old_dw, old_db))
    if old_dw is not None:
        dw = dw + odw
    if old_db is not None:
        db = db + odb
    # exact in fp32 in any order: every partial sum is a whole number of quanta (the largest power of two all terms are multiples of) and
    # stays at or below 2^24 of them
    for total, quantum in ((np.abs(DZ) @ np.abs(W), _quantum(DZ) * _quantum(W)),
                           (np.abs(DZ).T @ np.abs(X) + np.abs(odw), min(_quantum(DZ) * _quantum(X), _quantum(odw))),
                           (np.abs(DZ).sum(axis=0) + np.abs(odb), min(_quantum(DZ), _quantum(odb)))):
        assert total.size == 0 or total.max() / quantum <= 2.0 ** 24, "the grid no longer guarantees exact fp32 sums"
    assert dx.size == 0 or np.abs(dx).max() < fp.F16_MAX, "an exact dX leaves the fp16 range: shrink w"
    assert (dw.astype(np.float32) == dw).all() and (db.astype(np.float32) == db).all()
    return dx.astype(np.float16), dw.astype(np.float32), db.astype(np.float32)


def _quantum(a):
    """the largest power of two every element of `a` is a multiple of (1.0 for an all-zero or empty array)"""
    nz = np.abs(a[a != 0])
    if nz.size == 0:
        return 1.0
    e = 0
    while not (nz * 2.0 ** -e == np.round(nz * 2.0 ** -e)).all():
        e -= 1
    while e < 64 and (nz * 2.0 ** -(e + 1) == np.round(nz * 2.0 ** -(e + 1))).all():  # (upwards too: dy under a loss scale is a multiple of 32)
        e += 1
    return 2.0 ** e


def assert_equal(got, want, m, label):
    dx, dw, db = want
    for name, g, wnt in (("dx", got["dx"][:m], dx), ("dw", got["dw"], dw), ("db", got["db"], db)):
        bad = np.argwhere(~(g == wnt))
        if bad.size:
            i = tuple(bad[0])
            pytest.fail(f"{label}: {name} differs at {len(bad)} of {g.size} elements; first at {i}: got {float(g[i])!r}, exact {float(wnt[i])!r}")
        assert g.dtype == wnt.dtype


def grid_inputs(M, N, K, seed, loss_scale=False):
    x, w, dy = (fp.grid(shape, seed + i, dtype=np.float16) for i, shape in enumerate(((M, K), (N, K), (M, N))))
    if loss_scale:  # dy x 2^8 as under a loss scale; w shrunk by 2^-4 so that no exact dX leaves the fp16 range (asserted in exact_grid)
        w, dy = (w.astype(np.float32) / 16).astype(np.float16), (dy.astype(np.float32) * 256).astype(np.float16)
    return x, w, dy


def test_some_tested_shape_is_split():
    from multihop_dense_retrieval_amd import linear
    split = [(M, N, K) + linear.backward_chunks(M, N, K) for N, K in ref.SMALL_NK + ref.MODEL_NK + ref.READER_NK for M in ms_for(N, K)]
    assert any(S > 1 for *_, S, _ in split)
    # M_SWEEP's 63 .. 65 and 127 .. 129 are -1, 0, +1 around one and two chunks wherever the shape is split
    for M, N, K, S, rpc in split:
        assert (S, rpc) == ref.chunks(M, N, K)
        if S > 1 and (N, K) in ref.SMALL_NK:
            assert rpc == 64, (M, N, K, S, rpc)


def test_large_shapes_reach_the_steady_state_and_the_persistent_gemm():
    """LARGE_MNK against the LIBRARY's split: three slabs or more per chunk, S >= 3, a ragged last chunk (linear_grad_ref.assert_large). dX of
    the FFN2 shape leaves the one-tile kernels on this device: launch_gemm (csrc/mdr_encoder.hip) is called with the GEMM's N = the Linear's
    K, its K = the Linear's N and M_est = M, and gemm_ref.flavour reports the choice it makes (persistent from (N / 128) * ceil(M_est / 256) >=
    3/2 of the compute units on); at M = 300 the same Linear stays on a one-tile kernel."""
    import gemm_ref
    from multihop_dense_retrieval_amd import linear
    props = ref.assert_large(chunks_of=linear.backward_chunks)
    assert props == ref.assert_large()
    assert FFN2_LARGE in ref.LARGE_MNK
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    M, N, K = FFN2_LARGE
    assert gemm_ref.flavour(0, M, M, K, N, 0, ncu) in ("persist", "big", "quad"), (ncu, gemm_ref.flavour(0, M, M, K, N, 0, ncu))
    assert gemm_ref.flavour(0, 300, 300, K, N, 0, ncu) in ("small", "mid")


def test_reader_shapes_have_two_long_chunks_and_reach_the_persistent_gemm():
    """TWO_CHUNK_MNK against the LIBRARY's split: S = 2 with 17 slabs a chunk and a ragged last one (linear_grad_ref.assert_two_chunks). dX of
    the PERSIST_DX_MNK shapes (GEMM N = the Linear's K = 1024, GEMM K = 3072 and 4096) leaves the one-tile kernels on this device, and stays
    on them at the largest M below the threshold that M = 300 and 2051 stand for; FFN1's chunk there is 97 slabs. dX of the reader's FFN2 has
    GEMM N = 4096 > kPersistBiasMax: a one-tile kernel at every M, so no large M is run for it."""
    import gemm_ref
    from multihop_dense_retrieval_amd import linear
    props = ref.assert_two_chunks(chunks_of=linear.backward_chunks)
    assert props == ref.assert_two_chunks()
    assert [(rpc, last) for *_, rpc, last in props] == [(17 * ref.SLAB, 15 * ref.SLAB + 3)] * 2
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    for M, N, K in ref.PERSIST_DX_MNK:
        assert gemm_ref.flavour(0, M, M, K, N, 0, ncu) in ("persist", "big", "quad"), (M, N, K, ncu, gemm_ref.flavour(0, M, M, K, N, 0, ncu))
        for small_m in (300, 2051):
            assert gemm_ref.flavour(0, small_m, small_m, K, N, 0, ncu) in ("small", "mid"), (small_m, N, K)
    assert linear.backward_chunks(12300, 4096, 1024) == (2, 97 * ref.SLAB)
    N, K = READER_FFN2
    assert READER_FFN2 in ref.READER_NK and (2051, N, K) in ref.TWO_CHUNK_MNK
    for M in (300, 2051, 12300, 32768, 65536):
        assert gemm_ref.flavour(0, M, M, K, N, 0, ncu) in ("small", "mid"), (M, gemm_ref.flavour(0, M, M, K, N, 0, ncu))


@pytest.mark.parametrize("loss_scale", [False, True], ids=["unit", "x256"])
@pytest.mark.parametrize("M,N,K", ALL_NK + POOLER + PERSIST_DX)
def test_exact_grid_equality(M, N, K, loss_scale):
    for M in ms_for(N, K, M):
        x, w, dy = grid_inputs(M, N, K, 3, loss_scale)
        assert_equal(run(x, w, dy), exact_grid(x, w, dy), M, f"M={M} N={N} K={K}")


@pytest.mark.parametrize("M,N,K", ALL_NK)
def test_accumulate_on_the_grid(M, N, K):
    for M in ms_for(N, K, M):
        x, w, dy = grid_inputs(M, N, K, 5)
        old_dw, old_db = fp.grid((N, K), 8, 4.0), fp.grid((N,), 9, 4.0)
        got = run(x, w, dy, old_dw=old_dw, old_db=old_db, accumulate=True)
        assert_equal(got, exact_grid(x, w, dy, None, old_dw, old_db), M, f"accumulate M={M} N={N} K={K}")
        got = run(x, w, dy, old_dw=old_dw, old_db=old_db, accumulate=False)
        assert_equal(got, exact_grid(x, w, dy), M, f"overwrite M={M} N={N} K={K}")


def check_bound(got, rb, m, label):
    for name in ("dx", "dw", "db"):
        g = got[name][:m] if name == "dx" else got[name]
        r, bnd = rb[name]
        worst = fp.assert_within(g, r, bnd, f"{label}: {name}")
        print(f"RATIO {label} {name} worst |err| / bound = {worst:.4f}")


@pytest.mark.parametrize("scale", [1.0, 256.0], ids=["unit", "x256"])
@pytest.mark.parametrize("M,N,K", ALL_NK + POOLER)
def test_realistic_rows_within_the_derived_bound(M, N, K, scale):
    """Identity and GELU path (u from the forward hook with epilogue 0), and the GELU path with one invalid row of NaN behind m = M - 1 (the
    pooler's shapes too, beside their calls without a device-side row count)."""
    for M in ms_for(N, K, M):
        x, w, dy = ref.realistic(M, N, K, 11, scale)
        check_bound(run(x, w, dy), ref.reference_and_bound(x, w, dy), M, f"identity M={M} N={N} K={K} scale={scale}")
        u = forward_hook(x, w, ref.bias(N, 11), 0)
        check_bound(run(x, w, dy, u), ref.reference_and_bound(x, w, dy, u), M, f"gelu M={M} N={N} K={K} scale={scale}")
    if 1 < M <= 300:  # (the large shapes have their rows behind m in test_rows_behind_m_dev_do_not_exist)
        xb, dyb, ub = x.copy(), dy.copy(), u.copy()
        xb[M - 1], dyb[M - 1], ub[M - 1] = np.nan, np.inf, np.nan
        got = run(xb, w, dyb, ub, m=M - 1)
        check_bound(got, ref.reference_and_bound(x, w, dy, u, M - 1), M - 1, f"gelu m=M-1 M={M} N={N} K={K} scale={scale}")


def test_subnormal_operand_columns_within_the_derived_bound():
    """FFN2's dW on the last layer's CLS rows, as tests/test_encoder_chain_gpu.py met it on its four-layer geometry: M = 4 rows, and columns of
    x (GELU outputs far in the negative tail) that are fp16 subnormals in EVERY row, so that a dW element is a sum of subnormal x normal
    products alone; the row with the largest dy holds the smallest x (1 or 2 x 2^-22), the others 33 .. 63 x 2^-22 under a dy 2^-8 times
    smaller. The fp16 MFMA aligns the products to the largest exponent FIELD, which for a subnormal is 2^-14 whatever its value, keeps 24 bits
    below it and cuts the other rows' products there: the sum comes out with up to ten bits fewer (line 1 of linear_grad_ref's derivation, the
    term F). The last RATIO line prints the share of the bound WITHOUT F (the host's model of the alignment, linear_grad_ref.aligned_dw, gives
    3.7 for these inputs and 0.07 with F: tests/test_linear_grad_host.py). With M in the hundreds such columns vanish next to their
    neighbours' terms, which is why no shape of M_SWEEP and no geometry with a single full layer showed it."""
    x, w, dy = ref.subnormal_columns_case()
    M, K = x.shape
    N = w.shape[0]
    rb = ref.reference_and_bound(x, w, dy)
    got = run(x, w, dy)
    check_bound(got, rb, M, f"subnormal columns M={M} N={N} K={K}")
    r, bnd = rb["dw"]
    without_f = bnd - ref.field_floor_term(np.abs(dy.astype(np.float64)).T, np.abs(x.astype(np.float64)))
    print(f"RATIO subnormal columns dw against the bound WITHOUT the exponent-field term: {fp.worst_ratio(got['dw'], r, without_f)[0]:.4f}")


@pytest.mark.parametrize("M,N,K", ALL_NK)
def test_gelu_at_zero_is_exactly_one_half(M, N, K):
    """u = 0 everywhere: gelu'(0) = 1/2 exactly (the polynomial gives 2^-1 at 0), dZ = dY / 2, and all three outputs are bit-exact on the grid."""
    for M in ms_for(N, K, M):
        x, w, dy = grid_inputs(M, N, K, 13)
        dz = (dy.astype(np.float32) / 2).astype(np.float16)
        assert_equal(run(x, w, dy, np.zeros((M, N), np.float16)), exact_grid(x, w, dz), M, f"gelu0 M={M} N={N} K={K}")


def large_ms(M, N, K):
    """valid-row counts for a split shape: none, one row into the second slab of chunk 1, one row short of the seam behind chunk 1, a count
    that cuts the last chunk but one and leaves the whole last chunk behind it, all"""
    S, rpc = ref.chunks(M, N, K)
    ms = (0, rpc + ref.SLAB + 1, 2 * rpc - 1, (S - 2) * rpc + ref.SLAB + 6, M)
    assert S >= 3 and rpc >= 2 * ref.SLAB and list(ms) == sorted(set(ms)) and ms[3] <= (S - 1) * rpc < M
    return ms


def two_chunk_ms(M, N, K):
    """valid-row counts for a shape of two long chunks (large_ms needs S >= 3): none, one row into the second slab of chunk 0, one row short of
    the seam, the seam itself (chunk 1 all zero-fill), a count that cuts chunk 1 in its second slab, all"""
    S, rpc = ref.chunks(M, N, K)
    ms = (0, ref.SLAB + 1, rpc - 1, rpc, rpc + ref.SLAB + 6, M)
    assert S == 2 and rpc >= 3 * ref.SLAB and list(ms) == sorted(set(ms))
    return ms


def valid_rows(M, N, K):
    if M == 200:
        return (0, 1, M - 1, M)
    if (M, N, K) in ref.TWO_CHUNK_MNK:
        return two_chunk_ms(M, N, K)
    if (M, N, K) in ref.PERSIST_DX_MNK:  # one count: one row into the last row tile of dX's persistent GEMM (256 rows, and 128 in its tail)
        m = (M - 1) // 256 * 256 + 1
        assert M - 128 < m - 1 and m < M
        return (m,)
    return large_ms(M, N, K)


# the small shapes at M = 200 on both paths; (2051, 768, 768) and FFN2 at 4099 rows (dX through a persistent GEMM whose device-side row count
# lies well below the cap) once each, one on either path; the reader's FFN1 (the GELU path in the model) and FFN2 with their two long chunks;
# the reader's QKV and FFN1 at 12300 rows, dX through a persistent GEMM whose row count ends one row into the last row tile
ROWS_BEHIND = [pytest.param(200, N, K, g, id=f"{'gelu0' if g else 'identity'}-N{N}-K{K}") for g in (False, True) for N, K in ((128, 128), (256, 384), (768, 768))] + \
              [pytest.param(2051, 768, 768, False, id="identity-M2051-N768-K768"), pytest.param(*FFN2_LARGE, True, id="gelu0-M4099-N768-K3072"),
               pytest.param(2051, 4096, 1024, True, id="gelu0-M2051-N4096-K1024"), pytest.param(2051, 1024, 4096, False, id="identity-M2051-N1024-K4096"),
               pytest.param(12300, 3072, 1024, False, id="identity-M12300-N3072-K1024"), pytest.param(12300, 4096, 1024, True, id="gelu0-M12300-N4096-K1024")]


@pytest.mark.parametrize("M,N,K,gelu0", ROWS_BEHIND)
def test_rows_behind_m_dev_do_not_exist(M, N, K, gelu0):
    """m in {0, 1, M - 1, M} (the large shapes: valid_rows), rows at or behind m of x, dy and pre NaN and Inf: outputs finite and equal, bit for
    bit, to the call on the first m rows alone (on the grid every sum is exact, so the different split of the shorter call does not matter);
    dx rows at or behind m keep the sentinel (run() asserts it); m = 0 gives zeros, or the old value with accumulate."""
    x, w, dy = grid_inputs(M, N, K, 17)
    pre = np.zeros((M, N), np.float16) if gelu0 else None
    old_dw, old_db = fp.grid((N, K), 18), fp.grid((N,), 19)
    for m in valid_rows(M, N, K):
        xb, dyb = x.copy(), dy.copy()
        xb[m:], dyb[m:] = np.nan, np.inf
        xb[m + 1::2], dyb[m + 1::2] = -np.inf, np.nan
        pb = None
        if gelu0:
            pb = pre.copy()
            pb[m:] = np.nan
            pb[m + 1::2] = np.inf
        got = run(xb, w, dyb, pb, m=m)
        assert all(np.isfinite(got[k]).all() for k in ("dw", "db")) and np.isfinite(got["dx"][:m]).all()
        if m == 0:
            assert not got["dw"].any() and not got["db"].any()
            acc = run(xb, w, dyb, pb, m=0, old_dw=old_dw, old_db=old_db, accumulate=True)
            assert np.array_equal(acc["dw"], old_dw) and np.array_equal(acc["db"], old_db)
        else:
            alone = run(x[:m], w, dy[:m], None if pre is None else pre[:m])
            for k in ("dw", "db"):
                assert np.array_equal(got[k], alone[k]), (m, k)
            assert np.array_equal(got["dx"][:m], alone["dx"]), (m, "dx")
            dz = (dy.astype(np.float32) / 2).astype(np.float16) if gelu0 else dy
            assert_equal(got, exact_grid(x, w, dz, m), m, f"m={m} M={M} N={N} K={K}")


def test_nan_in_a_valid_row_reaches_only_what_it_touches():
    M, N, K = 150, 192, 128
    x, w, dy = grid_inputs(M, N, K, 23)
    clean = run(x, w, dy)
    xb = x.copy()
    xb[70, 5] = np.nan  # dW[:, 5] only
    got = run(xb, w, dy)
    assert np.isnan(got["dw"][:, 5]).all()
    keep = np.ones(K, bool)
    keep[5] = False
    assert np.array_equal(got["dw"][:, keep], clean["dw"][:, keep]) and np.array_equal(got["db"], clean["db"]) and np.array_equal(got["dx"], clean["dx"])
    dyb = dy.copy()
    dyb[70, 9] = np.nan  # dX[70, :], dW[9, :], db[9]
    got = run(x, w, dyb)
    assert np.isnan(got["dx"][70]).all() and np.isnan(got["dw"][9]).all() and np.isnan(got["db"][9])
    rows, cols = np.arange(M) != 70, np.arange(N) != 9
    assert np.array_equal(got["dx"][rows], clean["dx"][rows]) and np.array_equal(got["dw"][cols], clean["dw"][cols])
    assert np.array_equal(got["db"][cols], clean["db"][cols])


@pytest.mark.parametrize("M,N,K", [pytest.param(300, 256, 384, id="N256-K384"), pytest.param(300, 768, 768, id="N768-K768"),
                                   pytest.param(*FFN2_LARGE, id="M4099-N768-K3072")])
def test_two_runs_and_a_larger_workspace_give_the_same_bits(M, N, K):
    x, w, dy = ref.realistic(M, N, K, 29)
    u = forward_hook(x, w, ref.bias(N, 29), 0)
    for pre in (None, u):
        a, b, c = run(x, w, dy, pre), run(x, w, dy, pre), run(x, w, dy, pre, ws_extra=4096 + 16)
        for k in ("dx", "dw", "db"):
            assert np.array_equal(a[k].view(np.uint16 if k == "dx" else np.uint32), b[k].view(np.uint16 if k == "dx" else np.uint32)), k
            assert np.array_equal(a[k].view(np.uint16 if k == "dx" else np.uint32), c[k].view(np.uint16 if k == "dx" else np.uint32)), k


def test_single_outputs_match_the_full_call():
    """each output alone (the other pointers NULL) gives the bits of the call that computes all three"""
    M, N, K = 129, 192, 64
    x, w, dy = ref.realistic(M, N, K, 31)
    full = run(x, w, dy)
    for outs, k in (("x", "dx"), ("w", "dw"), ("b", "db")):
        assert np.array_equal(run(x, w, dy, outs=outs)[k], full[k]), k


def test_host_validation_writes_nothing():
    from multihop_dense_retrieval_amd import _lib, linear
    lib = linear.lib()
    M, N, K = 70, 128, 64
    x, w, dy = (dev(a) for a in grid_inputs(M, N, K, 37))
    pre = torch.zeros((M, N), dtype=torch.float16, device="cuda")
    dx = torch.full((M, K), SENTINEL, dtype=torch.float16, device="cuda")
    dw = torch.full((N, K), SENTINEL, dtype=torch.float32, device="cuda")
    db = torch.full((N,), SENTINEL, dtype=torch.float32, device="cuda")
    need = int(lib.mdr_linear_backward_workspace_bytes(M, N, K, 15))
    ws = torch.full((need,), 0x5A, dtype=torch.uint8, device="cuda")
    cases = [
        ("NULL x", E_INVALID, dict(x=None)), ("NULL w", E_INVALID, dict(w=None)), ("NULL dy", E_INVALID, dict(dy=None)),
        ("no outputs", E_INVALID, dict(dx=None, dw=None, db=None)), ("M = 0", E_INVALID, dict(M=0)), ("M < 0", E_INVALID, dict(M=-3)),
        ("N = 0", E_INVALID, dict(N=0)), ("N = 96", E_INVALID, dict(N=96)), ("K = 0", E_INVALID, dict(K=0)), ("K = 100", E_INVALID, dict(K=100)),
        ("N < 0", E_INVALID, dict(N=-64)), ("short workspace", E_WORKSPACE, dict(ws_bytes=need - 1)), ("NULL workspace", E_WORKSPACE, dict(ws=None)),
    ]
    for label, code, change in cases:
        a = dict(x=x, w=w, dy=dy, pre=pre, M=M, m_dev=None, N=N, K=K, dx=dx, dw=dw, db=db, accumulate=0, ws=ws, ws_bytes=need)
        a.update(change)
        rc = raw_call(**a)
        assert rc == code, (label, rc)
        assert lib.mdr_last_error(), label
    torch.cuda.synchronize()
    assert (dx == SENTINEL).all() and (dw == SENTINEL).all() and (db == SENTINEL).all() and (ws == 0x5A).all(), "a rejected call wrote something"
    with pytest.raises(ValueError, match=r"\(70, 128\)|\[70, 128\]"):
        linear.linear_backward(x, w, dy[:, :64].contiguous())
    with pytest.raises(ValueError):
        linear.packed_linear(x, w.float()[:, :32].contiguous(), torch.zeros(N, device="cuda"))
    with pytest.raises(ValueError):
        linear.packed_linear(x, w, torch.zeros(N, device="cuda"))  # the weight must be the fp32 master


@pytest.mark.parametrize("rows", [False, True], ids=["all-rows", "rows"])
@pytest.mark.parametrize("gelu", [False, True], ids=["identity", "gelu"])
def test_packed_linear(gelu, rows):
    from multihop_dense_retrieval_amd import linear
    M, N, K = 150, 256, 384
    m = M - 3 if rows else None
    x, w16, g = ref.realistic(M, N, K, 41)
    b = ref.bias(N, 41)
    w32 = w16.astype(np.float32) * np.float32(1 + 2.0 ** -13)  # an fp32 master that is NOT fp16-exact and rounds to w16 (under a quarter of an fp16 ulp away)
    assert np.array_equal(w32.astype(np.float16), w16)
    tx = dev(x).requires_grad_(True)
    tw, tb = dev(w32).requires_grad_(True), dev(b).requires_grad_(True)
    tr = None if m is None else torch.tensor([m], dtype=torch.int32, device="cuda")
    y = linear.packed_linear(tx, tw, tb, gelu=gelu, rows=tr)
    assert y.dtype == torch.float16 and tuple(y.shape) == (M, N)
    assert np.array_equal(y.detach().cpu().numpy().view(np.uint16), forward_hook(x, w16, b, 1 if gelu else 0, m).view(np.uint16)), "forward bits differ from the encoder's GEMM"
    (y.float() * dev(g).float()).sum().backward()
    torch.cuda.synchronize()
    assert tx.grad.dtype == torch.float16 and tw.grad.dtype == torch.float32 and tb.grad.dtype == torch.float32
    assert tuple(tx.grad.shape) == (M, K) and tuple(tw.grad.shape) == (N, K) and tuple(tb.grad.shape) == (N,)
    mm = M if m is None else m
    u = forward_hook(x, w16, b, 0, m) if gelu else None
    got = {"dx": tx.grad.cpu().numpy(), "dw": tw.grad.cpu().numpy(), "db": tb.grad.cpu().numpy()}
    assert not got["dx"][mm:].any()
    check_bound(got, ref.reference_and_bound(x, w16, g, u, m), mm, f"packed_linear gelu={gelu} rows={rows}")
