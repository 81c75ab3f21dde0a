"""GPU parity tests (-m gpu) of the int8 screening tier (k = 1, F32X2H storage, d = 768; csrc/mdr_mips.hip, mips_screen8*_kernel):
whatever the tier does -- decide alone, hand over to the fp16 screen, hand over twice -- ids and scores are those of the exact
stream kernel, and the telemetry hook says which way it went. Reference: faiss.IndexFlatIP.search as called at
/root/reference/scripts/eval/eval_mhop_retrieval.py:155,179 (exact inner products, ties to the lowest id)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
D_ = 768


@pytest.fixture(scope="module")
def mdr():
    from multihop_dense_retrieval_amd import _lib, index
    _lib.lib()
    return index


def exact(idx, q):
    idx.set_variant(2)
    try:
        return idx.search(q, 1)
    finally:
        idx.set_variant(0)


def check(idx, q, *, expect_i8_decides=None):
    De, Ie = exact(idx, q)
    for v in (0, 4):  # int8 tier in front / fp16 screen alone
        idx.set_variant(v)
        D, I = idx.search(q, 1)
        t = idx.telemetry(q.shape[0], 1)
        idx.set_variant(0)
        assert torch.equal(I, Ie), v
        assert torch.equal(D, De) or float((D - De).abs().max()) <= 2e-6 * float(De.abs().max()) + 1e-30, v
        assert t["i8_tier"] == (v == 0)
        if v == 0 and expect_i8_decides is not None:
            assert (not t["i8_overflow"]) == expect_i8_decides, t
    return t


@pytest.mark.parametrize("n", [1, 31, 32, 33, 95, 4097])
@pytest.mark.parametrize("nq", [1, 100, 130])
def test_small_and_ragged_indexes(mdr, n, nq):
    g = torch.Generator(device="cuda").manual_seed(n * 1000 + nq)
    idx = mdr.IndexFlatIP(D_)
    idx.add(torch.randn((n, D_), generator=g, device="cuda"))
    check(idx, torch.randn((nq, D_), generator=g, device="cuda"))


def test_no_clear_winner_queries_are_decided_by_the_tier(mdr):
    """iid queries against iid rows: hundreds of rows per query sit inside the int8 band; most candidates are emitted early against a
    loose bound and dropped before re-scoring."""
    g = torch.Generator(device="cuda").manual_seed(3)
    idx = mdr.IndexFlatIP(D_)
    idx.reserve(600_000)
    for _ in range(3):  # several add() calls: the plane and its bound constants accumulate
        idx.add(torch.randn((200_000, D_), generator=g, device="cuda"))
    for nq in (100, 200, 300, 800):  # 16 queries per wave / 32 per wave / two and four groups of 256 (a shard's load at N = 8, weak scaling)
        q = torch.randn((nq, D_), generator=g, device="cuda")
        idx.set_variant(0)
        idx.search(q, 1)
        t = idx.telemetry(nq, 1)
        assert t["i8_tier"] and not t["i8_overflow"] and t["fallback"] == 0
        groups = -(-nq // 256)  # `candidates` counts what the LAST group of 256 emitted, `i8_refined` what all groups re-scored
        assert 0 < t["i8_refined"] <= t["candidates"] * 2 * groups + 1
        assert ("mips_screen8w_kernel" if nq > 128 else "mips_screen8_kernel") in idx.last_kernel()
        check(idx, q, expect_i8_decides=True)


def test_growth_keeps_the_int8_plane(mdr):
    g = torch.Generator(device="cuda").manual_seed(5)
    idx = mdr.IndexFlatIP(D_)  # no reserve: the planes are re-allocated and copied as the index grows
    rows = []
    for n in (1000, 37, 5000, 64):
        x = torch.randn((n, D_), generator=g, device="cuda")
        idx.add(x)
        rows.append(x)
        q = torch.cat(rows)[-40:] + 0.02 * torch.randn((40, D_), generator=g, device="cuda")
        check(idx, q, expect_i8_decides=True)


def test_rows_and_queries_of_very_different_scales(mdr):
    """Per-row scales: rows spanning 9 orders of magnitude (F32X2H storage takes |x| <= 32768), an all-zero row, an all-zero query, a query with one huge element."""
    g = torch.Generator(device="cuda").manual_seed(7)
    x = torch.randn((20_000, D_), generator=g, device="cuda")
    x *= torch.logspace(-6, 3, 20_000, device="cuda")[torch.randperm(20_000, generator=g, device="cuda")][:, None]
    x[123] = 0
    idx = mdr.IndexFlatIP(D_)
    idx.add(x)
    q = torch.randn((64, D_), generator=g, device="cuda")
    q[5] = 0
    q[6, 17] = 3e4
    q[7] *= 1e-20
    q[8] *= 1e20
    check(idx, q)


def test_loose_bound_hands_over_to_the_fp16_screen(mdr):
    """Heavy-tailed rows (one element carries the row: its scale wipes out the rest) and rows with a large common mean make the int8
    bound wide: thousands of survivors per query -> the tier declares itself overflowed and the fp16 screen decides."""
    g = torch.Generator(device="cuda").manual_seed(9)
    n = 100_000
    x = torch.randn((n, D_), generator=g, device="cuda")
    x[torch.arange(n, device="cuda"), torch.randint(0, D_, (n,), generator=g, device="cuda")] = 400.0
    idx = mdr.IndexFlatIP(D_)
    idx.add(x)
    q = torch.randn((100, D_), generator=g, device="cuda")
    t = check(idx, q)
    idx.set_variant(0)
    idx.search(q, 1)
    t = idx.telemetry(100, 1)
    assert t["i8_tier"] and t["i8_overflow"], t
    assert t["fallback"] == 0, t  # ... and the fp16 screen behind it needs no exact pass


def test_env_switch_leaves_the_plane_out(mdr, monkeypatch):
    """MDR_MIPS_I8=0 is read once per process, so this only checks the variant-4 spelling of the same thing."""
    g = torch.Generator(device="cuda").manual_seed(11)
    idx = mdr.IndexFlatIP(D_)
    idx.add(torch.randn((5000, D_), generator=g, device="cuda"))
    q = torch.randn((10, D_), generator=g, device="cuda")
    idx.set_variant(4)
    idx.search(q, 1)
    assert "mips_screen_kernel" in idx.last_kernel() and not idx.telemetry(10, 1)["i8_tier"]
    idx.set_variant(0)
    idx.search(q, 1)
    assert "mips_screen8_kernel" in idx.last_kernel()


def test_compact_storage_is_the_same_index_without_the_plane(mdr):
    """MDR_STORE_F32X2H_COMPACT: FAISS's 4 bytes per element, no int8 screening copy; the ids of the default storage, scores from the same exact re-scoring."""
    g = torch.Generator(device="cuda").manual_seed(12)
    x = torch.randn((40000, D_), generator=g, device="cuda")
    q = torch.randn((100, D_), generator=g, device="cuda")
    a, b = mdr.IndexFlatIP(D_), mdr.IndexFlatIP(D_, storage="compact")
    a.add(x)
    b.add(x)
    for k in (1, 4):
        Da, Ia = a.search(q, k)
        Db, Ib = b.search(q, k)
        assert torch.equal(torch.as_tensor(Ia), torch.as_tensor(Ib))
        Da, Db = torch.as_tensor(Da), torch.as_tensor(Db)
        assert torch.equal(Da, Db) or float((Da - Db).abs().max()) <= 2e-6 * float(Da.abs().max())
    b.search(q, 1)
    assert "mips_screen_kernel" in b.last_kernel() and not b.telemetry(100, 1)["i8_tier"]
    a.search(q, 1)
    assert a.telemetry(100, 1)["i8_tier"]
    free0 = torch.cuda.mem_get_info()[0]
    c = mdr.IndexFlatIP(D_, storage="compact")
    c.reserve(1_000_000)
    used_compact = free0 - torch.cuda.mem_get_info()[0]
    d = mdr.IndexFlatIP(D_)
    d.reserve(1_000_000)
    used_default = free0 - used_compact - torch.cuda.mem_get_info()[0]
    assert used_compact <= 1_000_000 * D_ * 4 * 1.02 and used_default >= 1_000_000 * D_ * 5 * 0.98


@pytest.mark.parametrize("seed", range(12))
def test_randomised_differential_against_the_exact_kernel(mdr, seed):
    """Random sizes, query counts and data families (gaussian, uniform, sparse, low-rank + noise, clustered with exact duplicates and
    near-duplicates, mixed scales): the k = 1 answer of the tiered search is the exact kernel's, whichever tier decides."""
    rng = np.random.RandomState(1000 + seed)
    g = torch.Generator(device="cuda").manual_seed(2000 + seed)
    n = int(rng.choice([257, 4096, 33_333, 120_001, 300_000]))
    nq = int(rng.choice([1, 17, 100, 128, 129, 200, 256, 257, 300]))
    fam = ["gauss", "uniform", "sparse", "lowrank", "clusters", "scales"][seed % 6]
    x = torch.randn((n, D_), generator=g, device="cuda")
    if fam == "uniform":
        x = torch.rand((n, D_), generator=g, device="cuda") - 0.3
    elif fam == "sparse":
        x = x * (torch.rand((n, D_), generator=g, device="cuda") < 0.05)
    elif fam == "lowrank":
        x = torch.randn((n, 8), generator=g, device="cuda") @ torch.randn((8, D_), generator=g, device="cuda") + 0.05 * x
    elif fam == "clusters":
        c = torch.randn((50, D_), generator=g, device="cuda")
        x = c[torch.randint(0, 50, (n,), generator=g, device="cuda")] + 0.01 * x
        x[n // 2] = x[3]                      # an exact duplicate: lowest id wins
        x[n // 3] = x[3] * (1 - 1e-5)         # and a near-duplicate
    elif fam == "scales":
        x = x * torch.exp(4 * torch.randn((n, 1), generator=g, device="cuda"))
        x = x.clamp(-3e4, 3e4)
    idx = mdr.IndexFlatIP(D_)
    idx.add(x.contiguous())
    q = torch.randn((nq, D_), generator=g, device="cuda")
    if fam in ("clusters", "lowrank"):
        q[: min(nq, 8)] = x[torch.randint(0, n, (min(nq, 8),), generator=g, device="cuda")] + 0.001 * q[: min(nq, 8)]
        q[0] = x[3]
    check(idx, q.contiguous())


def test_more_than_128_queries_with_the_wide_kernels_switched_off():
    """with MDR_MIPS_WIDE=0 (measurement knob: every call stays on the 128-queries-per-pass kernels) a k = 1 call with more
    than 128 queries used to reach run_screen8, which serves ONE group of 128: queries 128.. came back as -1. The int8 tier is now
    only planned for nq <= 128 or with the wide kernels; otherwise the fp16 screen, which loops over groups, decides. The variable is
    read once per process, hence the subprocess."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = """
import torch
from multihop_dense_retrieval_amd import index as mi
g = torch.Generator(device='cuda').manual_seed(5)
xb = torch.randn((60000, 768), generator=g, device='cuda')
q = torch.randn((300, 768), generator=g, device='cuda')
q[:150] = xb[torch.arange(150, device='cuda') * 397] + 0.05 * q[:150]
idx = mi.IndexFlatIP(768)
idx.add(xb)
D, I = idx.search_device(q, 1)
kern = idx.last_kernel()
idx.set_variant(2)
De, Ie = idx.search_device(q, 1)
assert torch.equal(I, Ie) and bool((I >= 0).all()), int((I != Ie).sum())
assert float((D - De).abs().max()) <= 1e-3
assert torch.equal(I[:150, 0], torch.arange(150, device='cuda') * 397)
print('ok', kern)
"""
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, MDR_MIPS_WIDE="0"), capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0 and "ok mips_screen_kernel<24,1>" in r.stdout, (r.stdout[-1500:], r.stderr[-1500:])


@pytest.mark.parametrize("nq", [100, 200])
def test_query_split_on_rows_with_a_large_common_component(mdr, nq):
    """Round 6: rows AND queries that share a large common vector (what LayerNorm outputs of one trained encoder look like: |c| = 3 x the spread around it). The
    index decides for the query split with its centre (telemetry bit `i8_query_split`), the int8 tier alone decides every query, and the answer is the exact
    kernel's -- for queries of the corpus' kind, for queries WITHOUT the common component (lambda ~ 0: the split must not hurt them) and for queries pointing
    AWAY from it (negative lambda). An i.i.d. corpus keeps the split off."""
    g = torch.Generator(device="cuda").manual_seed(77)
    n = 200_000
    c = 1.0 * torch.randn((D_,), generator=g, device="cuda")           # |c| ~ 27.7
    x = c + 0.33 * torch.randn((n, D_), generator=g, device="cuda")     # spread ~ 9.1
    idx = mdr.IndexFlatIP(D_)
    idx.add(x)
    noise = torch.randn((nq, D_), generator=g, device="cuda")
    kinds = {"same kind": c + 0.33 * noise, "planted": x[torch.arange(nq, device="cuda") * 997] + 0.02 * noise, "no common part": 0.33 * noise,
             "opposite": -c + 0.33 * noise}
    for name, q in kinds.items():
        t = check(idx, q.contiguous(), expect_i8_decides=True)
        idx.search(q.contiguous(), 1)
        t = idx.telemetry(nq, 1)
        assert t["i8_query_split"] and t["i8_tier"] and not t["i8_overflow"] and t["fallback"] == 0, (name, t)
        print(f"query split, nq {nq}, {name}: candidates emitted {t['candidates']}, re-scored {t['i8_refined']}")
    iid = mdr.IndexFlatIP(D_)
    iid.add(torch.randn((50_000, D_), generator=g, device="cuda"))
    iid.search(noise.contiguous(), 1)
    assert not iid.telemetry(nq, 1)["i8_query_split"]


def test_query_split_on_the_hip_encoders_own_outputs(mdr):
    """Rows = this repo's RobertaCtxEncoder outputs for 150 k synthetic passages (random-init roberta-base geometry: a shared LayerNorm bias, nearly collapsed rows --
    the corpus of bench.py's `structured.encoder_geometry`, scripts/structured_corpora.py), queries from the same encoder. The index switches the query split on,
    the int8 tier alone decides, and every id / score is the exact kernel's (round 5's code handed such a corpus over to the slower tiers at 5 M rows)."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
    import structured_corpora as sc
    from multihop_dense_retrieval_amd.retriever import RobertaCtxEncoder
    dev = torch.device("cuda")
    model = RobertaCtxEncoder.random_init(device=dev, seed=3)
    idx = mdr.IndexFlatIP(D_)
    n = 150_000
    idx.reserve(n)
    first = None
    for _, x in sc.encoder_rows(model, n, 8, 24, dev):
        first = x[:50_000].clone() if first is None else first
        idx.add(x)
    assert idx.ntotal == n
    c = first.mean(0)
    assert float(c.norm()) > 2.0 * float((first - c).norm(dim=1).mean())  # the geometry the split is for: the common component dominates
    for nq in (100, 200):
        q = sc.encoder_queries(model, nq, 8, 24, dev)
        t = check(idx, q, expect_i8_decides=True)
        idx.search(q, 1)
        t = idx.telemetry(nq, 1)
        assert t["i8_query_split"] and t["i8_tier"] and not t["i8_overflow"] and t["fallback"] == 0, t
        print(f"encoder-geometry rows, nq {nq}: candidates emitted {t['candidates']}, re-scored {t['i8_refined']}")


# ---- rows at the far end of fp32 (add() takes any finite fp32) ----------------------------------------------------------------------
# The first add() sets the int8 plane's centre c from rows c + 0.33 n (a common component: the query split turns on); a second add() brings rows
# s (c + 0.33 n'). From s ~ 4e35 on, a large row's term b_r = c.(x_r - c) ~ s |c|^2 and sum_i |c_i (x_ri - c_i)| overflow fp32 while every score
# stays finite; its split bound would be lambda_q * inf (NaN for lambda_q = 0, -inf for lambda_q < 0) and the row could never become a candidate.
# From s ~ 1e36 on, the non-split bound constant overflows as well (+inf bounds: the lists overflow, the fp16 tier decides).
# Storage note (include/mdr_hip.h, dynamic range of F32X2H): the first add's rows lie ~2^110 below the largest element and are stored as zeros.
# The queries are therefore built so that the true top-(k + 1) are large rows with positive scores, where the stored values are fp32-accurate:
# (a) rows' kind, (b) pointing away from c (q.c < 0, lambda_q < 0) and (c) orthogonal to c (lambda_q ~ 0).
EXTREME_SCALES = [1e34, 3e35, 5e35, 1e36, 3e36]


def extreme_corpus(n1, n2, s, nq=96, seed=41):
    g = torch.Generator(device="cuda").manual_seed(seed)
    c = torch.randn((D_,), generator=g, device="cuda")
    first = c + 0.33 * torch.randn((n1, D_), generator=g, device="cuda")
    base = c + 0.33 * torch.randn((n2, D_), generator=g, device="cuda")
    noise = torch.randn((nq, D_), generator=g, device="cuda")
    q = torch.empty((nq, D_), device="cuda")
    kind = torch.arange(nq, device="cuda") % 3
    ortho = noise - (noise @ c)[:, None] * c / (c @ c)
    ortho = ortho / ortho.norm(dim=1, keepdim=True)
    q[kind == 0] = c + 0.33 * noise[kind == 0]
    q[kind == 1] = ortho[kind == 1] - 0.2 * c / (c @ c)  # q.c = -0.2: lambda_q < 0, and the best large rows still score > 0
    q[kind == 2] = ortho[kind == 2]
    q = q / q.norm(dim=1, keepdim=True)
    return first, (base * s).contiguous(), q.contiguous(), kind.cpu().numpy()


def extreme_case(idx_factory, n1, n2, s, ks=(1, 8)):
    """Variants 0 (int8 tier in front), 4 (fp16 screen) and 2 (exact stream) against the fp64 inner products of the fp32 rows. Returns the telemetry of variant 0, k = 1."""
    from test_oracle_mips import check_against_truth
    first, big, q, kind = extreme_corpus(n1, n2, s)
    idx = idx_factory()
    idx.add(first)
    idx.add(big)
    kmax = max(ks)
    S = q.double() @ torch.cat([first, big]).double().T
    assert float(S.abs().max()) < 1e38  # legal input: every score is a finite fp32
    St, It = torch.sort(S, dim=1, descending=True, stable=True)
    Dt, It = St[:, : kmax + 1].cpu().numpy(), It[:, : kmax + 1].cpu().numpy()
    assert (It >= n1).all() and (Dt > 0).all(), "the truth must lie among the large rows (the first add's rows are stored as zeros)"
    tele = None
    for v in (0, 4, 2):
        idx.set_variant(v)
        for k in ks:
            D, I = idx.search(q, k)
            if v == 0 and k == 1:
                tele = idx.telemetry(q.shape[0], 1)
                assert tele["i8_tier"], tele
            D, I = D.cpu().numpy().astype(np.float64), I.cpu().numpy()
            for kd in range(3):
                m = kind == kd
                tol = 2e-6 * float(np.abs(Dt[m]).max())
                try:
                    check_against_truth(D[m], I[m], Dt[m, :k], It[m, :k], Dt[m, k - 1] - Dt[m, k], tol=tol)
                except AssertionError as e:
                    bad = np.nonzero(I[m, 0] != It[m, 0])[0]
                    raise AssertionError(f"s {s:g} variant {v} k {k} query kind {kd}: {len(bad)} wrong top-1 ids of {int(m.sum())} "
                                         f"(e.g. got {I[m][bad[:3], 0]} want {It[m][bad[:3], 0]})") from e
    idx.set_variant(0)
    return tele


@pytest.mark.parametrize("s", EXTREME_SCALES)
@pytest.mark.parametrize("n1,n2", [(1024, 3072), (8192, 192_000)])
def test_rows_near_the_top_of_fp32_after_a_centred_first_add(mdr, n1, n2, s):
    """A finite row whose split row term overflows must still be found: the index switches the query split off for good (telemetry
    `i8_query_split`) once such a row is stored, and every tier returns the fp64 answer. Below the overflow the split stays on."""
    tele = extreme_case(lambda: mdr.IndexFlatIP(D_), n1, n2, s)
    overflow = s >= 5e35
    assert tele["i8_query_split"] == (not overflow), tele


def test_row_term_overflow_state_rolls_back_with_a_rejected_add(mdr):
    """A rejected add() restores every statistic of the int8 tier, the row-term overflow state included: host rows go up in chunks of
    32 k rows, the first chunks are converted (and raise the state) before the NaN in the last one rejects the call. The split stays on
    for the rows that were really added."""
    first, big, q, _ = extreme_corpus(8192, 192_000, 5e35)
    idx = mdr.IndexFlatIP(D_)
    idx.add(first)
    bad = big.cpu().numpy()
    bad[-1, 5] = np.nan
    with pytest.raises(Exception):
        idx.add(bad)
    assert idx.ntotal == 8192
    idx.search(q, 1)
    assert idx.telemetry(q.shape[0], 1)["i8_query_split"]
    idx.add(big)
    idx.search(q, 1)
    assert not idx.telemetry(q.shape[0], 1)["i8_query_split"]


def test_forced_query_split_does_not_bring_the_row_term_overflow_back():
    """MDR_MIPS_I8_CB=1 (read once per process, hence the child) forces the split on -- except where a row term overflowed."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = """
import sys
sys.path.insert(0, 'tests')
import test_mips_i8_gpu as t
from multihop_dense_retrieval_amd import index as mi
for n1, n2 in ((1024, 3072), (8192, 192_000)):
    tele = t.extreme_case(lambda: mi.IndexFlatIP(768), n1, n2, 5e35)
    assert not tele['i8_query_split'], tele
tele = t.extreme_case(lambda: mi.IndexFlatIP(768), 1024, 3072, 1e34)
assert tele['i8_query_split'], tele
print('ok')
"""
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, MDR_MIPS_I8_CB="1"), capture_output=True, text=True, timeout=900, cwd=root)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
