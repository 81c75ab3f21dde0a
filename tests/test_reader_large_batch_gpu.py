"""GPU (-m gpu): the answer reader at the batch sizes it ships at (profiles/reader_bench.md: B = 32-128, L = 384-512, ELECTRA-large).

tests/test_reader_gpu.py stops at 3 x 512 tokens, where launch_gemm (csrc/mdr_encoder.hip) still picks the one-tile-per-block GEMMs. Here every case is
large enough for the persistent 256x256 kernels (gemm_big_kernel, gemm_quad_kernel, their 128x128 tail tiles) and is checked three ways:

a. against HF ElectraModel in fp64 on the device plus the fp64 heads (test_reader_gpu._reference, 8 rows at a time), under the bars of that file;
b. against the same rows run 4 at a time through the small-tile path those tests pin: every GEMM flavour accumulates K in the same order with the same
   MFMA, attention and LayerNorm work per sequence / per token, so the fp16 logits, rank and sp scores must be BIT-IDENTICAL;
c. `layer_gemm_plan` below asks the library which kernel launch_gemm picks for each GEMM of a layer (gemm_ref.flavour -> mdr_test_gemm_choice, the function
   the launcher switches on), and each case asserts that the kernels it means to test were chosen: it is what keeps this file from silently testing small tiles.

Plus: workspace reuse after a large call, decode(with_logits=False) (the CLI's call: logits live in the workspace), B > 1024 (chunked scan, no length
sort) and a non-default stream. Run time on one MI355X: see profiles/reader_bench.md."""
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
transformers = pytest.importorskip("transformers")

import gemm_ref  # noqa: E402
import test_reader_gpu as rg  # noqa: E402  (the helpers of the small-batch reader tests; tests/ is on sys.path through conftest.py)

DEV = "cuda"
N_SENT = 10

# ---- (c) launch_gemm's choice, as the library reports it ------------------------------------------------------------------------------------------------
def layer_gemm_plan(B, L, H, F, residual_fp32, num_cus):
    """The four GEMMs of one reader layer as mdr_reader_forward calls launch_gemm: M_cap = B * L, M_est = B * L - B * L / 3; the out-projection and FFN2
    write fp16 in residual mode 2 (epilogue 0) and fp32 in modes 1 (epilogue 3) and 0 (epilogue 2, which the persistent kernels run as 3); the choice
    reads an epilogue's output width only, so FFN1's GELU stands as epilogue 0.
    -> gemm_ref.flavour's names; "small" and "mid" are gemm_f16_kernel, one 64x64 / 128x128 tile per block."""
    T = B * L
    est = T - T // 3
    wide = {2: 0, 1: 3, 0: 2}[residual_fp32]
    return {"qkv": gemm_ref.flavour(0, T, est, 3 * H, H, 0, num_cus), "out": gemm_ref.flavour(0, T, est, H, H, wide, num_cus),
            "ffn1": gemm_ref.flavour(0, T, est, F, H, 0, num_cus), "ffn2": gemm_ref.flavour(0, T, est, H, F, wide, num_cus)}


PERSISTENT = ("quad", "big", "persist")

# ---- geometries, models and references, built once per module -----------------------------------------------------------------------------------------
GEOMETRIES = {  # name: (hidden, layers, ffn, seed)
    "large": (1024, 24, 4096, 8),  # ELECTRA-large, 16 heads
    "base": (768, 12, 3072, 12),   # ELECTRA-base / BERT-base geometry, 12 heads
    "two": (1024, 2, 4096, 13),    # ELECTRA-large's GEMM shapes on 2 layers
}
# The 12-layer bar: twice the worst error of the 4-rows-at-a-time path against fp64 on the base case below, measured on an MI355X over both residual modes
# (mode 2: logits 4.0e-3 / 4.6e-3, rank 4.6e-3, sp 9.9e-3; mode 0: 4.2e-3 / 3.6e-3, 3.4e-3, 9.0e-3 -- profiles/reader_bench.md, "Parity error"): 2 x 9.9e-3.
# That is about the headroom TOL_TINY and TOL_LARGE have over their measured 7.7e-3 and 4.6e-2.
TOL_BASE = 0.0198
TOL = {"large": rg.TOL_LARGE, "base": TOL_BASE, "two": rg.TOL_TINY}
_cache = {}


def _geometry(name):
    if ("geom", name) not in _cache:
        hidden, layers, ffn, seed = GEOMETRIES[name]
        cfg = rg._electra(hidden, layers, ffn, vocab=2000)
        sd = rg._random_state_dict(cfg, "electra", True, seed=seed)
        _cache[("geom", name)] = (cfg, sd, rg._reference_fn(cfg, "electra", sd, True))
    return _cache[("geom", name)]


def _hip_model(name, residual_fp32):
    if ("hip", name, residual_fp32) not in _cache:
        cfg, sd, _ = _geometry(name)
        _cache[("hip", name, residual_fp32)] = _fresh_model(cfg, sd, residual_fp32)
    return _cache[("hip", name, residual_fp32)]


def _fresh_model(cfg, sd, residual_fp32=2):
    import types
    m = rg.reader.QAModel(cfg, types.SimpleNamespace(model_name="google/electra-test-discriminator", sp_pred=True))
    m.residual_fp32 = residual_fp32
    m.load_state_dict(sd)
    return m.to(DEV).eval()


def _ragged_lens(B, L, seed, lo=40, hi=300):
    """A few full rows (0, 7 and B - 2), one row of a single token (5), the others lo .. hi."""
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(lo, min(hi, L) + 1, (B,), generator=g).tolist()
    lens[0] = lens[7] = lens[B - 2] = L
    lens[5] = 1
    return lens


def _lens_with_total(B, L, total, seed):
    """Ragged lengths whose sum, the packed row count the GEMMs read from the device, is exactly `total`."""
    lens = _ragged_lens(B, L, seed, lo=40, hi=180)
    free = [i for i, n in enumerate(lens) if 1 < n < L]
    d, i = total - sum(lens), 0
    while d:
        j, step = free[i % len(free)], 1 if d > 0 else -1
        if 2 <= lens[j] + step <= L - 1:
            lens[j] += step
            d -= step
        i += 1
    assert sum(lens) == total
    return lens


# case: (geometry, B, L, row lengths, residual modes). The edge totals: 7680 = 256 * 30, 7681 = 256 * 30 + 1, 7679 = 128 * 59 + 127, all below
# M_est / 2 = 10923, where the launcher plans for 86 row tiles of 256 and the device finds 30 or 31 (QKV: 12 column tiles, 360 / 372 tiles = one complete
# round of 256 workgroups on 21 row tiles + a 128x128 tail over the other 9 / 10, whose last tile has 128, 1 or 127 rows).
CASES = {
    "large-full": ("large", 64, 512, [512] * 64, (2,)),
    "large-ragged": ("large", 64, 512, _ragged_lens(64, 512, 31), (2, 1, 0)),
    "large-48x384": ("large", 48, 384, _ragged_lens(48, 384, 32), (2,)),
    "base-ragged": ("base", 96, 512, _ragged_lens(96, 512, 33), (2, 0)),
    "edge-256k": ("two", 64, 512, _lens_with_total(64, 512, 7680, 34), (2,)),
    "edge-256k+1": ("two", 64, 512, _lens_with_total(64, 512, 7681, 35), (2,)),
    "edge-128k+127": ("two", 64, 512, _lens_with_total(64, 512, 7679, 36), (2,)),
}


def _case(name):
    """(cfg, batch, fp64 reference computed 8 rows at a time), cached: the residual modes of a case share them."""
    if ("case", name) not in _cache:
        geom, B, L, lens, _ = CASES[name]
        cfg, sd, ref_fn = _geometry(geom)
        batch = rg._batch(cfg, lens, L, N_SENT, seed=len(name) + B)
        _cache[("case", name)] = (cfg, batch, rg._reference(cfg, "electra", sd, batch, True, rows=8, fn=ref_fn))
    return _cache[("case", name)]


def _four_at_a_time(m, batch):
    """The small-tile path tests/test_reader_gpu.py pins: 4 rows per call, concatenated."""
    B = batch["input_ids"].shape[0]
    parts = [m(rg._rows(batch, i, i + 4)) for i in range(0, B, 4)]
    return {k: torch.cat([p[k] for p in parts]) for k in ("start_logits", "end_logits", "rank_score", "sp_score")}


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.float16 else t


def _assert_same_bits(got, want, keys, label):
    for k in keys:
        a, b = got[k], want[k]
        assert a.dtype == b.dtype and a.shape == b.shape, (label, k)
        if not torch.equal(_bits(a), _bits(b)):
            diff = _bits(a) != _bits(b)
            rows = torch.nonzero(diff.reshape(diff.shape[0], -1).any(1)).flatten().tolist()
            worst = (a.double() - b.double())[diff].abs().max().item()
            raise AssertionError(f"{label}: {k} differs in {int(diff.sum())} of {diff.numel()} elements, rows {rows[:12]} ({len(rows)} rows), max |diff| {worst:.3e}")


LOGIT_KEYS = ("start_logits", "end_logits", "rank_score", "sp_score")
DECODE_KEYS = ("start", "end", "span_score", "rank_score", "sp_prob")


@pytest.mark.parametrize("case,residual_fp32", [(c, r) for c, v in CASES.items() for r in v[4]])
def test_forward_at_production_shapes(case, residual_fp32):
    geom, B, L, lens, _ = CASES[case]
    cfg, batch, ref = _case(case)
    label = f"{case} {B}x{L} r{residual_fp32} tokens={sum(lens)}"
    # (c) the kernels this case is here for
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    plan = layer_gemm_plan(B, L, cfg.hidden_size, cfg.intermediate_size, residual_fp32, ncu)
    print(f"[reader {label}] {ncu} CUs, GEMMs of a layer: {plan}")
    assert any(v in PERSISTENT for v in plan.values()), (label, plan)
    if geom in ("large", "two") and (B, L) == (64, 512):
        assert plan["qkv"] in PERSISTENT and plan["out"] in PERSISTENT and plan["ffn2"] in PERSISTENT and plan["ffn1"] in ("small", "mid"), (label, plan)
    if case.startswith("edge"):
        assert sum(lens) < (B * L - B * L // 3) / 2
    m = _hip_model(geom, residual_fp32)
    # (b), first half: the same rows through the small-tile path, and that path's own error (the figure TOL_BASE comes from)
    small = _four_at_a_time(m, batch)
    print(f"[reader {label}] 4 rows at a time, max |err| / mean |logit|: " + ", ".join(f"{k} {v:.2e}" for k, v in rg._errors(small, ref).items()))
    # (a) against fp64 (and _check's exact conditions: the -inf pattern, decode == forward, the sp sigmoid, the span search)
    rg._check(m, ref, batch, TOL[geom], label)
    # (b) bit-identical
    _assert_same_bits(m(batch), small, LOGIT_KEYS, label + ": whole batch vs 4 rows at a time")


def test_workspace_is_reused_after_a_large_call():
    """QAModel keeps one workspace and only grows it: a small batch after a 64 x 512 one runs in the large call's memory (stale packed rows, `order`,
    `total`) and must return the bits of a fresh model."""
    cfg, big_batch, _ = _case("edge-256k+1")
    _, sd, _ = _geometry("two")
    small_batch = rg._batch(cfg, [90, 33, 61], 90, N_SENT, seed=41)
    used = _hip_model("two", 2)
    used(big_batch)
    assert used._ws is not None and used._ws.numel() >= int(rg.reader.lib().mdr_reader_workspace_bytes(used._h, 64, 512, N_SENT))
    got = used.decode(small_batch, 30, with_logits=True)
    want = _fresh_model(cfg, sd).decode(small_batch, 30, with_logits=True)
    _assert_same_bits(got, want, LOGIT_KEYS + DECODE_KEYS, "after a 64 x 512 call vs a fresh model")


def test_decode_without_logits_returns_the_same_answers():
    """decode(with_logits=False) is what the CLI runs: the logits then live in the workspace (rw.start16 / rw.end16) instead of caller tensors."""
    cfg, batch, _ = _case("large-ragged")
    m = _hip_model("large", 2)
    for label, b in (("64 x 512 ragged", batch), ("B = 1, full row", rg._rows(batch, 0, 1)), ("B = 1, short row", rg._batch(cfg, [77], 77, N_SENT, seed=42))):
        with_l, without = m.decode(b, 30, with_logits=True), m.decode(b, 30)
        assert "start_logits" not in without
        _assert_same_bits(without, with_l, DECODE_KEYS, label)


def test_more_than_1024_rows():
    """B > 1024: enc_scan_kernel scans in chunks of 1024 and skips the length sort (order == nullptr)."""
    cfg = rg._electra(128, 1, 512)
    sd = rg._random_state_dict(cfg, "electra", True, seed=14)
    B, L = 1100, 32
    g = torch.Generator().manual_seed(15)
    lens = torch.randint(1, L + 1, (B,), generator=g).tolist()
    lens[0] = lens[1023] = lens[1024] = lens[B - 1] = L
    batch = rg._batch(cfg, lens, L, 4, seed=16)
    m = _fresh_model(cfg, sd)
    rg._check(m, rg._reference(cfg, "electra", sd, batch, True), batch, rg.TOL_TINY, f"B={B} L={L}")
    out = m(batch)
    for lo in (0, B - 4):
        alone = m(rg._rows(batch, lo, lo + 4))
        _assert_same_bits({k: out[k][lo:lo + 4] for k in LOGIT_KEYS}, alone, LOGIT_KEYS, f"rows {lo}..{lo + 3} of {B} vs alone")


def test_non_default_stream_returns_the_same_bits():
    _, batch, _ = _case("large-ragged")
    batch = {k: v.to(DEV) for k, v in batch.items()}
    m = _hip_model("large", 2)
    want = m.decode(batch, 30, with_logits=True)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got = m.decode(batch, 30, with_logits=True)
    s.synchronize()
    _assert_same_bits(got, want, LOGIT_KEYS + DECODE_KEYS, "stream of its own vs the default stream")
