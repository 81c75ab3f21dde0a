"""GPU (-m gpu): the MIPS search under every schedule knob of include/mdr_hip.h (MDR_MIPS_EVEN_GROUPS 0-3 x MDR_MIPS_I8_CB unset / 0 / 1,
MDR_MIPS_WIDE=0, MDR_MIPS_I8=0) against fp64 inner products, and across the knobs against each other.

The header promises that none of the knobs changes a result; the library reads each of them once per process, so every setting runs in a
fresh child process (this file run as a script) that builds the corpora, searches the whole grid and writes D / I / last_kernel() /
telemetry() to an .npz. The parent computes the truth once on the device in fp64 and does all the comparing:
  * every result against the fp64 top-(k + 1) (test_oracle_mips.check_against_truth; bf16 storage: against the bf16-rounded rows);
  * across MDR_MIPS_EVEN_GROUPS at a fixed MDR_MIPS_I8_CB: D and I bit-identical;
  * across MDR_MIPS_I8_CB: ids identical, scores within the bar of test_mips_i8_gpu.check();
  * each setting really ran the path it names (telemetry bits, kernel names).
Children run one after the other; one that dies by a signal or hits its time limit fails every later case without starting another."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D_ = 768
N_ROWS = 120_000
NQS = [1, 31, 32, 100, 128, 129, 256, 257, 288, 300, 513, 800]  # 257 / 288: mode 2's narrow second group; 800: the old cut's 32-query rest
KS = [1, 2, 8, 32, 33, 100, 250]
NQ_MAX = max(NQS)
SMALL_N, SMALL_NQS = 4096, (65535, 65536)  # the last and the first call off the int8 tier (16-bit query field of its candidates)
DUP = (4095, 4096, 70015)  # exact duplicates: rows 4095 / 4096 sit in 32-row super-blocks 127 / 128; the lowest id comes first
CORPORA = ("iid", "mean", "iid_bf16", "mean_bf16")
TELE = ("fallback", "candidates", "path", "i8_tier", "i8_overflow", "i8_query_split", "i8_refined")
CHILD_TIMEOUT = 900


def _settings():
    out = []
    for eg in (0, 1, 2, 3):
        for cb in (None, 0, 1):
            env = {"MDR_MIPS_EVEN_GROUPS": str(eg)}
            if cb is not None:
                env["MDR_MIPS_I8_CB"] = str(cb)
            out.append((f"even{eg}-cb{'unset' if cb is None else cb}", env, KS if cb is None else [1]))  # the query split is a k = 1 matter
    out.append(("wide0", {"MDR_MIPS_WIDE": "0"}, KS))
    out.append(("i8off", {"MDR_MIPS_I8": "0"}, KS))
    return out


SETTINGS = _settings()
KNOBS = ("MDR_MIPS_EVEN_GROUPS", "MDR_MIPS_I8_CB", "MDR_MIPS_WIDE", "MDR_MIPS_I8")


def make_corpus(torch, name):
    """-> rows (float32 cuda; what add() gets), storage, queries [NQ_MAX, d]. Seeded: the parent rebuilds exactly what the child added."""
    g = torch.Generator(device="cuda").manual_seed(1 + CORPORA.index(name))
    x = torch.randn((N_ROWS, D_), generator=g, device="cuda")
    noise = torch.randn((NQ_MAX, D_), generator=g, device="cuda")
    if name.startswith("mean"):  # a common component 3 x the spread around it: the index turns the int8 tier's query split on by itself
        c = torch.randn((D_,), generator=g, device="cuda")
        x = c + 0.33 * x
        q = c + 0.33 * noise
    else:
        q = noise.clone()
    x[list(DUP)] = 1.5 * x[DUP[0]]  # a longer row: its copies are the top 3 of query 1 in every corpus
    planted = torch.arange(0, NQ_MAX, 4, device="cuda")  # every 4th query is a near-copy of a row: every query group holds decided queries
    rows = (planted * 7919 + 13) % N_ROWS
    q[planted] = x[rows] + 0.05 * noise[planted]
    q[1] = x[DUP[0]]
    return x.contiguous(), ("bf16" if name.endswith("bf16") else "f32x2h"), q.contiguous()


def make_small(torch):
    g = torch.Generator(device="cuda").manual_seed(99)
    x = torch.randn((SMALL_N, D_), generator=g, device="cuda")
    q = torch.randn((max(SMALL_NQS), D_), generator=g, device="cuda")
    planted = torch.arange(0, q.shape[0], 4, device="cuda")
    q[planted] = x[planted % SMALL_N] + 0.05 * q[planted]
    return x, q


# ---------------------------------------------------------------------------------------------------------------------------------------
# child: python tests/test_mips_modes_gpu.py OUT.npz KS (environment = the setting)
def _child(out, ks):
    import torch
    sys.path.insert(0, ROOT)
    from multihop_dense_retrieval_amd import index as mi
    res = {}

    def run(idx, tag, q, nq, k):
        D, I = idx.search_device(q[:nq].contiguous(), k)
        kern = idx.last_kernel()
        t = idx.telemetry(nq, k)
        res[f"{tag}.nq{nq}.k{k}.D"] = D.cpu().numpy()
        res[f"{tag}.nq{nq}.k{k}.I"] = I.cpu().numpy()
        res[f"{tag}.nq{nq}.k{k}.kernel"] = np.array(kern)
        res[f"{tag}.nq{nq}.k{k}.tele"] = np.array([int(t[f]) for f in TELE], np.int64)

    for name in CORPORA:
        x, storage, q = make_corpus(torch, name)
        idx = mi.IndexFlatIP(D_, storage=storage) if storage == "bf16" else mi.IndexFlatIP(D_)
        idx.add(x)
        for nq in NQS:
            for k in ks:
                run(idx, name, q, nq, k)
        del idx, x, q
        torch.cuda.empty_cache()
    x, q = make_small(torch)
    idx = mi.IndexFlatIP(D_)
    idx.add(x)
    for nq in SMALL_NQS:
        run(idx, "small", q, nq, 1)
    torch.cuda.synchronize()
    np.savez(out, **res)


if __name__ == "__main__":
    _child(sys.argv[1], [int(k) for k in sys.argv[2].split(",")])
    sys.exit(0)


# ---------------------------------------------------------------------------------------------------------------------------------------
# parent
pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
from test_oracle_mips import SCORE_TOL, check_against_truth  # noqa: E402

_DEAD = []      # a child that died by a signal or timed out: nothing more is started
RESULTS = {}    # setting name -> {key: array}
_T0 = []


def _sorted_topk(S, kk):
    """fp64 scores [nq, n] -> top-kk (scores, ids) ordered by score, then id (FAISS's tie rule)."""
    v, i = torch.topk(S, kk + 8, dim=1)
    v, i = v.cpu().numpy(), i.cpu().numpy()
    o = np.lexsort((i, -v), axis=1)
    return np.take_along_axis(v, o, 1)[:, :kk], np.take_along_axis(i, o, 1)[:, :kk]


@pytest.fixture(scope="module")
def truth():
    out = {}
    for name in CORPORA:
        x, storage, q = make_corpus(torch, name)
        xr = (x.to(torch.bfloat16) if storage == "bf16" else x).double()  # bf16 storage: the index holds the bf16-rounded rows
        assert all(torch.equal(xr[r], xr[DUP[0]]) for r in DUP)
        S = q.double() @ xr.T
        S[:, list(DUP[1:])] = S[:, DUP[0]:DUP[0] + 1]  # bit-identical rows: one score (whatever the GEMM's blocking did)
        Dt, It = _sorted_topk(S, max(KS) + 1)
        assert list(It[1, :3]) == list(DUP) and Dt[1, 0] == Dt[1, 2] > Dt[1, 3], (It[1, :4], Dt[1, :4])
        out[name] = (Dt, It)
        del x, xr, q
    x, q = make_small(torch)
    parts = [_sorted_topk(q[a: a + 8192].double() @ x.double().T, 2) for a in range(0, q.shape[0], 8192)]
    out["small"] = (np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]))
    torch.cuda.empty_cache()
    return out


def _tol(Dt):
    return max(SCORE_TOL, 2e-6 * float(np.abs(Dt).max()))


@pytest.mark.parametrize("name,env,ks", SETTINGS, ids=[s[0] for s in SETTINGS])
def test_setting_matches_fp64(truth, tmp_path, name, env, ks):
    if _DEAD:
        pytest.fail(f"not started: an earlier child died ({_DEAD[0]})")
    if not _T0:
        _T0.append(time.time())
    out = str(tmp_path / f"{name}.npz")
    cenv = {k: v for k, v in os.environ.items() if k not in KNOBS}
    cenv.update(env)
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), out, ",".join(map(str, ks))], env=cenv, cwd=ROOT, capture_output=True,
                           text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        _DEAD.append(f"{name}: timed out after {CHILD_TIMEOUT} s")
        pytest.fail(_DEAD[-1])
    if r.returncode < 0 or r.returncode >= 128:
        _DEAD.append(f"{name}: exit status {r.returncode}")
    assert r.returncode == 0, (name, r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    with np.load(out) as z:
        res = {k: z[k] for k in z.files}
    cb = env.get("MDR_MIPS_I8_CB")
    wide_off, i8_off = env.get("MDR_MIPS_WIDE") == "0", env.get("MDR_MIPS_I8") == "0"
    for corpus in CORPORA:
        Dt, It = truth[corpus]
        tol = _tol(Dt)
        f32 = not corpus.endswith("bf16")
        for nq in NQS:
            for k in ks:
                key = f"{corpus}.nq{nq}.k{k}"
                D, I, kern, tele = res[key + ".D"], res[key + ".I"], str(res[key + ".kernel"]), dict(zip(TELE, res[key + ".tele"]))
                where = (name, key, kern)
                check_against_truth(D.astype(np.float64), I, Dt[:nq, :k], It[:nq, :k], Dt[:nq, k - 1] - Dt[:nq, k], tol=tol)
                if nq > 1:
                    assert list(I[1, :3]) == list(DUP[:k]), where  # exact duplicates across a super-block boundary: lowest id first
                # --- the setting ran the path it names ---
                i8 = f32 and k == 1 and not i8_off and (nq <= 128 or not wide_off)
                assert bool(tele["i8_tier"]) == i8, (where, tele)
                if i8:
                    split = bool(int(cb)) if cb is not None else corpus.startswith("mean")
                    assert bool(tele["i8_query_split"]) == split, (where, tele)
                if nq > 128 and not wide_off:
                    assert ("8w" in kern) if i8 else ("32" in kern), where
                if nq > 128 and wide_off and k == 1:
                    assert kern == ("mips_screen_kernel<24,1>" if f32 else "mips_screen_kernel<24,1,bf16>"), where
    Dt, It = truth["small"]
    for nq in SMALL_NQS:
        key = f"small.nq{nq}.k1"
        D, I, tele = res[key + ".D"], res[key + ".I"], dict(zip(TELE, res[key + ".tele"]))
        check_against_truth(D.astype(np.float64), I, Dt[:nq, :1], It[:nq, :1], Dt[:nq, 0] - Dt[:nq, 1], tol=_tol(Dt))
        assert bool(tele["i8_tier"]) == (nq < 65536 and not wide_off and not i8_off), (name, key, tele)
    RESULTS[name] = res
    print(f"{name}: child {len(res) // 4} searches; module wall time so far {time.time() - _T0[0]:.0f} s")


def _need(*names):
    missing = [n for n in names if n not in RESULTS]
    if missing:
        pytest.fail(f"settings {missing} did not run to the end (see their own failures)")
    return [RESULTS[n] for n in names]


@pytest.mark.parametrize("cb", ["unset", "0", "1"])
def test_even_groups_modes_are_bit_identical(cb):
    """MDR_MIPS_EVEN_GROUPS only moves queries between corpus passes (and in mode 2 onto the 16-queries-per-wave kernels): same bits."""
    modes = _need(*[f"even{m}-cb{cb}" for m in (0, 1, 2, 3)])
    keys = [k for k in modes[0] if k.endswith(".D") or k.endswith(".I")]
    assert keys
    for m, res in enumerate(modes[1:], 1):
        for key in keys:
            assert np.array_equal(res[key], modes[0][key]), (f"mode {m} vs mode 0", cb, key)


@pytest.mark.parametrize("eg", [0, 1, 2, 3])
def test_query_split_settings_agree(eg):
    """MDR_MIPS_I8_CB forced off / on against the index's own choice: the same ids, scores within the bar of test_mips_i8_gpu.check()."""
    base, off, on = _need(f"even{eg}-cbunset", f"even{eg}-cb0", f"even{eg}-cb1")
    keys = [k[:-2] for k in off if k.endswith(".D")]
    assert len(keys) == len(CORPORA) * len(NQS) + len(SMALL_NQS)
    for other in (off, on):
        for key in keys:
            assert np.array_equal(other[key + ".I"], base[key + ".I"]), (eg, key)
            D, De = other[key + ".D"], base[key + ".D"]
            assert np.array_equal(D, De) or float(np.abs(D - De).max()) <= 2e-6 * float(np.abs(De).max()) + 1e-30, (eg, key)
