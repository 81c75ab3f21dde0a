"""bench.py --dump-outputs and the split between a plain run and --full. CPU: what dump_outputs writes (float32 / float64 .npy per array, a fixed
row sample beyond the size limit). GPU (-m gpu): a plain run prints the headline without the --full sub-results, and the outputs it dumps are the
arrays the timed loop returned -- the same as --dump-ids and the same as a --full run of the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _load_dir(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_writes_every_array_as_float32_or_float64(tmp_path):
    g = torch.Generator().manual_seed(0)
    out = {"q": torch.randn((4, 8), generator=g), "I": torch.tensor([[3], [2 ** 40 + 1], [0], [7]]), "mask2": torch.ones((2, 3), dtype=torch.bool),
           "score": torch.randn((4, 1), generator=g).half(), "ids2": None}
    bench.dump_outputs(out, str(tmp_path / "d"))
    got = _load_dir(str(tmp_path / "d"))
    assert set(got) == {"q", "I", "mask2", "score"}
    assert got["q"].dtype == np.float32 and np.array_equal(got["q"], out["q"].numpy())
    assert got["I"].dtype == np.float64 and np.array_equal(got["I"].astype(np.int64), out["I"].numpy())  # ids stay exact
    assert got["mask2"].dtype == np.float64 and (got["mask2"] == 1).all()
    assert got["score"].dtype == np.float32 and np.array_equal(got["score"], out["score"].float().numpy())


def test_dump_outputs_keeps_a_fixed_row_sample_beyond_the_limit(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 8192)
    out = {"a": torch.arange(4000, dtype=torch.float32).view(1000, 4), "b": torch.arange(500).view(500, 1)}
    bench.dump_outputs(out, str(tmp_path / "one"))
    bench.dump_outputs(out, str(tmp_path / "two"))
    one, two = _load_dir(str(tmp_path / "one")), _load_dir(str(tmp_path / "two"))
    assert sum(a.nbytes for a in one.values()) <= 8192
    for k in one:
        assert np.array_equal(one[k], two[k]), k  # the same sample every run
    rows = one["a"][:, 0] / 4
    assert len(rows) > 1 and (np.diff(rows) > 0).all() and np.array_equal(one["a"], out["a"].numpy()[rows.astype(int)])
    assert (np.diff(one["b"][:, 0]) > 0).all() and one["b"][-1, 0] < 500


def _bench(argv):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "TORCHELASTIC_RUN_ID"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + argv, env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_what_the_loop_returned(tmp_path):
    common = ["--gpus", "1", "--rows", "200000", "--steps", "4", "--warmup", "2"]
    plain_dir, full_dir, ids = str(tmp_path / "plain"), str(tmp_path / "full"), str(tmp_path / "ids.npz")
    p = _bench(common + ["--dump-outputs", plain_dir, "--dump-ids", ids])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in p, k
    assert p["steps"] == 4 and p["higher_is_better"] is True and p["ms_per_step"] > 0
    assert abs(p["value"] - p["config"]["global_batch"] * 1e3 / p["ms_per_step"]) <= 1e-3 * p["value"]
    for k in ("self_check", "sequential", "numerics_modes", "anisotropic", "structured", "cpu_baseline"):
        assert k not in p, k  # --full only
    got, z = _load_dir(plain_dir), np.load(ids)
    assert {"q", "q2", "D", "I", "D2", "I2", "hop1", "hop2", "score"} <= set(got)
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    for k in ("I", "I2"):
        assert np.array_equal(got[k].astype(np.int64), z[k]), k
    for k in ("D", "D2"):
        assert np.array_equal(got[k], z[k]), k

    f = _bench(common + ["--dump-outputs", full_dir, "--full", "--no-cpu-baseline"])
    assert f["self_check"]["full_size_exact"] and "sequential" in f and "numerics_modes" in f
    full = _load_dir(full_dir)
    assert set(full) == set(got)
    for k in got:  # same arguments -> same inputs -> same outputs
        if got[k].dtype == np.float64:
            assert np.array_equal(full[k], got[k]), k
        else:
            assert np.abs(full[k] - got[k]).max() <= 1e-3, k
