"""GPU (-m gpu): the sizes the MIPS search plans (make_plan, csrc/mdr_mips_search.inl) against a recorded table.

mdr_index_search_workspace_bytes() and mdr_index_queries_per_pass() are pure host arithmetic over the index's shape, the device's CU
count and (nq, k): grid sizes, candidate-list regions, query padding. No test pinned them, so a change of the grid arithmetic could
shrink a region some kernel writes or grow the workspace of every call unnoticed. tests/golden/mips_plan.json holds both numbers for
every case below as the commit before the host drivers were unified plans them for a device of 256 CUs (an MI355X). Run as a script,
this file writes the same table for the loaded library and the visible device:

    python tests/test_mips_plan_gpu.py OUT.json

No search kernel runs: the indexes only need their row count, so they are filled with zeros. Default environment only; the schedule
knobs are test_mips_modes_gpu.py's subject."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "mips_plan.json")
NQS = [1, 128, 129, 256, 257, 300, 800, 65535, 65536]
KS = [1, 2, 32, 33, 128, 129, 256, 257]
# 4,096 rows = 128 super-blocks of 32 rows: below the CU count, every grid equals its units; 20,000 rows = 625: the grids saturate.
# d = 768 is the screen path (with the int8 tier for f32x2h, without it for bf16 and compact), d = 256 the generic kernel.
CASES = [(storage, 768, n) for storage in ("f32x2h", "bf16", "compact") for n in (4096, 20000)] + [("f32x2h", 256, n) for n in (4096, 20000)]


def case_name(storage, d, n):
    return f"{storage}.d{d}.n{n}"


def plan_table(torch, mi):
    """-> {case: {"workspace_bytes": [nq][k], "queries_per_pass": [nq][k]}} of the loaded library on the current device."""
    from multihop_dense_retrieval_amd import _lib
    L = _lib.lib()
    table = {}
    for storage, d, n in CASES:
        idx = mi.IndexFlatIP(d) if storage == "f32x2h" else mi.IndexFlatIP(d, storage=storage)
        idx.add(torch.zeros((n, d), device="cuda"))
        table[case_name(storage, d, n)] = {
            "workspace_bytes": [[int(L.mdr_index_search_workspace_bytes(idx._h, nq, k)) for k in KS] for nq in NQS],
            "queries_per_pass": [[idx.queries_per_pass(nq, k) for k in KS] for nq in NQS]}
    return table


if __name__ == "__main__":  # record the table
    import torch
    sys.path.insert(0, ROOT)
    from multihop_dense_retrieval_amd import index as mi
    doc = {"num_cus": torch.cuda.get_device_properties(0).multi_processor_count, "nqs": NQS, "ks": KS, "cases": plan_table(torch, mi)}
    with open(sys.argv[1], "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    sys.exit(0)


import pytest  # noqa: E402

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def test_planned_sizes_match_the_recorded_table():
    from multihop_dense_retrieval_amd import index as mi
    with open(GOLDEN) as f:
        gold = json.load(f)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if cus != gold["num_cus"]:
        pytest.skip(f"the table was recorded on a device with {gold['num_cus']} CUs, this one has {cus}")
    assert gold["nqs"] == NQS and gold["ks"] == KS and sorted(gold["cases"]) == sorted(case_name(*c) for c in CASES)
    got = plan_table(torch, mi)
    for case, want in gold["cases"].items():
        for field in ("workspace_bytes", "queries_per_pass"):
            for i, nq in enumerate(NQS):
                for j, k in enumerate(KS):
                    assert got[case][field][i][j] == want[field][i][j], (case, field, nq, k, got[case][field][i][j], want[field][i][j])
