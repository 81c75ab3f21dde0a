"""CPU (-m "not gpu"): every device kernel of the product library compiles for gfx950 without scratch memory and without register spills.

The hand-scheduled kernels depend on it: the wide int8 kernel (mips_screen8w_kernel<12,*,3,true>) uses 254 of 256 VGPRs and its
row terms brs[] must stay in the registers its inline-asm reads and counted waits were written for; gemm_quad_kernel's K-loop is
generated around fixed AGPR / VGPR assignments (scripts/check_quad_agprs.py). A compiler update or a small edit that pushes one of
them into scratch changes no result on the CPU and fails nothing else, so the compiler's own resource report is checked here, with
the flags of the product build (multihop_dense_retrieval_amd/build.py)."""
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

from multihop_dense_retrieval_amd import build

# SGPR spills go to VGPR lanes (v_writelane / v_readlane), not to memory (ScratchSize stays 0). Five kernels had them when this check was
# written -- the generic fp32 MIPS kernel (the fallback for shapes the MFMA kernels do not serve) and the register-tiled attention
# kernels -- and they are pinned at those counts; no other kernel may spill anything, and no kernel may use scratch or spill VGPRs.
SGPR_SPILL_ALLOWED = {"mips_generic_kernel<true>": 4, "mips_generic_kernel<false>": 8,
                      "attention_kernel<8>": 2, "attention_kernel<24>": 192, "attention_kernel<32>": 290}


_TYPES = {"f": "float", "d": "double", "t": "unsigned short", "i": "int", "c": "char", "h": "unsigned char", "DF16_": "_Float16"}


def short_name(mangled):
    """'_ZN3mdr12_GLOBAL__N_120mips_screen8w_kernelILi12ELi0ELi3ELb1EEEv...' -> 'mips_screen8w_kernel<12,0,3,true>' (integer, bool and
    builtin-type template arguments; anything else ends the list with '...'). Kernels are keyed by their mangled names; this is a label."""
    s = re.sub(r"^_ZN(?:3mdr)?12_GLOBAL__N_1", "", mangled)
    m = re.match(r"(\d+)", s)
    if not m:
        return mangled
    n0 = len(m.group(1))
    name, rest = s[n0: n0 + int(m.group(1))], s[n0 + int(m.group(1)):]
    if not rest.startswith("I"):
        return name
    rest, args = rest[1:], []
    while rest and not rest.startswith("E"):
        a = re.match(r"L([ijb])(n?\d+)E", rest)
        t = next((k for k in _TYPES if rest.startswith(k)), None)
        if a:
            v = a.group(2).replace("n", "-")
            args.append({"0": "false", "1": "true"}[v] if a.group(1) == "b" else v)
            rest = rest[a.end():]
        elif t:
            args.append(_TYPES[t])
            rest = rest[len(t):]
        else:
            args.append("...")
            break
    return f"{name}<{','.join(args)}>"


def parse_resource_remarks(text):
    """-Rpass-analysis=kernel-resource-usage output -> {mangled name: {key: int}} (one remark line per key, each kernel's block
    opened by its 'Function Name' line)."""
    kernels, cur = {}, None
    for m in re.finditer(r"remark: +([A-Za-z][A-Za-z ]*?(?: \[[^\]]*\])?): (\S+) \[-Rpass-analysis=kernel-resource-usage\]", text):
        key, val = m.group(1), m.group(2)
        if key == "Function Name":
            cur = kernels.setdefault(val, {})
        elif cur is not None and re.fullmatch(r"-?\d+", val):
            cur[key] = int(val)
    return kernels


def _compile(src):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc] + build.hipcc_flags() + ["--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage", src,
                        "-o", os.devnull], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stderr


@pytest.fixture(scope="module")
def resources():
    with ThreadPoolExecutor(max_workers=len(build.sources())) as ex:
        texts = list(ex.map(_compile, build.sources()))
    kernels = {}
    for t in texts:
        kernels.update(parse_resource_remarks(t))
    return {(short_name(n), n): r for n, r in kernels.items()}


def test_parser_reads_a_remark_block():
    text = ("x.hip:1:2: remark: Function Name: _Z1kv [-Rpass-analysis=kernel-resource-usage]\n"
            "x.hip:1:2: remark:     VGPRs: 28 [-Rpass-analysis=kernel-resource-usage]\n"
            "x.hip:1:2: remark:     VGPRs Spill: 3 [-Rpass-analysis=kernel-resource-usage]\n"
            "x.hip:1:2: remark:     ScratchSize [bytes/lane]: 16 [-Rpass-analysis=kernel-resource-usage]\n"
            "x.hip:1:2: remark: Function Name: _Z1jv [-Rpass-analysis=kernel-resource-usage]\n"
            "x.hip:1:2: remark:     SGPRs Spill: 0 [-Rpass-analysis=kernel-resource-usage]\n")
    assert parse_resource_remarks(text) == {"_Z1kv": {"VGPRs": 28, "VGPRs Spill": 3, "ScratchSize [bytes/lane]": 16}, "_Z1jv": {"SGPRs Spill": 0}}
    assert short_name("_ZN3mdr12_GLOBAL__N_120mips_screen8w_kernelILi12ELi1ELi3ELb1EEEvPKcxiS3_PKDv4_fiiPjPyPiS9_S8_PKyPKf") == \
        "mips_screen8w_kernel<12,1,3,true>"
    assert short_name("_ZN3mdr12_GLOBAL__N_122convert_to_frag_kernelIDF16_Lb0EEEvPKT_xxixPcS5_Pif") == "convert_to_frag_kernel<_Float16,false>"
    assert short_name("_ZN3mdr12_GLOBAL__N_121attention_ring_kernelEPKDF16_PKiS4_iiiiPDF16_") == "attention_ring_kernel"
    assert short_name("_ZN12_GLOBAL__N_123scale_flag_float_kernelEPif") == "scale_flag_float_kernel"


def test_every_kernel_is_reported(resources):
    """A parse failure or a missing remark must not pass as 'no spills': the count and the kernels the hand scheduling is about are pinned."""
    assert len(resources) >= 101, len(resources)
    for key, r in resources.items():
        assert {"VGPRs", "VGPRs Spill", "SGPRs Spill", "ScratchSize [bytes/lane]"} <= set(r), (key, r)
    labels = {label: r for label, _ in resources for r in [resources[(label, _)]]}
    for mode_cb in ("0,3,true", "1,3,true", "0,3,false", "1,3,false"):
        assert f"mips_screen8w_kernel<12,{mode_cb}>" in labels, sorted(labels)
    assert labels["mips_screen8w_kernel<12,1,3,true>"]["VGPRs"] > 128  # the report really is the wide kernel's (one workgroup per CU)
    assert sum(label.startswith("gemm_quad_kernel<") for label, _ in resources) == 3, sorted(labels)
    assert "attention_ring_kernel" in labels, sorted(labels)
    assert "grad_strand_reduce_kernel" in labels, sorted(labels)  # one definition serves the LayerNorm and the embedding backward


def test_no_kernel_uses_scratch_or_spills(resources):
    bad = {}
    for (label, mangled), r in resources.items():
        if r["ScratchSize [bytes/lane]"] or r["VGPRs Spill"] or r["SGPRs Spill"] > SGPR_SPILL_ALLOWED.get(label, 0):
            bad[label] = r
    assert not bad, bad
