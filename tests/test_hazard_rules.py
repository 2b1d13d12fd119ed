"""The hazard checker's rule table is the compiler's own (CPU only: cross-compiles gfx950).

tests/hazard_probes.hip holds one asm-free kernel per producer -> consumer pair of
tools/check_dpp_hazards.py RULES.  hipcc pads these pairs in code it generates, so the wait states
between each pair in its listing are the target's requirement as this toolchain knows it.  They
are counted here with the checker's own classification and counting functions and must equal the
table's entry: a toolchain that changes a rule fails this test instead of leaving the scan of the
inline asm (tests/test_asm_hazards.py) and the generator (tools/gen_ipm_asm.py) on a stale number."""
import os
import shutil
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
import check_dpp_hazards as chk  # noqa: E402

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC) and shutil.which("hipcc") is None,
                                reason="hipcc not available")

# probe kernel -> (consumer role, producer class) of the rule it measures
PROBES = {
    "probe_valu_dpp": ("dpp_src", "valu_vgpr"),
    "probe_vcc_mask": ("valu_vcc", "valu_vcc"),
    "probe_vcc_operand": ("valu_vcc", "valu_vcc"),
    "probe_sgpr_mask": ("valu_sgpr", "valu_sgpr"),
    "probe_lane_sgpr_operand": ("valu_sgpr", "valu_sgpr"),
    "probe_trans_valu": ("valu_vgpr", "trans_vgpr"),
    "probe_valu_readfirstlane": ("lane_src", "valu_vgpr"),
    "probe_valu_readlane": ("lane_src", "valu_vgpr"),
    "probe_sgpr_lane_select": ("lane_sel", "valu_sgpr"),
}
# rules no plain C++ reaches on this target: the compiler writes EXEC from the SALU only
UNPROBED = {"dpp_exec": "probe_exec_dpp", "lane_exec": "probe_exec_readlane"}
PADDING = ("s_nop", "s_waitcnt")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """kernel name -> its instructions, from one compile of the probes"""
    out = tmp_path_factory.mktemp("probes") / "hazard_probes.s"
    subprocess.run([HIPCC, "-std=c++17", "-O3", "--offload-arch=gfx950", "--cuda-device-only",
                    "-S", "-o", str(out), os.path.join(REPO, "tests", "hazard_probes.hip")],
                   check=True, capture_output=True)
    insts = chk.parse(out.read_text().split("\n"))
    found, name = {}, None
    for x in insts:
        if x.label and not x.label.startswith(".L"):   # a function's entry (or the listing's tail)
            name = x.label if x.label.startswith("probe_") else None
            found.setdefault(name, [])
        elif name:
            found[name].append(x)
    del found[None]
    return found


def test_every_rule_is_probed_or_accounted_for():
    probed = {(c, p) for c, p in PROBES.values()}
    for r in chk.RULES:
        assert r.consumer in UNPROBED or any((r.consumer, p) in probed for p in r.producer), r


@pytest.mark.parametrize("kernel", sorted(PROBES))
def test_compiler_pads_what_the_table_says(kernels, kernel):
    consumer, producer = PROBES[kernel]
    r = chk.rule(consumer, producer)
    insts = kernels[kernel]
    found = [(i, j) for i, j in chk.pairs(insts, r) if producer in insts[i].prod]
    assert found, f"{kernel}: no {r.name} pair in the compiler's code:\n" + \
        "\n".join(x.text for x in insts)
    for i, j in found:
        between = [x.op for x in insts[i + 1:j]]
        listing = "\n".join(x.text for x in insts[i:j + 1])
        assert all(op in PADDING for op in between), f"{kernel} is a bad probe:\n{listing}"
        waits = chk.wait_states(insts, i, j)
        print(f"{kernel}: {r.name}: {waits} wait states")
        assert waits == r.waits, f"{r.name}: compiler pads {waits}, table says {r.waits}\n{listing}"


@pytest.mark.parametrize("consumer", sorted(UNPROBED))
def test_compiler_writes_exec_from_the_salu_only(kernels, consumer):
    # the probe's consumer is there, behind a change of EXEC that no VALU instruction made
    insts = kernels[UNPROBED[consumer]]
    assert any(consumer in x.cons for x in insts)
    assert any(x.op.startswith("s_") and "exec" in x.text for x in insts)
    for name, body in kernels.items():
        assert not [x.text for x in body if "valu_exec" in x.prod], name
