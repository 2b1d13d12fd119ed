"""Static hazard scan of every device unit's generated assembly (CPU only: cross-compiles gfx950).

hipcc's hazard recognizer does not look inside inline asm, so every pair of tools/
check_dpp_hazards.py RULES whose producer or consumer is in an asm statement must be padded, or
arranged, by the project (osc_device.hpp's lane-mask and DPP helpers, osc_ipm_ldl.hpp, the
generated osc_ipm_asm.hpp).  Each unit of build.DEVICE_SOURCES is compiled to a listing with the
flags of the product build and scanned whole, compiler code and asm alike, loop back edges and
branch joins included: no hazard of any class, and no mnemonic in an asm region that the checker
has no class for.  The rule table is held to the compiler's own padding by
tests/test_hazard_rules.py; the checker is tested on seeded listings in
tests/test_hazard_checker.py."""
import os
import shutil
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "operational-space-control_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))
import check_dpp_hazards as chk  # noqa: E402
from osc_amd.build import DEVICE_SOURCES, UNIT_FLAGS  # noqa: E402

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def listing(unit, out):
    """compile csrc/<unit> to assembly with the product build's flags -> its lines"""
    src = os.path.join(REPO, "operational-space-control_amd", "csrc", unit)
    subprocess.run([HIPCC, "-std=c++17", "-O3", "--offload-arch=gfx950", "--cuda-device-only",
                    *UNIT_FLAGS.get(unit, []),   # the flags the product build uses
                    "-S", "-I", os.path.join(REPO, "include"), "-o", str(out), src],
                   check=True, capture_output=True)
    return out.read_text().split("\n")


def test_the_unit_list_is_every_hip_file():
    csrc = os.path.join(REPO, "operational-space-control_amd", "csrc")
    assert sorted(DEVICE_SOURCES) == sorted(f for f in os.listdir(csrc) if f.endswith(".hip"))


@pytest.mark.skipif(not os.path.exists(HIPCC) and shutil.which("hipcc") is None,
                    reason="hipcc not available")
@pytest.mark.parametrize("unit", [u[:-len(".hip")] for u in DEVICE_SOURCES])
def test_no_dpp_hazards_in_kernels(tmp_path, unit):
    out = tmp_path / f"{unit}.s"
    listing(unit + ".hip", out)
    # through the command line, as a developer runs it: exit status and the summary line
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "check_dpp_hazards.py"),
                        str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    assert r.stdout.strip().endswith("0 hazards, 0 unclassified"), r.stdout[-3000:]
