#!/usr/bin/env python3
"""Static instruction census of the assembly kernel, per phase (CPU only, no GPU).

    python tools/setup_mix.py [--kernel SUBSTRING] [--asm FILE] [--src-dir DIR] > mix.json

With four waves per SIMD the assembly kernel's VALU is busy about two thirds of the waves'
lifetime, so what it issues is what it costs.  This compiles osc_setup.hip with
the product's flags plus -DOSC_PHASE_MARKS (osc_device.hpp: the stamp macros become `;@@BEGIN` /
`;@@END <slot>` comments in the listing), takes the named kernel (default: the headline's, Go2's
lean assembly) and counts the instructions between each BEGIN and the
END that follows it in the listing, by class.  Static counts in layout order: a rolled loop's body
counts once, both arms of a branch count.  --src-dir compiles another checkout's csrc/ (a parent
commit's) with this tool.

Classes, by mnemonic: f64 arithmetic (plain and DPP), MFMA, v_cndmask, v_cmp, v_mov, integer /
address VALU (v_mul_lo_u32 listed apart), SALU / SMEM, branches (s_cbranch_execz apart), s_nop
(and the wait states they hold), s_waitcnt, LDS, VMEM (global / buffer stores apart).
"""
from __future__ import annotations

import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "operational-space-control_amd"))

HEADLINE = "osc_setup_kernelINS_4DimsILi18ELi12ELi4ELi5ELb0EEELb1E"
PHASES = {0: "A staging", 1: "B Ha", 2: "C base block / X^", 6: "C2 Schur factor", 7: "C2 solves",
          8: "C2 x_b + X store", 9: "WH rows", 10: "WH basis", 4: "D T1, Hr | g", 5: "hand-off"}
CLASSES = ("f64", "f64_dpp", "mfma", "v_cndmask", "v_cmp", "v_mov", "int_valu", "salu", "branch",
           "nop", "waitcnt", "lds", "vmem", "other")


def compile_asm(src_dir: str | None) -> str:
    from osc_amd.build import CSRC, HIPCC, UNIT_FLAGS, compile_flags
    src = os.path.join(src_dir or CSRC, "osc_setup.hip")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "osc_setup.s")
        subprocess.run([HIPCC, *compile_flags(["-DOSC_PHASE_MARKS"]),
                        *UNIT_FLAGS.get("osc_setup.hip", []), "--cuda-device-only", "-S", src,
                        "-o", out], check=True, stderr=subprocess.DEVNULL)
        with open(out) as f:
            return f.read()


def classify(m: str) -> str:
    if m.startswith("s_waitcnt"):
        return "waitcnt"
    if m.startswith("s_nop"):
        return "nop"
    if m.startswith(("s_cbranch", "s_branch")):
        return "branch"
    if m.startswith("s_"):
        return "salu"
    if m.startswith("v_mfma"):
        return "mfma"
    if m.startswith("v_cndmask"):
        return "v_cndmask"
    if m.startswith("v_cmp"):
        return "v_cmp"
    if m.startswith("v_") and "_f64" in m:
        return "f64_dpp" if m.endswith("_dpp") else "f64"
    if m.startswith(("v_mov", "v_accvgpr")):
        return "v_mov"
    if m.startswith("v_"):
        return "int_valu"
    if m.startswith("ds_"):
        return "lds"
    if m.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vmem"
    return "other"


def kernel_lines(asm: str, kernel: str):
    lines = asm.splitlines()
    starts = [i for i, ln in enumerate(lines) if ln.split(";")[0].rstrip().endswith(":")
              and kernel in ln and not ln.startswith((" ", "\t", "."))]
    if not starts:
        raise SystemExit(f"no function matches {kernel!r}")
    name = lines[starts[0]].split(";")[0].rstrip()[:-1]
    body = []
    for ln in lines[starts[0] + 1:]:
        if ln.strip().startswith(".Lfunc_end"):
            break
        body.append(ln)
    return name, body


def census(body):
    """-> ({phase: counts}, whole-kernel counts); instructions outside any BEGIN/END pair go to
    the phase "outside"."""
    phases, total = {}, new_counts()
    cur = None
    for ln in body:
        if ";@@BEGIN" in ln:
            cur = new_counts()
            continue
        m_end = re.search(r";@@END\s+(\d+)", ln)
        if m_end:
            slot = int(m_end.group(1))
            into = phases.setdefault(PHASES.get(slot, f"slot {slot}"), new_counts())
            for k, v in (cur or {}).items():
                into[k] += v
            cur = None
            continue
        s = ln.split(";")[0].strip()
        if not s or s.endswith(":") or s.startswith("."):
            continue
        ops = s.split()
        m = ops[0]
        tgt = cur if cur is not None else phases.setdefault("outside", new_counts())
        for c in (tgt, total):
            add(c, m, s)
    return phases, total


def new_counts():
    c = dict.fromkeys(CLASSES, 0)
    c.update(all=0, nop_wait_states=0, v_mul_lo_u32=0, cbranch_execz=0, stores=0, stores_16b=0,
             stores_sc1=0)
    return c


def add(c, m, s):
    c[classify(m)] += 1
    c["all"] += 1
    if m.startswith("s_nop"):
        c["nop_wait_states"] += int(s.split()[1], 0) + 1
    if m.startswith("v_mul_lo_u32"):
        c["v_mul_lo_u32"] += 1
    if m.startswith("s_cbranch_execz"):
        c["cbranch_execz"] += 1
    if m.startswith(("global_store", "buffer_store", "flat_store")):
        c["stores"] += 1
        c["stores_16b"] += m.endswith("dwordx4")
        c["stores_sc1"] += " sc1" in s


def metadata(asm: str, name: str) -> dict:
    at = asm.find(f".name:           {name}\n")
    lo = asm.rfind("  - .agpr_count", 0, at)
    hi = asm.find("  - .agpr_count", at)
    seg = asm[lo:hi if hi > 0 else len(asm)]
    out = {}
    for key in ("vgpr_count", "sgpr_count", "sgpr_spill_count", "vgpr_spill_count",
                "group_segment_fixed_size", "private_segment_fixed_size"):
        m = re.search(rf"\.{key}:\s+(\d+)", seg)
        out[key] = int(m.group(1)) if m else None
    return out


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--kernel", default=HEADLINE, help="substring of the mangled kernel name")
    ap.add_argument("--asm", default=None, help="read this listing instead of compiling")
    ap.add_argument("--src-dir", default=None, help="csrc/ of another checkout to compile")
    a = ap.parse_args()
    if a.asm:
        with open(a.asm) as f:
            asm = f.read()
    else:
        asm = compile_asm(a.src_dir)
    name, body = kernel_lines(asm, a.kernel)
    phases, total = census(body)
    print(json.dumps({"kernel": name, "total": total, "phases": phases, **metadata(asm, name)},
                     indent=1))


if __name__ == "__main__":
    main()
