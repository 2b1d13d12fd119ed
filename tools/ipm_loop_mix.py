#!/usr/bin/env python3
"""Static instruction mix of an interior-point kernel's iteration loop (CPU only, no GPU).

    python tools/ipm_loop_mix.py [--unit osc_ipm_go2] [--kernel SUBSTRING] [--asm FILE] > mix.json

A lone wavefront issues one instruction every ~4.5 clocks whatever the instruction is (DESIGN.md §5
"Issue slots"), so the one-wave kernel's time is its instruction count.  This compiles one
interior-point unit with the product's flags (osc_amd.build: compile_flags + UNIT_FLAGS) to
assembly, takes the named kernel (default: the headline, Go2's one-wave cold solve with the fused
refinement) and reports, as one JSON object:

* per-iteration instruction counts by broad class.  The iteration loop is the cycle of basic
  blocks (strongly connected component of the control-flow graph) that holds the block with the
  most v_fmac_f64_dpp -- the LDL^T factorisation -- and the predictor/corrector pass loop, the
  largest loop nested in it that does not hold that block, is counted twice.  Static counts:
  every block of the cycle is counted, the rarely taken ones (re-centring, warm start) too;
* the number of basic blocks of one iteration;
* the static size of the refinement region: what is laid out after the loop's last block,
  through the end of the refinement's rounds loop (the next loop that holds a factorisation);
* vgpr_count, sgpr_spill_count and vgpr_spill_count from the kernel's metadata.

Instructions are classified by mnemonic prefix only.
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

HEADLINE = "osc_ipm_kernelINS_4DimsILi18ELi12ELi4ELi5ELb0EEELb1ELb0ELi2EEE"
CLASSES = ("f64_valu", "v_cndmask", "v_cmp", "accvgpr", "other_valu", "salu", "lds", "vmem",
           "waitcnt", "nop", "other")


def compile_asm(unit: str, defines=()) -> str:
    from osc_amd.build import CSRC, HIPCC, UNIT_FLAGS, compile_flags
    src = os.path.join(CSRC, unit + ".hip")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, unit + ".s")
        subprocess.run([HIPCC, *compile_flags(defines), *UNIT_FLAGS.get(unit + ".hip", []),
                        "--cuda-device-only", "-S", src, "-o", out], check=True,
                       stderr=subprocess.DEVNULL)
        with open(out) as f:
            return f.read()


def classify(m: str) -> str:
    if m.startswith("s_waitcnt"):
        return "waitcnt"
    if m.startswith("s_nop"):
        return "nop"
    if m.startswith("v_accvgpr"):
        return "accvgpr"
    if m.startswith("v_cndmask"):
        return "v_cndmask"
    if m.startswith("v_cmp"):
        return "v_cmp"
    if m.startswith("v_") and "_f64" in m:
        return "f64_valu"
    if m.startswith("v_"):
        return "other_valu"
    if m.startswith("s_"):
        return "salu"
    if m.startswith("ds_"):
        return "lds"
    if m.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vmem"
    return "other"


def function_blocks(asm: str, kernel: str):
    """[(label or None, [mnemonic...], [branch targets], falls_through)] of the kernel's body."""
    lines = asm.splitlines()
    starts = [i for i, ln in enumerate(lines) if ln.split(";")[0].rstrip().endswith(":")
              and kernel in ln and not ln.startswith((" ", "\t", "."))]
    if len(starts) != 1:
        raise SystemExit(f"{len(starts)} functions match {kernel!r}")
    name = lines[starts[0]].split(";")[0].rstrip()[:-1]
    blocks, cur = [], {"label": None, "ins": [], "targets": [], "fall": True}

    def close():
        nonlocal cur
        blocks.append(cur)
        cur = {"label": None, "ins": [], "targets": [], "fall": True}

    for ln in lines[starts[0] + 1:]:
        s = ln.split(";")[0].strip()
        if not s:
            continue
        if s.startswith(".Lfunc_end"):
            break
        if s.endswith(":"):
            if cur["ins"] or cur["label"]:
                close()
            cur["label"] = s[:-1]
            continue
        if s.startswith("."):
            continue
        m = s.split()[0]
        cur["ins"].append(m)
        if m.startswith(("s_cbranch", "s_branch")):
            cur["targets"].append(s.split()[-1])
            cur["fall"] = m != "s_branch"
            close()
        elif m.startswith(("s_endpgm", "s_setpc")):
            cur["fall"] = False
            close()
    close()
    return name, [b for b in blocks if b["ins"] or b["label"]]


def successors(blocks):
    at = {b["label"]: i for i, b in enumerate(blocks) if b["label"]}
    succ = []
    for i, b in enumerate(blocks):
        s = [at[t] for t in b["targets"] if t in at]
        if b["fall"] and i + 1 < len(blocks):
            s.append(i + 1)
        succ.append(s)
    return succ


def sccs(nodes, succ):
    """Tarjan, iterative; only edges inside `nodes`."""
    nodes = set(nodes)
    index, low, on, stack, out, n = {}, {}, set(), [], [], 0
    for root in sorted(nodes):
        if root in index:
            continue
        work = [(root, iter(succ[root]))]
        index[root] = low[root] = n
        n += 1
        stack.append(root)
        on.add(root)
        while work:
            v, it = work[-1]
            for w in it:
                if w not in nodes:
                    continue
                if w not in index:
                    index[w] = low[w] = n
                    n += 1
                    stack.append(w)
                    on.add(w)
                    work.append((w, iter(succ[w])))
                    break
                if w in on:
                    low[v] = min(low[v], index[w])
            else:
                work.pop()
                if work:
                    low[work[-1][0]] = min(low[work[-1][0]], low[v])
                if low[v] == index[v]:
                    comp = []
                    while True:
                        w = stack.pop()
                        on.discard(w)
                        comp.append(w)
                        if w == v:
                            break
                    out.append(sorted(comp))
    return out


def loops(nodes, succ):
    return [c for c in sccs(nodes, succ) if len(c) > 1 or c[0] in succ[c[0]]]


def count(blocks, ids, weight=None):
    c = dict.fromkeys(CLASSES, 0)
    for i in ids:
        for m in blocks[i]["ins"]:
            c[classify(m)] += (weight or {}).get(i, 1)
    return c


def metadata(asm: str, name: str) -> dict:
    out = {}
    at = asm.find(f".name:           {name}\n")
    if at < 0:
        at = asm.find(f".name: {name}")
    lo = asm.rfind("  - .agpr_count", 0, at)
    hi = asm.find("  - .agpr_count", at)
    seg = asm[lo:hi if hi > 0 else len(asm)]
    for key in ("vgpr_count", "agpr_count", "sgpr_count", "sgpr_spill_count", "vgpr_spill_count",
                "group_segment_fixed_size", "private_segment_fixed_size"):
        m = re.search(rf"\.{key}:\s+(\d+)", seg)
        out[key] = int(m.group(1)) if m else None
    return out


def analyse(asm: str, kernel: str) -> dict:
    name, blocks = function_blocks(asm, kernel)
    succ = successors(blocks)
    dpp = [sum(m.startswith("v_fmac_f64_dpp") for m in b["ins"]) for b in blocks]
    # (the first such block that lies on a cycle: a kernel with the start peeled has one more
    # factorisation, straight-line, ahead of the loop)
    cyclic = [i for c in loops(range(len(blocks)), succ) for i in c]
    ldl = max(sorted(cyclic), key=dpp.__getitem__)
    outer = next(c for c in loops(range(len(blocks)), succ) if ldl in c)
    # loops nested in the iteration loop: its cycles once the blocks it is entered at are gone
    # (two of them: the start's iteration enters ahead of the others' stop test)
    entries = {i for i in outer if any(i in succ[p] for p in range(len(blocks)) if p not in outer)}
    inner = [c for c in loops([i for i in outer if i not in entries], succ) if ldl not in c]
    size = lambda ids: sum(len(blocks[i]["ins"]) for i in ids)
    twice = max(inner, key=size) if inner else []
    weight = {i: 2 for i in twice}
    per_iter = count(blocks, outer, weight)
    # the refinement: laid out after the loop, through the end of its rounds loop -- the next
    # loop that holds a factorisation (as many DPP FMAs in one block as the LDL block has)
    later = [c for c in loops(range(outer[-1] + 1, len(blocks)), succ)
             if any(dpp[i] == dpp[ldl] for i in c)]
    end = min(c[-1] for c in later) + 1 if later else len(blocks)
    region = range(outer[-1] + 1, end)
    return {
        "kernel": name,
        "per_iteration": {**per_iter, "all": sum(per_iter.values())},
        "basic_blocks": len(outer),
        "pass_loop": {"blocks": len(twice), "instructions_once": size(twice)},
        "refinement_region": {**count(blocks, region), "all": size(region),
                              "basic_blocks": len(region)},
        "function_instructions": size(range(len(blocks))),
        **metadata(asm, name),
    }


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--unit", default="osc_ipm_go2")
    ap.add_argument("--kernel", default=HEADLINE, help="substring of the mangled kernel name")
    ap.add_argument("--asm", default=None, help="read this assembly file instead of compiling")
    ap.add_argument("-D", dest="defines", action="append", default=[])
    a = ap.parse_args()
    if a.asm:
        with open(a.asm) as f:
            asm = f.read()
    else:
        asm = compile_asm(a.unit, ["-D" + d for d in a.defines])
    res = analyse(asm, a.kernel)
    print(json.dumps({"unit": a.unit, **res}, indent=1))


if __name__ == "__main__":
    main()
