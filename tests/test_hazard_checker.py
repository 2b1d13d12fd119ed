"""Tests of the hazard checker itself (tools/check_dpp_hazards.py; CPU only): a checker that
silently matched nothing would pass every scan of tests/test_asm_hazards.py.

For every rule of its table a synthetic listing one wait state short must be flagged with the
consumer's and the producer's line numbers, and the same listing padded must pass -- on a straight
line, across a loop's back edge and across a branch join (there the branch itself is one wait
state, so only the rules that need two or more can be left short).  And the real thing: in the
finished Go2 interior-point listing, taking out one s_nop that guards a DPP read inside an asm
region, and shortening one compare -> select distance, must each be flagged."""
import os
import shutil
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
sys.path.insert(0, os.path.join(REPO, "operational-space-control_amd"))
import check_dpp_hazards as chk  # noqa: E402

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
DPP = "row_newbcast:1 row_mask:0xf bank_mask:0xf"
# consumer role -> (a producer, a consumer of what it wrote)
PAIRS = {
    "dpp_src": ("v_add_f64 v[2:3], v[4:5], v[6:7]", f"v_mov_b64_dpp v[8:9], v[2:3] {DPP}"),
    "valu_vcc": ("v_cmp_eq_u32_e32 vcc, 1, v0", "v_cndmask_b32_e32 v1, v2, v3, vcc"),
    "valu_sgpr": ("v_cmp_lt_u32_e64 s[2:3], 1, v0", "v_cndmask_b32_e64 v1, 0, v2, s[2:3]"),
    "valu_vgpr": ("v_rcp_f64_e32 v[2:3], v[4:5]", "v_mul_f64 v[6:7], v[2:3], v[4:5]"),
    "lane_src": ("v_add_u32_e32 v2, s4, v0", "v_readfirstlane_b32 s0, v2"),
    "lane_sel": ("v_readfirstlane_b32 s2, v0", "v_readlane_b32 s3, v1, s2"),
    "dpp_exec": ("v_cmpx_lt_u32_e64 s[4:5], 1, v0", f"v_mov_b32_dpp v1, v2 {DPP}"),
    "lane_exec": ("v_cmpx_lt_u32_e64 s[4:5], 1, v0", "v_readlane_b32 s0, v1, 3"),
}
FILLER = ["v_mov_b32_e32 v40, v41"] * (chk.MAX_WAITS + 1)   # touches nothing the pairs use
RULES = list(chk.RULES)
IDS = [r.consumer for r in RULES]


def pad(n, nop=True):
    """n wait states: one s_nop, or n independent instructions"""
    if n <= 0:
        return []
    return [f"s_nop {n - 1}"] if nop else FILLER[:n]


def run(body):
    """scan a kernel made of the lines of body -> [(rule name, consumer line, producer line)]"""
    lines = ["\t.text", "kernel:"] + ["\t" + t if not t.endswith(":") else t for t in body] + \
        ["\ts_endpgm"]
    bad, unknown = chk.check(lines)
    assert not unknown
    return [(r.name, c.line, p.line) for r, c, p, _ in bad], lines


def lineno(lines, text, last=False):
    hits = [n + 1 for n, l in enumerate(lines) if l.strip() == text]
    return hits[-1] if last else hits[0]


def test_every_rule_has_a_pair():
    assert {r.consumer for r in RULES} == set(PAIRS)
    assert chk.MAX_WAITS == max(r.waits for r in RULES) >= 4


@pytest.mark.parametrize("nop", [True, False], ids=["s_nop", "instructions"])
@pytest.mark.parametrize("r", RULES, ids=IDS)
def test_straight_line(r, nop):
    prod, cons = PAIRS[r.consumer]
    short, lines = run(FILLER + [prod] + pad(r.waits - 1, nop) + [cons])
    assert short == [(r.name, lineno(lines, cons), lineno(lines, prod))]
    good, _ = run(FILLER + [prod] + pad(r.waits, nop) + [cons])
    assert good == []


@pytest.mark.parametrize("r", [r for r in RULES if r.waits >= 2],
                         ids=[r.consumer for r in RULES if r.waits >= 2])
def test_loop_back_edge(r):
    # the producer closes the loop's body, the consumer opens it: only the back edge joins them
    prod, cons = PAIRS[r.consumer]

    def loop(n):
        return FILLER + [".LBB0_1:"] + pad(n) + [cons] + FILLER + [prod, "s_cbranch_scc1 .LBB0_1"]
    short, lines = run(loop(r.waits - 2))          # + the branch's own wait state: one short
    assert short == [(r.name, lineno(lines, cons), lineno(lines, prod))]
    good, _ = run(loop(r.waits - 1))
    assert good == []


@pytest.mark.parametrize("taken", [True, False], ids=["branch", "fall-through"])
@pytest.mark.parametrize("r", [r for r in RULES if r.waits >= 2],
                         ids=[r.consumer for r in RULES if r.waits >= 2])
def test_branch_join(r, taken):
    # two ways into the consumer's block, the producer on one of them: the worst one decides
    prod, cons = PAIRS[r.consumer]

    def join(n):
        if taken:     # the producer's side jumps to the join, the clean side falls into it
            return ["s_cbranch_scc1 .LBB0_2", prod, "s_branch .LBB0_3", ".LBB0_2:"] + FILLER + \
                [".LBB0_3:"] + pad(n) + [cons]
        return ["s_cbranch_scc1 .LBB0_2"] + FILLER + ["s_branch .LBB0_3", ".LBB0_2:", prod,
                                                     "s_cmp_eq_u32 s20, 0", ".LBB0_3:"] + pad(n) + [cons]
    short, lines = run(join(r.waits - 2))          # (one wait state on either way in already)
    assert short == [(r.name, lineno(lines, cons), lineno(lines, prod))]
    good, _ = run(join(r.waits - 1))
    assert good == []


def test_an_unconditional_branch_ends_the_fall_through():
    prod, cons = PAIRS["dpp_src"]
    got, _ = run([prod, "s_branch .LBB0_9", ".LBB0_5:", cons, ".LBB0_9:"] + FILLER +
                 ["s_cbranch_scc1 .LBB0_5"])
    assert got == []


def test_the_nearest_producer_is_reported_and_a_function_entry_ends_the_walk():
    prod, cons = PAIRS["valu_sgpr"]
    got, lines = run([prod, prod, cons])
    assert got == [(chk.rule("valu_sgpr").name, lineno(lines, cons), lineno(lines, prod, last=True))]
    bad, _ = chk.check(["first:", "\t" + prod, "second:", "\t" + cons])
    assert bad == []


def test_implicit_vcc_and_carries():
    name = chk.rule("valu_vcc").name
    for prod, cons in [("v_cmp_eq_u32_e32 vcc, 1, v0", "v_cndmask_b32 v1, v2, v3, vcc"),
                       ("v_add_co_u32_e32 v1, vcc, v2, v3", "v_addc_co_u32_e32 v4, vcc, v5, v6, vcc"),
                       ("v_cmp_lt_f32_e32 vcc, s2, v2", "v_add_u32_e32 v0, vcc_lo, v0"),
                       ("v_cmp_class_f64_e64 vcc, v[2:3], s10", "v_cndmask_b32_e32 v1, v2, v3")]:
        got, lines = run([prod, "s_nop 0", cons])
        assert got == [(name, lineno(lines, cons), lineno(lines, prod))], (prod, cons)
        assert run([prod, "s_nop 1", cons])[0] == []


def test_unclassified_mnemonics_fail_inside_asm_only():
    op = "v_permlane32_swap_b32_e32 v1, v2"
    bad, unknown = chk.check(["kernel:", "\t;;#ASMSTART", "\t" + op, "\t;;#ASMEND", "\t" + op])
    assert bad == [] and [(x.line, x.text) for x in unknown] == [(3, op)]
    known = ["v_fmac_f64_dpp v[0:1], v[2:3], v[4:5] " + DPP, "s_waitcnt lgkmcnt(0)",
             "ds_write_b64 v0, v[2:3] offset:8", "global_load_dwordx2 v[0:1], v4, s[2:3]",
             "v_rcp_f64_e32 v[2:3], v[8:9]", "v_readlane_b32 s0, v7, 3", "s_mov_b32 s4, 0x11"]
    assert chk.check(["kernel:", "\t;;#ASMSTART"] + ["\t" + t for t in known] + ["\t;;#ASMEND"])[1] == []


def test_command_line(tmp_path):
    prod, cons = PAIRS["dpp_src"]
    tool = os.path.join(REPO, "tools", "check_dpp_hazards.py")
    for body, rc, tail in ([prod, "s_nop 0", cons], 1, "1 hazards, 0 unclassified"), \
                          ([prod, "s_nop 1", cons], 0, "0 hazards, 0 unclassified"):
        f = tmp_path / f"k{rc}.s"
        f.write_text("kernel:\n" + "".join(f"\t{t}\n" for t in body))
        r = subprocess.run([sys.executable, tool, str(f)], capture_output=True, text=True)
        assert r.returncode == rc and r.stdout.strip().endswith(tail), r.stdout
        if rc:
            assert "line 4:" in r.stdout and "<- line 2 (1 wait states" in r.stdout, r.stdout


# ---- mutations of the finished Go2 listing ----------------------------------------------------------

@pytest.fixture(scope="module")
def go2(tmp_path_factory):
    """(the listing's lines, its instructions without the labels)"""
    if not os.path.exists(HIPCC) and shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    from test_asm_hazards import listing
    lines = listing("osc_ipm_go2.hip", tmp_path_factory.mktemp("go2") / "osc_ipm_go2.s")
    return lines, [x for x in chk.parse(lines) if not x.label]


def scan_around(lines, line, blank):
    """the hazards of the listing with the lines `blank` taken out, scanned on the 400 lines
    around `line` (a whole scan of the unit is tests/test_asm_hazards.py's)"""
    lines = [("" if n + 1 in blank else l) for n, l in enumerate(lines)]
    lo = max(0, line - 200)
    bad, _ = chk.check(["window:"] + lines[lo:line + 200])
    return [(r.name, c.line + lo - 1, p.line + lo - 1) for r, c, p, _ in bad]


def test_go2_without_one_dpp_guard_is_flagged(go2):
    go2, insts = go2
    r = chk.rule("dpp_src")
    # an s_nop inside asm, a DPP read right after it, the VALU write of its source right before
    site = next((a, b, c) for a, b, c in zip(insts, insts[1:], insts[2:])
                if b.in_asm and b.op == "s_nop" and c.in_asm and "dpp_src" in c.cons
                and a.prod.get("valu_vgpr", set()) & c.cons["dpp_src"])
    prod, nop, cons = site
    assert scan_around(go2, cons.line, set()) == []
    assert (r.name, cons.line, prod.line) in scan_around(go2, cons.line, {nop.line})


def test_go2_with_one_compare_nearer_its_select_is_flagged(go2):
    go2, insts = go2
    hits = 0
    for consumer in ("valu_vcc", "valu_sgpr"):      # the VCC form and the SGPR-pair form
        r = chk.rule(consumer)
        i, j = next((i, j) for i, j in chk.pairs(insts, r, reach=16)
                    if insts[i].in_asm and insts[j].in_asm and insts[i].op.startswith("v_cmp")
                    and insts[j].op.startswith("v_cndmask") and j - i > 1
                    and chk.wait_states(insts, i, j) >= r.waits)
        prod, cons = insts[i], insts[j]
        assert scan_around(go2, cons.line, set()) == []
        between = {x.line for x in insts[i + 2:j]}   # all but one instruction between them
        if insts[i + 1].cost > 1:                    # (an s_nop of two or more is all of them)
            between = {x.line for x in insts[i + 1:j]}
        assert (r.name, cons.line, prod.line) in scan_around(go2, cons.line, between)
        hits += 1
    assert hits == 2
