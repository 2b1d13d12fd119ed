"""Static check of the data hazards of a hipcc -S listing that the hardware does not interlock
(gfx950) and that hipcc pads in its own code only: an `asm` statement is one opaque instruction to
the compiler, so nothing inside it, or between two of them, is padded for it.

RULES below is the one table of producer -> consumer pairs and their wait states.  It is not taken
from a document: tests/hazard_probes.hip holds one asm-free kernel per pair, and
tests/test_hazard_rules.py compiles them and requires that the compiler's own padding equals the
table, counted by wait_states() below.  tools/gen_ipm_asm.py schedules by the same table.

The scan walks the whole listing, compiler code and asm alike.  For every instruction that reads a
register in a consumer role it walks back over at most the largest rule's wait states (s_nop N
counts N + 1, any other instruction 1) and reports a producer of the rule's class that wrote the
register too close.  At a label the walk goes on through every predecessor: the fall-through
(unless the instruction above is an unconditional branch or the end of the program) and every
branch that names the label; the worst path decides.  As the compiler's own recognizer does, the
walk does not stop at a later non-VALU write of the register.

Every mnemonic between ;;#ASMSTART and ;;#ASMEND has to fall into a class the table reasons about
(a plain or transcendental VALU op, a DPP op, a lane access, scalar, LDS or vector-memory
instructions, which produce and consume nothing in this table); any other is reported as
unclassified and fails the scan, so a new instruction in an asm string is never unchecked.

    python tools/check_dpp_hazards.py file.s      (exit status 1 on a hazard or an unclassified op)
"""
import collections
import re
import sys

Rule = collections.namedtuple("Rule", "name producer consumer waits")

# producer classes (what a VALU instruction writes):
#   valu_vgpr   any VALU write of a VGPR            trans_vgpr  a transcendental's VGPR result
#   valu_vcc    a VALU write of VCC                 valu_sgpr   a VALU write of another SGPR
#   valu_exec   a VALU write of EXEC
# consumer roles (how an instruction reads):
#   dpp_src     the DPP-shuffled source (src0) of a *_dpp instruction
#   lane_src    the VGPR source of v_readlane / v_readfirstlane
#   lane_sel    the SGPR lane select of v_readlane / v_writelane
#   valu_vcc / valu_sgpr   VCC / another SGPR read by a VALU instruction, as a wave mask, a carry
#               or a plain operand
#   valu_vgpr   a VGPR read by a VALU instruction that is not transcendental
#   dpp_exec / lane_exec   the EXEC every DPP instruction / lane access depends on
RULES = (
    Rule("VALU VGPR write -> DPP source", ("valu_vgpr",), "dpp_src", 2),
    Rule("VALU VCC write -> VALU VCC read", ("valu_vcc",), "valu_vcc", 2),
    Rule("VALU SGPR write -> VALU SGPR read", ("valu_sgpr",), "valu_sgpr", 2),
    Rule("trans VGPR write -> VALU VGPR read", ("trans_vgpr",), "valu_vgpr", 1),
    Rule("VALU VGPR write -> lane-access source", ("valu_vgpr",), "lane_src", 1),
    Rule("VALU SGPR write -> lane select", ("valu_sgpr", "valu_vcc"), "lane_sel", 4),
    # The compiler writes EXEC with scalar instructions only on this target (the probes show no
    # VALU write of it), so these two cannot be read off its output: they are the LLVM AMDGPU
    # hazard recognizer's published values, and the probe test fails if a VALU EXEC write appears.
    Rule("VALU EXEC write -> DPP", ("valu_exec",), "dpp_exec", 5),
    Rule("VALU EXEC write -> lane access", ("valu_exec",), "lane_exec", 4),
)
MAX_WAITS = max(r.waits for r in RULES)


def rule(consumer, producer=None):
    """the table's entry for a consumer role (the generator and the tests look rules up here)"""
    for r in RULES:
        if r.consumer == consumer and (producer is None or producer in r.producer):
            return r
    raise KeyError((consumer, producer))


TRANS = ("v_exp_", "v_log_", "v_rcp_", "v_rsq_", "v_sqrt_", "v_sin_", "v_cos_")
# VALU-encoded instructions with wait-state rules of their own that this table does not hold
UNMODELLED = ("v_mfma_", "v_smfmac_", "v_permlane", "v_swap_", "v_div_fmas_", "v_movrel",
              "v_accvgpr_", "v_interp_", "v_cvt_scale")
SDST = ("v_add_co_", "v_sub_co_", "v_subrev_co_", "v_addc_co_", "v_subb_co_", "v_subbrev_co_",
        "v_div_scale_", "v_mad_u64_u32", "v_mad_i64_i32")
CARRY_IN = ("v_addc_co_", "v_subb_co_", "v_subbrev_co_", "v_cndmask_")
ACCUM = ("v_fmac_", "v_mac_", "v_dot2c_", "v_dot4c_", "v_dot8c_", "v_pk_fmac_")
LANE = ("v_readlane_b32", "v_readfirstlane_b32", "v_writelane_b32")
ENDS = ("s_branch", "s_endpgm", "s_setpc_b64")
VCC, EXEC = (106, 107), (126, 127)

_TOK = re.compile(r"\b(?:([vsa])\[(\d+):(\d+)\]|([vsa])(\d+)\b|(vcc|exec)(_lo|_hi)?\b)")


def regs(text):
    """(VGPRs, SGPR-file registers) named in an operand's text; VCC and EXEC by their numbers"""
    v, s = set(), set()
    for m in _TOK.finditer(text):
        if m.group(1):
            (v if m.group(1) == "v" else s if m.group(1) == "s" else set()).update(
                range(int(m.group(2)), int(m.group(3)) + 1))
        elif m.group(4):
            (v if m.group(4) == "v" else s if m.group(4) == "s" else set()).add(int(m.group(5)))
        else:
            pair = VCC if m.group(6) == "vcc" else EXEC
            s.update(pair if not m.group(7) else pair[:1] if m.group(7) == "_lo" else pair[1:])
    return v, s


class Inst:
    """one instruction (or label) of the listing, with what it produces and consumes"""
    __slots__ = ("line", "text", "op", "ops", "label", "in_asm", "kind", "cost", "prod", "cons",
                 "target")

    def __init__(self, line, text, in_asm=False):
        self.line, self.text, self.in_asm = line, text, in_asm
        self.label = text[:-1] if text.endswith(":") else None
        parts = text.split(None, 1)
        self.op = "" if self.label else parts[0]
        self.ops = [o.strip() for o in parts[1].split(",")] if len(parts) > 1 else []
        self.prod, self.cons, self.target = {}, {}, None
        self.cost = 1
        self.kind = "label" if self.label else self._classify()

    def _classify(self):
        op, ops = self.op, self.ops
        if op == "s_nop":
            self.cost = int(ops[0], 0) + 1
            return "salu"
        if op.startswith("s_"):
            if op.startswith(("s_cbranch_", "s_branch")) and ops:
                self.target = ops[0]
            return "salu"
        if op.startswith("ds_"):
            return "lds"
        if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
            return "vmem"
        if not op.startswith("v_"):
            return "unknown"
        if op.startswith(UNMODELLED):
            # a VALU write all the same, so that the compiler's own pairs stay visible
            if ops and op.startswith(("v_accvgpr_read", "v_mfma_", "v_smfmac_")):
                self.prod["valu_vgpr"] = regs(ops[0])[0]
            return "unknown"
        if op == "v_nop":
            return "valu"
        self._valu()
        return "valu"

    def _valu(self):
        op, ops = self.op, self.ops
        trans = op.startswith(TRANS)
        dv, ds = regs(ops[0]) if ops else (set(), set())
        srcs = ops[1:]
        if op.startswith(SDST) and len(ops) > 1:
            sv, ss = regs(ops[1])
            if not sv and ss:            # the carry / scale flag out
                ds = ds | ss
                srcs = ops[2:]
            elif op.endswith("_e32"):    # VOP2 carry-out to an unnamed VCC
                ds = ds | set(VCC)
        if op.startswith("v_cmp") and not ds:
            ds = set(VCC)                # an _e32 compare without its VCC spelled out
        if op.startswith("v_cmpx"):
            ds = ds | set(EXEC)
        rv, rs = set(), set()
        for o in srcs:
            a, b = regs(o)
            rv |= a
            rs |= b
        if op.startswith(CARRY_IN) and len(ops) == 3 + (1 if op.startswith(SDST) else 0):
            rs |= set(VCC)               # VOP2 carry-in / select mask from an unnamed VCC
        if op.startswith(ACCUM):
            rv |= dv
        if dv:
            self.prod["valu_vgpr"] = dv
            if trans:
                self.prod["trans_vgpr"] = dv
        for name, pair in (("valu_vcc", VCC), ("valu_exec", EXEC)):
            if ds & set(pair):
                self.prod[name] = ds & set(pair)
        rest = ds - set(VCC) - set(EXEC)
        if rest:
            self.prod["valu_sgpr"] = rest
        dpp = "_dpp" in op
        if op in LANE:
            if op != "v_writelane_b32" and srcs:
                self.cons["lane_src"] = regs(srcs[0])[0]
            if op != "v_readfirstlane_b32" and len(srcs) > 1:
                self.cons["lane_sel"] = regs(srcs[1])[1]
            self.cons["lane_exec"] = set(EXEC)
        if dpp:
            if srcs:
                self.cons["dpp_src"] = regs(srcs[0].split()[0])[0]
            self.cons["dpp_exec"] = set(EXEC)
        if rs & set(VCC):
            self.cons["valu_vcc"] = rs & set(VCC)
        if rs - set(VCC) - set(EXEC):
            self.cons["valu_sgpr"] = rs - set(VCC) - set(EXEC)
        if rv and not trans:
            self.cons["valu_vgpr"] = rv
        self.cons = {k: v for k, v in self.cons.items() if v}


def parse(lines):
    """the listing's instructions and labels in order; directives and comments dropped"""
    insts, in_asm = [], False
    for n, l in enumerate(lines):
        if ";;#ASMSTART" in l:
            in_asm = True
        elif ";;#ASMEND" in l:
            in_asm = False
        t = l.split(";")[0].strip()
        if not t or t.startswith(".") and not re.match(r"^\.L\S*:$", t):
            continue
        insts.append(Inst(n + 1, t, in_asm))
    return insts


def wait_states(insts, i, j):
    """wait states between instruction i and the later instruction j on the straight line"""
    return sum(x.cost for x in insts[i + 1:j] if not x.label)


def pairs(insts, r, reach=None):
    """yields every (producer index, consumer index) of rule r on straight-line code: for each
    consumer the nearest earlier producer of the register, looked for up to the enclosing label
    or `reach` instructions back (the probe test measures the compiler's padding with this and
    wait_states)"""
    for j, c in enumerate(insts):
        res = c.cons.get(r.consumer)
        if not res:
            continue
        for i in range(j - 1, -1 if reach is None else max(-1, j - 1 - reach), -1):
            if insts[i].label:
                break
            if any(insts[i].prod.get(p, frozenset()) & res for p in r.producer):
                yield i, j
                break


def predecessors(insts):
    """label name -> indices of the branches that name it"""
    preds = collections.defaultdict(list)
    for i, x in enumerate(insts):
        if x.target:
            preds[x.target].append(i)
    return preds


def scan(insts):
    """-> (hazards, unclassified); a hazard is (rule, consumer Inst, producer Inst, wait states)"""
    preds = predecessors(insts)
    found = {}

    def walk(j, w, cons, needs, seen):
        # j: the next instruction to look at, going back; w: wait states between it and cons
        while j >= 0 and w < MAX_WAITS:
            x = insts[j]
            if x.label:
                if not x.label.startswith(".L"):
                    return                      # a function's entry: nothing before it
                for b in preds.get(x.label, ()):
                    if (b, w) not in seen:
                        seen.add((b, w))
                        walk(b, w, cons, needs, seen)
                if j and insts[j - 1].op in ENDS:
                    return
                j -= 1
                continue
            for r, res in needs:
                if w < r.waits and any(x.prod.get(p, frozenset()) & res for p in r.producer):
                    key = (r.name, cons.line)
                    if key not in found or found[key][3] > w:
                        found[key] = (r, cons, x, w)
            w += x.cost
            j -= 1

    for i, c in enumerate(insts):
        if not c.cons:
            continue
        needs = [(r, c.cons[r.consumer]) for r in RULES if r.consumer in c.cons]
        if needs:
            walk(i - 1, 0, c, needs, set())
    unclassified = [x for x in insts if x.in_asm and x.kind == "unknown"]
    return sorted(found.values(), key=lambda h: (h[1].line, h[0].name)), unclassified


def check(lines):
    return scan(parse(lines))


def main():
    lines = open(sys.argv[1]).read().split("\n")
    bad, unknown = check(lines)
    for r, c, p, w in bad:
        print(f"line {c.line}: {c.text}\n   <- line {p.line} ({w} wait states, {r.name} needs "
              f"{r.waits}): {p.text}")
    for x in unknown:
        print(f"line {x.line}: unclassified in asm: {x.text}")
    by = collections.Counter(r.name for r, _, _, _ in bad)
    for name, n in sorted(by.items()):
        print(f"  {n:6d}  {name}")
    print(f"{by[RULES[0].name]} DPP hazards")   # (the line of the one-rule checker, still read)
    print(f"{len(bad)} hazards, {len(unknown)} unclassified")
    sys.exit(1 if bad or unknown else 0)


if __name__ == "__main__":
    main()
