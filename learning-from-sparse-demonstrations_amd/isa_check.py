"""Build-time check of the gfx950 assembly hipcc produced for a model library (lfsd_amd.runtime.build_library).

What it looks for.  Round 6 found two builds of the wide OC kernel that were WRONG with sources the emulator, the sanitizers and
every other build of the same text agreed on (profiles/r06_f_wide_stale_cost.txt, r06_v_spill_before_exec_restore.txt):

    s_and_saveexec_b64 s[0:1], vcc        ; lanes b < n of a copy loop
    s_cbranch_execz .LBB4_487
    ...                                   ; the loop; exec shrinks as lanes finish
  .LBB4_487:                              ; JOIN block
    v_accvgpr_write_b32 a12, v10          ; <- the register allocator's spill of a value every lane needs later ...
    v_accvgpr_write_b32 a1, v178
    ...
    s_or_b64 exec, exec, s[0:1]           ; <- ... placed BEFORE the lanes are switched back on

The spill stores only the lanes that were active in the region; the others keep what the spill slot held before (here: the cost
of the previous iterate in every lane >= n -- a uniform value that later `v_cmp` + `s_cbranch_vccnz` pairs read from all lanes).
The compiler keeps such spills behind the exec restore unless the join block begins with SGPR-spill lane writes (`v_writelane`),
which both wrong builds had.  Nothing in the source is wrong and nothing in the source controls it; whether it happens changes with
any perturbation of the kernel (a printf, a clock read, another instruction scheduler).

So every build is scanned: in a block that is the target of an `s_cbranch_execz` (a join block) or that follows the back edge of a
divergent loop (`s_cbranch_execnz`: the loop's exit), between the label and the
`s_or_b64 exec, exec, ...` (or `s_or_saveexec` / `s_andn2_saveexec` / `s_xor_b64 exec`: the entry of an else-region) that re-enables lanes,
  * a VGPR spill store (`v_accvgpr_write_b32 aN, vM`, `scratch_store_* ; ... Folded Spill`) is a HAZARD;
  * a spill reload (`v_accvgpr_read_b32`, `scratch_load_* ; ... Folded Reload`) is a hazard when the reloaded register is read
    after the restore before it is written again (inactive lanes would read what the register held before).
`v_writelane_b32` / `v_readlane_b32` (SGPR spills) do not depend on exec and are fine there.

Pure text processing: no GPU, no toolchain.
"""
import re

_FUNC = re.compile(r"^([A-Za-z_][\w$.]*):")
_BLOCK = re.compile(r"^(\.LBB\d+_\d+):")
_EXECZ = re.compile(r"^\s+s_cbranch_execz\s+(\.LBB\d+_\d+)")
_EXECNZ = re.compile(r"^\s+s_cbranch_execnz\s+(\.LBB\d+_\d+)")
# what switches lanes back on at the top of a join block: the plain restore, and the entry of an else-region / of the next round of a
# waterfall (s_or_saveexec, s_andn2_saveexec, s_xor exec): a spill in front of any of them stores the lanes of the region just left
_RESTORE = re.compile(r"^(s_or_b64\s+exec,\s*exec,|s_or_saveexec_b64|s_andn2_saveexec_b64|s_xor_b64\s+exec,\s*exec,)")
_SPILL_STORE = re.compile(r"^(v_accvgpr_write_b32\s+a\d+,\s*v\d+|scratch_store_\w+\s.*Folded Spill)")
_SPILL_LOAD = re.compile(r"^(v_accvgpr_read_b32\s+(v\d+),\s*a\d+|scratch_load_(\w+)\s+(v\d+|v\[\d+:\d+\]),.*Folded Reload)")
_VREG = re.compile(r"\bv(\d+)\b|\bv\[(\d+):(\d+)\]")
_EXEC_WRITE = re.compile(r"^s_\w*saveexec|^s_\w+\s+exec\b|^s_mov_b64\s+exec|^s_cmov\w*\s+exec")


def _regs(text):
    out = set()
    for m in _VREG.finditer(text):
        if m.group(1) is not None:
            out.add(int(m.group(1)))
        else:
            out.update(range(int(m.group(2)), int(m.group(3)) + 1))
    return out


def _operands(instr):
    """(registers written, registers read) of a vector instruction line, by position: the first operand is the destination of
    every instruction this scan meets behind an exec restore (stores have none).  Conservative where it cannot tell."""
    body = instr.split(";")[0]
    parts = body.split(None, 1)
    if len(parts) < 2:
        return set(), set()
    op, args = parts
    ops = [a.strip() for a in args.split(",")]
    if op.startswith(("global_store", "scratch_store", "ds_write", "buffer_store", "flat_store", "s_")) or op.startswith("v_cmp") and not op.endswith("_e64"):
        return set(), _regs(args)
    # v_cmp*_e64 writes an SGPR pair; v_readlane writes an SGPR: the first operand holds no VGPR then
    if "mac" in op or op.startswith(("v_writelane", "v_dot", "v_mfma", "v_smfmac")):      # the destination is an operand too
        return _regs(ops[0]), _regs(args)
    return _regs(ops[0]), _regs(",".join(ops[1:]))


def find_exec_hazards(asm_text):
    """-> list of {"function", "block", "line", "kind": "spill"|"reload", "instr"} for the pattern in the module docstring."""
    lines = asm_text.split("\n")
    hazards = []
    func, targets = None, set()
    # execz targets per function (labels are unique per function: .LBB<function index>_<n>)
    for ln in lines:
        m = _EXECZ.match(ln)
        if m:
            targets.add(m.group(1))
    n = len(lines)
    for i, ln in enumerate(lines):
        m = _FUNC.match(ln)
        if m and not ln.startswith(".L"):
            func = m.group(1)
            continue
        m = _BLOCK.match(ln)
        if m and m.group(1) in targets:
            label = m.group(1)
        elif _EXECNZ.match(ln):      # the fall-through behind the back edge of a divergent loop is its exit whether or not a skip branch targets it
            label = "behind line %d" % (i + 1)
        else:
            continue
        j, stores, loads, restore_at = i + 1, [], [], -1
        while j < n and (not lines[j].strip() or lines[j].strip().startswith(";") or (label.startswith("behind") and _BLOCK.match(lines[j]))):
            if _BLOCK.match(lines[j]) and _BLOCK.match(lines[j]).group(1) in targets:
                break                # (that block is examined under its own label)
            j += 1
        if j < n and _BLOCK.match(lines[j]) and label.startswith("behind"):
            continue
        while j < n:
            t = lines[j].strip()
            if not t or t.startswith(";"):
                j += 1
                continue
            if t.startswith(".L") or t.startswith(("s_branch", "s_cbranch", "s_endpgm", "s_setpc")):
                break
            if _RESTORE.match(t):
                restore_at = j
                break
            if _EXEC_WRITE.match(t):
                break
            if _SPILL_STORE.match(t):
                stores.append((j + 1, t))
            else:
                ml = _SPILL_LOAD.match(t)
                if ml:
                    loads.append((j + 1, t, _regs(ml.group(2) or ml.group(4))))
            j += 1
        if restore_at < 0:
            continue
        for at, t in stores:
            hazards.append({"function": func, "block": label, "line": at, "kind": "spill", "instr": t})
        for at, t, regs in loads:
            # the reloaded registers: read behind the restore before they are written again?
            pending, k = set(regs), restore_at + 1
            bad = False
            while k < n and pending:
                u = lines[k].strip()
                if not u or u.startswith(";"):
                    k += 1
                    continue
                if u.startswith(".L") or u.startswith(("s_branch", "s_cbranch", "s_endpgm", "s_setpc")):
                    break
                w, r = _operands(u)
                if r & pending:
                    bad = True
                    break
                pending -= w
                k += 1
            if bad:
                hazards.append({"function": func, "block": label, "line": at, "kind": "reload", "instr": t})
    return hazards


# ---- wait states in front of DPP instructions -------------------------------------------------------------------------------------
# A DPP instruction reads its src0 from OTHER lanes, early in the pipeline.  gfx9 / CDNA wants
#   * 2 wait states between a vector instruction that writes the VGPR and the DPP instruction that reads it as src0,
#   * 5 wait states between a vector instruction that writes EXEC (v_cmpx*, v_readlane / v_readfirstlane into exec) and ANY DPP instruction,
# and, as for every vector instruction, a distance between a matrix instruction and a reader of its result (by the number of passes)
# and 1 wait state behind a transcendental one.  The compiler's hazard recognizer inserts s_nop for the DPP instructions it emits
# itself; it does NOT look into an `asm` statement (cpdp_common.h: fmac2_row_bcast writes v_fmac_f32_dpp by hand), and which
# instructions the register allocator and the scheduler put in front of the statement -- a v_accvgpr_read_b32 that brings the operand
# back from an AGPR, say -- is nothing the source controls.  A DPP instruction that comes too early reads the register's PREVIOUS
# value: wrong numbers, no fault.  So every `*_dpp` instruction of every build is examined, the compiler's own included (they must
# come out clean, which checks the scan), along every path that leads to it: a label's predecessors are the instruction in front
# of it and every branch to it.  An instruction is one wait state, `s_nop N` is N + 1; a taken branch counts as one like any other.
_DPP = re.compile(r"^(v_\w+_dpp)\s+(.*?)\s+(?:quad_perm:|row_\w+|wave_\w+|bank_mask:|bound_ctrl:|fi:)")
_LABEL = re.compile(r"^(\.L[\w$.]+):")
_BRANCH = re.compile(r"^s_c?branch\w*\s+(\.L[\w$.]+)")
_END = ("s_branch", "s_endpgm", "s_setpc_b64")      # nothing falls through these
_TRANS = ("v_exp_", "v_log_", "v_rcp_", "v_rsq_", "v_sqrt_", "v_sin_", "v_cos_")
_NOP = re.compile(r"^s_nop\s+(\d+)")
_MFMA_SHAPE = re.compile(r"_(\d+)x\d+x?\d*")
DPP_SRC0_WAIT, DPP_EXEC_WAIT, TRANS_WAIT = 2, 5, 1


def _mfma_wait(op):
    """wait states between a matrix instruction and a vector read of its result: 2 / 8 / 16 passes -> 5 / 11 / 19 (the larger figure
    where one tile edge comes with two pass counts)."""
    m = _MFMA_SHAPE.search(op)
    edge = int(m.group(1)) if m else 32
    return 5 if edge <= 4 else (11 if edge <= 16 else 19)


def _vector_writes(instr):
    """VGPRs a vector instruction writes (compares write SGPRs / EXEC; the swaps write both operands)."""
    parts = instr.split(";")[0].split(None, 1)
    if len(parts) < 2 or not parts[0].startswith("v_") or parts[0].startswith("v_cmp"):
        return set()
    ops = parts[1].split(",")
    if parts[0].startswith("v_swap") or (parts[0].startswith("v_permlane") and "swap" in parts[0]):
        return _regs(",".join(ops[:2]))
    return _regs(ops[0])


def _writes_exec_vector(instr):
    op = instr.split(None, 1)[0]
    return op.startswith("v_cmpx") or (op.startswith(("v_readlane", "v_readfirstlane")) and re.match(r"^\S+\s+exec", instr) is not None)


def find_dpp_hazards(asm_text):
    """-> list of {"function", "block", "line", "kind": "dpp-src0"|"dpp-exec"|"dpp-mfma"|"dpp-trans", "instr", "writer", "writer_line"}: DPP
    instructions with too few wait states behind a writer (see above)."""
    ins, line_of, func_of, labelled, first = [], [], [], [], set()      # instructions; per instruction: line, function, labels in front
    branches = {}                                                       # label -> instructions that branch to it
    func, pending, entry = None, [], True
    for i, ln in enumerate(asm_text.split("\n")):
        t = ln.strip()
        if not t or t.startswith(";"):
            continue
        m = _FUNC.match(ln)
        if m and not ln.startswith(".L"):
            func, pending, entry = m.group(1), [], True
            continue
        m = _LABEL.match(t)
        if m:
            pending.append(m.group(1))
            continue
        if t.startswith(".") or t.endswith(":"):      # directives
            continue
        t = t.split(";")[0].strip()
        if not t:
            continue
        k = len(ins)
        ins.append(t)
        line_of.append(i + 1)
        func_of.append(func)
        labelled.append(pending)
        if entry:
            first.add(k)
        pending, entry = [], False
        m = _BRANCH.match(t)
        if m:
            branches.setdefault(m.group(1), []).append(k)

    def preds(p):
        out = []
        if p not in first and p > 0 and not ins[p - 1].startswith(_END):
            out.append(p - 1)
        for lab in labelled[p]:
            out.extend(branches.get(lab, ()))
        return out

    def writer_within(d, window, is_writer):
        stack, seen = [(d, window)], {}
        while stack:
            p, w = stack.pop()
            for q in preds(p):
                if is_writer(ins[q]):
                    return q
                nop = _NOP.match(ins[q])
                w2 = w - (int(nop.group(1)) + 1 if nop else 1)
                if w2 > 0 and seen.get(q, 0) < w2:
                    seen[q] = w2
                    stack.append((q, w2))
        return None

    hazards = []
    for d, t in enumerate(ins):
        m = _DPP.match(t)
        if not m:
            continue
        ops = m.group(2).split(",")
        src0 = _regs(ops[1]) if len(ops) > 1 else set()
        reads = _regs(",".join(ops[1:])) | (_regs(ops[0]) if "mac" in m.group(1) else set())
        rules = [("dpp-src0", DPP_SRC0_WAIT, lambda u: bool(_vector_writes(u) & src0)),
                 ("dpp-exec", DPP_EXEC_WAIT, _writes_exec_vector),
                 ("dpp-trans", TRANS_WAIT, lambda u: u.startswith(_TRANS) and bool(_vector_writes(u) & reads))]
        for edge_wait in (5, 11, 19):
            rules.append(("dpp-mfma", edge_wait, lambda u, e=edge_wait: u.startswith(("v_mfma", "v_smfmac")) and _mfma_wait(u.split(None, 1)[0]) >= e
                          and bool(_vector_writes(u) & reads)))
        for kind, window, is_writer in rules:
            q = writer_within(d, window, is_writer)
            if q is not None:
                hazards.append({"function": func_of[d], "block": (labelled[d] or ["line %d" % line_of[d]])[0], "line": line_of[d], "kind": kind,
                                "instr": t, "writer": ins[q], "writer_line": line_of[q]})
                break
    return hazards


def find_hazards(asm_text):
    """Everything a build is rejected for."""
    return find_exec_hazards(asm_text) + find_dpp_hazards(asm_text)


def summary(asm_text):
    """Counts for the build record: functions, join blocks examined."""
    targets = set(m.group(1) for m in (_EXECZ.match(ln) for ln in asm_text.split("\n")) if m)
    nfunc = sum(1 for ln in asm_text.split("\n") if ln.startswith(".Lfunc_end"))
    return {"functions": nfunc, "join_blocks": len(targets)}


def dpp_count(asm_text):
    """DPP instructions find_dpp_hazards examines (for the build record)."""
    return sum(1 for ln in asm_text.split("\n") if _DPP.match(ln.strip()))
