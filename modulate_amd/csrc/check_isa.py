#!/usr/bin/env python3
""" -- build-time guard over the gfx950 assembly of the kernel TUs (run by the Makefile right after a TU is
compiled to assembly and before its object exists; the TUs' CPU test files run it again and feed it deliberately broken builds).

The streaming kernels' keystream is one hand-scheduled assembly block per 16-byte word (cycle_kernel_impl.h,
ks_word_carry) that works in FIXED registers, v[120:127] and s[94:95], which the kernels keep out of the register
allocator's reach with amdgpu_num_vgpr(120) / amdgpu_num_sgpr(94).  Whether a compiler honours that is visible only in
its output, so the output is what is checked:
  * nothing outside the blocks touches the fixed registers, and no operand the compiler chose for a block lies in them
    (round 3: as plain clobbers the allocator handed them to inputs of the block -- wrong keystream, no error);
  * every block ends with the s_nop 0 that covers the SDWA dst_sel forwarding hazard towards the compiler's next instruction;
  * register counts stay inside the budget, nothing spills, no scratch;
  * what each TU needs beyond that -- the form of its atomics, its cache policies, its barriers -- is in the table of TUs below
    (TUS), one entry per TU, each rule once (the functions above the table), the reason for a rule or a parameter next to it.
For EVERY kernel of every TU, whatever its arithmetic (round 6):
  * no instruction directly behind an SDWA write with dst_sel BYTE_n / WORD_n reads the register that write touched (gfx940+:
    such a partial write needs one wait state before a VALU reads the register; LLVM's hazard recognizer does not look into
    inline assembly, and the small shape's put_byte is one such instruction per asm statement -- whether something else ended up
    between two of them was the instruction scheduler's habit, now it is a rule);
  * every s_barrier is reached with the EXEC mask the wave had when it entered the kernel: the kernel's control flow is
    followed with a stack of the masks saved by s_*_saveexec / narrowed by s_andn2 exec, and the stack must be EMPTY at a
    barrier on every path.  (The host-fed kernel's lab form hung a workgroup because lanes 1..63 of one wave went round the
    trip loop's back edge without lane 0 and met the barrier a second time; tools/archive/ubench_pcie_persist.hip.)
Exit status 0 = all of it holds; 1 = findings on stdout."""
import re
import sys
from collections import namedtuple

BLOCK = re.compile(r";;#ASMSTART\n(.*?);;#ASMEND", re.S)


def kernel_bodies(asm):
    """mangled name -> text from its label to its s_endpgm -- the LAST one of the function: a kernel with an early way out (the
    out-of-place kernel's digest loop returns before the stream loop) has one s_endpgm per exit, and the rules are for all of its loops"""
    out = {}
    for m in re.finditer(r"^(_Z\d+modgpu_cycle_\w+):", asm, re.M):
        end = re.compile(r"^\.Lfunc_end\d+:", re.M).search(asm, m.end())
        out[m.group(1)] = asm[m.end():asm.rindex("s_endpgm", m.end(), end.start() if end else len(asm))]
    return out


def kernel_texts(asm):
    """mangled name -> ALL of the kernel's text (a kernel may place blocks behind its first s_endpgm): up to its .Lfunc_end label"""
    out = {}
    for m in re.finditer(r"^(_Z\d+modgpu_cycle_\w+):", asm, re.M):
        end = re.compile(r"^\.Lfunc_end\d+:", re.M).search(asm, m.end())
        out[m.group(1)] = asm[m.end():end.start() if end else len(asm)]
    return out


def metadata(asm, name):
    """the scalar fields of one kernel's record in amdhsa.kernels (a record starts at "  - .agpr_count")"""
    meta = asm[asm.index("amdhsa.kernels"):]
    at = meta.index(".name:           " + name + "\n")
    start = meta.rfind("  - .agpr_count", 0, at)
    end = meta.find("  - .agpr_count", at)
    rec = meta[start:end if end > 0 else len(meta)]
    return {k: int(v) for k, v in re.findall(r"^\s+(?:- )?\.(\w+):\s+(\d+)\s*$", rec, re.M) if k not in ("offset", "size")}


def source_name(mangled):
    """_Z<length><name><template arguments, parameter types> -> (the kernel's name in the source, the rest)"""
    m = re.match(r"_Z(\d+)", mangled)
    end = m.end() + int(m.group(1))
    return mangled[m.end():end], mangled[end:]


# ---- rules for every kernel ------------------------------------------------------------------------------------------------------
INSN = re.compile(r"^\s+([a-z_0-9]+)\b(.*)$")


def instructions(fn):
    """[(label or None, mnemonic, operand text)] of a kernel body in text order; labels are attached to the instruction they precede"""
    out, pending = [], []
    for ln in fn.splitlines():
        code = ln.split(";")[0].rstrip()
        if not code.strip():
            continue
        m = re.match(r"^\s*(\.?[A-Za-z_][\w.$]*):", code)
        if m:
            pending.append(m.group(1))
            continue
        m = INSN.match(code)
        if not m or m.group(1).startswith("."):
            continue
        out.append((tuple(pending), m.group(1), m.group(2).strip()))
        pending = []
    return out


def vgprs(text):
    """the VGPR numbers an operand text names: v7, v[4:7]"""
    regs = set()
    for a, b in re.findall(r"\bv\[(\d+):(\d+)\]", text):
        regs.update(range(int(a), int(b) + 1))
    regs.update(int(x) for x in re.findall(r"\bv(\d+)\b", text))
    return regs


def sdwa_forwarding_hazards(name, fn):
    """gfx940+ hasDstSelForwardingHazard: one wait state between an SDWA write of part of a VGPR and a read of that VGPR"""
    bad = []
    ins = instructions(fn)
    for k, (_, op, args) in enumerate(ins[:-1]):
        m = re.search(r"dst_sel:(BYTE|WORD)_\d", args)
        if not op.endswith("_sdwa") or not m:
            continue
        dst = vgprs(args.split(",")[0])
        _, nop, nargs = ins[k + 1]
        if nop in ("s_nop", "s_waitcnt", "s_sleep") or nop.startswith("s_"):
            continue  # any instruction in between is the wait state
        operands = [a.strip() for a in nargs.split(",")]
        reads = set()
        for i, a in enumerate(operands):
            # operand 0 of a VALU / load is written, not read -- unless the instruction keeps the rest of it (SDWA UNUSED_PRESERVE)
            # or it is a store / atomic, whose operands are all read
            writes_op0 = i == 0 and not ("UNUSED_PRESERVE" in nargs) and not re.match(r"(buffer|global|flat|ds)_(store|write|atomic)", nop)
            if not writes_op0:
                reads |= vgprs(a)
        if dst & reads:
            bad.append("%s: %s reads v%d directly behind the SDWA partial write `%s %s` (dst_sel forwarding hazard: one wait state needed)"
                       % (name, nop, min(dst & reads), op, args.split(" dst_sel")[0]))
    return bad


def barriers_at_full_exec(name, fn):
    """follows the control flow with a stack of saved EXEC masks; every s_barrier must be reached with the stack empty"""
    ins = instructions(fn)
    at = {}
    for k, (labels, _, _) in enumerate(ins):
        for lb in labels:
            at[lb] = k
    bad, seen, work = [], set(), [(0, ())]
    while work:
        k, stack = work.pop()
        while k < len(ins) and (k, stack) not in seen:
            seen.add((k, stack))
            _, op, args = ins[k]
            ops = [a.strip() for a in args.split(",")]
            if re.match(r"s_\w+_saveexec_b64", op):
                if ops[0] not in stack:
                    stack = stack + (ops[0],)
            elif op == "s_andn2_b64" and ops[0] == "exec" and ops[1] == "exec":  # a loop's lanes leaving one by one
                if ops[2] not in stack:
                    stack = stack + (ops[2],)
            elif op == "s_or_b64" and ops[0] == "exec" and ops[1] == "exec":  # back to the mask saved in ops[2] (and out of everything nested inside)
                if ops[2] in stack:
                    stack = stack[:stack.index(ops[2])]
            elif op in ("s_mov_b64", "s_and_b64", "s_andn2_b64", "s_xor_b64", "s_or_b64") and ops[0] == "exec" and not stack:
                if not (op == "s_xor_b64" and len(ops) == 3):
                    bad.append("%s: EXEC is rewritten outside any saved-mask region: %s %s" % (name, op, args))
            elif op == "s_barrier" and stack:
                bad.append("%s: an s_barrier can be reached with part of the wave masked off (saved masks on the way: %s)" % (name, ", ".join(stack)))
            if op == "s_endpgm":
                break
            if op == "s_branch":
                k = at[ops[0]]
                continue
            if op.startswith("s_cbranch_"):
                work.append((at[ops[0]], stack))
            k += 1
    return sorted(set(bad))


# ---- the rules of the TUs, each once.  A kernel rule takes a Kernel (and the parameters its entry in TUS gives it) and returns its
# findings; `name` is what the findings call the kernel (its mangled name), `source` its name in the source, `fn` its body up to
# s_endpgm, `md` its metadata record. ----
Kernel = namedtuple("Kernel", "name source fn md")


def code_lines(fn, mnemonic):
    """the instructions of a body whose mnemonic starts with `mnemonic`, without their comments"""
    return [ln.split(";")[0].rstrip() for ln in fn.splitlines() if re.match(r"\s+" + mnemonic, ln)]


def register_budget(k, vgprs=128, who=""):
    """128 VGPRs / 102 SGPRs: 4 waves per SIMD and the keystream blocks' fixed registers above the allocator's.  64 VGPRs for a kernel
    that lives on occupancy (512 per SIMD lane / 8 waves); `who` is how its finding begins"""
    if vgprs == 128:
        if k.md.get("vgpr_count", 999) > 128 or k.md.get("sgpr_count", 999) > 102:
            return ["%s: register counts beyond the budget: %s" % (k.name, k.md)]
    elif k.md.get("vgpr_count", 999) > vgprs:
        return ["%s: %s%d VGPRs -- more than %d, fewer than %d waves per SIMD" % (k.name, who, k.md.get("vgpr_count", 999), vgprs, 512 // vgprs)]
    return []


def no_spills(k, apart=False):
    """no spills, no scratch instruction, no private segment (`apart`: the main TU's wording, scratch reported on its own)"""
    spills = k.md.get("vgpr_spill_count", 0) or k.md.get("sgpr_spill_count", 0) or k.md.get("private_segment_fixed_size", 0)
    scratch = "scratch_" in k.fn
    if apart:
        return (["%s: spills or a private segment: %s" % (k.name, k.md)] if spills else []) + (["%s: scratch instructions" % k.name] if scratch else [])
    return ["%s: spills, scratch or a private segment: %s" % (k.name, k.md)] if spills or scratch else []


def atomic_optimizer_off(k, what):
    """LLVM's atomic optimizer turns an atomic into a wave-aggregated one (v_mbcnt ...) followed at once by s_waitcnt vmcnt(0); `what` it
    would have rewritten: a ticket fetch must stay ONE plain returning atomic whose value is waited for a trip later"""
    if "v_mbcnt" in k.fn:
        return ["%s: the atomic optimizer rewrote %s (build the TU with -mllvm -amdgpu-atomic-optimizer-strategy=None)" % (k.name, what)]
    return []


# a block family: its words in findings, its fixed registers, the block's own uses of them, its instruction mix
Blocks = namedtuple("Blocks", "a outside operand fixed own mads addc")
KEYSTREAM = Blocks("keystream", "a fixed temporary is touched OUTSIDE the keystream blocks", "the compiler gave a block operand a fixed temporary",
                   re.compile(r"\bv12[0-7]\b|v\[\d+:12[0-7]\]|\bs9[45]\b|s\[\d+:9[45]\]"),
                   re.compile(r"v\[12[0246]:12[1357]\]|s\[94:95\]|\bv12[0246]\b|\bv127\b"), 30, 15)
# cycle_rekey_impl.h, ks_word2_carry: both streams' words in one block, fixed temporaries v[112:127] and s[94:95]
TWO_KEYSTREAM = Blocks("two-keystream", "a fixed temporary of the two-keystream block is touched OUTSIDE the blocks",
                       "the compiler gave a two-keystream block operand a fixed temporary",
                       re.compile(r"\bv11[2-9]\b|\bv12[0-7]\b|v\[\d+:(?:11[2-9]|12[0-7])\]|\bs9[45]\b|s\[\d+:9[45]\]"),
                       re.compile(r"v\[(?:11[2468]|12[0246]):(?:11[3579]|12[1357])\]|s\[94:95\]|\bv(?:11[2468]|12[0246])\b|\bv12[57]\b"), 60, 30)


def carry_blocks(fn):
    return [b for b in BLOCK.findall(fn) if "s[94:95]" in b]


def block_discipline(k, family):
    """the fixed-temporary discipline, the trailing s_nop 0 and the instruction mix of every block of the kernel"""
    bad = []
    for ln in BLOCK.sub("", k.fn).splitlines():
        if family.fixed.search(ln) and not ln.strip().startswith(";"):
            bad.append("%s: %s: %s" % (k.name, family.outside, ln.strip()))
    for b in carry_blocks(k.fn):
        lines = [ln for ln in b.splitlines() if ln.strip()]
        for ln in lines:
            if family.fixed.search(family.own.sub("", ln)):
                bad.append("%s: %s: %s" % (k.name, family.operand, ln.strip()))
        if not lines or lines[-1].split(";")[0].strip() != "s_nop 0":
            bad.append("%s: a %s block does not end with s_nop 0 (dst_sel forwarding hazard)" % (k.name, family.a))
        if len([ln for ln in lines if "v_addc_co_u32_sdwa" in ln]) != family.addc or len([ln for ln in lines if "v_mad_u64_u32" in ln]) != family.mads:
            bad.append("%s: a %s block is not %d mads + %d addc" % (k.name, family.a, family.mads, family.addc))
    return bad


def keystream_blocks(k, required=True):
    """ks_word_carry's blocks (30 mads + 15 addc).  A kernel without the block may use any register; `required`: it must carry one"""
    if not carry_blocks(k.fn):
        return ["%s: no keystream block (ks_word_carry)" % k.name] if required else []
    return block_discipline(k, KEYSTREAM)


def rekey_blocks(k):
    """ks_word2_carry's blocks (60 mads + 30 addc), and one three-input XOR (v_bitop3_b32 bitop3:0x96; gfx950 has no v_xor3_b32) per
    dword of every block"""
    blocks = carry_blocks(k.fn)
    if not blocks:
        return ["%s: no two-keystream block (ks_word2_carry)" % k.name]
    bad = block_discipline(k, TWO_KEYSTREAM)
    xor3 = len(re.findall(r"v_bitop3_b32 .*bitop3:0x96", k.fn))
    if xor3 != 4 * len(blocks):
        bad.append("%s: %d three-input XORs (v_bitop3_b32 0x96) for %d two-keystream blocks, expected one per dword (4 per block)" % (k.name, xor3, len(blocks)))
    return bad


def move_loop(k):
    """the rekey kernel's second loop (cycle_rekey_kernel.h: a destination that partly overlaps its source).  Per unrolled trip (2): a
    barrier behind the chunk's blocks, thread 0's poll of the other chunks' flags, a barrier in front of the stores -- with the stream
    loop's 4 and the one behind each of the first two tickets, 12 s_barrier.  In front of the first of them every wave waits, in an asm
    statement of its own, until the chunk's loads have returned: the flag must not go up before.  The poll sleeps between reads (s_sleep) and is bounded by the
    constant-rate clock (s_memrealtime: one stamp where it starts, one per round); flags are read and written at agent scope (sc1)
    and NOTHING is fenced: a release or acquire there (buffer_wbl2 / buffer_inv) would drain the loads of the next chunk -- the hazard
    is write-after-read, the flag speaks for loads that have returned.  Both loops' ticket fetches are plain returning atomics: the
    stream loop's 2, the move loop's 2 and the two that draw its first positions a barrier apart (+ the exit count = 7)."""
    bad = []
    counts = {m: len(code_lines(k.fn, m)) for m in ("s_barrier", "s_sleep", "s_memrealtime", "buffer_wbl2", "buffer_inv", "global_atomic_add", "global_atomic_cmpswap")}
    if counts["s_barrier"] != 12:
        bad.append("%s: %d s_barrier, expected 12 (stream loop 4, move loop 2 + 2 x 3)" % (k.name, counts["s_barrier"]))
    if counts["s_sleep"] != 2 or counts["s_memrealtime"] != 4:
        bad.append("%s: the move loop's poll is not a sleeping, clock-bounded one (%d s_sleep, %d s_memrealtime; expected 2 and 4)"
                   % (k.name, counts["s_sleep"], counts["s_memrealtime"]))
    if counts["buffer_wbl2"] or counts["buffer_inv"]:
        bad.append("%s: a cache write-back or invalidate inside the kernel (the move loop's flags need no fence)" % k.name)
    # the explicit wait for the chunk's loads: one asm statement per unrolled trip, s_waitcnt vmcnt(the next chunk's loads: 4 words, twice
    # that through the funnel <..., true>), and between it and the next s_barrier no store and no flag access
    waits = [m for m in BLOCK.finditer(k.fn) if re.fullmatch(r"\s*s_waitcnt vmcnt\([1-9]\d*\)\s*", m.group(1))]  # (vmcnt(0): the exit's)
    ahead = 8 if "ELb1EEv" in k.name else 4
    if len(waits) != 2 or any(m.group(1).strip() != "s_waitcnt vmcnt(%d)" % ahead for m in waits):
        bad.append("%s: the move loop's wait for the chunk's loads is not one `s_waitcnt vmcnt(%d)` per unrolled trip (found %s)"
                   % (k.name, ahead, [m.group(1).strip() for m in waits]))
    for m in waits:
        upto = k.fn.find("s_barrier", m.end())
        if upto < 0 or re.search(r"^\s+(buffer_store|global_store|global_load|global_atomic)", k.fn[m.end():upto], re.M):
            bad.append("%s: a store or a flag access lies between the wait for the chunk's loads and the barrier behind it" % k.name)
    polls = code_lines(k.fn, "global_load_dword v")
    flags = [ln for ln in polls if ln.endswith(" sc1")]
    if len(flags) != 4:
        bad.append("%s: %d agent-scope flag reads (global_load_dword ... sc1), expected 4 (first look + poll, per unrolled trip)" % (k.name, len(flags)))
    ups = [ln for ln in code_lines(k.fn, "global_store_dword v") if ln.endswith(" sc1") and " sc0" not in ln]
    if len(ups) != 4:
        bad.append("%s: %d agent-scope dword stores, expected 4 (a flag per unrolled trip + the pair's reset)" % (k.name, len(ups)))
    if counts["global_atomic_add"] != 7 or counts["global_atomic_cmpswap"] != 2:
        bad.append("%s: %d global_atomic_add and %d global_atomic_cmpswap, expected 7 (tickets 2 + 2 + 2, the exit count) and 2 (the status word)"
                   % (k.name, counts["global_atomic_add"], counts["global_atomic_cmpswap"]))
    return bad


def table_move_loop(k):
    """the move kernel of the rekey move table call (cycle_rekey_move_table_kernel.h): the rekey kernel's move loop per chunk of a table.
    Per unrolled trip (2): the barrier at its top, a barrier behind the chunk's blocks, thread 0's poll of the flags of the chunk's
    window, a barrier in front of the stores -- with the one behind each of the first two tickets, 8 s_barrier.  In front of the barrier
    behind the blocks every wave waits, in an asm statement of its own, until the chunk's loads have returned: vmcnt(4) when the next
    chunk's loads are 4 words, vmcnt(8) when they took the funnel's extra dwords -- one of each per trip, a uniform branch apart.  The
    poll sleeps between reads and is bounded by the constant-rate clock; flags are read and written at agent scope (sc1) and NOTHING is
    fenced.  Tickets are plain returning atomics: one per trip and the two that draw the first positions a barrier apart.  A chunk's
    entry and its window come through scalar loads: the only vector loads besides the data are the flag reads and the lane's two
    start-up table lookups."""
    bad = []
    counts = {m: len(code_lines(k.fn, m)) for m in ("s_barrier", "s_sleep", "s_memrealtime", "buffer_wbl2", "buffer_inv", "global_atomic_add", "global_atomic_cmpswap")}
    if counts["s_barrier"] != 8:
        bad.append("%s: %d s_barrier, expected 8 (2 x 3 in the loop, one behind each of the first two tickets)" % (k.name, counts["s_barrier"]))
    if counts["s_sleep"] != 2 or counts["s_memrealtime"] != 4:
        bad.append("%s: the poll is not a sleeping, clock-bounded one (%d s_sleep, %d s_memrealtime; expected 2 and 4)"
                   % (k.name, counts["s_sleep"], counts["s_memrealtime"]))
    if counts["buffer_wbl2"] or counts["buffer_inv"]:
        bad.append("%s: a cache write-back or invalidate inside the kernel (the flags need no fence)" % k.name)
    waits = [m for m in BLOCK.finditer(k.fn) if re.fullmatch(r"\s*s_waitcnt vmcnt\([1-9]\d*\)\s*", m.group(1))]
    if sorted(m.group(1).strip() for m in waits) != ["s_waitcnt vmcnt(4)"] * 2 + ["s_waitcnt vmcnt(8)"] * 2:
        bad.append("%s: the wait for the chunk's loads is not one `s_waitcnt vmcnt(4)` and one `s_waitcnt vmcnt(8)` per unrolled trip (found %s)"
                   % (k.name, [m.group(1).strip() for m in waits]))
    for m in waits:
        upto = k.fn.find("s_barrier", m.end())
        if upto < 0 or re.search(r"^\s+(buffer_store|global_store|global_load|global_atomic)", k.fn[m.end():upto], re.M):
            bad.append("%s: a store or a flag access lies between the wait for the chunk's loads and the barrier behind it" % k.name)
    vec = code_lines(k.fn, "(?:global|flat)_load")
    flags = [ln for ln in vec if re.match(r"\s+global_load_dword v", ln) and ln.endswith(" sc1")]
    if len(flags) != 4 or len(vec) - len(flags) > 2 or k.fn.count("s_load_dwordx16") < 2:
        bad.append("%s: %d agent-scope flag reads (expected 4: first look + poll, per unrolled trip), %d other vector loads besides the data "
                   "(at most the 2 start-up lookups), %d s_load_dwordx16 (the entry search is scalar)" % (k.name, len(flags), len(vec) - len(flags), k.fn.count("s_load_dwordx16")))
    ups = [ln for ln in code_lines(k.fn, "global_store_dword v") if ln.endswith(" sc1") and " sc0" not in ln]
    if len(ups) != 2 or len(code_lines(k.fn, "global_store")) != 2:
        bad.append("%s: %d agent-scope dword stores among %d global stores, expected 2 and 2 (a flag per unrolled trip)" % (k.name, len(ups), len(code_lines(k.fn, "global_store"))))
    fetches = code_lines(k.fn, "global_atomic_add")
    if len(fetches) != 4 or not all(ln.endswith(" sc0") for ln in fetches) or counts["global_atomic_cmpswap"] != 2:
        bad.append("%s: %d global_atomic_add (expected 4 returning ones: tickets 2 + 2) and %d global_atomic_cmpswap (expected 2: the status word)"
                   % (k.name, len(fetches), counts["global_atomic_cmpswap"]))
    return bad


def block_count(k, family, expected, made_of):
    blocks = len(carry_blocks(k.fn))
    return ["%s: %d %s blocks, expected %d (%s)" % (k.name, blocks, family.a, expected, made_of)] if blocks != expected else []


def no_block(k, who):
    return ["%s: %s carries a keystream block" % (k.name, who)] if carry_blocks(k.fn) else []


def loads_nt(k):
    """every chunk is read once: data loads (the buffer loads) are non-temporal"""
    loads = code_lines(k.fn, "buffer_load_dword")
    return [] if loads and all(ln.endswith(" nt") for ln in loads) else ["%s: a data load is not nt" % k.name]


def stores(k, policy, what="a data store"):
    """data stores (the buffer stores) by cache policy: "nt sc1" into HBM, "sc1" without nt across PCIe (nt measured 15-20 % slower there)"""
    lines = code_lines(k.fn, "buffer_store_dword")
    if policy == "nt sc1":
        return [] if lines and all(ln.endswith(" nt sc1") for ln in lines) else ["%s: %s is not nt sc1" % (k.name, what)]
    if lines and all(ln.endswith(" sc1") and " nt" not in ln for ln in lines):
        return []
    return ["%s: %s is not `sc1` without nt (nt stores across PCIe: -15..20 %%)" % (k.name, what)]


def stores_nt_sc1_at_least(k, n):
    return ["%s: fewer than %d nt sc1 stores" % (k.name, n)] if len([ln for ln in code_lines(k.fn, "buffer_store_dword") if ln.endswith("nt sc1")]) < n else []


def keep_store_bursts(k):
    """the keep kernel's two bursts in the unrolled stream loop: as many `sc1`-only stores (the resident chunks') as `nt sc1` stores (the
    streaming chunks'), 4 words x 2 trips each; the cut first chunk's loop (cold, not unrolled) stores once, streaming"""
    lines = code_lines(k.fn, "buffer_store_dword")
    streaming = len([ln for ln in lines if ln.endswith(" nt sc1")])
    resident = len([ln for ln in lines if ln.endswith(" sc1") and " nt" not in ln])
    bad = []
    if streaming + resident != len(lines):
        bad.append("%s: a data store is neither nt sc1 nor sc1" % k.name)
    if resident != 8 or streaming - 1 != 8:
        bad.append("%s: %d sc1-only and %d nt sc1 stores in the stream loop, expected 8 of each (4 words x 2 unrolled trips, one burst per "
                   "cache policy)" % (k.name, resident, streaming - 1))
    return bad


def scalar_entry_search(k):
    """a table call's stream kernel finds a chunk's entry with scalar loads only (s_load_dwordx16 of the search levels and of the entry's
    plan; no vector load besides the lane's two start-up table lookups): a vector-memory search would wait for the chunk loads in flight"""
    vec = len(re.findall(r"^\s+(?:global|flat)_load", k.fn, re.M))
    if k.fn.count("s_load_dwordx16") < 2 or vec > 2:
        return ["%s: the entry search is not scalar (%d s_load_dwordx16, %d vector loads besides the data)" % (k.name, k.fn.count("s_load_dwordx16"), vec)]
    return []


def read_only_stream(k, who, no_store_at_all=False):
    """a verify kernel reads its inputs and nothing else: no buffer store or atomic, no flat access.  `no_store_at_all`: the table forms
    write through atomics and into their LDS mailbox only, so no store instruction of any kind"""
    bad = []
    if no_store_at_all:
        if re.search(r"^\s+(buffer|global|flat|scratch)_store", k.fn, re.M):
            bad.append("%s: %s stores through a buffer descriptor or a pointer (its inputs are read-only; the stream has no store at all)" % (k.name, who))
        if re.search(r"^\s+(buffer|flat)_atomic", k.fn, re.M) or re.search(r"^\s+flat_", k.fn, re.M):
            bad.append("%s: buffer atomics or flat_ accesses (LDS must be ds_ instructions, results global_ atomics)" % k.name)
        return bad
    if re.search(r"^\s+buffer_(store|atomic)", k.fn, re.M):
        bad.append("%s: %s stores through a buffer descriptor (its inputs are read-only; the stream has no store at all)" % (k.name, who))
    if re.search(r"^\s+flat_", k.fn, re.M):
        bad.append("%s: flat_ accesses (LDS must be ds_ instructions, results global_)" % k.name)
    return bad


def one_global_store(k):
    found = re.findall(r"^\s+(global_store_\w+)", k.fn, re.M)
    return ["%s: global stores %s, expected the one global_store_dwordx2 of the entry's n" % (k.name, found)] if found != ["global_store_dwordx2"] else []


def result_atomics(k, tickets=0, sums=0):
    """a verify kernel's results: 64-bit adds (the count) and unsigned mins (the lowest index), as many of the one as of the other, and
    nothing else.  `tickets`: the returning 32-bit ticket fetches that come on top (one per unrolled trip of each loop), the results then
    not returning.  `sums`: the 64-bit adds of a digest loop in the same kernel (digest_table_loop), which have no min beside them"""
    bad = []
    atomics = [(m.group(1), m.group(2)) for m in re.finditer(r"^\s+(global_atomic_\w+)\b([^;\n]*)", k.fn, re.M)]
    if tickets:
        fetches = [args for op, args in atomics if op == "global_atomic_add"]
        if len(fetches) != tickets or not all(args.rstrip().endswith(" sc0") for args in fetches):
            bad.append("%s: %d 32-bit global_atomic_add, expected the ticket fetch of each unrolled trip (%d), each returning (sc0)" % (k.name, len(fetches), tickets))
        atomics = [(op, args) for op, args in atomics if op != "global_atomic_add"]
    ops = [op for op, _ in atomics]
    adds, mins = ops.count("global_atomic_add_x2") - sums, ops.count("global_atomic_umin_x2")
    if adds <= 0 or adds != mins or adds + sums + mins != len(ops) or (tickets and any(" sc0" in args for _, args in atomics)):
        bad.append("%s: result atomics %s, expected %s64-bit adds and unsigned mins in equal numbers%s and nothing else"
                   % (k.name, sorted(set(ops)), "non-returning " if tickets else "", " (beside the digest loop's %d adds)" % sums if sums else ""))
    return bad


def digest_table_loop(k):
    """the verify table kernel's second loop (cycle_verify_table_kernel.h: VERIFY_TABLE_DIGEST, one uniform branch apart from the
    compare).  It reads one side and sends a pair of 64-bit atomic adds onto the entry's record when its workgroup leaves the entry:
    the sums are taken with v_dot4_u32_u8, no 64-bit atomic of the kernel returns a value (the loop would wait for it), the fold that
    precedes them goes through LDS (ds_add_u32) and not through memory, and the kernel still has no store of any kind -- a digest
    that wrote anywhere but into its records would write into what it reads"""
    bad = []
    if "v_dot4_u32_u8" not in k.fn:
        bad.append("%s: no v_dot4_u32_u8 (the digest loop's byte and position sums)" % k.name)
    wide = [(m.group(1), m.group(2)) for m in re.finditer(r"^\s+(global_atomic_\w+_x2)\b([^;\n]*)", k.fn, re.M)]
    if any(" sc0" in args for _, args in wide):
        bad.append("%s: a 64-bit atomic returns its value (sc0): the digest loop's sums are non-returning global_atomic_add_x2" % k.name)
    if not code_lines(k.fn, "ds_add_u32"):
        bad.append("%s: no ds_add_u32 (the digest loop folds a workgroup's sums in LDS, one pair per wave)" % k.name)
    if re.search(r"^\s+(buffer|global|flat|scratch)_store", k.fn, re.M):
        bad.append("%s: a store in the kernel of the digest loop (it sends 64-bit atomic adds to the records and nothing else)" % k.name)
    return bad


def cycle_digest_table_loop(k, loop="cycle digest"):
    """the out-of-place table kernel's second loop (cycle_table_kernel.h: CYCLE_TABLE_DIGEST, one uniform branch apart from the plain
    loop).  It cycles as the plain loop does and sums what it stores, or what it read: the sums are taken with v_dot4_u32_u8; every
    64-bit atomic of the kernel is a non-returning add (the pair per unrolled trip that goes onto the entry's record: 4; the loop would
    wait for a value that came back); the fold that precedes them goes through LDS (ds_add_u32) and not through memory; both loops
    draw one plain returning 32-bit ticket per unrolled trip (4); and every store of the kernel is a whole word through a buffer
    descriptor with the streaming policy -- 4 words x 2 unrolled trips in each loop, nt sc1 -- and nothing through a pointer.  `loop`: what
    the findings call it (the rekey table kernel's second loop is held to the same rules)"""
    bad = []
    if "v_dot4_u32_u8" not in k.fn:
        bad.append("%s: no v_dot4_u32_u8 (the %s loop's byte and position sums)" % (k.name, loop))
    atomics = [(m.group(1), m.group(2)) for m in re.finditer(r"^\s+(global_atomic_\w+)\b([^;\n]*)", k.fn, re.M)]
    wide = [(op, args) for op, args in atomics if op.endswith("_x2")]
    if any(" sc0" in args for _, args in wide):
        bad.append("%s: a 64-bit atomic returns its value (sc0): the %s loop's sums are non-returning global_atomic_add_x2" % (k.name, loop))
    if len(wide) != 4 or any(op != "global_atomic_add_x2" for op, _ in wide):
        bad.append("%s: 64-bit atomics %s, expected 4 global_atomic_add_x2 (a pair per unrolled trip of the %s loop) and nothing else"
                   % (k.name, [op for op, _ in wide], loop))
    fetches = [args for op, args in atomics if op == "global_atomic_add"]
    if len(fetches) != 4 or not all(args.rstrip().endswith(" sc0") for args in fetches) or len(atomics) != len(wide) + len(fetches):
        bad.append("%s: %d 32-bit global_atomic_add among %d atomics, expected the ticket fetch of each unrolled trip of both loops (4), each "
                   "returning (sc0), and the 64-bit adds" % (k.name, len(fetches), len(atomics)))
    if not code_lines(k.fn, "ds_add_u32"):
        bad.append("%s: no ds_add_u32 (the %s loop folds a workgroup's sums in LDS, one pair per wave)" % (k.name, loop))
    data = code_lines(k.fn, "buffer_store_")
    if len(data) != 16 or any(not ln.lstrip().startswith("buffer_store_dwordx4") or not ln.endswith(" nt sc1") for ln in data):
        bad.append("%s: a store of the %s loop is not nt sc1 (%d buffer stores, expected 16 whole words, all nt sc1: %s in each loop)"
                   % (k.name, loop, len(data), TRIPS))
    if re.search(r"^\s+(global|flat|scratch)_store", k.fn, re.M):
        bad.append("%s: a store through a pointer in the kernel of the %s loop (records take 64-bit atomic adds, data goes through "
                   "the destination's descriptor)" % (k.name, loop))
    return bad


def rekey_digest_table_loop(k):
    """the rekey table kernel's second loop (cycle_rekey_table_kernel.h: REKEY_TABLE_DIGEST, one uniform branch apart from the plain
    loop).  It rekeys as the plain loop does and sums the word it stores, the word it read or the plaintext between the two keystreams;
    what it sends to memory and how is the cycle digest loop's, rule for rule.  (The summed word's own v_bitop3_b32 carry the truth
    table 0x78, p ^ (q & r): rekey_blocks' count of 0x96 stays one per dword of a block.)"""
    return cycle_digest_table_loop(k, "rekey digest")


def digest_loop(k):
    """the out-of-place kernel's second loop (cycle_to_kernel.h: the pass whose destination is a sum).  Everything it sends to memory
    besides an entry's own output is a 64-bit atomic add onto a record the host zeroed: the kernel's 64-bit atomics are
    global_atomic_add_x2 and nothing else, none of them returning; the sums are taken with v_dot4_u32_u8, one per dword and weight;
    and nothing is stored through a SOURCE descriptor (the kernel's buffer stores are counted)"""
    bad = []
    wide = [(m.group(1), m.group(2)) for m in re.finditer(r"^\s+(global_atomic_\w+_x2)\b([^;\n]*)", k.fn, re.M)]
    if not wide or any(op != "global_atomic_add_x2" or " sc0" in args for op, args in wide):
        bad.append("%s: 64-bit atomics %s, expected non-returning global_atomic_add_x2 only (the digest loop's sums)" % (k.name, sorted({op for op, _ in wide})))
    if "v_dot4_u32_u8" not in k.fn:
        bad.append("%s: no v_dot4_u32_u8 (the digest loop's byte and position sums)" % k.name)
    # a descriptor's register quad is reused over a kernel's life, so a store through a SOURCE descriptor shows in the count alone: each
    # loop stores 4 words in each of its 2 unrolled trips and once in its cut first chunk's (cold, not unrolled) loop, all whole words
    n_stores = len(code_lines(k.fn, "buffer_store_"))
    if n_stores != 18 or n_stores != len(code_lines(k.fn, "buffer_store_dwordx4")):
        bad.append("%s: %d buffer stores, expected 18 whole words (stream loop and digest loop: %s each): the digest loop stores an entry's output "
                   "through its destination's descriptor and nothing through its source's" % (k.name, n_stores, TRIPS_AND_CUT))
    return bad


def xfer_list_digest(k):
    """the funnel transfer kernels' list loop in digest mode (cycle_xfer_kernel.h: DIGEST MODE, one uniform branch per segment and per word
    trip apart from the plain list loop).  The sums are taken with v_dot4_u32_u8; every 64-bit atomic of the kernel is a non-returning
    global_atomic_add_x2 onto the entry's record (a trip would wait for a value that came back).  That the fold before them uses no LDS
    and no barrier is what the kernel's LDS and barrier rules already say"""
    bad = []
    if "v_dot4_u32_u8" not in k.fn:
        bad.append("%s: no v_dot4_u32_u8 (the list digest mode's byte and position sums)" % k.name)
    wide = [(m.group(1), m.group(2)) for m in re.finditer(r"^\s+(global_atomic_\w+_x2)\b([^;\n]*)", k.fn, re.M)]
    if not wide or any(op != "global_atomic_add_x2" for op, _ in wide):
        bad.append("%s: 64-bit atomics %s, expected global_atomic_add_x2 only (the list digest mode's sums)" % (k.name, sorted({op for op, _ in wide})))
    if any(" sc0" in args for _, args in wide):
        bad.append("%s: a 64-bit atomic returns its value (sc0): the list digest mode's sums are non-returning global_atomic_add_x2" % k.name)
    return bad


def no_digest(k):
    """the plain transfer kernels have no list loop and so no digest mode: no 64-bit atomic and no v_dot4"""
    if re.search(r"^\s+global_atomic_\w+_x2\b", k.fn, re.M) or "v_dot4" in k.fn:
        return ["%s: a 64-bit atomic or a v_dot4 in a plain transfer kernel (the digest mode belongs to the funnel kernels' list loop)" % k.name]
    return []


def lds_bytes(k, n, of):
    if k.md.get("group_segment_fixed_size", -1) != n:
        return ["%s: LDS is %s bytes, expected the %d of %s" % (k.name, k.md.get("group_segment_fixed_size"), n, of)]
    return []


def two_barriers(k):
    if k.fn.count("s_barrier") != 2:
        return ["%s: %d s_barrier, expected 2 (one behind thread 0's region, one at the end of the trip)" % (k.name, k.fn.count("s_barrier"))]
    return []


def mailbox_read_scalar(k):
    """a host-fed trip's ticket and ok word go from the LDS mailbox into scalar registers (v_readfirstlane) behind the first barrier.
    Text order is not execution order: the trip's first barrier is the one followed by the LDS read of the mailbox"""
    ins = instructions(k.fn)
    follows = [i for i, (_, op, _) in enumerate(ins) if op == "s_barrier" and any(o.startswith("ds_read") for _, o, _ in ins[i + 1:i + 3])]
    if len(follows) != 1 or sum(1 for _, o, _ in ins[follows[0] + 1:follows[0] + 8] if o == "v_readfirstlane_b32") < 2:
        return ["%s: the ticket and the ok word are not read into scalar registers right behind the trip's first barrier" % k.name]
    return []


def alg1_mix(k):
    if k.fn.count("v_add_u32_sdwa") != 15:
        return ["%s: keystream instruction mix changed (%d v_add_u32_sdwa, expected 15: ALG 1)" % (k.name, k.fn.count("v_add_u32_sdwa"))]
    return []


def carry_mix(k, blocks):
    if k.fn.count("v_addc_co_u32_sdwa") != blocks * 15 or "v_add_u32_sdwa" in k.fn:
        return ["%s: keystream instruction mix changed (%d addc)" % (k.name, k.fn.count("v_addc_co_u32_sdwa"))]
    return []


def atomic_adds(k, n):
    return ["%s: %d global_atomic_add, expected %d" % (k.name, k.fn.count("global_atomic_add"), n)] if k.fn.count("global_atomic_add") != n else []


def mailbox_is_ds(k):
    return ["%s: flat_ accesses (the LDS mailbox must be ds_ instructions)" % k.name] if "flat_" in k.fn else []


def mailbox_traffic(k, n):
    if k.fn.count("ds_write_b32") != n or k.fn.count("ds_read_b32") != n:
        return ["%s: ticket mailbox traffic changed: %d ds_write_b32, %d ds_read_b32" % (k.name, k.fn.count("ds_write_b32"), k.fn.count("ds_read_b32"))]
    return []


def init_only_stores(k):
    if re.search(r"^\s+(buffer|global)_load", k.fn, re.M) or not re.search(r"^\s+global_store_dword", k.fn, re.M) or "global_atomic" in k.fn:
        return ["%s: the init kernel does something other than store its results" % k.name]
    return []


# ---- rules of a whole TU.  They take a Unit: the TU's words, the source names of ALL kernels of the file, and (not yet in a spec's
# `first` rules, which run before any kernel is looked at and end the check when they find something) its own Kernels. ----
Unit = namedtuple("Unit", "words names kernels")


def kernel_count(u, n, note=""):
    return ["%s holds %d kernels, expected %d%s" % (u.words, len(u.names), n, note)] if len(u.names) != n else []


def one_of_each(u, *sources):
    return ["%s holds %d %s, expected 1" % (u.words, u.names.count(s), s) for s in sources if u.names.count(s) != 1]


def verify_kernel_counts(u):
    init, stream = u.names.count("modgpu_cycle_verify_init"), u.names.count("modgpu_cycle_verify_kernel")
    return ["%s holds %d init and %d stream kernels, expected 1 and 4" % (u.words, init, stream)] if (init, stream) != (1, 4) else []


def one_queue_kernel(u):
    n = u.names.count("modgpu_cycle_queue_kernel")
    return ["expected exactly one work-queue kernel, found %d" % n] if n != 1 else []


def block_in_two_kernels(u):
    n = sum(1 for k in u.kernels if carry_blocks(k.fn))
    return ["expected the keystream block in exactly the two streaming kernels, found it in %d" % n] if n != 2 else []


def on_kernel(u, source, name, rules):
    """further rules for the kernels of one source name, whose findings call it `name`"""
    return [f for k in u.kernels if k.source == source for f in run(rules, k._replace(name=name))]


def run(rules, subject):
    """a rule is a function of the subject, or a tuple of one and its further arguments"""
    bad = []
    for rule in rules:
        fn, *args = rule if isinstance(rule, tuple) else (rule,)
        bad += fn(subject, *args)
    return bad


# ---- the TUs.  file: what the Makefile hands over; words: how findings call the TU; kinds: the kernels it may hold, by source name
# and, where forms of one template differ, a pattern over the rest of the mangled name (the first kind that fits is the kernel's), each
# with its rules in the order their findings are printed; first / then: rules of the whole TU before / behind its kernels'. ----
Kind = namedtuple("Kind", "source rules form", defaults=("",))
TU = namedtuple("TU", "file words kinds first then", defaults=((), ()))

BUDGET = [register_budget, no_spills]
TICKET = (atomic_optimizer_off, "the ticket atomic")
TRIPS = "4 words x 2 unrolled trips"
TRIPS_AND_CUT = TRIPS + " + the cut first chunk"
# the in-place TU (its spill finding is worded apart); none of its kernels is required to carry the block: exactly two of the three do
MAIN = [register_budget, (no_spills, True)]
# the work-queue loop (cycle_kernel_impl.h, modgpu_cycle_queue_kernel; the keep kernel is the same loop): one ticket fetch per unrolled
# trip (2) + a helper's first tickets + the exit count = 4 global_atomic_add; the mailbox's 3 writes and 3 reads are ds_ instructions;
# 9 blocks of 15 addc and no v_add_u32_sdwa (that is ALG 1's): 4 words x 2 unrolled trips + the peeled first chunk
QUEUE_LOOP = [(atomic_adds, 4), mailbox_is_ds, (mailbox_traffic, 3)]
# a host-fed trip (cycle_feed_kernel.h): occupancy-bound (<= 64 VGPRs, 8 waves per SIMD), 8 bytes of LDS, thread 0 fetches the ticket
# and the ok word between exactly two barriers, ALG 1
HOST_FED = [(lds_bytes, 8, "the ticket / ok mailbox"), two_barriers]
XFER = [(register_budget, 64), no_spills] + HOST_FED + [mailbox_read_scalar, alg1_mix, loads_nt]
# the table calls' three launches (cycle_table_kernel.h): no atomic of any of them is wave-aggregated; plan and finish carry no block
TABLE_HEAD = BUDGET + [(atomic_optimizer_off, "an atomic")]
PLANNING = [(keystream_blocks, False), (no_block, "a planning kernel")]
REKEY_PLANNING = [(no_block, "a planning kernel")]
# a verify stream (cycle_verify_kernel.h): it reads its inputs and nothing else; 16 bytes of LDS; its only global store the 8 bytes of
# the entry's n
VERIFY_HEAD = BUDGET + [(keystream_blocks, False), (read_only_stream, "a verify kernel")]
VERIFY_TAIL = [loads_nt, one_global_store, result_atomics, (lds_bytes, 16, "the workgroup's count and lowest index")]


def table_tu(file, words, stem, planning, stream):
    """a table call's TU: <stem>_plan, <stem>_finish and the stream kernel <stem>_kernel, one of each"""
    sources = (stem + "_plan", stem + "_finish", stem + "_kernel")
    return TU(file, words, tuple(Kind(s, TABLE_HEAD + (stream if s.endswith("_kernel") else planning)) for s in sources), then=[(one_of_each,) + sources])


TUS = (
    # the in-place TU: the small shape <1, 256, ...> (one word per lane, launch-latency-bound sizes and every launch across PCIe; ALG 1,
    # no block) has no pipeline of its own and lives on occupancy; the big shape and the work-queue kernel carry the block.  The queue
    # kernel's stores: 4 words x 2 unrolled trips (+ the cold peel loop)
    TU("cycle_kernel.s", "the streaming kernels' TU",
       (Kind("modgpu_cycle_kernel", MAIN + [(register_budget, 64, "the small shape needs "), (keystream_blocks, False)], "^ILi1ELi256E"),
        Kind("modgpu_cycle_kernel", MAIN + [(keystream_blocks, False)]),
        Kind("modgpu_cycle_queue_kernel", MAIN + [(keystream_blocks, False)])),
       first=[one_queue_kernel],
       then=[block_in_two_kernels,
             (on_kernel, "modgpu_cycle_queue_kernel", "queue kernel", [TICKET] + QUEUE_LOOP + [loads_nt, (stores_nt_sc1_at_least, 8), (carry_mix, 9)])]),
    # the host-fed kernel of the host-buffer routes: its stores go across PCIe
    TU("cycle_feed_kernel.s", "the host-fed kernel's TU",
       (Kind("modgpu_cycle_feed_kernel", [no_spills, (register_budget, 64)] + HOST_FED + [loads_nt, (stores, "sc1"), mailbox_read_scalar, alg1_mix]),),
       first=[(kernel_count, 1)]),
    # out-of-place, plain and funnel: the work-queue loop with a destination of its own, and the digest loop (static chunks, no block
    # count pinned: one uniform branch chooses between the two)
    TU("cycle_to_kernel.s", "the out-of-place kernel's TU",
       (Kind("modgpu_cycle_to_kernel", BUDGET + [keystream_blocks, TICKET, loads_nt, (stores, "nt sc1"), digest_loop]),)),
    # transfer, each direction plain and funnel: host-fed trips; the upload <true, .> stores into HBM, the download across PCIe; the
    # funnel <., true> kernels hold the list loop and its digest mode, the plain ones neither
    TU("cycle_xfer_kernel.s", "the transfer kernels' TU",
       (Kind("modgpu_cycle_xfer_kernel", XFER + [(stores, "nt sc1", "an upload store into HBM"), xfer_list_digest], "^ILb1ELb1E"),
        Kind("modgpu_cycle_xfer_kernel", XFER + [(stores, "nt sc1", "an upload store into HBM"), no_digest], "^ILb1E"),
        Kind("modgpu_cycle_xfer_kernel", XFER + [(stores, "sc1", "a download store across PCIe"), xfer_list_digest], "^ILb0ELb1E"),
        Kind("modgpu_cycle_xfer_kernel", XFER + [(stores, "sc1", "a download store across PCIe"), no_digest]))),
    # rekey, plain and funnel: one uniform branch chooses between the stream loop and the move loop; the fixed registers, the ticket's
    # form, the cache policies, the budget (and, for every kernel, barriers at full EXEC) hold over both
    TU("cycle_rekey_kernel.s", "the rekey kernel's TU",
       (Kind("modgpu_cycle_rekey_kernel", BUDGET + [rekey_blocks, (block_count, TWO_KEYSTREAM, 17, TRIPS + " in the stream and in the move loop + the cut first chunk"),
                                                   TICKET, loads_nt, (stores, "nt sc1"), move_loop]),)),
    # table of out-of-place entries.  The stream kernel has two loops, the plain one and the cycle digest loop (one uniform branch
    # chooses): twice the blocks, the ticket fetches and the stores, and the second loop's pair of 64-bit adds per unrolled trip
    table_tu("cycle_table_kernel.s", "the table kernels' TU", "modgpu_cycle_table", PLANNING,
             [keystream_blocks, (block_count, KEYSTREAM, 16, TRIPS + " in the plain and in the cycle digest loop"), loads_nt, (stores, "nt sc1"),
              cycle_digest_table_loop, scalar_entry_search]),
    # table of rekey entries.  The stream kernel has two loops, the plain one and the rekey digest loop (one uniform branch chooses):
    # twice the blocks, the ticket fetches and the stores, and the second loop's pair of 64-bit adds per unrolled trip
    table_tu("cycle_rekey_table_kernel.s", "the rekey table kernels' TU", "modgpu_cycle_rekey_table", REKEY_PLANNING,
             [rekey_blocks, (block_count, TWO_KEYSTREAM, 16, TRIPS + " in the plain and in the rekey digest loop"), loads_nt, (stores, "nt sc1"),
              rekey_digest_table_loop, scalar_entry_search]),
    # verify: the init kernel and the stream kernel plain / funnel x keyed <..., true> (compares with src ^ keystream) / identity (compares
    # the buffers as they are: no block).  Chunks are assigned statically: no ticket, nothing for the atomic optimizer to rewrite
    TU("cycle_verify_kernel.s", "the verify kernels' TU",
       (Kind("modgpu_cycle_verify_init", VERIFY_HEAD + [(no_block, "the init kernel"), init_only_stores]),
        Kind("modgpu_cycle_verify_kernel", VERIFY_HEAD + [(block_count, KEYSTREAM, 9, TRIPS_AND_CUT)] + VERIFY_TAIL, "Lb1EEv15CycleVerifyArgs$"),
        Kind("modgpu_cycle_verify_kernel", VERIFY_HEAD + [(no_block, "an identity form")] + VERIFY_TAIL)),
       then=[verify_kernel_counts]),
    # table of verify entries: chunks come from a ticket counter, ONE plain returning 32-bit fetch per unrolled trip (2).  The stream
    # kernel has two loops, the compare and the digest (one uniform branch chooses): twice the blocks and the ticket fetches, and the
    # digest loop's pair of 64-bit adds per unrolled trip (4) beside the compare's adds and mins
    table_tu("cycle_verify_table_kernel.s", "the verify table kernels' TU", "modgpu_cycle_verify_table", PLANNING,
             [keystream_blocks, (block_count, KEYSTREAM, 16, TRIPS + " in the compare and in the digest loop"), loads_nt,
              (read_only_stream, "a verify kernel", True), (result_atomics, 4, 4), digest_table_loop, scalar_entry_search]),
    # rekey verify (verify against two keystreams), plain and funnel
    TU("cycle_rekey_verify_kernel.s", "the rekey verify kernel's TU",
       (Kind("modgpu_cycle_rekey_verify_kernel", BUDGET + [rekey_blocks, (block_count, TWO_KEYSTREAM, 9, TRIPS_AND_CUT), (read_only_stream, "a rekey verify kernel")] + VERIFY_TAIL),),
       then=[(kernel_count, 2, " (plain and funnel)")]),
    # keep: the work-queue kernel with a cache policy per chunk
    TU("cycle_keep_kernel.s", "the keep kernel's TU",
       (Kind("modgpu_cycle_keep_kernel", BUDGET + [keystream_blocks, TICKET] + QUEUE_LOOP + [(carry_mix, 9), loads_nt, keep_store_bursts]),),
       then=[(kernel_count, 1)]),
    # table of rekey verify entries: the rules of both parents
    table_tu("cycle_rekey_verify_table_kernel.s", "the rekey verify table kernels' TU", "modgpu_cycle_rekey_verify_table", REKEY_PLANNING,
             [rekey_blocks, (block_count, TWO_KEYSTREAM, 8, TRIPS), loads_nt, (read_only_stream, "a rekey verify kernel", True), (result_atomics, 2), scalar_entry_search]),
    # table of rekey entries moved with memmove rules: the rekey table call's planning kernels with a window and a place launch, and
    # the rekey TU's move loop over the chunks of a table
    TU("cycle_rekey_move_table_kernel.s", "the rekey move table kernels' TU",
       tuple(Kind("modgpu_cycle_rekey_move_table_" + s, TABLE_HEAD + REKEY_PLANNING) for s in ("plan", "finish", "window", "place")) +
       (Kind("modgpu_cycle_rekey_move_table_kernel", TABLE_HEAD + [rekey_blocks, (block_count, TWO_KEYSTREAM, 8, TRIPS), loads_nt, (stores, "nt sc1"), table_move_loop]),),
       then=[(one_of_each,) + tuple("modgpu_cycle_rekey_move_table_" + s for s in ("plan", "finish", "window", "kernel", "place"))]),
)
OWNER = {kind.source: tu for tu in TUS for kind in tu.kinds}
__doc__ = "check_isa.py " + " | ".join("<%s>" % tu.file for tu in TUS) + __doc__


def check(asm):
    """one TU's assembly: the rules for every kernel, then those of the TU it is -- the one that owns the first kernel whose source name is
    in the table"""
    bad = []
    bodies = kernel_bodies(asm)
    for name, fn in kernel_texts(asm).items():
        bad += sdwa_forwarding_hazards(name, fn)
        bad += barriers_at_full_exec(name, fn)
    named = {name: source_name(name) for name in bodies}
    tu = next((OWNER[source] for source, _ in named.values() if source in OWNER), None)
    if tu is None:
        return bad + ["expected exactly one work-queue kernel, found 0"]
    names = [source for source, _ in named.values()]
    found = run(tu.first, Unit(tu.words, names, []))
    if found:
        return bad + found
    kernels = []
    for name, fn in bodies.items():
        source, form = named[name]
        kind = next((kd for kd in tu.kinds if kd.source == source and re.search(kd.form, form)), None)
        if kind is None:
            bad.append("%s: %s holds another kernel" % (name, tu.words))
            continue
        kernels.append(Kernel(name, source, fn, metadata(asm, name)))
        bad += run(kind.rules, kernels[-1])
    return bad + run(tu.then, Unit(tu.words, names, kernels))


def main():
    bad, n_kernels = [], 0
    for path in sys.argv[1:]:
        asm = open(path).read()
        bad += check(asm)
        n_kernels += len(kernel_bodies(asm))
    for b in bad[:40]:
        print("check_isa:", b)
    if bad:
        print("check_isa: %d finding(s) -- the kernel TUs must not ship like this" % len(bad))
        return 1
    print("check_isa: ok (%d kernels)" % n_kernels)
    return 0


if __name__ == "__main__":
    sys.exit(main())
