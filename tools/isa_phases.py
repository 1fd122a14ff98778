#!/usr/bin/env python3
"""Instruction mix per phase of a kernel's main loop in a hipcc -S listing (sibling of isa_mix.py, which counts the whole kernel):
    isa_phases.py file.s substring [substring...]        e.g.  isa_phases.py g1.s k_fast_rows_multiI Li4224E Li6ELb1E
    hipcc <csrc/Makefile's CXXFLAGS> --cuda-device-only -S kernels_rows_multi_g1.hip -o g1.s
The loop is the depth-1 loop of the kernel that holds the most instructions (the walk over maps of the row kernels): the header
block (the back-edge target, "Loop Header: Depth=1" in the listing) and every block the compiler annotates "in Loop: Header=<it>".
One iteration is walked from the header to the back edge and a new segment starts after every s_barrier; blocks of the loop that
the compiler laid out behind the back edge (cold paths such as the first map's P1) are summed in the column "cold".  The count
is static: both sides of a branch inside a phase are counted (the cropped and the uncropped store burst of P5, for instance),
so a column is an upper bound of what one iteration issues.  --arith prints, instead, the multiset of fp32 arithmetic instructions (opcode + modifiers, registers
dropped) of every matching kernel: equal multisets in two builds = the same floating-point work.  --nops prints, instead, every
s_nop of the loop by segment and by the pair of instructions around it (nop_pairs)."""
import collections, re, sys

CLASSES = ["pk_arith", "fp_other", "v_mov", "v_int", "v_cmp", "v_lane", "v_other", "lds", "global", "salu", "s_waitcnt", "s_nop", "s_barrier", "branch"]
FP = re.compile(r"^v_(pk_)?(add|sub|subrev|mul|fma|fmac|mac|mad|max|min)_(legacy_)?f(16|32|64)")


def classify(op):
    if op.startswith("v_pk_") and FP.match(op): return "pk_arith"
    if FP.match(op): return "fp_other"
    if op.startswith(("v_mov_b", "v_accvgpr")): return "v_mov"
    if op.startswith("v_cmp"): return "v_cmp"
    if op.startswith(("v_writelane", "v_readlane")): return "v_lane"      # scalar registers parked in the lanes of a vector register
    if re.match(r"^v_(add|sub|subrev|mul|mad|lshl|lshr|ashr|and|or|xor|not|bfe|bfi|add3|lshl_add|add_lshl|lshl_or|and_or|or3|xad|min|max|cndmask|readfirstlane|mbcnt)", op): return "v_int"
    if op.startswith("v_"): return "v_other"
    if op.startswith("ds_"): return "lds"
    if op.startswith(("global_", "flat_", "buffer_", "scratch_")): return "global"
    if op.startswith("s_waitcnt"): return "s_waitcnt"
    if op.startswith("s_nop"): return "s_nop"
    if op.startswith("s_barrier"): return "s_barrier"
    if op.startswith(("s_cbranch", "s_branch", "s_endpgm")): return "branch"
    if op.startswith("s_"): return "salu"
    return None


def kernels(lines, pats):
    starts = [i for i, l in enumerate(lines) if re.match(r"^_Z\S+:", l)]
    for si, st in enumerate(starts):
        name = lines[st].split(":")[0]
        if all(p in name for p in pats):
            yield name, lines[st:starts[si + 1] if si + 1 < len(starts) else len(lines)]


def blocks(body):
    """[(label, header or None ('self' for a loop header), [instruction lines])] in layout order, up to s_endpgm"""
    out = [("entry", None, [])]
    for l in body[1:]:
        m = re.match(r"^(?:(\.LBB\d+_\d+):|; %bb\.(\d+):)\s*(;.*)?$", l)
        if m:
            note = m.group(3) or ""
            h = re.search(r"in Loop: Header=BB(\d+_\d+) Depth=1\b", note)
            hdr = ".LBB" + h.group(1) if h else ("self" if re.search(r"Loop Header: Depth=1\b", note) else None)
            out.append((m.group(1) or "%bb." + m.group(2), hdr, []))
            continue
        s = l.strip()
        m = re.match(r"^([a-z_0-9]+)(\s|$)", s)
        if m and not s.startswith((".", ";")):
            out[-1][2].append(s)
            if m.group(1) == "s_endpgm": break
    return out


def phases(body):
    """(header label, [Counter per segment], Counter of the out-of-line blocks) of the kernel's largest depth-1 loop"""
    bl = blocks(body)
    size = collections.Counter()
    for label, hdr, ins in bl:
        size[label if hdr == "self" else hdr] += len(ins)
    size.pop(None, None)
    if not size: return None, [], collections.Counter()
    head = max(size, key=size.get)
    member = [(label, ins) for label, hdr, ins in bl if (hdr == "self" and label == head) or hdr == head]
    at = [m[0] for m in member].index(head)
    latch, chain = member[:at], member[at:]      # the latch blocks are laid out ahead of the header they fall into
    back = {m[0] for m in latch} | {head}
    end = next((i for i, (label, ins) in enumerate(chain) if ins and re.match(r"s_branch\s+(\S+)", ins[-1]) and ins[-1].split()[1] in back),
               len(chain) - 1)
    cold = collections.Counter(classify(s.split()[0]) for label, ins in chain[end + 1:] for s in ins)
    cols, cur = [], collections.Counter()
    for label, ins in chain[:end + 1] + latch:   # one iteration: header ... back edge
        for s in ins:
            op = s.split()[0]
            cur[classify(op)] += 1
            if op == "s_barrier":
                cols.append(cur)
                cur = collections.Counter()
    cols.append(cur)
    return head, cols, cold


def regs(operand):
    """the set of registers an operand names: v7 -> {('v', 7)}, s[4:7] -> {('s', 4) ... ('s', 7)}, vcc -> {('vcc', 0)}"""
    out = set()
    for kind, lo, hi, one in re.findall(r"\b(?:([vsa])\[(\d+):(\d+)\]|([vsa]\d+))", operand):
        if one: out.add((one[0], int(one[1:])))
        else: out.update((kind, i) for i in range(int(lo), int(hi) + 1))
    for name in ("vcc", "exec", "m0", "scc"):
        if re.search(r"\b%s(_lo|_hi)?\b" % name, operand): out.add((name, 0))
    return out


def nop_pairs(body):
    """Counter of (segment, wait states, instruction ahead, instruction behind, what links them) over the s_nop of one iteration
    of the loop (and of its cold blocks, segment 'cold').  The instruction ahead is the nearest one that is no s_nop, the one
    behind the first after the run of s_nop; the wait states of a run are summed (s_nop n stalls n + 1 cycles).  The link is
    what the pair shares: 'dst->src' a register the first writes (its first operand) and the second reads, 'dst->dst' one
    both write, '-' nothing (the hazard then lies further back than one instruction, or is one of a kind of instructions)."""
    bl = blocks(body)
    size = collections.Counter()
    for label, hdr, ins in bl:
        size[label if hdr == "self" else hdr] += len(ins)
    size.pop(None, None)
    out = collections.Counter()
    if not size: return out
    head = max(size, key=size.get)
    member = [(label, ins) for label, hdr, ins in bl if (hdr == "self" and label == head) or hdr == head]
    at = [m[0] for m in member].index(head)
    latch, chain = member[:at], member[at:]
    back = {m[0] for m in latch} | {head}
    end = next((i for i, (label, ins) in enumerate(chain) if ins and re.match(r"s_branch\s+(\S+)", ins[-1]) and ins[-1].split()[1] in back),
               len(chain) - 1)

    def walk(seq, seg0, count_barriers):
        seg, prev, wait = seg0, None, 0
        for s in seq:
            op = s.split()[0]
            if op == "s_nop":
                wait += int(s.split()[1]) + 1
                continue
            if wait:
                link = "-"
                if prev:
                    pa, na = (x.split(None, 1)[1] if " " in x else "" for x in (prev, s))
                    po, no = (re.split(r",(?![^\[]*\])", x) for x in (pa, na))
                    stores = lambda o: o.split()[0].startswith(("global_store", "ds_write", "ds_store", "buffer_store", "scratch_store", "flat_store"))
                    pd = set() if stores(prev) else regs(po[0])
                    ns = regs(na) if stores(s) else regs(",".join(no[1:]))
                    nd = set() if stores(s) else regs(no[0])
                    link = "dst->src" if pd & ns else "dst->dst" if pd & nd else "-"
                out[(seg, wait, prev.split()[0] if prev else "(block start)", op, link)] += 1
                wait = 0
            prev = s
            if count_barriers and op == "s_barrier": seg += 1
        return seg

    walk([s for label, ins in chain[:end + 1] + latch for s in ins], 0, True)
    for label, ins in chain[end + 1:]:
        walk(ins, "cold", False)
    return out


def arith_multiset(body):
    c = collections.Counter()
    for label, hdr, ins in blocks(body):
        for s in ins:
            op = s.split()[0]
            if FP.match(op):
                mods = " ".join(sorted(t for t in re.split(r"\s+", s)[1:] if re.match(r"^(op_sel|op_sel_hi|neg_lo|neg_hi|clamp|mul:|div:)", t)))
                neg = "".join("n" if t.lstrip().startswith("-") else "a" if t.lstrip().startswith("|") else "." for t in s.split(None, 1)[1].split(","))
                c[(op, mods, neg if set(neg) - {"."} else "")] += 1
    return c


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    lines = open(args[0]).read().splitlines()
    for name, body in kernels(lines, args[1:]):
        if "--arith" in sys.argv:
            ms = arith_multiset(body)
            print(name[:160], " fp arithmetic instructions:", sum(ms.values()))
            for k, v in sorted(ms.items()): print("    %5d  %s %s %s" % (v, k[0], k[1], k[2]))
            continue
        if "--nops" in sys.argv:
            pairs = nop_pairs(body)
            print(name[:160])
            print("  s_nop of the loop by the instructions around them: %d runs, %d wait states" % (sum(pairs.values()), sum(k[1] * v for k, v in pairs.items())))
            print("  %-5s %5s %6s  %-26s %-26s %s" % ("seg", "runs", "states", "ahead", "behind", "link"))
            for (seg, wait, a, b, link), v in sorted(pairs.items(), key=lambda kv: (str(kv[0][0]), -kv[1] * kv[0][1], kv[0][2:])):
                print("  %-5s %5d %6d  %-26s %-26s %s" % (seg if seg == "cold" else "seg%d" % seg, v, v * wait, a, b, link))
            continue
        head, cols, outl = phases(body)
        print(name[:160])
        print("  loop header %s; seg0 starts at the header, a new segment after every s_barrier, the last one ends at the back edge" % head)
        hdr = ["seg%d" % i for i in range(len(cols))] + ["cold", "loop"]
        allc = cols + [outl]
        tot = collections.Counter()
        for c in allc: tot.update(c)
        print("  %-10s" % "" + "".join("%7s" % h for h in hdr))
        for k in CLASSES:
            print("  %-10s" % k + "".join("%7d" % c[k] for c in allc) + "%7d" % tot[k])
        valu = lambda c: sum(c[k] for k in CLASSES if k.startswith(("v_", "pk_", "fp_")))
        nona = lambda c: sum(c[k] for k in ("v_mov", "v_int", "v_cmp", "v_lane", "v_other"))
        print("  %-10s" % "VALU" + "".join("%7d" % valu(c) for c in allc) + "%7d" % valu(tot))
        print("  %-10s" % "non-arith" + "".join("%7d" % nona(c) for c in allc) + "%7d" % nona(tot))


if __name__ == "__main__":
    main()
