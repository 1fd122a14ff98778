#!/usr/bin/env python3
"""Is the device code of two builds the same?  Compares the kernels of two directories of hipcc -S listings:
    make -C cuda-fft-convolution_amd/csrc -j16 listings LISTDIR=/tmp/new      (and the same in a checkout of the parent commit)
    isa_same.py /tmp/parent /tmp/new
For every <unit>.s that both directories hold and every function symbol in it (the kernels, and any device function that was
not inlined), the instruction lines are compared one by one: directives, comments and labels are dropped, basic-block labels
lose the function number the compiler gave them.  A kernel is
    identical        every instruction line is the same;
    operand order    the same number of lines, and every line that differs is ONE instruction with the same mnemonic, the same
                     destination and the same source operands in another order (what the compiler does to a commutative
                     instruction when the expression it came from was written the other way round) -- each such line is listed:
                     whether the instruction commutes is for the reader to say, this tool knows no instruction by name;
    different        anything else; these kernels are named, with the first differing line.
Kernels are matched by their mangled names.  Exit status 1 if any kernel is different or exists on one side only, if a unit
exists in one directory only (they are named), or if a unit holds no kernel at all."""
import os, re, sys


def instructions(body):
    out = []
    for l in body:
        s = l.split(";")[0].strip()
        if not s or s.startswith(".") or re.match(r"^\S+:$", s):
            continue
        out.append(re.sub(r"\.LBB\d+_", ".LBB_", " ".join(s.split())))
    return out


def kernels(path):
    """{name: (name, [instruction lines])} of the function symbols of a listing; {} if it holds no kernel"""
    lines = open(path).read().split("\n")
    if not any(l.strip().startswith(".amdhsa_kernel ") for l in lines):
        return {}
    names = {m.group(1) for m in (re.match(r"\s*\.type\s+(\S+),@function", l) for l in lines) if m}
    out, i = {}, 0
    while i < len(lines):
        m = re.match(r"^(\S+):", lines[i])
        if m and m.group(1) in names:
            j = i + 1
            while j < len(lines) and not lines[j].startswith(".Lfunc_end"):
                j += 1
            out[m.group(1)] = (m.group(1), instructions(lines[i + 1:j]))
            i = j
        i += 1
    return out


def reordered(a, b):
    """one instruction, same mnemonic and destination, the same sources in another order"""
    pa, pb = a.split(None, 1), b.split(None, 1)
    if len(pa) != 2 or len(pb) != 2 or pa[0] != pb[0]:
        return False
    oa, ob = ([o.strip() for o in re.split(r",(?![^\[]*\])", p[1])] for p in (pa, pb))      # (not the commas inside op_sel:[1,0])
    return len(oa) == len(ob) and oa[0] == ob[0] and oa[1:] != ob[1:] and sorted(oa[1:]) == sorted(ob[1:])


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    da, db = sys.argv[1], sys.argv[2]
    la, lb = ({f for f in os.listdir(d) if f.endswith(".s")} for d in (da, db))
    units, lone, empty = sorted(la & lb), sorted(la ^ lb), []
    for u in lone:
        print("%-28s only in %s" % (u[:-2], da if u in la else db))
    tot = [0, 0, 0]
    for u in units:
        ka, kb = kernels(os.path.join(da, u)), kernels(os.path.join(db, u))
        if not ka or not kb:
            empty.append(u)
            print("%-28s NO KERNELS in %s" % (u[:-2], " and ".join(d for d, k in ((da, ka), (db, kb)) if not k)))
            continue
        same, order, diff = 0, [], []
        for key in sorted(set(ka) | set(kb)):
            if key not in ka or key not in kb:
                diff.append((key, "only in %s" % (da if key in ka else db)))
                continue
            ia, ib = ka[key][1], kb[key][1]
            if ia == ib:
                same += 1
                continue
            pairs = [(n, x, y) for n, (x, y) in enumerate(zip(ia, ib)) if x != y]
            if len(ia) == len(ib) and all(reordered(x, y) for _, x, y in pairs):
                order.append((kb[key][0], pairs))
            else:
                where = pairs[0] if pairs else (min(len(ia), len(ib)), "(end)", "(end)")
                diff.append((kb[key][0], "%d / %d instructions, first difference at %d: %s | %s" % (len(ia), len(ib), where[0], where[1], where[2])))
        print("%-28s %3d kernels: %3d identical, %3d operand order only, %3d different" % (u[:-2], same + len(order) + len(diff), same, len(order), len(diff)))
        for name, pairs in order:
            print("    operand order: %s" % name)
            for n, x, y in pairs:
                print("        %6d  %s %s  ->  %s" % (n, x.split()[0], x.split(None, 1)[1], y.split(None, 1)[1]))
        for name, what in diff:
            print("    DIFFERENT: %s: %s" % (name, what))
        tot = [tot[0] + same, tot[1] + len(order), tot[2] + len(diff)]
    print("total: %d units, %d kernels: %d identical, %d operand order only, %d different" % (len(units), sum(tot), tot[0], tot[1], tot[2]))
    sys.exit(1 if tot[2] or not units or lone or empty else 0)


if __name__ == "__main__":
    main()
