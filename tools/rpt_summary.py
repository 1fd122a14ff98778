#!/usr/bin/env python3
"""Register / spill / occupancy table of every kernel from the build's csrc/*.rpt files
(hipcc -Rpass-analysis=kernel-resource-usage, written by csrc/Makefile).
usage: rpt_summary.py [--all] [substring ...]     (default: kernels that spill or use scratch)
       rpt_summary.py --compare CSRC_A CSRC_B     (two builds, kernel by kernel: every resource line equal?  exit 1 if not)
e.g. rpt_summary.py --all k_fast_cols16 k_cols_c2r16 k_crop_maps16 k_pad_maps16     (the 16-bit-map kernels, plan option "map_format")"""
import glob, os, re, subprocess, sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "cuda-fft-convolution_amd", "csrc")


def kernels(csrc=CSRC):
    out = []
    for f in sorted(glob.glob(os.path.join(csrc, "*.rpt"))):
        cur = None
        for line in open(f, errors="replace"):
            m = re.search(r"remark:\s+Function Name: (\S+)", line)
            if m:
                cur = {"unit": os.path.basename(f)[:-4], "mangled": m.group(1)}
                out.append(cur)
                continue
            m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\S+) \[-Rpass", line)
            if m and cur is not None:
                cur[m.group(1).strip()] = m.group(2)
    names = "\n".join(k["mangled"] for k in out)
    try:
        dem = subprocess.run(["c++filt"], input=names, capture_output=True, text=True).stdout.splitlines()
    except Exception:
        dem = names.splitlines()
    for k, d in zip(out, dem):
        d = d.replace("fc::(anonymous namespace)::", "").replace("fc::", "")
        k["name"] = re.sub(r"\(.*$", "", d).replace("void ", "")
    return out


def compare(csrc_a, csrc_b):
    skip = ("unit", "mangled", "name")
    A, B = ({(k["unit"], k["mangled"]): {f: v for f, v in k.items() if f not in skip} for k in kernels(c)} for c in (csrc_a, csrc_b))
    diff = [k for k in sorted(set(A) | set(B)) if A.get(k) != B.get(k)]
    print("%d kernels in %s, %d in %s; %d with a differing resource line" % (len(A), csrc_a, len(B), csrc_b, len(diff)))
    for k in diff:
        print("   ", k[0], k[1], A.get(k), B.get(k))
    if A:
        print("resource lines compared per kernel:", ", ".join(sorted(next(iter(A.values())))))
    return 1 if diff or not A else 0


if __name__ == "__main__":
    if "--compare" in sys.argv:
        sys.exit(compare(*sys.argv[sys.argv.index("--compare") + 1:][:2]))
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    show_all = "--all" in sys.argv
    for k in kernels():
        spill, scratch = int(k.get("VGPRs Spill", 0)), int(k.get("ScratchSize", 0))
        if args and not any(a in k["name"] for a in args):
            continue
        if not args and not show_all and not spill and not scratch:
            continue
        print("%-24s vgpr %3s  scratch %4d  spill %3d  occ %s  sgpr %3s  %s" % (k["unit"], k.get("VGPRs"), scratch, spill, k.get("Occupancy"),
                                                                               k.get("TotalSGPRs"), k["name"]))
