#!/usr/bin/env python3
"""A/B of per-map extrema (fftconv_plan_set_extrema): off, fused, scanned, and the caller's own reduction.

    python tools/extrema_ab.py [--parent-tree /path/to/built/parent/checkout] [--rounds 3] [--out profiles/extrema_ab.txt]

Fresh processes alternating on one box, as tools/match_score_ab.py does.  Per geometry (cfg3's with 64 maps: 4096^2 (x) 127^2; cfg2's
with 16 maps: 1024^2 (x) 63^2), per score (raw maps, 1 CCOEFF_NORMED, 4 SQDIFF) and per mode
    parent   (a) the parent commit's library (--parent-tree), no extrema: the step as it was
    off      (b) this library, extrema off
    fused    (c) extrema on, "extrema_store" 1: found by the output kernel in its store, then one fold launch
    scanned  (d) extrema on, "extrema_store" 0: the scan kernel reads the delivered maps, then the fold
    caller   (e) extrema off, then the caller's own torch reduction over the packed maps: amax + argmax and amin + argmin per map
a device-resident convolve is timed with HIP events (one process per mode and round, the three scores one after the other in it);
median over the rounds and the spread (min .. max), microseconds.  Beside it the output-column kernel's own time per convolve from the
plan's profile (PK_OUT_COLS: the fused store against its plain sibling; the fold and the scan are launches of their own and not in
it).  With --parent-tree also bench.py's default line there against this tree's, alternating."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOMETRIES = {  # name: H, W, kh, kw, maps, steps
    "cfg3 4096^2 (x) 127^2, 64 maps": (4096, 4096, 127, 127, 64, 6),
    "cfg2 1024^2 (x) 63^2, 16 maps": (1024, 1024, 63, 63, 16, 30),
}
SCORES = (0, 1, 4)
MODES = ("parent", "off", "fused", "scanned", "caller")


def worker(tree, name, mode):
    sys.path.insert(0, os.path.join(tree, "tests"))
    import torch
    import util
    fc = util.load_package()
    H, W, kh, kw, n, steps = GEOMETRIES[name]
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(3)
    img = torch.randn((1, W, H), generator=g).to(dev)
    ker = torch.randn((n, 1, kw, kh), generator=g).to(dev)
    stream = torch.cuda.Stream(dev)
    res = {}
    with torch.cuda.stream(stream), fc.Plan(H, W, 1, kh, kw, stream=stream.cuda_stream) as p:
        i = p.info
        out = torch.empty((n, i.fft_w * i.fft_h), dtype=torch.float32, device=dev)
        if mode in ("fused", "scanned"):
            p.set_extrema(1, n)
            p.set_option("extrema_store", 1 if mode == "fused" else 0)

        def convolve():
            p.convolve_packed_device(n, ker.data_ptr(), kh, kw, out.data_ptr())
            if mode == "caller":      # what a caller does without the entry: four reductions over the maps, 4P bytes read by each
                return (torch.amax(out, dim=1), torch.argmax(out, dim=1), torch.amin(out, dim=1), torch.argmin(out, dim=1))

        for score in SCORES:
            p.set_match_score(score, kh if score else 0, kw if score else 0)
            r = {"direct": p.get_option("extrema_direct") if mode in ("fused", "scanned") else -1}
            for _ in range(2):
                p.set_image_device(img.data_ptr())
                convolve()
            torch.cuda.synchronize()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * steps)]
            for s in range(steps):
                ev[2 * s].record(stream)
                convolve()
                ev[2 * s + 1].record(stream)
            torch.cuda.synchronize()
            r["convolve_us"] = statistics.median(ev[2 * s].elapsed_time(ev[2 * s + 1]) for s in range(steps)) * 1e3
            p.set_option("profile", 1)
            p.profile(reset=True)
            for s in range(steps):
                convolve()
            prof = p.profile(reset=True)
            p.set_option("profile", 0)
            r["out_cols_us"] = prof["cols_c2r"]["ms"] / steps * 1e3      # PK_OUT_COLS
            res[str(score)] = r
    print("EXTREMA_AB " + json.dumps(res))


def run_worker(tree, name, mode):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", tree, name, mode], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=300)
    for line in r.stdout.splitlines():
        if line.startswith("EXTREMA_AB "):
            return json.loads(line[len("EXTREMA_AB "):])
    raise RuntimeError("worker %s / %s failed (%d):\n%s" % (name, mode, r.returncode, r.stdout[-2000:]))


def run_bench(tree):
    r = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", "10", "--warmup", "3", "--no-cpu-baseline", "--no-extras"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=tree, timeout=400)
    for line in reversed(r.stdout.splitlines()):
        if line.startswith("{") and "\"value\"" in line:
            return json.loads(line)["value"]
    raise RuntimeError("bench.py failed (%d):\n%s" % (r.returncode, r.stdout[-2000:]))


def fmt(vals):
    return "%9.1f  (%.1f .. %.1f)" % (statistics.median(vals), min(vals), max(vals))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", nargs=3, default=None)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "extrema_ab.txt"))
    a = ap.parse_args()
    if a.worker:
        return worker(*a.worker)
    modes = [m for m in MODES if m != "parent" or a.parent_tree]
    lines = ["per-map extrema: off / fused / scanned / the caller's own torch reduction, fresh processes alternating on one box, %d rounds; "
             "microseconds per convolve, median (min .. max)" % a.rounds,
             "(parent: the parent commit's library; caller: extrema off, then amax + argmax + amin + argmin over the packed maps; out_cols: the "
             "output-column kernel alone, from the plan's profile -- the fold and the scan are launches of their own)"]
    try:
        for name in GEOMETRIES:
            runs = {m: [] for m in modes}
            for _ in range(a.rounds):
                for m in modes:
                    runs[m].append(run_worker(os.path.abspath(a.parent_tree) if m == "parent" else ROOT, name, "off" if m == "parent" else m))
            lines.append("")
            lines.append(name)
            first = len(lines)
            for score in SCORES:
                k = str(score)
                lines.append("  score %d" % score)
                for m in modes:
                    rs = [r[k] for r in runs[m]]
                    lines.append("    %-8s extrema_direct %2d  convolve %s   out_cols %s" % (m, rs[0]["direct"], fmt([r["convolve_us"] for r in rs]),
                                                                                           fmt([r["out_cols_us"] for r in rs])))
                c = {m: [r[k]["convolve_us"] for r in runs[m]] for m in modes}
                if "parent" in c:
                    lines.append("    off within the spread of parent: %s" % ("yes" if min(c["off"]) <= max(c["parent"]) and min(c["parent"]) <= max(c["off"]) else "NO"))
                lines.append("    fused faster than scanned beyond the spread: %s;  fused faster than the caller's reduction beyond the spread: %s" %
                             ("yes" if max(c["fused"]) < min(c["scanned"]) else "NO", "yes" if max(c["fused"]) < min(c["caller"]) else "NO"))
            print("\n".join(lines[first - 1:]), flush=True)
    except (RuntimeError, subprocess.TimeoutExpired) as e:      # (the figures above are kept)
        lines.append("A/B incomplete: %s" % str(e)[-1500:])
        a.parent_tree = None      # (nothing more is started on the device after a worker failed)
    if a.parent_tree:
        vals = {"parent": [], "this": []}
        try:
            for _ in range(a.rounds):
                vals["parent"].append(run_bench(os.path.abspath(a.parent_tree)))
                vals["this"].append(run_bench(ROOT))
        except (RuntimeError, subprocess.TimeoutExpired) as e:
            lines.append("bench.py A/B incomplete: %s" % str(e)[-1500:])
        lines.append("")
        lines.append("bench.py --gpus 1 --steps 10 --warmup 3 (Gpixel-filters/s), alternating")
        for k in ("parent", "this"):
            if vals[k]:
                lines.append("  %-6s %s" % (k, fmt(vals[k])))
        print("\n".join(lines[-3:]), flush=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
