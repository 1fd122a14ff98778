#!/usr/bin/env python3
"""A/B of matching score 4, SQDIFF (fftconv_plan_set_match_score): fused, staged, and the caller's own pass, on ONE library.

    python tools/match_score_ab.py [--parent-tree /path/to/built/parent/checkout] [--rounds 3] [--out profiles/match_score_ab.txt]

Fresh processes alternating on one box, as tools/ncc_ab.py does.  Per geometry (cfg3's with 64 maps: 4096^2 (x) 127^2; cfg2's with 16
maps: 1024^2 (x) 63^2) and mode
    fused    score 4, "norm_store" 1: the output kernel stores v + (Q + c) itself
    staged   score 4, "norm_store" 0: the fp32 window is staged, and Q + c is added while it is cropped
    caller   score 0: the raw maps are stored, then ONE torch elementwise kernel computes -2 * map + (E + c) in place on a precomputed
             E + c per map -- what a caller does without the entry (E's own computation, the box sums of I^2, is NOT in the
             figure: compare the set_image steps)
    ncc      score 1, fused: for the set_image step alone (the window statistics of score 4 against those of score 1)
a device-resident step is timed with HIP events: set_image(DEVICE) alone and the convolve (for `caller`: plus the elementwise pass)
alone.  Median over the rounds and the spread (min .. max), microseconds.
With --parent-tree (a built checkout of the parent commit): bench.py's default line there against this tree's, alternating too."""
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
MODES = ("fused", "staged", "caller", "ncc")


def worker(name, mode):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
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
        if mode in ("fused", "staged"):
            p.set_match_score(fc.SCORE_SQDIFF, kh, kw)
            p.set_option("norm_store", 1 if mode == "fused" else 0)
        elif mode == "ncc":
            p.set_match_score(fc.SCORE_CCOEFF_NORMED, kh, kw)
        res["norm_direct"] = p.get_option("norm_direct")
        i = p.info
        out = torch.empty((n, i.fft_w, i.fft_h), dtype=torch.float32, device=dev)
        if mode == "caller":      # the caller's own pass: E + c precomputed per map (generous to the caller: c is folded into E ahead of time)
            Ec = torch.rand((n, i.fft_w, i.fft_h), dtype=torch.float32, device=dev)

        def convolve():
            p.convolve_packed_device(n, ker.data_ptr(), kh, kw, out.data_ptr())
            if mode == "caller":
                torch.add(Ec, out, alpha=-2.0, out=out)      # ONE elementwise kernel: -2 * map + (E + c), 4P + 4P read and 4P written per map

        for _ in range(2):
            p.set_image_device(img.data_ptr())
            convolve()
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3 * steps)]
        for s in range(steps):
            ev[3 * s].record(stream)
            p.set_image_device(img.data_ptr())
            ev[3 * s + 1].record(stream)
            convolve()
            ev[3 * s + 2].record(stream)
        torch.cuda.synchronize()
        res["set_image_us"] = statistics.median(ev[3 * s].elapsed_time(ev[3 * s + 1]) for s in range(steps)) * 1e3
        res["convolve_us"] = statistics.median(ev[3 * s + 1].elapsed_time(ev[3 * s + 2]) for s in range(steps)) * 1e3
    print("MATCH_SCORE_AB " + json.dumps(res))


def run_worker(name, mode):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", name, mode], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=240)
    for line in r.stdout.splitlines():
        if line.startswith("MATCH_SCORE_AB "):
            return json.loads(line[len("MATCH_SCORE_AB "):])
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
    ap.add_argument("--worker", nargs=2, default=None)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "match_score_ab.txt"))
    a = ap.parse_args()
    if a.worker:
        return worker(*a.worker)
    lines = ["matching score 4 (SQDIFF): fused / staged / the caller's own pass on one library, fresh processes alternating, %d rounds; "
             "microseconds, median (min .. max)" % a.rounds,
             "(caller: raw maps, then one torch elementwise kernel -2 * map + (E + c) on a precomputed E + c per map; ncc: score 1, for the "
             "set_image step)"]
    try:
        for name in GEOMETRIES:
            runs = {m: [] for m in MODES}
            for _ in range(a.rounds):
                for m in MODES:
                    runs[m].append(run_worker(name, m))
            lines.append("")
            lines.append(name)
            for m in MODES:
                rs = runs[m]
                lines.append("  %-6s norm_direct %d  set_image %s   convolve %s" % (m, rs[0]["norm_direct"], fmt([r["set_image_us"] for r in rs]),
                                                                                   fmt([r["convolve_us"] for r in rs])))
            f, s = [r["convolve_us"] for r in runs["fused"]], [r["convolve_us"] for r in runs["staged"]]
            lines.append("  fused beats staged beyond the spread: %s" % ("yes" if max(f) < min(s) else "NO"))
            print("\n".join(lines[-6:]), flush=True)
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
