#!/usr/bin/env python3
"""A/B of peak lists (fftconv_plan_set_peaks): off, on at two thresholds, the extrema scan for scale, and the caller's own suppression.

    python tools/peaks_ab.py [--parent-tree /path/to/built/parent/checkout] [--rounds 3] [--trace] [--skip-ab | --skip-bench] [--out profiles/peaks_ab.txt]

Fresh processes alternating on one box, as tools/extrema_ab.py does.  Per geometry (cfg3's with 64 maps: 4096^2 (x) 127^2; cfg2's with
16 maps: 1024^2 (x) 63^2), raw fp32 maps of the whole window, radius (3, 3), max_peaks 256, and per mode
    parent   (a) the parent commit's library (--parent-tree), no peaks: the step as it was
    off      (b) this library, peaks off
    few      (c) peaks on at the threshold that leaves map 0 eight candidates (its 8th largest element)
    many     (d) peaks on at the one that leaves it 300 candidates: about max_peaks peaks
    all      (e) peaks on at -inf: every element a candidate, 49 loads each -- the pathological line
    extrema  (f) peaks off, per-map extrema on with "extrema_store" 0: the extrema scan alone, for scale
    caller   (g) peaks off, then the caller's alternative today in torch on the delivered maps: max_pool2d over 7 x 7, compare, threshold,
                 nonzero
a device-resident convolve is timed with HIP events (one process per mode and round); median over the rounds and the spread
(min .. max), microseconds.  --trace: one more process per geometry and threshold under rocprofv3 --kernel-trace --stats, for the time
per map of the three kernels and pass A's rate against the 4P' bytes it reads.  With --parent-tree also bench.py's default line there
against this tree's, alternating."""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOMETRIES = {  # name: H, W, kh, kw, maps, steps
    "cfg3 4096^2 (x) 127^2, 64 maps": (4096, 4096, 127, 127, 64, 6),
    "cfg2 1024^2 (x) 63^2, 16 maps": (1024, 1024, 63, 63, 16, 30),
}
MODES = ("parent", "off", "few", "many", "all", "extrema", "caller")
RADIUS, MAX_PEAKS = 3, 256
CANDIDATES = {"few": 8, "many": 300}


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
        p.set_image_device(img.data_ptr())
        p.convolve_packed_device(n, ker.data_ptr(), kh, kw, out.data_ptr())
        torch.cuda.synchronize()
        threshold = float("-inf")
        if mode in CANDIDATES or mode == "caller":      # (the caller's alternative at the threshold of `few`)
            threshold = float(torch.topk(out[0], CANDIDATES.get(mode, CANDIDATES["few"])).values[-1])
        if mode in ("few", "many", "all"):
            p.set_peaks(fc.PEAKS_MAX, n, MAX_PEAKS, threshold, (RADIUS, RADIUS))
        if mode == "extrema":
            p.set_extrema(1, n)
            p.set_option("extrema_store", 0)
        maps4 = out.view(n, 1, i.fft_w, i.fft_h)

        def convolve():
            p.convolve_packed_device(n, ker.data_ptr(), kh, kw, out.data_ptr())
            if mode == "caller":
                pooled = torch.nn.functional.max_pool2d(maps4, 2 * RADIUS + 1, stride=1, padding=RADIUS)
                return ((maps4 == pooled) & (maps4 >= threshold)).nonzero()

        for _ in range(2):
            convolve()
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * steps)]
        for s in range(steps):
            ev[2 * s].record(stream)
            convolve()
            ev[2 * s + 1].record(stream)
        torch.cuda.synchronize()
        res["convolve_us"] = statistics.median(ev[2 * s].elapsed_time(ev[2 * s + 1]) for s in range(steps)) * 1e3
        res["map_elems"] = i.fft_w * i.fft_h
        if mode in ("few", "many", "all"):
            found = p.peaks()[0]
            res["found"] = [int(found.min()), int(statistics.median(found.tolist())), int(found.max())]
    print("PEAKS_AB " + json.dumps(res))


def run_worker(tree, name, mode, prefix=()):
    r = subprocess.run(list(prefix) + [sys.executable, os.path.abspath(__file__), "--worker", tree, name, mode], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=300)
    for line in r.stdout.splitlines():
        if line.startswith("PEAKS_AB "):
            return json.loads(line[len("PEAKS_AB "):])
    raise RuntimeError("worker %s / %s failed (%d):\n%s" % (name, mode, r.returncode, r.stdout[-2000:]))


def run_trace(name, mode):
    """{kernel family: (calls, average ns)} of the k_peaks_* kernels of one worker under a kernel trace (counters are not collected)"""
    with tempfile.TemporaryDirectory() as d:
        res = run_worker(ROOT, name, mode, prefix=("rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "peaks", "--"))
        out = {}
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                for family in ("k_peaks_count", "k_peaks_offsets", "k_peaks_write"):
                    if family in row.get("Name", ""):
                        out[family] = (int(row["Calls"]), float(row["AverageNs"]))
        return res, out


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
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--skip-ab", action="store_true", help="bench.py's line alone")
    ap.add_argument("--skip-bench", action="store_true", help="the step times alone")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "peaks_ab.txt"))
    a = ap.parse_args()
    if a.worker:
        return worker(*a.worker)
    modes = [m for m in MODES if m != "parent" or a.parent_tree]
    lines = ["peak lists: off / on at three thresholds / the extrema scan / the caller's own torch suppression, fresh processes alternating on one box, "
             "%d rounds; microseconds per convolve, median (min .. max)" % a.rounds,
             "(raw fp32 maps of the whole window, radius (%d, %d), max_peaks %d; found: the least, the median and the most peaks of a map)" % (RADIUS, RADIUS, MAX_PEAKS)]
    try:
        for name in ([] if a.skip_ab else GEOMETRIES):
            runs = {m: [] for m in modes}
            for _ in range(a.rounds):
                for m in modes:
                    runs[m].append(run_worker(os.path.abspath(a.parent_tree) if m == "parent" else ROOT, name, "off" if m == "parent" else m))
            lines.append("")
            lines.append(name)
            first = len(lines)
            for m in modes:
                found = runs[m][0].get("found")
                lines.append("    %-8s convolve %s%s" % (m, fmt([r["convolve_us"] for r in runs[m]]), "   found %d / %d / %d" % tuple(found) if found else ""))
            c = {m: [r["convolve_us"] for r in runs[m]] for m in modes}
            if "parent" in c:
                lines.append("    off within the spread of parent: %s" % ("yes" if min(c["off"]) <= max(c["parent"]) and min(c["parent"]) <= max(c["off"]) else "NO"))
            lines.append("    few faster than the caller's suppression beyond the spread: %s" % ("yes" if max(c["few"]) < min(c["caller"]) else "NO"))
            if a.trace:
                n, elems = GEOMETRIES[name][4], runs["off"][0]["map_elems"]
                for m in ("few", "many"):
                    try:
                        _, k = run_trace(name, m)
                    except (OSError, KeyError, ValueError) as e:      # (no profiler, or statistics in another layout; a worker that failed ends the A/B)
                        k = {"error": str(e)[-300:]}
                    if len(k) != 3:
                        lines.append("    kernel trace (%s): not measured (%s)" % (m, k.get("error", "no k_peaks_* rows in the trace's statistics")))
                        continue
                    convolves = 2 + GEOMETRIES[name][5]               # (of a worker under peaks: two warm, the timed steps)
                    per_map = {f: k[f][0] * k[f][1] / (convolves * n) / 1e3 for f in k}
                    lines.append("    kernel trace (%s): per map, microseconds: k_peaks_count %.2f (%.0f GB/s against its %d bytes)  k_peaks_offsets %.3f  k_peaks_write %.2f"
                                 % (m, per_map["k_peaks_count"], 4 * elems / per_map["k_peaks_count"] / 1e3, 4 * elems, per_map["k_peaks_offsets"], per_map["k_peaks_write"]))
            print("\n".join(lines[first - 1:]), flush=True)
    except (RuntimeError, subprocess.TimeoutExpired) as e:      # (the figures above are kept)
        lines.append("A/B incomplete: %s" % str(e)[-1500:])
        a.parent_tree = None      # (nothing more is started on the device after a worker failed)
    if a.parent_tree and not a.skip_bench:
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
        if vals["parent"] and vals["this"]:
            lines.append("  the ranges overlap: %s" % ("yes" if min(vals["this"]) <= max(vals["parent"]) and min(vals["parent"]) <= max(vals["this"]) else "NO"))
        print("\n".join(lines[-4:]), flush=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
