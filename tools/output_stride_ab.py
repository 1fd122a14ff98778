#!/usr/bin/env python3
"""A/B of strided result maps (fftconv_plan_set_output_stride): fused, staged, and the caller's own strided copy, on ONE library.

    python tools/output_stride_ab.py [--parent-tree /path/to/built/parent/checkout] [--rounds 3] [--out profiles/output_stride_ab.txt]

Fresh processes alternating on one box, as tools/match_score_ab.py does.  Per geometry (cfg3's with 64 maps: 4096^2 (x) 127^2; cfg2's
with 16 maps: 1024^2 (x) 63^2), stride ((2,2), (4,4), (1,2), (2,1)) and mode
    fused    "stride_store" 1: the output kernel samples in its store
    staged   "stride_store" 0: the fp32 window is staged, and the crop samples it
    caller   stride (1, 1): the dense maps are stored, then the caller's own strided copy -- the torch slice [:, ::sw, ::sh] of the
             packed maps and .contiguous()
a device-resident convolve step is timed with HIP events (`caller`: plus the copy), and the output kernel alone with the plan's own
profile (option "profile": the event pair around the output launch; the crop and the caller's copy are not in it).  Median over the
rounds and the spread (min .. max), microseconds.  The byte model of the output kernel is 8C + 4P / (sh * sw) against
8C + 4P per map, C = (M + 1) * fft_w complex elements of the intermediate and P = fft_h * fft_w: the predicted fraction stands
beside the measured one (fused output kernel / dense output kernel).
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
STRIDES = ((2, 2), (4, 4), (1, 2), (2, 1))
MODES = ("fused", "staged", "caller")


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
    for sh, sw in STRIDES:
        with torch.cuda.stream(stream), fc.Plan(H, W, 1, kh, kw, stream=stream.cuda_stream) as p:
            if mode != "caller":
                p.set_option("stride_store", 1 if mode == "fused" else 0)
                p.set_output_stride(sh, sw)
            i = p.info
            out = torch.empty((n, i.out_w, i.out_h), dtype=torch.float32, device=dev)
            keep = []

            def convolve():
                p.convolve_packed_device(n, ker.data_ptr(), kh, kw, out.data_ptr())
                if mode == "caller":
                    keep[:] = [out[:, ::sw, ::sh].contiguous()]      # the caller's own strided copy: 4P read (in lines), 4P / (sh sw) written

            p.set_image_device(img.data_ptr())
            for _ in range(2):
                convolve()
            torch.cuda.synchronize()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * steps)]
            for s in range(steps):
                ev[2 * s].record(stream)
                convolve()
                ev[2 * s + 1].record(stream)
            torch.cuda.synchronize()
            p.set_option("profile", 1)
            p.profile()
            for s in range(steps):
                convolve()
            torch.cuda.synchronize()
            pr = p.profile()["cols_c2r"]
            res["%d,%d" % (sh, sw)] = {
                "direct": p.get_option("stride_direct"),
                "convolve_us": statistics.median(ev[2 * s].elapsed_time(ev[2 * s + 1]) for s in range(steps)) * 1e3,
                "out_kernel_us": pr["ms"] * 1e3 / steps,
                "C": (i.transform_h // 2 + 1) * i.fft_w, "P": i.fft_h * i.fft_w,
            }
    print("OUTPUT_STRIDE_AB " + json.dumps(res))


def run_worker(name, mode):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", name, mode], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=300)
    for line in r.stdout.splitlines():
        if line.startswith("OUTPUT_STRIDE_AB "):
            return json.loads(line[len("OUTPUT_STRIDE_AB "):])
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "output_stride_ab.txt"))
    a = ap.parse_args()
    if a.worker:
        return worker(*a.worker)
    lines = ["strided result maps: fused / staged / the caller's own strided copy on one library, fresh processes alternating, %d rounds; "
             "microseconds, median (min .. max)" % a.rounds,
             "(caller: stride (1, 1) maps, then the torch slice [:, ::sw, ::sh] and .contiguous(); output kernel: the plan's own profile of the "
             "output launch alone -- the crop of `staged` and the copy of `caller` are in the convolve step only)"]
    try:
        for name in GEOMETRIES:
            runs = {m: [] for m in MODES}
            for _ in range(a.rounds):
                for m in MODES:
                    runs[m].append(run_worker(name, m))
            lines.append("")
            lines.append(name)
            for sh, sw in STRIDES:
                key = "%d,%d" % (sh, sw)
                lines.append("  stride (%d, %d)" % (sh, sw))
                for m in MODES:
                    rs = [r[key] for r in runs[m]]
                    lines.append("    %-6s stride_direct %d  convolve %s   output kernel %s" % (m, rs[0]["direct"], fmt([r["convolve_us"] for r in rs]),
                                                                                               fmt([r["out_kernel_us"] for r in rs])))
                f, s, c = ([r[key]["convolve_us"] for r in runs[m]] for m in MODES)
                C, P = runs["fused"][0][key]["C"], runs["fused"][0][key]["P"]
                measured = statistics.median(r[key]["out_kernel_us"] for r in runs["fused"]) / statistics.median(r[key]["out_kernel_us"] for r in runs["caller"])
                lines.append("    output kernel, fused / dense: measured %.3f, byte model (8C + 4P / %d) / (8C + 4P) = %.3f" %
                             (measured, sh * sw, (8.0 * C + 4.0 * P / (sh * sw)) / (8.0 * C + 4.0 * P)))
                lines.append("    fused not slower than staged beyond the spread: %s; than the caller's copy: %s" %
                             ("yes" if min(f) <= max(s) else "NO", "yes" if min(f) <= max(c) else "NO"))
            print("\n".join(lines[-(2 + 6 * len(STRIDES)):]), flush=True)
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
