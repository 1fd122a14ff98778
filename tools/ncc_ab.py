#!/usr/bin/env python3
"""A/B of normalised cross-correlation maps (fftconv_plan_set_normalisation): off, fused and staged on ONE library.

    python tools/ncc_ab.py [--parent-tree /path/to/built/parent/checkout] [--rounds 3] [--out profiles/ncc_ab.txt]

Fresh processes alternating on one box, as tools/image_batch_ab.py does.  Per geometry (cfg3's with 64 maps: 4096^2 (x) 127^2;
cfg2's with 16 maps: 1024^2 (x) 63^2) and mode
    off     normalisation off: the raw maps
    fused   mode 1, "norm_store" 1: the output kernel multiplies by D ahead of its store
    staged  mode 1, "norm_store" 0: the fp32 window is staged and scaled while it is cropped
a device-resident step is timed with HIP events: set_image(DEVICE) alone (with and without the window statistics), the convolve
alone, and from a second, profiled pass (plan option "profile") the output kernel per map -- the staged mode's extra pass is not
in that slot, it shows in the convolve.  Median over the rounds and the spread (min .. max), microseconds.  The output kernel's
time is set against its bytes: 8C + 4P per map with normalisation off, 8C + 4P + 4P fused if D came from memory every time.
With --parent-tree (a built checkout of the parent commit: its Python stub binds the symbols of ITS header): bench.py's default
line there against this tree's, alternating too."""
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
MODES = ("off", "fused", "staged")


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
        if mode != "off":
            p.set_normalisation(1, kh, kw)
            p.set_option("norm_store", 1 if mode == "fused" else 0)
        res["norm_direct"] = p.get_option("norm_direct")
        i = p.info
        out = torch.empty((n * i.fft_h * i.fft_w,), dtype=torch.float32, device=dev)
        for _ in range(2):
            p.set_image_device(img.data_ptr())
            p.convolve_packed_device(n, ker.data_ptr(), kh, kw, out.data_ptr())
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3 * steps)]
        for s in range(steps):
            ev[3 * s].record(stream)
            p.set_image_device(img.data_ptr())
            ev[3 * s + 1].record(stream)
            p.convolve_packed_device(n, ker.data_ptr(), kh, kw, out.data_ptr())
            ev[3 * s + 2].record(stream)
        torch.cuda.synchronize()
        res["set_image_us"] = statistics.median(ev[3 * s].elapsed_time(ev[3 * s + 1]) for s in range(steps)) * 1e3
        res["convolve_us"] = statistics.median(ev[3 * s + 1].elapsed_time(ev[3 * s + 2]) for s in range(steps)) * 1e3
        p.set_option("profile", 1)
        p.profile()
        for _ in range(steps):
            p.convolve_packed_device(n, ker.data_ptr(), kh, kw, out.data_ptr())
        p.synchronize()
        pr = p.profile()["cols_c2r"]
        res["out_kernel_us_per_map"] = pr["ms"] * 1e3 / max(1, pr["units"])
        # bytes per map of the output kernel: the intermediate (8 bytes per complex bin of the transform's half spectrum) and the map
        res["C"] = (i.transform_h // 2 + 1) * i.fft_w
        res["P"] = i.fft_h * i.fft_w
    print("NCC_AB " + json.dumps(res))


def run_worker(name, mode):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", name, mode], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=240)
    for line in r.stdout.splitlines():
        if line.startswith("NCC_AB "):
            return json.loads(line[7:])
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ncc_ab.txt"))
    a = ap.parse_args()
    if a.worker:
        return worker(*a.worker)
    lines = ["normalised maps: off / fused / staged on one library, fresh processes alternating, %d rounds; microseconds, median (min .. max)" % a.rounds]
    for name in GEOMETRIES:
        runs = {m: [] for m in MODES}
        for _ in range(a.rounds):
            for m in MODES:
                runs[m].append(run_worker(name, m))
        lines.append("")
        lines.append(name)
        for m in MODES:
            rs = runs[m]
            C, P = rs[0]["C"], rs[0]["P"]
            byt = 8 * C + 4 * P + (4 * P if m == "fused" else 0)
            us = statistics.median(r["out_kernel_us_per_map"] for r in rs)
            lines.append("  %-6s norm_direct %d  set_image %s   convolve %s   output kernel per map %s   = %.2f TB/s of %s bytes" % (
                m, rs[0]["norm_direct"], fmt([r["set_image_us"] for r in rs]), fmt([r["convolve_us"] for r in rs]),
                fmt([r["out_kernel_us_per_map"] for r in rs]), byt / us / 1e6, "8C + 8P" if m == "fused" else "8C + 4P"))
        print("\n".join(lines[-4:]), flush=True)
    if a.parent_tree:
        vals = {"parent": [], "this": []}
        try:
            for _ in range(a.rounds):
                vals["parent"].append(run_bench(os.path.abspath(a.parent_tree)))
                vals["this"].append(run_bench(ROOT))
        except (RuntimeError, subprocess.TimeoutExpired) as e:      # (the figures above are kept)
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
