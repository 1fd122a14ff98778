#!/usr/bin/env python3
"""A/B of border modes (fftconv_plan_set_border): what a bordered image costs in the device-resident set_image / set_images step.

    python tools/border_ab.py [--parent-tree /path/to/built/parent/checkout] [--rounds 3] [--out profiles/border_ab.txt]

Fresh processes alternating on one box, as tools/ncc_ab.py does; every process runs under its own time limit and the first one
that fails ends the run.  The timed step is the device-resident set_images step (HIP events around the call) and the image
column pass alone (the plan's profile, slot "image_cols": the staged extension is counted in it), per shape (cfg5's 2048^2,
cfg3's 4096^2, cfg1's 256^2 with B = 64) and route
    zero        no border (the parent tree's library with --parent-tree, else this tree's)
    direct      mode 4 (reflect-101), "border_store" 1: the column kernel maps the indices in its load
    staged      mode 4, "border_store" 0: k_extend_image writes the extended image, the plain column kernel runs on it
    caller pad  what a caller does without the entry: torch.nn.functional.pad(mode="reflect") of the image by (lead, trail), then
                set_images on a zero-border plan of the PADDED size (its window and transform length are printed)
and, at cfg3's shape, one full step (set_image + convolve_packed of 64 maps) for direct against caller pad (the padded plan
with the rectangle that removes the rim, so both store the same H x W maps).
Median over the rounds and the spread (min .. max), microseconds.  With --parent-tree: bench.py's default line there against
this tree's, alternating too."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {  # name: H, W, kh, kw, B, steps
    "cfg5 2048^2 (x) 63^2": (2048, 2048, 63, 63, 1, 20),
    "cfg3 4096^2 (x) 127^2": (4096, 4096, 127, 127, 1, 10),
    "cfg1 256^2 (x) 31^2, B = 64": (256, 256, 31, 31, 64, 20),
}
VARIANTS = ("zero", "direct", "staged", "caller pad")
STEP_SHAPE, STEP_MAPS = "cfg3 4096^2 (x) 127^2", 64
MODE = 4


def worker(tree, name, variant, what):
    sys.path.insert(0, os.path.join(tree, "tests"))
    import numpy as np
    import torch
    import util
    fc = util.load_package()
    H, W, kh, kw, B, steps = SHAPES[name]
    dev = torch.device("cuda", 0)
    img = torch.from_numpy(np.random.default_rng(3).standard_normal((B, 1, W, H), dtype=np.float32)).to(dev)      # [b][f][w][h]
    lh, lw = kh // 2, kw // 2
    pads = (lh, kh - 1 - lh, lw, kw - 1 - lw)      # (last dimension first: h, then w)
    padded = variant == "caller pad"
    PH, PW = (H + kh - 1, W + kw - 1) if padded else (H, W)
    stream = torch.cuda.Stream(dev)
    res = {}
    with torch.cuda.stream(stream), fc.Plan(PH, PW, 1, kh, kw, stream=stream.cuda_stream) as p:
        res["window"] = "%d x %d" % (p.info.fft_h, p.info.fft_w)
        res["transform"] = "%d x %d" % (p.info.transform_h, p.info.transform_w)
        if variant in ("direct", "staged"):
            p.set_option("border_store", 1 if variant == "direct" else 0)
            p.set_border(MODE)
            res["border_direct"] = p.get_option("border_direct")
        elif padded:      # the rectangle that removes the rim: the same H x W maps as the bordered plan's
            p.set_output_rect(kh - 1, kw - 1, H, W)
        keep = []

        def set_dev():
            if padded:
                e = torch.nn.functional.pad(img, pads, mode="reflect")
                keep[:] = [e]
                p.set_images_device(e.data_ptr(), B)
            else:
                p.set_images_device(img.data_ptr(), B)

        n = STEP_MAPS if what == "step" else 0
        if n:
            ker = torch.from_numpy(np.random.default_rng(4).standard_normal((n, 1, kw, kh), dtype=np.float32)).to(dev)
            out = torch.empty((n, W, H), dtype=torch.float32, device=dev)
            assert (p.info.out_h, p.info.out_w) == (H, W)

        def step():
            set_dev()
            if n:
                p.convolve_packed_device(n, ker.data_ptr(), kh, kw, out.data_ptr())

        for _ in range(2):
            step()
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * steps)]
        for s in range(steps):
            ev[2 * s].record(stream)
            step()
            ev[2 * s + 1].record(stream)
        torch.cuda.synchronize()
        res["device_us"] = statistics.median(ev[2 * s].elapsed_time(ev[2 * s + 1]) for s in range(steps)) * 1e3
        if not n:
            p.set_option("profile", 1)
            p.profile()
            for _ in range(steps):
                set_dev()
            p.synchronize()
            pr = p.profile()["image_cols"]
            res["device_cols_us"] = pr["ms"] * 1e3 / max(1, pr["launches"])
            p.set_option("profile", 0)
    print("BORDER_AB " + json.dumps(res))


def run_worker(tree, name, variant, what="image"):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", tree, name, variant, what], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=180)
    for line in r.stdout.splitlines():
        if line.startswith("BORDER_AB "):
            return json.loads(line[10:])
    raise RuntimeError("worker %s / %s / %s failed (%d):\n%s" % (name, variant, what, r.returncode, r.stdout[-2000:]))


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
    ap.add_argument("--worker", nargs=4, default=None)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "border_ab.txt"))
    a = ap.parse_args()
    if a.worker:
        return worker(*a.worker)
    parent = os.path.abspath(a.parent_tree) if a.parent_tree else None
    lines = ["border modes (mode %d): the device-resident set_images step, fresh processes alternating, %d rounds; microseconds, median (min .. max); zero: %s" % (
        MODE, a.rounds, "the parent commit's library" if parent else "this tree's library")]
    try:
        measure(a, parent, lines)
    finally:      # (what was measured before a failure is kept)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def measure(a, parent, lines):
    for name in SHAPES:
        runs = {v: [] for v in VARIANTS}
        for _ in range(a.rounds):      # (a worker that fails or runs out of time raises: nothing more is started)
            for v in VARIANTS:
                runs[v].append(run_worker(parent if (v == "zero" and parent) else ROOT, name, v))
        lines.append("")
        lines.append(name)
        for v in VARIANTS:
            rs = runs[v]
            lines.append("  %-10s border_direct %s  window %-11s transform %-11s  device-resident call %s   image column pass %s" % (
                v, rs[0].get("border_direct", "-"), rs[0]["window"], rs[0]["transform"], fmt([r["device_us"] for r in rs]),
                fmt([r["device_cols_us"] for r in rs])))
        print("\n".join(lines[-(len(VARIANTS) + 1):]), flush=True)
    steps = {v: [] for v in ("direct", "caller pad")}
    for _ in range(a.rounds):
        for v in steps:
            steps[v].append(run_worker(ROOT, STEP_SHAPE, v, "step"))
    lines.append("")
    lines.append("one full step at %s: set_image + convolve_packed of %d maps (H x W maps both ways)" % (STEP_SHAPE, STEP_MAPS))
    for v, rs in steps.items():
        lines.append("  %-10s window %-11s transform %-11s  %s" % (v, rs[0]["window"], rs[0]["transform"], fmt([r["device_us"] for r in rs])))
    print("\n".join(lines[-3:]), flush=True)
    if parent:
        vals = {"parent": [], "this": []}
        for _ in range(a.rounds):
            vals["parent"].append(run_bench(parent))
            vals["this"].append(run_bench(ROOT))
        lines.append("")
        lines.append("bench.py --gpus 1 --steps 10 --warmup 3 (Gpixel-filters/s), alternating")
        for k in ("parent", "this"):
            lines.append("  %-6s %s" % (k, fmt(vals[k])))
        print("\n".join(lines[-3:]), flush=True)


if __name__ == "__main__":
    main()
