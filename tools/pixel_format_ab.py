#!/usr/bin/env python3
"""A/B of typed image pixels (fftconv_plan_set_images_typed): the fp32 set_images of the parent commit on the same values against
uint8 staged, uint8 direct and fp16 direct of this tree.

    python tools/pixel_format_ab.py [--parent-tree /path/to/built/parent/checkout] [--rounds 3] [--out profiles/pixel_format_ab.txt]

Fresh processes alternating on one box, as tools/ncc_ab.py does; every process runs under its own time limit and the first one
that fails ends the run.  The timed step is the set_images step alone, per shape (cfg5's 2048^2 image -- the streamed-image
shape --, cfg3's 4096^2, cfg1's 256^2 with B = 64) and variant
    fp32        set_images of the exact fp32 values (the parent tree's library with --parent-tree, else this tree's)
    u8 staged   "pixel_store" 0: H2D of the bytes, one conversion kernel, then the fp32 call from device memory
    u8 direct   "pixel_store" 1: the column kernel converts in its load
    f16 direct  the same with fp16 elements
device-resident (HIP events around the call) and host-in (the wall clock of the blocking call, pageable NumPy array in, stream
synchronised), plus the image column pass from the plan's profile (slot "image_cols"; the staged conversion is counted in it).
Median over the rounds and the spread (min .. max), microseconds.  With --parent-tree: bench.py's default line there against
this tree's, alternating too."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {  # name: H, W, kh, kw, B, steps
    "cfg5 2048^2 (x) 63^2": (2048, 2048, 63, 63, 1, 20),
    "cfg3 4096^2 (x) 127^2": (4096, 4096, 127, 127, 1, 10),
    "cfg1 256^2 (x) 31^2, B = 64": (256, 256, 31, 31, 64, 20),
}
VARIANTS = ("fp32", "u8 staged", "u8 direct", "f16 direct")


def worker(tree, name, variant):
    sys.path.insert(0, os.path.join(tree, "tests"))
    import numpy as np
    import torch
    import util
    fc = util.load_package()
    H, W, kh, kw, B, steps = SHAPES[name]
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(3)
    u8 = np.asfortranarray(rng.integers(0, 256, (H, W, 1, B), dtype=np.uint16).astype(np.uint8))
    host = {"fp32": u8.astype(np.float32), "u8 staged": u8, "u8 direct": u8, "f16 direct": u8.astype(np.float16)}[variant]
    host = np.asfortranarray(host)
    flat = np.ascontiguousarray(np.transpose(host, (3, 2, 1, 0))).reshape(-1)
    d = torch.from_numpy(flat.view(np.int16) if flat.dtype == np.float16 else flat).to(dev)
    fmt = {"fp32": 0, "u8 staged": 1, "u8 direct": 1, "f16 direct": 3}[variant]
    stream = torch.cuda.Stream(dev)
    res = {}
    with torch.cuda.stream(stream), fc.Plan(H, W, 1, kh, kw, stream=stream.cuda_stream) as p:
        if fmt:
            p.set_option("pixel_store", 0 if variant.endswith("staged") else 1)
            res["pixel_direct"] = p.get_option("pixel_direct")
            set_dev = lambda: p.set_images_typed_device(d.data_ptr(), fmt, B)
            set_host = lambda: p.set_images_typed(host)
        else:
            set_dev = lambda: p.set_images_device(d.data_ptr(), B)
            set_host = lambda: p.set_images(host)
        for _ in range(2):
            set_dev()
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * steps)]
        for s in range(steps):
            ev[2 * s].record(stream)
            set_dev()
            ev[2 * s + 1].record(stream)
        torch.cuda.synchronize()
        res["device_us"] = statistics.median(ev[2 * s].elapsed_time(ev[2 * s + 1]) for s in range(steps)) * 1e3
        p.set_option("profile", 1)
        p.profile()
        for _ in range(steps):
            set_dev()
        p.synchronize()
        pr = p.profile()["image_cols"]
        res["device_cols_us"] = pr["ms"] * 1e3 / max(1, pr["launches"])
        p.set_option("profile", 0)
        for _ in range(2):
            set_host()
        p.synchronize()
        ts = []
        for _ in range(steps):
            t0 = time.perf_counter()
            set_host()
            p.synchronize()
            ts.append((time.perf_counter() - t0) * 1e6)
        res["host_us"] = statistics.median(ts)
        res["host_bytes"] = int(host.nbytes)
    print("PIXEL_AB " + json.dumps(res))


def run_worker(tree, name, variant):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", tree, name, variant], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=180)
    for line in r.stdout.splitlines():
        if line.startswith("PIXEL_AB "):
            return json.loads(line[9:])
    raise RuntimeError("worker %s / %s failed (%d):\n%s" % (name, variant, r.returncode, r.stdout[-2000:]))


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pixel_format_ab.txt"))
    a = ap.parse_args()
    if a.worker:
        return worker(*a.worker)
    parent = os.path.abspath(a.parent_tree) if a.parent_tree else None
    lines = ["typed image pixels: the set_images step, fresh processes alternating, %d rounds; microseconds, median (min .. max); fp32: %s" % (
        a.rounds, "the parent commit's library" if parent else "this tree's library")]
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
                runs[v].append(run_worker(parent if (v == "fp32" and parent) else ROOT, name, v))
        lines.append("")
        lines.append(name)
        for v in VARIANTS:
            rs = runs[v]
            lines.append("  %-10s pixel_direct %s  device-resident call %s   image column pass %s   host-in call %s  (%d bytes in)" % (
                v, rs[0].get("pixel_direct", "-"), fmt([r["device_us"] for r in rs]), fmt([r["device_cols_us"] for r in rs]),
                fmt([r["host_us"] for r in rs]), rs[0]["host_bytes"]))
        print("\n".join(lines[-(len(VARIANTS) + 1):]), flush=True)
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
