#!/usr/bin/env python3
"""A/B of image batches: B images through one plan, per-image calls against one batch.

    python tools/image_batch_ab.py --parent-lib /path/to/parent/libfftconv.so [--rounds 5] [--out profiles/image_batch_ab.txt]

A device-resident step, timed with HIP events on the plan's stream, in fresh processes that alternate between the two libraries
(FFTCONV_LIB; the tool binds the six entries it calls itself):
    loop   B x (set_image(DEVICE) + convolve_packed)          -- what a caller of the parent library does; measured on BOTH libraries
    batch  set_images(DEVICE, B) + convolve_packed             -- this tree's library only
Shapes: BASELINE cfg1 (256^2 (x) 31^2, N = 1) at B = 16 and 64, cfg2 (1024^2 (x) 63^2, N = 16) at B = 8, cfg5 (2048^2 (x) 63^2,
N = 64) at B = 4.  Per shape and mode: the median over the rounds and the spread (min .. max), microseconds per step; the spread
of the alternating runs is the yardstick for "no slower".  The B = 1 headline is bench.py's own line on either library.

    python tools/image_batch_ab.py --image-walk [--rounds 5] [--out profiles/image_walk_ab.txt]

A/B of plan option "image_walk" on ONE library (this tree's): set_images(DEVICE, B) + convolve_packed with the option at 0 and at
1, fresh processes alternating.  Per shape and setting: the step time (HIP events around the timed steps), and from a second,
profiled pass (plan option "profile") the spectral-row kernel's time per map; "image_walk_active" and the walk the plan's rule
picks are printed beside them."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [  # name, H, W, kh, kw, N, B, steps
    ("cfg1 256^2 (x) 31^2 N=1 B=16", 256, 256, 31, 31, 1, 16, 60),
    ("cfg1 256^2 (x) 31^2 N=1 B=64", 256, 256, 31, 31, 1, 64, 30),
    ("cfg2 1024^2 (x) 63^2 N=16 B=8", 1024, 1024, 63, 63, 16, 8, 20),
    ("cfg5 2048^2 (x) 63^2 N=64 B=4", 2048, 2048, 63, 63, 64, 4, 8),
]
# --image-walk: name, H, W, kh, kw, N, B, batch_maps (0: default), rows_group (0: automatic), steps
WALK_SHAPES = [
    ("cfg1 256^2 (x) 31^2 N=1 B=16", 256, 256, 31, 31, 1, 16, 0, 0, 60),
    ("cfg1 256^2 (x) 31^2 N=1 B=64", 256, 256, 31, 31, 1, 64, 0, 0, 30),
    ("cfg1 256^2 (x) 31^2 N=1 B=64 rows_group 16", 256, 256, 31, 31, 1, 64, 0, 16, 30),     # (the automatic walk of so small a batch is one image)
    ("cfg2 1024^2 (x) 63^2 N=16 B=8", 1024, 1024, 63, 63, 16, 8, 0, 0, 20),
    ("cfg2 1024^2 (x) 63^2 N=16 B=8 batch_maps 256", 1024, 1024, 63, 63, 16, 8, 256, 0, 20),
    ("cfg5 2048^2 (x) 63^2 N=64 B=4 batch_maps 256", 2048, 2048, 63, 63, 64, 4, 256, 0, 8),
    ("4096^2 (x) 127^2 N=4 B=8", 4096, 4096, 127, 127, 4, 8, 0, 0, 6),
]


def bind(path):
    """the six entries a step needs, bound here: the parent's library has no fftconv_plan_set_images, and the package's stub
    binds every symbol of this tree's header"""
    import ctypes
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import util
    util.load_package()._preload_hip_runtime()        # one HIP runtime per process: torch's copy
    lib = ctypes.CDLL(path)
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.fftconv_last_error.restype = ctypes.c_char_p
    lib.fftconv_plan_create.argtypes = [ctypes.POINTER(vp), ci, ci, ci, ci, ci, ci, vp]
    lib.fftconv_plan_destroy.argtypes = [vp]
    lib.fftconv_plan_set_image.argtypes = [vp, vp, ci]
    lib.fftconv_plan_convolve_packed.argtypes = [vp, ci, vp, ci, ci, vp]
    lib.fftconv_plan_synchronize.argtypes = [vp]
    if hasattr(lib, "fftconv_plan_set_images"):
        lib.fftconv_plan_set_images.argtypes = [vp, vp, ci, ci]
    return lib


def child(modes):
    import ctypes
    import torch
    lib = bind(os.environ.get("FFTCONV_LIB") or os.path.join(ROOT, "cuda-fft-convolution_amd", "libfftconv.so"))

    def ok(rc):
        if rc:
            raise RuntimeError(lib.fftconv_last_error().decode())

    dev = torch.device("cuda", 0)
    DEVICE = 1
    res = {}
    for name, H, W, kh, kw, N, B, steps in SHAPES:
        s = torch.cuda.Stream(dev)
        with torch.cuda.stream(s):
            g = torch.Generator(device="cpu").manual_seed(11)
            imgs = torch.rand((B, 1, W, H), generator=g, dtype=torch.float32).to(dev)
            ker = torch.rand((N, 1, kw, kh), generator=g, dtype=torch.float32).to(dev)
            fh, fw = (H + kh - 1 + 15) // 16 * 16, (W + kw - 1 + 15) // 16 * 16
            me = fh * fw
            out = torch.empty((B * N * me,), dtype=torch.float32, device=dev)
            per_img = H * W * 4
            p = ctypes.c_void_p(None)
            ok(lib.fftconv_plan_create(ctypes.byref(p), H, W, 1, kh, kw, 0, ctypes.c_void_p(s.cuda_stream)))

            def loop():
                for b in range(B):
                    ok(lib.fftconv_plan_set_image(p, ctypes.c_void_p(imgs.data_ptr() + b * per_img), DEVICE))
                    ok(lib.fftconv_plan_convolve_packed(p, N, ctypes.c_void_p(ker.data_ptr()), kh, kw, ctypes.c_void_p(out.data_ptr() + b * N * me * 4)))

            def batch():
                ok(lib.fftconv_plan_set_images(p, ctypes.c_void_p(imgs.data_ptr()), B, DEVICE))
                ok(lib.fftconv_plan_convolve_packed(p, N, ctypes.c_void_p(ker.data_ptr()), kh, kw, ctypes.c_void_p(out.data_ptr())))

            for mode in modes:
                step = loop if mode == "loop" else batch
                for _ in range(max(3, steps // 4)):
                    step()
                ok(lib.fftconv_plan_synchronize(p))
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                for _ in range(steps):
                    step()
                e1.record(s)
                e1.synchronize()
                res["%s | %s" % (name, mode)] = e0.elapsed_time(e1) * 1000.0 / steps
            ok(lib.fftconv_plan_synchronize(p))
            ok(lib.fftconv_plan_destroy(p))
    print("RESULT " + json.dumps(res))


def walk_child(walk):
    """every WALK_SHAPES entry with "image_walk" = walk: us per step, us of the spectral-row kernel per map"""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import util
    fc = util.load_package()
    dev = torch.device("cuda", 0)
    res = {}
    for name, H, W, kh, kw, N, B, batch_maps, rows_group, steps in WALK_SHAPES:
        s = torch.cuda.Stream(dev)
        with fc.Plan(H, W, 1, kh, kw) as probe:       # (a block-wise plan holds one image: such a size is measured as one pass)
            one_pass = {"blockwise": 1} if probe.get_option("blockwise") else None
        with torch.cuda.stream(s), fc.Plan(H, W, 1, kh, kw, stream=s.cuda_stream, options=one_pass) as p:
            g = torch.Generator(device="cpu").manual_seed(11)
            imgs = torch.rand((B, 1, W, H), generator=g, dtype=torch.float32).to(dev)
            ker = torch.rand((N, 1, kw, kh), generator=g, dtype=torch.float32).to(dev)
            out = torch.empty((B * N, p.info.fft_w, p.info.fft_h), dtype=torch.float32, device=dev)
            p.set_option("image_walk", walk)
            if batch_maps:
                p.set_option("batch_maps", batch_maps)
            if rows_group:
                p.set_option("rows_group", rows_group)

            def step():
                p.set_images_device(imgs.data_ptr(), B)
                p.convolve_packed_device(N, ker.data_ptr(), kh, kw, out.data_ptr())

            for _ in range(max(3, steps // 4)):
                step()
            p.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            for _ in range(steps):
                step()
            e1.record(s)
            e1.synchronize()
            p.set_option("profile", 1)
            p.profile(reset=True)
            for _ in range(3):
                step()
            p.synchronize()
            rows = p.profile(reset=True)["spectral_rows"]
            res[name] = {"step_us": e0.elapsed_time(e1) * 1000.0 / steps, "rows_us_per_map": rows["ms"] * 1000.0 / max(1, rows["units"]),
                         "active": p.get_option("image_walk_active"), "transform": "%dx%d" % (p.info.transform_h, p.info.transform_w),
                         "launches": rows["launches"] // 3}
    print("RESULT " + json.dumps(res))


def walk_main(a):
    runs = {}
    for r in range(a.rounds):
        for walk in (0, 1):
            o = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "walk%d" % walk], stdout=subprocess.PIPE, text=True, timeout=900)
            if o.returncode != 0:
                sys.exit("child failed (image_walk %d, round %d): exit %d" % (walk, r, o.returncode))
            line = [l for l in o.stdout.splitlines() if l.startswith("RESULT ")][-1]
            for k, v in json.loads(line[7:]).items():
                runs.setdefault((k, walk), []).append(v)
    lines = ["image walk: set_images(DEVICE, B) + convolve_packed, plan option image_walk 0 against 1 on the same library",
             "median of %d fresh processes per setting, alternating (min .. max); device-resident, HIP events; rows = the spectral-row" % a.rounds,
             "kernel's time per map from the plan's profile (a second, profiled pass of three steps)", ""]
    for name, *_ in WALK_SHAPES:
        base = statistics.median(v["step_us"] for v in runs[(name, 0)])
        for walk in (0, 1):
            v = runs[(name, walk)]
            st, rw = [x["step_us"] for x in v], [x["rows_us_per_map"] for x in v]
            lines.append("%-46s image_walk %d (active %d, %s, %d row launches)  step %9.1f us (%.1f .. %.1f) x%.3f   rows %7.2f us/map (%.2f .. %.2f)" % (
                name, walk, v[0]["active"], v[0]["transform"], v[0]["launches"], statistics.median(st), min(st), max(st), statistics.median(st) / base,
                statistics.median(rw), min(rw), max(rw)))
        lines.append("")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--image-walk", action="store_true", help="A/B of plan option image_walk on this tree's library")
    ap.add_argument("--parent-lib")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child and a.child.startswith("walk"):
        return walk_child(int(a.child[4:]))
    if a.child:
        return child(a.child.split(","))
    if a.image_walk:
        return walk_main(a)
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        sys.exit("--parent-lib: the parent commit's libfftconv.so")
    runs = {}
    for r in range(a.rounds):
        for which, lib, modes in (("parent", a.parent_lib, "loop"), ("this", None, "loop,batch")):
            env = dict(os.environ)
            env.pop("FFTCONV_LIB", None)
            if lib:
                env["FFTCONV_LIB"] = os.path.abspath(lib)
            o = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", modes], env=env, stdout=subprocess.PIPE, text=True, timeout=600)
            if o.returncode != 0:
                sys.exit("child failed (%s library, round %d): exit %d" % (which, r, o.returncode))
            line = [l for l in o.stdout.splitlines() if l.startswith("RESULT ")][-1]
            for k, v in json.loads(line[7:]).items():
                runs.setdefault("%s | %s" % (k, which), []).append(v)
    lines = ["image batches: microseconds per step of B images (median of %d fresh processes per library, alternating; min .. max)" % a.rounds,
             "loop = B x (set_image + convolve_packed), batch = set_images + convolve_packed; device-resident, HIP events", ""]
    for name, *_ in SHAPES:
        base = runs["%s | loop | parent" % name]
        for key in ("loop | parent", "loop | this", "batch | this"):
            v = runs["%s | %s" % (name, key)]
            lines.append("%-34s %-14s %10.1f   (%.1f .. %.1f)   x%.3f of the parent's loop" % (name, key, statistics.median(v), min(v), max(v),
                                                                                             statistics.median(v) / statistics.median(base)))
        lines.append("")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
