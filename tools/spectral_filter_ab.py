#!/usr/bin/env python3
"""A/B of the spectral filters (fftconv_plan_set_spectral_filter): modes 0 / 1 / 2 on ONE library, beside the caller's own route.

    python tools/spectral_filter_ab.py [--parent-tree /path/to/built/parent/checkout] [--rounds 3] [--out profiles/spectral_filter_ab.txt]

Fresh processes alternating on one box, as tools/output_stride_ab.py does.  Per geometry (cfg3's with 64 maps: 4096^2 (x) 127^2;
cfg2's with 16 maps: 1024^2 (x) 63^2) and mode
    product  mode 0: the plain kernel (k_fast_rows_multi)
    phase    mode 1: P / |P| in the product phase of k_fast_rows_filter
    wiener   mode 2: I^ conj(K^) / (|K^|^2 + lambda), lambda = 1e-3 of the mean |K^|^2
a device-resident convolve step is timed with HIP events, and the spectral-row kernel alone with the plan's own profile (option
"profile": the event pair around the row launch).  Beside them the only thing a caller could do without the entry, `torch`:
torch.fft.rfft2 of the padded image (once, outside the step) and of the padded kernels, the filter on the half spectra, irfft2 -- at
the plan's own transform lengths, per step of all maps (in chunks of 16 maps: 64 padded 4224^2 spectra do not fit beside each other
comfortably).  Median over the rounds and the spread (min .. max), microseconds.
With --parent-tree (a built checkout of the parent commit): bench.py's default line there against this tree's, alternating too --
mode 0 must be where it was."""
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
MODES = ("product", "phase", "wiener", "torch")


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
    lam = 1e-3 * float((ker.double() ** 2).sum() / n)          # (Parseval: the mean |K^|^2 over the bins is sum k^2)
    stream = torch.cuda.Stream(dev)
    res = {}
    with torch.cuda.stream(stream), fc.Plan(H, W, 1, kh, kw, stream=stream.cuda_stream) as p:
        i = p.info
        Lh, Lw = i.transform_h, i.transform_w
        res.update(transform="%dx%d" % (Lh, Lw), window="%dx%d" % (i.fft_h, i.fft_w))
        if mode == "torch":
            # [w][h] planes as the library holds them: the transform is over both axes, so the layout is only a transpose of the map
            spec = torch.fft.rfft2(img[0], s=(Lw, Lh))
            chunk = 16
            keep = []

            def convolve():
                for c0 in range(0, n, chunk):
                    K = torch.fft.rfft2(ker[c0:c0 + chunk, 0], s=(Lw, Lh))
                    P = spec * K
                    keep[:] = [torch.fft.irfft2(P / P.abs().clamp_min(1e-30), s=(Lw, Lh))[:, :i.fft_w, :i.fft_h]]

            def convolve_wiener():
                for c0 in range(0, n, chunk):
                    K = torch.fft.rfft2(ker[c0:c0 + chunk, 0], s=(Lw, Lh))
                    keep[:] = [torch.fft.irfft2(spec * K.conj() / (K.real ** 2 + K.imag ** 2 + lam), s=(Lw, Lh))[:, :i.fft_w, :i.fft_h]]

            for what, fn in (("phase", convolve), ("wiener", convolve_wiener)):
                for _ in range(2):
                    fn()
                torch.cuda.synchronize()
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * steps)]
                for s in range(steps):
                    ev[2 * s].record(stream)
                    fn()
                    ev[2 * s + 1].record(stream)
                torch.cuda.synchronize()
                res[what] = {"convolve_us": statistics.median(ev[2 * s].elapsed_time(ev[2 * s + 1]) for s in range(steps)) * 1e3}
                keep[:] = []
        else:
            fmode = {"product": fc.FILTER_PRODUCT, "phase": fc.FILTER_PHASE, "wiener": fc.FILTER_WIENER}[mode]
            p.set_spectral_filter(fmode, lam if fmode == fc.FILTER_WIENER else 0.0)
            out = torch.empty((n, i.out_w, i.out_h), dtype=torch.float32, device=dev)

            def convolve():
                p.convolve_packed_device(n, ker.data_ptr(), kh, kw, out.data_ptr())

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
            pr = p.profile()["spectral_rows"]
            res[mode] = {"convolve_us": statistics.median(ev[2 * s].elapsed_time(ev[2 * s + 1]) for s in range(steps)) * 1e3,
                         "rows_us": pr["ms"] * 1e3 / steps, "fast": p.get_option("spectral_filter_fast")}
    print("SPECTRAL_FILTER_AB " + json.dumps(res))


def run_worker(name, mode):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", name, mode], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=300)
    for line in r.stdout.splitlines():
        if line.startswith("SPECTRAL_FILTER_AB "):
            return json.loads(line[len("SPECTRAL_FILTER_AB "):])
    raise RuntimeError("worker %s / %s failed (%d):\n%s" % (name, mode, r.returncode, r.stdout[-2000:]))


def run_bench(tree):
    r = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", "10", "--warmup", "3", "--no-cpu-baseline", "--no-extras"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=tree, timeout=400)
    for line in reversed(r.stdout.splitlines()):
        if line.startswith("{") and "\"value\"" in line:
            return json.loads(line)["value"]
    raise RuntimeError("bench.py failed (%d):\n%s" % (r.returncode, r.stdout[-2000:]))


def fmt(vals):
    return "%10.1f  (%.1f .. %.1f)" % (statistics.median(vals), min(vals), max(vals))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", nargs=2, default=None)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spectral_filter_ab.txt"))
    a = ap.parse_args()
    if a.worker:
        return worker(*a.worker)
    lines = ["spectral filters: modes 0 / 1 / 2 on one library and the caller's own torch.fft route, fresh processes alternating, %d rounds; "
             "microseconds per step of all maps, median (min .. max)" % a.rounds,
             "(row kernel: the plan's own profile of the spectral-row launch alone; torch: rfft2 of the padded kernels at the plan's transform "
             "lengths, the filter on the half spectra against the image's spectrum, irfft2, the window sliced -- the image's rfft2 is outside the step)"]
    try:
        for name in GEOMETRIES:
            runs = {m: [] for m in MODES}
            for _ in range(a.rounds):
                for m in MODES:
                    runs[m].append(run_worker(name, m))
            lines.append("")
            lines.append("%s (transform %s, window %s)" % (name, runs["product"][0]["transform"], runs["product"][0]["window"]))
            for m in ("product", "phase", "wiener"):
                rs = [r[m] for r in runs[m]]
                lines.append("  %-8s spectral_filter_fast %d  convolve %s   row kernel %s" % (m, rs[0]["fast"], fmt([r["convolve_us"] for r in rs]),
                                                                                           fmt([r["rows_us"] for r in rs])))
            base_step = statistics.median(r["product"]["convolve_us"] for r in runs["product"])
            base_rows = statistics.median(r["product"]["rows_us"] for r in runs["product"])
            for m in ("phase", "wiener"):
                t = [r[m]["convolve_us"] for r in runs["torch"]]
                step = statistics.median(r[m]["convolve_us"] for r in runs[m])
                rows = statistics.median(r[m]["rows_us"] for r in runs[m])
                lines.append("  torch    %-6s                   convolve %s" % (m, fmt(t)))
                lines.append("  %-6s / product: step x %.3f, row kernel x %.3f; torch / %s: x %.1f" % (m, step / base_step, rows / base_rows, m, statistics.median(t) / step))
            print("\n".join(lines[-8:]), flush=True)
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
