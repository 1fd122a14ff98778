#!/usr/bin/env python3
"""Are the maps of two builds of libfftconv.so the same to the bit?  One seeded run per case of tests/test_rows_nonarith_gpu.py
(every row-kernel path: 4224 / 2112 / 1152, cropped and not, F = 1 and 3, tiled and row-major intermediate) per build:
    FFTCONV_LIB=<build A> python tools/rows_bit_identity.py a.json
    FFTCONV_LIB=<build B> python tools/rows_bit_identity.py b.json          (a fresh process per build: one library per process)
    python tools/rows_bit_identity.py --compare a.json b.json
Per map it records the SHA-256 of the fp32 bytes, the float64 sum, a seeded sample of 16 elements and the error against NumPy's
float64 transforms (max |map - ref| / max |ref|); --compare prints the maps that differ (with the sums and the first differing
sample), per case the largest error of either build, and exits 1 if any map differs.
EXTRA_CASES: one exact_window plan per row length with a 16-point stage 1 (2560 ... 8448), where the compiler contracts a
product and a sum of the last stage-1 butterfly differently once the store-address branch no longer cuts that block.
COLUMN_CASES: the cases above are whole plans, so their maps pass through all four specialised bodies, but their columns are
all short (M = 144).  These turn the shape rule round -- long columns, narrow maps -- for the column transforms M = 576
(16-column tiles, padded LDS image), 1056 (16 columns), 2112 (8 columns, padded, tile queue) and 2560 (4 columns): 48 columns wide
(the rows then run on the generic kernel and the output kernel reads the row-major intermediate) and 288 wide (specialised rows,
tiled intermediate), with F = 3, fp16 maps, an output rectangle at odd offsets and kernel_path 2 once each, and the 15-map shape
whose last round of tiles the output kernel deals in column slices (tests/test_map_format_gpu.py)."""
import hashlib, json, os, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


# name: ((H, W, F, kh, kw, n), plan options): W + kw - 1 = the row length, 5 maps walked 2 at a time
EXTRA_CASES = {"%d-radix16" % L: ((40, L - 62, 1, 9, 63, 5), {"exact_window": 1, "rows_group": 2}) for L in (2560, 3072, 5632, 6144, 7680, 8448)}
# ... and the one F > 1 kernel whose listing grew (3360 = 10.24.14, NZ2 = 5: a path of its walk is laid out twice)
EXTRA_CASES["3360-F3-nz5"] = ((40, 3360 - 62, 3, 9, 63, 3), {"exact_window": 1, "rows_group": 2})
# name: ((H, W, F, kh, kw, n), plan options, options set on the plan, output rectangle or None): H + kh - 1 = the column length
COLS = {"rows_group": 2, "blockwise": 1}
COLUMN_CASES = {"cols-%d" % L: ((L - 62, 40, 1, 63, 9, 5), COLS, {}, None) for L in (1152, 2112, 4224, 5120)}
COLUMN_CASES["cols-2112-F3"] = ((2112 - 62, 40, 3, 63, 9, 5), COLS, {}, None)
COLUMN_CASES.update({"cols-%d-tiled" % L: ((L - 62, 280, 1, 63, 9, 5), COLS, {}, None) for L in (1152, 2112, 4224, 5120)})
COLUMN_CASES["cols-2112-tiled-F3"] = ((2112 - 62, 280, 3, 63, 9, 5), COLS, {}, None)
COLUMN_CASES["cols-4224-tiled-fp16"] = ((4224 - 62, 280, 1, 63, 9, 5), COLS, {"map_format": 1}, None)
COLUMN_CASES["cols-1152-tiled-odd-rect"] = ((1152 - 62, 280, 1, 63, 9, 5), COLS, {}, (3, 1, 1001, 277))
COLUMN_CASES["cols-2112-row-major"] = ((2112 - 62, 280, 1, 63, 9, 5), dict(COLS, kernel_path=2), {}, None)
COLUMN_CASES["cols-1152-tiled-sliced-tail"] = ((1060, 270, 1, 20, 11, 15), {}, {}, None)


def record(path):
    import numpy as np
    import test_rows_nonarith_gpu as tg
    import util
    fc = util.load_package()
    out = {"library": fc.LIB_PATH, "cases": {}}
    row_cases = [(name, shape, options, {}, None) for name, (shape, options, *_rest) in list(tg.CASES.items()) + list(EXTRA_CASES.items())]
    for name, shape, options, settings, rect in row_cases + [(name, *case) for name, case in COLUMN_CASES.items()]:
        H, W, F, kh, kw, n = shape
        data, ks = tg.make_inputs(shape, sum(shape))
        with fc.Plan(H, W, F, kh, kw, options=options) as p:
            if name in COLUMN_CASES:    # the column length as the case says, on the specialised kernels (-tiled: the rows too)
                spec = p.get_option("specialised_kernels")
                assert spec & 2 and (spec == 3 or "tiled" not in name) and p.get_option("blockwise") == 0 and p.info.transform_h == int(name.split("-")[1]), name
                print("%-28s transform %d x %d, window %d x %d, specialised_kernels %d" % (name, p.info.transform_h, p.info.transform_w, p.info.fft_h, p.info.fft_w, spec))
            else:
                assert p.get_option("specialised_kernels") & 1 and (name not in EXTRA_CASES or p.info.transform_w == W + kw - 1), name
            for key, value in settings.items():
                p.set_option(key, value)
            if rect:
                p.set_output_rect(*rect)
            p.set_image(data)
            maps = p.convolve(ks)
        ref = util.numpy_fft_conv(data, kh, kw, ks)
        if rect:
            ref = [r[rect[0]:rect[0] + rect[2], rect[1]:rect[1] + rect[3]] for r in ref]
        idx = np.random.default_rng(len(name)).integers(0, maps[0].size, 16)
        out["cases"][name] = [{"sha256": hashlib.sha256(np.ascontiguousarray(m).tobytes()).hexdigest(), "sum": float(m.sum(dtype=np.float64)),
                               "sample": [float(x) for x in np.ascontiguousarray(m).ravel()[idx]],
                               "err": float(np.abs(m.astype(np.float64) - r).max() / np.abs(r).max())} for m, r in zip(maps, ref)]
    with open(path, "w") as f:
        json.dump(out, f)
    print("recorded %d cases of %s in %s" % (len(out["cases"]), out["library"], path))


def compare(a, b):
    A, B = json.load(open(a)), json.load(open(b))
    bad = total = 0
    for name in A["cases"]:
        for i, (x, y) in enumerate(zip(A["cases"][name], B["cases"][name])):
            total += 1
            if x["sha256"] != y["sha256"]:
                bad += 1
                d = next(((p, q) for p, q in zip(x["sample"], y["sample"]) if p != q), None)
                print("DIFFERENT %s map %d: sums %.17g / %.17g, sample %s" % (name, i, x["sum"], y["sum"], d))
    for name in A["cases"]:
        ea, eb = [m["err"] for m in A["cases"][name]], [m["err"] for m in B["cases"][name]]
        print("%-28s error against float64, worst / best map: %.3e / %.3e   %.3e / %.3e" % (name, max(ea), min(ea), max(eb), min(eb)))
    print("%s vs %s: %d of %d maps differ in %d cases" % (A["library"], B["library"], bad, total, len(A["cases"])))
    return 1 if bad else 0


if __name__ == "__main__":
    if sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    record(sys.argv[1])
