"""Spectral filters (fftconv_plan_set_spectral_filter: phase correlation and Wiener maps) on the CPU tier.

Under a mode the product phase of the spectral-row kernels runs the pointwise function of csrc/spectral_filter.hpp instead of the
complex product: the specialised kernel in its FILTER instantiation (csrc/fast_rows_multi.hpp P3, kernels named
k_fast_rows_filter), the generic one behind a branch (csrc/kernels_body.hpp).  Checked here without a GPU:
  * tests/spectral_filter_host/spectral_filter_host.cpp, a stand-alone host program over the product's headers (built here with
    the host compiler): the pointwise function on edge bins, and the bodies through the emulator's contexts and the wrapper's own
    address arithmetic;
  * the build's resource reports: every filter kernel keeps its registers, the built lengths plus the not-built list are the 32
    row lengths, one kernel per (length, NZ2) of the built ones;
  * the surface that needs no device.

Error bars of the bodies.  Each mode's maps are held to a float64 row computation of the definition; the bar is relative to the
plain product's own error against float64 at the same configuration, twice the largest ratio measured on this tier
(spectral_filter_host.cpp: RATIO_BAR = 3.0 for phase, 11.1 for Wiener).  Measured, random rows, lambda = 1e-3 of the mean |K^|^2:
    configuration                       plain error   phase / plain   Wiener / plain
    288  (270x270 (*) 19x19)            2.19e-07      1.50            5.31
    384  (282x282 (*) 23x23, window 304) 2.20e-07     1.48            4.06
    2112 (250x2100 (*) 9x13)            3.14e-07      1.37            5.55
    2560 (250x2500 (*) 9x41, cropped)   5.05e-07      1.33            4.09
    1152 (40x1100 (*) 9x31, row-major)  2.81e-07      1.33            4.00
    generic 64 (40x52 (*) 7x5)          1.62e-07      1.24            3.83"""
import ctypes
import glob
import os
import re
import subprocess

import pytest

import util

CSRC = os.path.join(util.ROOT, "cuda-fft-convolution_amd", "csrc")
HOST_DIR = os.path.join(util.ROOT, "tests", "spectral_filter_host")


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("spectral_filter_host") / "spectral_filter_host")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-I", os.path.join(util.ROOT, "tests", "emu"),
                    os.path.join(HOST_DIR, "spectral_filter_host.cpp"), "-o", exe], check=True)
    return exe


def _run(exe, mode):
    r = subprocess.run([exe, mode], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout[-6000:])
    assert r.returncode == 0, r.stdout[-6000:]
    assert not any(line.startswith("FAIL") for line in r.stdout.splitlines())
    return r.stdout


def test_pointwise_function_on_edge_bins(host_program):
    """P = 0 gives 0, never NaN; lambda = 0 with K^ = 0 gives 0; denominators up to and past FLT_MAX and down to and below FLT_MIN
    stay finite; ordinary bins agree with float64 to 2e-6; the setter's argument check refuses what the header says"""
    out = _run(host_program, "point")
    assert "pointwise function ok" in out and " 0 failed" in out


def test_filter_bodies_match_the_definition(host_program):
    """FILTER = true at 288 (eight rows per workgroup, two store chains), 384 (six rows, window 304), 2112 (two rows), 2560 (one row,
    cropped window) and 1152 on the row-major intermediate, and the generic body at 64 points, each in modes 1 and 2: every row of
    the first, a middle and the last (partial) row group against float64 within the bars of the module docstring; walks of three
    maps and of one write the same bits; nothing outside the launch's slots; at mode 0 the FILTER body writes the plain body's bits"""
    out = _run(host_program, "rows")
    assert "spectral filter rows ok" in out and " 0 failed" in out
    ok = [l for l in out.splitlines() if l.startswith("ok ")]
    assert len(ok) == 6 and all("mode 0 bit-equal" in l and "ratio phase" in l and "ratio wiener" in l for l in ok)


def _resource_reports():
    subprocess.run(["make", "-C", CSRC], check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = {}
    for path in glob.glob(os.path.join(CSRC, "*.rpt")):
        cur = None
        for line in open(path):
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                cur = out.setdefault(m.group(1), {})
                continue
            for key, pat in (("vgpr", r" VGPRs: (\d+)"), ("spill", r"VGPRs Spill: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                             ("occ", r"Occupancy \[waves/SIMD\]: (\d+)")):
                m = re.search(pat, line)
                if m and cur is not None:
                    cur[key] = int(m.group(1))
    return out


def test_built_kernels_keep_their_registers():
    """every k_fast_rows_filter kernel of the build: no spilled vector register, no scratch, at least the waves per SIMD of its launch
    bounds (2 for the relaxed lengths, else 3); one kernel per (length, NZ2) of the built lengths, and with the lengths of
    FC_ROWS_FILTER_NOT_BUILT (csrc/fast_paths.hpp) the built ones are the 32 row lengths, none in both"""
    rep = {k: v for k, v in _resource_reports().items() if "k_fast_rows_filterI" in k}
    src = open(os.path.join(CSRC, "fast_paths.hpp")).read()
    relaxed = [int(x) for x in re.search(r"FC_ROWS_FILTER_TWO_WAVES\[\] = \{([^}]*)\}", src).group(1).split(",") if x.strip()]
    not_built = [int(x) for x in re.search(r"FC_ROWS_FILTER_NOT_BUILT\[\] = \{([^}]*)\}", src).group(1).split(",") if x.strip()]
    configs = [(int(l), int(nz)) for l, nz in re.findall(r"^\s+X\((\d+), \d+, \d+, \d+, \d+, \d+, (\d+)\)", src, re.M)]
    listed = sorted({l for l, _ in configs})
    assert len(listed) == 32 and len(configs) == len(set(configs))
    seen = []
    for k, v in rep.items():
        m = re.search(r"RowCfgILi(\d+)E.*?EEELi(\d+)EEEv", k)
        length, nz2 = int(m.group(1)), int(m.group(2))
        seen.append((length, nz2))
        assert v["spill"] == 0 and v["scratch"] == 0 and v["occ"] >= (2 if length in relaxed else 3), (k, v)
    built = sorted({l for l, _ in seen})
    assert not set(built) & set(not_built) and sorted(built + not_built) == listed, (built, not_built)
    assert sorted(seen) == sorted(c for c in configs if c[0] in built)
    assert set(relaxed) <= set(built)
    # the plain kernels are still there under their own name, one per configuration, and no filter kernel carries it
    plain = [k for k in _resource_reports() if "k_fast_rows_multiI" in k]
    assert len(plain) == len(configs) and not any("k_fast_rows_multi" in k for k in rep)


def test_surface_without_a_device(fftconv):
    header = open(os.path.join(util.ROOT, "include", "fftconv.h")).read()
    binding = open(os.path.join(util.ROOT, "cuda-fft-convolution_amd", "__init__.py")).read()
    assert "int fftconv_plan_set_spectral_filter(fftconv_plan *plan, int mode, float param);" in header
    assert "enum { FFTCONV_FILTER_PRODUCT = 0, FFTCONV_FILTER_PHASE = 1, FFTCONV_FILTER_WIENER = 2 };" in header
    for name in ('"spectral_filter"', '"spectral_filter_fast"'):
        assert name in header and name in binding, name
    doc = header[header.index("Spectral filters:"):header.index("int fftconv_plan_set_spectral_filter")]
    for word in ("exact_window", "transform_h", "flip_kernels", "kernel_path 1", "graph"):
        assert word in doc, word
    assert (fftconv.FILTER_PRODUCT, fftconv.FILTER_PHASE, fftconv.FILTER_WIENER) == (0, 1, 2)
    assert "fftconv_plan_set_spectral_filter" in fftconv.EXPORTED_SYMBOLS and hasattr(fftconv.Plan, "set_spectral_filter")
    assert ctypes.sizeof(fftconv.PlanOptions) == 40          # no new creation option
    lib = fftconv.load_library()
    assert lib.fftconv_plan_set_spectral_filter(None, 1, 0.0) == -1
    v = ctypes.c_long(7)
    assert lib.fftconv_plan_get_option(None, b"spectral_filter", ctypes.byref(v)) == -1
