"""Result maps of any rectangle of the window (fftconv_plan_set_output_rect) on the CPU tier.

The specialised output kernel stores the rectangle itself (csrc/fast_cols.hpp: the RECT variant of fast_cols_body).  Checked here
without a GPU:
  * the kernel bodies: tests/output_rect_host/output_rect_host.cpp, a stand-alone host program over the product's kernel headers
    (built here with the host compiler), stores the full fp32 window with the unchanged body and then a list of rectangles with
    the RECT body, through the product's launch decision (fast_paths.hpp: fast_cols_rect_launch_shape), in fp32, fp16 and bf16,
    static deal and dynamic tile queue; every element must be the window's element bit for bit, nothing else may be written;
  * the validation function of csrc/pipeline.hpp;
  * the build's resource reports: the new kernels keep the project's register rule, the existing ones are all still there;
  * the surface that needs no device: the exported symbol, and the argument check ahead of any device work."""
import glob
import os
import re
import subprocess

import pytest

import util

CSRC = os.path.join(util.ROOT, "cuda-fft-convolution_amd", "csrc")
HOST_DIR = os.path.join(util.ROOT, "tests", "output_rect_host")


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("output_rect_host") / "output_rect_host")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-I", os.path.join(util.ROOT, "tests", "emu"),
                    os.path.join(HOST_DIR, "output_rect_host.cpp"), "-o", exe], check=True)
    return exe


def test_rect_bodies_store_the_window_elements(host_program):
    """fast_cols_body<..., RECT> for T = 16 (M = 144), 8 (M = 2112) and 4 (M = 2560) on 288-column windows, and for the 1088-row
    window of the M = 576 transform: ten rectangles each (three for the short window) -- whole window, "same", "valid", odd offsets
    and pitches, one column, one row across a tile boundary, one tile, the last element, an aligned block -- in three formats, with
    the static deal and the dynamic queue, on aligned and on only element-aligned buffers.  Two maps per launch with a poisoned
    band around each; columns outside the launch's tiles are NaN in the intermediate."""
    r = subprocess.run([host_program, "bodies"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:]
    ok = [line for line in r.stdout.splitlines() if line.startswith("ok ")]
    assert "all bit-equal" in r.stdout and not any(line.startswith("FAIL") for line in r.stdout.splitlines())
    # per configuration: 10 rectangles x 3 formats x (static, dynamic), and both again on the other alignment for the five
    # rectangles whose rows are whole pairs (whole window, "same", "valid", one tile, the aligned block); the short window: 3 x 3 x 2 + 2 x 3 x 2
    assert len(ok) == 3 * (10 * 3 * 2 + 5 * 3 * 2) + (3 * 3 * 2 + 2 * 3 * 2), len(ok)
    for what in ("T=16", "T=8", "T=4", "short window"):
        mine = [line for line in ok if line.startswith("ok   %s " % what)]
        assert any(" wide:" in line for line in mine) and any(" elementwise:" in line for line in mine), what
        assert any(" dynamic " in line for line in mine) and any(" static " in line for line in mine), what
        for fmt in (0, 1, 2):
            assert any("format %d" % fmt in line for line in mine), (what, fmt)
    # the wide store only where every pair is whole and aligned: never with an odd offset, an odd pitch or a shifted buffer
    for line in ok:
        m = re.search(r"\((\d+), (\d+), (\d+), (\d+)\) format \d (static|dynamic) shift (\d) (wide|elementwise)", line)
        assert m, line
        even = int(m.group(1)) % 2 == 0 and int(m.group(3)) % 2 == 0 and m.group(6) == "0"
        assert (m.group(7) == "wide") == even, line


def test_rect_validation(host_program):
    """pipeline.hpp: output_rect_error -- inside and touching the edges passes; each way of leaving the window, negative offsets,
    empty and negative sizes (and sums that overflow an int) are named"""
    out = subprocess.run([host_program, "validate"], check=True, stdout=subprocess.PIPE, text=True).stdout.splitlines()
    res = {tuple(int(x) for x in l.split("|")[0].split()): l.split("|")[1].strip() for l in out}
    for ok in ((0, 0, 288, 288), (6, 5, 270, 272), (287, 287, 1, 1), (0, 287, 288, 1), (287, 0, 1, 288), (1, 1, 287, 287)):
        assert res[ok] == "ok", (ok, res[ok])
    for bad in ((1, 0, 288, 288), (0, 1, 288, 288), (0, 0, 289, 1), (0, 0, 1, 289), (288, 0, 1, 1), (0, 288, 1, 1),
                (2147483647, 0, 2147483647, 1), (0, 2147483647, 1, 2147483647)):
        assert "inside the window" in res[bad], (bad, res[bad])
    for bad in ((-1, 0, 10, 10), (0, -1, 10, 10)):
        assert "negative" in res[bad], (bad, res[bad])
    for bad in ((0, 0, 0, 10), (0, 0, 10, 0), (0, 0, -3, 10), (0, 0, 10, -3)):
        assert "at least 1" in res[bad], (bad, res[bad])
    assert len(res) == 20


def _resource_reports():
    """{kernel symbol: {vgpr, spill, scratch, occ}} from the build's csrc/*.rpt (as tests/test_host_logic.py reads them)"""
    subprocess.run(["make", "-C", CSRC], check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = {}
    for path in glob.glob(os.path.join(CSRC, "*.rpt")):
        cur = None
        for line in open(path):
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                cur = out.setdefault(m.group(1), {})
                continue
            for key, pat in ((("vgpr", r" VGPRs: (\d+)"), ("spill", r"VGPRs Spill: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                              ("occ", r"Occupancy \[waves/SIMD\]: (\d+)"))):
                m = re.search(pat, line)
                if m and cur is not None:
                    cur[key] = int(m.group(1))
    return out


def test_rect_kernels_keep_the_register_rule():
    """k_fast_cols_rect / k_fast_cols_rect16 in the build's own report: two instantiations (static deal, dynamic queue) per
    configuration and element class, none for the two configurations that are left to the staged crop; no spilled register, no
    scratch, 3 waves per SIMD, without exception.  The plain kernels are all still there: as many 16-bit as fp32 ones."""
    rep = _resource_reports()
    assert rep, "no csrc/*.rpt resource reports beside the objects"
    hot32 = {k: v for k, v in rep.items() if "k_fast_colsI" in k}
    hot16 = {k: v for k, v in rep.items() if "k_fast_cols16I" in k}
    rect32 = {k: v for k, v in rep.items() if "k_fast_cols_rectI" in k}
    rect16 = {k: v for k, v in rep.items() if "k_fast_cols_rect16I" in k}
    src = open(os.path.join(CSRC, "fast_paths.hpp")).read()
    cols = src[src.index("#define FC_FAST_COL_CONFIGS_G0(X)"):src.index("#define FC_FAST_COL_CONFIGS(X)")]
    nconf = len(re.findall(r"X\(\d+, \d+, \d+, \d+, \d+, \d+\)", cols))
    assert nconf >= 30 and len(hot32) == 3 * nconf + sum(1 for m in re.findall(r"X\((\d+),", cols) if int(m) <= 1056), (nconf, len(hot32))
    assert len(hot16) == len(hot32)
    # (M = 544 and M = 2080 are not built: their rectangle kernels would spill -- fast_paths.hpp: fast_cols_rect_built; the
    #  plans of those two transforms crop the staged window)
    assert len(rect32) == 2 * (nconf - 2) and len(rect16) == 2 * (nconf - 2), (len(rect32), len(rect16), nconf)
    for fam in (rect32, rect16):
        for k, v in fam.items():
            assert "ColCfgILi544E" not in k and "ColCfgILi2080E" not in k, k
            assert v["occ"] >= 3 and v["spill"] == 0 and v["scratch"] == 0, (k, v)
    for m in (2112, 576, 144):      # the benchmark's main shapes
        mine = {k: v for k, v in list(rect32.items()) + list(rect16.items()) if "ColCfgILi%dE" % m in k}
        assert len(mine) == 4 and not any(v["spill"] or v["scratch"] for v in mine.values()), mine


def test_entry_is_exported_and_checks_its_plan(fftconv):
    lib = fftconv.load_library()
    assert "fftconv_plan_set_output_rect" in fftconv.EXPORTED_SYMBOLS
    assert "int fftconv_plan_set_output_rect(fftconv_plan *plan, int off_h, int off_w, int out_h, int out_w);" in \
        open(os.path.join(util.ROOT, "include", "fftconv.h")).read()
    assert lib.fftconv_plan_set_output_rect(None, 0, 0, 1, 1) == -1
    assert "NULL" in lib.fftconv_last_error().decode()
    assert hasattr(fftconv.Plan, "set_output_rect")
