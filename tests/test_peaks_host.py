"""Peak lists (fftconv_plan_set_peaks) on the CPU tier.

The kernels of csrc/kernels_peaks.hip scan the delivered maps: every wave counts the thresholded local maxima of its unit, a scan of
the counts gives the offsets, a second pass stores the records in ascending index order.  The candidate test, the neighbourhood
walk, the sub-pixel fit, the record, the cut into units and the rank within a step are ONE header, csrc/peaks.hpp, which the
kernels and tests/peaks_host/peaks_host.cpp both compile.  Checked here without a GPU:
  * the rule on crafted maps against a brute-force restatement, both modes;
  * the cut of an unaligned map into units, the scan of the counts and the assembled lists;
  * the rank within a step against a serial count;
  * the sub-pixel fit;
  * 16-bit element values;
  * the refusals, from the rule tables;
  * the same program under AddressSanitizer and UndefinedBehaviorSanitizer (host compiler, stand-alone);
  * the build's resource reports of the new kernels;
  * the surface that needs no device."""
import os
import re
import subprocess

import numpy as np
import pytest

import util
from test_output_rect_host import _resource_reports

CSRC = os.path.join(util.ROOT, "cuda-fft-convolution_amd", "csrc")
HOST_DIR = os.path.join(util.ROOT, "tests", "peaks_host")


def _build(tmp_path_factory, name, extra):
    exe = str(tmp_path_factory.mktemp(name) / name)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + extra + ["-I", CSRC, "-I", os.path.join(util.ROOT, "tests", "emu"),
                                                                        os.path.join(HOST_DIR, "peaks_host.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    return _build(tmp_path_factory, "peaks_host", ["-O2"])


def _run(exe, mode):
    r = subprocess.run([exe, mode], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "FAIL" not in r.stdout, r.stdout[-3000:]
    return r.stdout


def test_rule_against_brute_force(host_program):
    """14 maps -- ties among few values, all equal, all zero, +-0 alternating (either first), NaN elements, all NaN, +inf and -inf
    planted twice, all -inf, 1 x 1, 1 x n, n x 1, random -- under 8 radii ((0, 0), square, oblong, one dimension only, beyond the
    map, INT_MAX) x 6 thresholds (-inf .. +inf): the header's peaks are the brute force's, index and bits; mode 2 on the negated
    map with the negated threshold gives the same indices.  One peak at index 0 for an all-equal map with a radius, every element
    without one; +-0 tie; an all-NaN map has none."""
    out = _run(host_program, "rule")
    assert re.search(r"rule: 14 of 14 maps agree with the brute force in all 48 cases \(radius x threshold, both modes\), 0 failures", out), out


def test_cut_scan_and_assembly(host_program):
    """4 map shapes (37 x 41, 1 x 263, 129 x 3, 1 x 1) x 4 starts (0 to 3 elements past a 16-byte address) x 3 radii x 2 thresholds,
    each cut into 1, 2, 7, 64 and 1000 units and walked as a wave walks them, with max_peaks below, at and above the count: found is
    the total, the records are the first min(found, max_peaks) peaks in ascending index, nothing beyond them is written."""
    out = _run(host_program, "cut")
    m = re.search(r"cut: (\d+) of (\d+) walks give the ascending-index list and the total, 0 failures", out)
    assert m and m.group(1) == m.group(2) and int(m.group(2)) == 4 * 4 * 3 * 2 * 5 * 3, out


def test_rank_within_a_step(host_program):
    out = _run(host_program, "rank")
    assert "rank: 800 flag sets, every rank the serial count, 0 failures" in out


def test_subpixel_fit(host_program):
    out = _run(host_program, "subpixel")
    assert re.search(r"subpixel: 20000 parabolas within \S+ of their vertex, edges, non-finite values and den == 0 give 0, 0 failures", out), out


def test_16_bit_elements(host_program):
    out = _run(host_program, "values16")
    assert "values16: 6 walks of 16-bit maps agree with the brute force on their fp32 values, 0 failures" in out


def test_refusals_come_from_the_rule_tables(host_program):
    out = _run(host_program, "rules")
    lines = [l for l in out.splitlines() if l.startswith("refusal |")]
    blockwise = [l for l in lines if "block-wise plan" in l]
    assert len(blockwise) == 2 and all("(12 blocks:" in l and "fftconv_plan_options.blockwise = 1" in l for l in blockwise)
    assert len(lines) == 3 and sum("an output window holds a part of a map" in l for l in lines) == 1
    # worded like the extrema rows
    rules = open(os.path.join(CSRC, "plan_rules.hpp")).read()
    ext = re.findall(r'"per-map extrema are ([^"]*)"', rules)
    pks = re.findall(r'"peak lists are ([^"]*)"', rules)
    assert len(ext) == 2 and [e.replace("fftconv_plan_set_extrema", "fftconv_plan_set_peaks") for e in ext] == pks
    # the entry and the group loop look the tables up; neither has a condition of its own
    api = open(os.path.join(CSRC, "fftconv_api.cpp")).read()
    assert "plan_refused(plan, AskPeaks::Peaks, mode)" in api and "plan_refused(p, AskPeaks::PeaksGroup, 1, sink.window != nullptr)" in api
    assert "setter_done(plan, SetterPeaks::Peaks" in api


def test_host_program_under_sanitizers(tmp_path_factory):
    """the same program, every mode, built with -fsanitize=address,undefined by the host compiler as a stand-alone program"""
    exe = _build(tmp_path_factory, "peaks_host_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    out = _run(exe, "all")
    assert "runtime error" not in out and "AddressSanitizer" not in out


def test_peaks_kernels_keep_the_register_rule():
    """the count and the write pass for fp32 and 16-bit elements and the offsets kernel, in the build's own reports: no spilled
    vector register, no scratch"""
    rep = _resource_reports()
    assert rep, "no csrc/*.rpt resource reports beside the objects"
    mine = {k: v for k, v in rep.items() if "k_peaks_" in k}
    assert len(mine) == 5, sorted(mine)
    for name, n in (("k_peaks_count", 2), ("k_peaks_write", 2), ("k_peaks_offsets", 1)):
        assert sum(1 for k in mine if name in k) == n, (name, sorted(mine))
    assert all(v["spill"] == 0 and v["scratch"] == 0 for v in mine.values()), mine


def test_entries_are_exported_and_check_their_plan(fftconv):
    lib = fftconv.load_library()
    header = open(os.path.join(util.ROOT, "include", "fftconv.h")).read()
    for decl in ("typedef struct { float value; int row, col; float d_row, d_col; } fftconv_peak;   /* 20 bytes */",
                 "int fftconv_plan_set_peaks(fftconv_plan *plan, int mode, int max_maps, int max_peaks,\n"
                 "                           float threshold, int radius_h, int radius_w);",
                 "int fftconv_plan_get_peaks(fftconv_plan *plan, int first_map, int n_maps, int *found_host, fftconv_peak *peaks_host);",
                 "int fftconv_plan_peaks_device(fftconv_plan *plan, void **found_device, void **peaks_device, size_t *peaks_bytes);"):
        assert decl in header, decl
    for name in ("fftconv_plan_set_peaks", "fftconv_plan_get_peaks", "fftconv_plan_peaks_device"):
        assert name in fftconv.EXPORTED_SYMBOLS
    assert lib.fftconv_plan_set_peaks(None, 1, 4, 16, 0.5, 1, 1) == -1 and "NULL" in lib.fftconv_last_error().decode()
    assert lib.fftconv_plan_get_peaks(None, 0, 1, None, None) == -1
    assert lib.fftconv_plan_peaks_device(None, None, None, None) == -1
    for method in ("set_peaks", "peaks", "peaks_device"):
        assert hasattr(fftconv.Plan, method)
    assert np.dtype(fftconv.PEAK_DTYPE).itemsize == 20
    assert (fftconv.PEAKS_OFF, fftconv.PEAKS_MAX, fftconv.PEAKS_MIN) == (0, 1, 2)
