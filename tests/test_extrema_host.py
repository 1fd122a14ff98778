"""Per-map extrema (fftconv_plan_set_extrema) on the CPU tier.

The output kernel finds the largest and the smallest element of every delivered map in its store (csrc/fast_cols.hpp: EXT); what it
cannot serve is read back by a scan kernel; both feed one fold (csrc/kernels_extrema.hip).  The per-element compare-and-take, the
tie rule, the sentinel and the fold step are ONE header, csrc/extrema.hpp, which the device kernels and
tests/extrema_host/extrema_host.cpp both compile.  Checked here without a GPU:
  * the fold over partials in shuffled orders and groupings: the lowest index among equals, +-0, NaN elements, an all-NaN map, the
    empty sentinel, -inf / +inf maps;
  * the 16-bit values the scan reads back, for every bit pattern;
  * the rectangle store's element walk and its indices for odd h_lo / rect_w_lo;
  * the route table: fused or scan for every combination, every pre-existing answer unchanged;
  * the refusals, from the rule table;
  * the same program under AddressSanitizer and UndefinedBehaviorSanitizer (host compiler, stand-alone);
  * the build's resource reports against the not-built lists of csrc/fast_paths.hpp;
  * the surface that needs no device."""
import os
import re
import subprocess

import numpy as np
import pytest

import util
from test_output_rect_host import _resource_reports

CSRC = os.path.join(util.ROOT, "cuda-fft-convolution_amd", "csrc")
HOST_DIR = os.path.join(util.ROOT, "tests", "extrema_host")
FAMILIES = {      # the EXT kernel, its sibling of the same store, its not-built list
    "k_fast_cols_rect_extI": ("k_fast_cols_rectI", "FC_COLS_RECT_EXT_NOT_BUILT"),
    "k_fast_cols_norm_extI": ("k_fast_cols_normI", "FC_COLS_NORM_EXT_NOT_BUILT"),
    "k_fast_cols_sqdiff_extI": ("k_fast_cols_sqdiffI", "FC_COLS_SQDIFF_EXT_NOT_BUILT"),
}


def _build(tmp_path_factory, name, extra):
    exe = str(tmp_path_factory.mktemp(name) / name)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + extra + ["-I", CSRC, "-I", os.path.join(util.ROOT, "tests", "emu"),
                                                                        os.path.join(HOST_DIR, "extrema_host.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    return _build(tmp_path_factory, "extrema_host", ["-O2"])


def _run(exe, mode):
    r = subprocess.run([exe, mode], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "FAIL" not in r.stdout, r.stdout[-3000:]
    return r.stdout


def not_built_lists():
    src = open(os.path.join(CSRC, "fast_paths.hpp")).read()
    return {name: tuple(int(x) for x in re.search(name + r"\[\] = \{([^}]*)\}", src).group(1).split(",")) for _, name in FAMILIES.values()}


def test_fold_yields_the_lowest_index_among_equals(host_program):
    """14 maps -- ties among few values, all equal, all zero, +-0 alternating (either first), NaN elements, a NaN between the
    extremes, all NaN (NaN, -1, -1), all -inf, all +inf, +-inf planted twice, one element, random -- each cut into 1, 2, 7, 64 and
    1000 partials by a random assignment of its elements and folded in a random order and grouping, 20 times each: always the
    first occurrence in memory order, with that element's bits.  The sentinel: empty -> NaN, -1, -1; merging it changes nothing; an
    element equal to its value still wins; a NaN is never taken."""
    out = _run(host_program, "fold")
    assert re.search(r"fold: 14 of 14 maps agree in all 100 shuffled folds, 0 failures", out), out


def test_16_bit_values_are_the_exact_fp32_of_the_element(host_program):
    out = _run(host_program, "values")
    assert "values: 131072 bit patterns, 200000 round trips, 0 failures" in out


def test_rectangle_store_indices(host_program):
    """the walk of the RECT stores over pairs of window rows, for the odd rectangle (3, 5, 2M - 17, 271) of the GPU cases, the whole
    window and five edge rectangles: every delivered element taken exactly once, at col * out_h + row"""
    out = _run(host_program, "index")
    assert "index: 7 of 7 rectangles walked exactly once at their memory-order indices, 0 failures" in out


def test_routes_fused_or_scanned(host_program):
    """output_route.hpp over sinks 4 x host_stream 2 x map sizes 2 x regions 6 x scores 5 x formats 3 x strides 2 (region 4: one) x
    the three "*_store" options 2 x EXT kernels built 8 x extrema_store 2 x plan kinds 4: with extrema off every answer is the
    record's without the new fields; with it on, Fused exactly where the group's store is one of the three fp32 rectangle stores
    (or the whole fp32 window of a one-pass plan on the tiled intermediate, which Rect then stands in for) and its EXT kernel is
    built and "extrema_store" is on -- everything else Scan, and every other answer stays."""
    out = _run(host_program, "routes")
    m = re.search(r"routes: (\d+) combinations, (\d+) unchanged with extrema off, (\d+) fused \((\d+) with the window standing in for a rectangle\), (\d+) scanned, 0 wrong", out)
    assert m, out
    combos, same, fused, swapped, scanned = (int(x) for x in m.groups())
    assert combos == 4 * 2 * 2 * (5 * 2 + 1) * 5 * 3 * 2 * 8 * 2 * 4 and same == combos
    assert fused + scanned == combos * 3 // 4 and fused > 0 and swapped > 0       # (a window sink is refused ahead of the route)
    assert "lists: 0 inconsistent" in out


def test_refusals_come_from_the_rule_table(host_program):
    out = _run(host_program, "rules")
    lines = [l for l in out.splitlines() if l.startswith("refusal |")]
    assert len(lines) == 4 and all("block-wise plan" in l and "fftconv_plan_options.blockwise = 1" in l for l in lines)
    assert "(12 blocks:" in out
    # the entry and the group loop look the tables up; neither has a condition of its own
    api = open(os.path.join(CSRC, "fftconv_api.cpp")).read()
    assert "plan_refused(plan, AskOutput::Extrema, mode)" in api and "plan_refused(p, AskOutput::ExtremaGroup, 1, sink.window != nullptr)" in api
    assert "setter_done(plan, SetterAdded::Extrema" in api


def test_host_program_under_sanitizers(tmp_path_factory):
    """the same program, every mode, built with -fsanitize=address,undefined by the host compiler as a stand-alone program"""
    exe = _build(tmp_path_factory, "extrema_host_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    out = _run(exe, "all")
    assert "runtime error" not in out and "AddressSanitizer" not in out


def test_extrema_kernels_keep_the_register_rule():
    """the three EXT families in the build's own reports: two instantiations (static deal, dynamic queue) per built configuration,
    none for a listed one; no spilled vector register, no scratch, and no wave per SIMD less than the sibling of the same store and
    deal.  Every listed configuration beyond the siblings' own (544, 2080) is listed for a reason that can be read off the
    numbers in fast_paths.hpp; the existing families are all still there, in the numbers they had."""
    rep = _resource_reports()
    assert rep, "no csrc/*.rpt resource reports beside the objects"
    src = open(os.path.join(CSRC, "fast_paths.hpp")).read()
    cols = src[src.index("#define FC_FAST_COL_CONFIGS_G0(X)"):src.index("#define FC_FAST_COL_CONFIGS(X)")]
    ms = [int(m) for m in re.findall(r"X\((\d+), \d+, \d+, \d+, \d+, \d+\)", cols)]
    lists = not_built_lists()
    key = re.compile(r"ColCfgILi(\d+)E.*?ELb([01])E")
    for ext, (sib, list_name) in FAMILIES.items():
        listed = lists[list_name]
        assert 544 in listed and 2080 in listed and all(m in ms for m in listed) and len(set(listed)) == len(listed)
        mine = {key.search(k).groups(): v for k, v in rep.items() if ext in k}
        theirs = {key.search(k).groups(): v for k, v in rep.items() if sib in k}
        assert len(mine) == 2 * (len(ms) - len(listed)), (ext, len(mine))
        for m in ms:
            assert sum(1 for (mm, _) in mine if int(mm) == m) == (0 if m in listed else 2), (ext, m)
        for k, v in mine.items():
            assert v["spill"] == 0 and v["scratch"] == 0 and v["occ"] >= 3 and v["occ"] >= theirs[k]["occ"], (ext, k, v, theirs[k])
    counts = {name: sum(1 for k in rep if name in k) for name in ("k_fast_colsI", "k_fast_cols16I", "k_fast_cols_rectI", "k_fast_cols_rect16I",
                                                                   "k_fast_cols_normI", "k_fast_cols_sqdiffI", "k_fast_cols_strideI")}
    nconf = len(ms)
    plain = 3 * nconf + sum(1 for m in ms if m <= 1056)
    assert counts == {"k_fast_colsI": plain, "k_fast_cols16I": plain, "k_fast_cols_rectI": 2 * (nconf - 2), "k_fast_cols_rect16I": 2 * (nconf - 2),
                      "k_fast_cols_normI": 2 * (nconf - 2), "k_fast_cols_sqdiffI": 2 * (nconf - 2), "k_fast_cols_strideI": 2 * (nconf - 2)}, counts
    # the scan and the fold: small kernels, no spills
    small = {k: v for k, v in rep.items() if "k_extrema_" in k}
    assert len(small) == 3 and all(v["spill"] == 0 and v["scratch"] == 0 for v in small.values()), small


def test_entries_are_exported_and_check_their_plan(fftconv):
    lib = fftconv.load_library()
    header = open(os.path.join(util.ROOT, "include", "fftconv.h")).read()
    for decl in ("typedef struct { float max_value; int max_row, max_col; float min_value; int min_row, min_col; } fftconv_extrema;",
                 "int fftconv_plan_set_extrema(fftconv_plan *plan, int mode, int max_maps);",
                 "int fftconv_plan_get_extrema(fftconv_plan *plan, int first_map, int n_maps, fftconv_extrema *out_host);",
                 "int fftconv_plan_extrema_device(fftconv_plan *plan, void **device_ptr, size_t *bytes);"):
        assert decl in header, decl
    for name in ("fftconv_plan_set_extrema", "fftconv_plan_get_extrema", "fftconv_plan_extrema_device"):
        assert name in fftconv.EXPORTED_SYMBOLS
    assert lib.fftconv_plan_set_extrema(None, 1, 4) == -1 and "NULL" in lib.fftconv_last_error().decode()
    assert lib.fftconv_plan_get_extrema(None, 0, 1, None) == -1
    assert lib.fftconv_plan_extrema_device(None, None, None) == -1
    for method in ("set_extrema", "extrema", "extrema_device"):
        assert hasattr(fftconv.Plan, method)
    assert np.dtype(fftconv.EXTREMA_DTYPE).itemsize == 24
