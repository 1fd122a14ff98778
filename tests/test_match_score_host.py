"""Template-matching scores (fftconv_plan_set_match_score) on the CPU tier.

  * the per-element bodies of the planes Dc = E^(-1/2) / Q = E and of the three kernel preparations with the constant c_k
    (csrc/ncc.hpp, what kernels_score.hip calls): tests/match_score_host/match_score_host.cpp, a stand-alone host program with its
    own main over the product's headers, runs them strip by strip as the launcher does and holds every element to the table of
    include/fftconv.h, brute force in long double -- exact zeros exactly where no non-zero pixel lies under the box; it also builds
    with -fsanitize=address,undefined and then runs directly;
  * the launch-shape decision of the fused additive store (fast_paths.hpp: fast_cols_rect_launch_shape with an Add plane) for the whole window and
    odd rectangles, and through it the ADD body of fast_cols.hpp on the host phase context, with a launch that starts and ends
    inside an image: every element the plain body's element + (Q + c), bit for bit;
  * fast_cols_sqdiff_available for every configuration, the direct predicate over every combination of settings, the argument checks;
  * the surface that needs no device: the exported symbol, the header's declaration, the argument check ahead of any device work."""
import os
import re
import subprocess

import pytest

import util

CSRC = os.path.join(util.ROOT, "cuda-fft-convolution_amd", "csrc")
HOST_DIR = os.path.join(util.ROOT, "tests", "match_score_host")
SOURCE = os.path.join(HOST_DIR, "match_score_host.cpp")
FLAGS = ["-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-I", os.path.join(util.ROOT, "tests", "emu")]


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("match_score_host") / "match_score_host")
    subprocess.run(["g++", "-O2"] + FLAGS + [SOURCE, "-o", exe], check=True)
    return exe


def _ok_lines(exe, what):
    r = subprocess.run([exe, what], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout[-6000:])
    assert r.returncode == 0 and "all within the definition" in r.stdout, r.stdout[-6000:]
    assert not any(line.startswith("FAIL") for line in r.stdout.splitlines())
    return [line for line in r.stdout.splitlines() if line.startswith("ok ")]


def test_planes_meet_the_definition(host_program):
    """40x36x2 / 9x7, 30x50x1 / 5x11, 23x17x3 / 3x3 with a block of zeros larger than the box and a +100 strip, in one strip,
    narrow strips and one column per strip; plain noise at the product's strip width; a box as large as the image; a zero image"""
    ok = _ok_lines(host_program, "planes")
    assert len(ok) == 3 * 4 + 2, ok
    for shape in ("40x36x2 box 9x7", "30x50x1 box 5x11", "23x17x3 box 3x3"):
        mine = [line for line in ok if shape in line]
        zeros = {line.split(" exact zeros")[0].rsplit(" ", 1)[1] for line in mine if "zero block" in line}
        assert len(mine) == 4 and len(zeros) == 1, mine      # the strips do not change a bit
        slack = [line.split(" exact zeros")[0].rsplit(" ", 1)[1] for line in mine if "noise" in line]
        assert int(zeros.pop()) > int(slack[0]) > 0, mine      # exact zeros inside the data too, under the zero block
    assert any("box as large as the image" in line for line in ok) and any("zero image" in line for line in ok)


def test_kernel_preparations_meet_the_definition(host_program):
    """noise, noise on an offset of 1000, a constant kernel and a zero kernel, F = 1 .. 4, up to 31 x 31: scores 2, 3, 4 and c_k"""
    ok = _ok_lines(host_program, "kernels")
    assert len(ok) == 5 * 4 + 1
    assert sum("(zero kernel)" in line for line in ok) == 5 and any("add order" in line for line in ok)


def test_launch_shape_and_fused_body(host_program):
    """five maps from slot 4 of a grid of three kernels per image (the launch is cut inside images 1 and 2; the plane of image 0 is
    NaN): the whole window, the odd rectangle (3, 5, 271, 271) and the last element on the M = 144 configuration, the whole window
    and a rectangle of the 1088-row window on the 1152-point transform; static deal and dynamic queue"""
    ok = _ok_lines(host_program, "shape")
    assert len(ok) == 2 * (3 + 2), ok
    for what in ("T=16 (0, 0, 288, 288)", "T=16 (3, 5, 271, 271)", "short window (0, 0, 1088, 288)", "short window (1001, 9, 87, 21)"):
        mine = [line for line in ok if what in line]
        assert len(mine) == 2 and any(" static " in line for line in mine) and any(" dynamic " in line for line in mine), (what, mine)
    assert all(" wide:" in line for line in ok if "(0, 0, " in line)
    assert all(" elementwise:" in line for line in ok if "(3, 5, " in line)


def _configs():
    src = open(os.path.join(CSRC, "fast_paths.hpp")).read()
    cols = src[src.index("#define FC_FAST_COL_CONFIGS_G0(X)"):src.index("#define FC_FAST_COL_CONFIGS(X)")]
    configs = [int(m) for m in re.findall(r"X\((\d+), \d+, \d+, \d+, \d+, \d+\)", cols)]
    not_built = [int(x) for x in re.search(r"FC_COLS_SQDIFF_NOT_BUILT\[\] = \{([^}]*)\}", src).group(1).split(",")]
    return configs, not_built


def test_direct_predicate_and_argument_checks(host_program):
    """norm_direct under every score: 0 for scores 0 and 2; scores 1 and 3 on the NORM kernels; score 4 on its own family -- each only
    with norm_store 1, a one-pass plan, fp32 maps, the window or a rectangle and a built configuration on the tiled intermediate"""
    ok = _ok_lines(host_program, "direct")
    assert len(ok) == 3
    configs, not_built = _configs()
    m = re.search(r"availability: (\d+) configurations, (\d+) built", ok[0])
    assert m and int(m.group(1)) == len(configs) and int(m.group(2)) == len(configs) - len(not_built), ok[0]
    m2 = re.search(r"predicate: (\d+) settings walked, (\d+) read 1", ok[1])
    assert m2 and int(m2.group(1)) == (len(configs) + 1) * 2 * 5 * 2 * 2 * 3 * 6 and int(m2.group(2)) == 2 * int(m.group(2)), ok[1]


def test_sanitized_build_runs_clean(tmp_path):
    """the same program with -fsanitize=address,undefined, run directly: the planes and the constants end with their last element"""
    exe = str(tmp_path / "match_score_host_san")
    subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] + FLAGS + [SOURCE, "-o", exe], check=True)
    r = subprocess.run([exe, "all"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "all within the definition" in r.stdout and "ERROR" not in r.stdout and "runtime error" not in r.stdout, r.stdout[-6000:]


def test_entry_is_exported_and_checks_its_plan(fftconv):
    lib = fftconv.load_library()
    assert "fftconv_plan_set_match_score" in fftconv.EXPORTED_SYMBOLS
    header = open(os.path.join(util.ROOT, "include", "fftconv.h")).read()
    assert "int fftconv_plan_set_match_score(fftconv_plan *plan, int score, int box_h, int box_w);" in header
    assert "FFTCONV_SCORE_NONE = 0" in header and "FFTCONV_SCORE_SQDIFF = 4" in header
    assert lib.fftconv_plan_set_match_score(None, 4, 3, 3) == -1
    assert "NULL" in lib.fftconv_last_error().decode()
    assert hasattr(fftconv.Plan, "set_match_score")
    assert (fftconv.SCORE_NONE, fftconv.SCORE_CCOEFF_NORMED, fftconv.SCORE_CCOEFF, fftconv.SCORE_CCORR_NORMED, fftconv.SCORE_SQDIFF) == (0, 1, 2, 3, 4)
    # fftconv_plan_set_normalisation keeps its argument check: modes 0 and 1 only
    ncc = open(os.path.join(CSRC, "ncc.hpp")).read()
    assert 'if (mode != 0 && mode != 1) return "normalisation mode is 0 (off) or 1' in ncc


def test_fused_kernels_keep_the_register_rule():
    """k_fast_cols_sqdiff in the build's own resource reports: two instantiations (static deal, dynamic queue) per configuration that
    fast_paths.hpp does not list in FC_COLS_SQDIFF_NOT_BUILT, none for the listed ones; no spilled register, no scratch, at least 3
    waves per SIMD, without exception.  The NORM family is as large as it was."""
    from test_output_rect_host import _resource_reports
    rep = _resource_reports()
    assert rep, "no csrc/*.rpt resource reports beside the objects"
    add = {k: v for k, v in rep.items() if "k_fast_cols_sqdiffI" in k}
    norm = {k: v for k, v in rep.items() if "k_fast_cols_normI" in k}
    configs, not_built = _configs()
    assert 544 in not_built and 2080 in not_built and set(not_built) <= set(configs)
    assert len(add) == 2 * (len(configs) - len(not_built)), (len(add), len(configs), not_built)
    assert len(norm) == 2 * (len(configs) - 2)
    for k, v in add.items():
        assert not any("ColCfgILi%dE" % m in k for m in not_built), k
        assert v["occ"] >= 3 and v["spill"] == 0 and v["scratch"] == 0, (k, v)
    for m in (2112, 576, 144):      # the benchmark's main shapes are fused
        assert sum(1 for k in add if "ColCfgILi%dE" % m in k) == 2, m
