"""Normalised cross-correlation maps (fftconv_plan_set_normalisation) on the CPU tier.

  * the per-element bodies of the window statistics and of the kernel normalisation (csrc/ncc.hpp, what kernels_ncc.hip calls):
    tests/ncc_host/ncc_host.cpp, a stand-alone host program with its own main over the product's header, runs them strip by
    strip as the launcher does and holds every element to the brute-force definition in long double -- exact zeros exactly where
    the definition floors; it also builds with -fsanitize=address,undefined and then runs directly;
  * the map-to-image index, the strip widths and the argument check of the same header;
  * the launch-shape decision of the fused scale (fast_paths.hpp: fast_cols_rect_launch_shape with a Scale plane) for the whole window and for
    rectangles, with image0 > 0 and per_image > 1, and through it the NORM body of fast_cols.hpp on the host phase context: every
    element the plain body's element times D of its map's image, bit for bit;
  * fast_cols_norm_available for every configuration and the norm_direct predicate over every combination of settings;
  * the surface that needs no device: the exported symbol, the header's declaration, the argument check ahead of any device work."""
import os
import subprocess

import pytest

import util

CSRC = os.path.join(util.ROOT, "cuda-fft-convolution_amd", "csrc")
HOST_DIR = os.path.join(util.ROOT, "tests", "ncc_host")


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ncc_host") / "ncc_host")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-I", os.path.join(util.ROOT, "tests", "emu"),
                    os.path.join(HOST_DIR, "ncc_host.cpp"), "-o", exe], check=True)
    return exe


def _ok_lines(exe, what):
    r = subprocess.run([exe, what], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout[-6000:])
    assert r.returncode == 0 and "all within the definition" in r.stdout, r.stdout[-6000:]
    assert not any(line.startswith("FAIL") for line in r.stdout.splitlines())
    return [line for line in r.stdout.splitlines() if line.startswith("ok ")]


def test_window_statistics_meet_the_definition(host_program):
    """40x36x2 / 9x7, 30x50x1 / 5x11, 23x17x3 / 3x3 with a flat patch larger than the box and a +100 strip, in one strip, narrow
    strips and one column per strip; plain noise at the product's strip width; box 1x1 (D = 0 everywhere); a box as large as the
    image; a constant and a zero image"""
    ok = _ok_lines(host_program, "stats")
    assert len(ok) == 3 * 5 + 3, ok
    for shape in ("40x36x2 box 9x7", "30x50x1 box 5x11", "23x17x3 box 3x3"):
        mine = [line for line in ok if shape in line]
        assert len(mine) == 4 and len({line.split(" exact zeros")[0].rsplit(" ", 1)[1] for line in mine if "patch+strip" in line}) == 1, mine
    assert sum("box 1x1" in line for line in ok) == 3 and any("box as large as the image" in line for line in ok)


def test_kernel_normalisation_meets_the_definition(host_program):
    """noise, noise on an offset of 1000, a constant kernel and one constant per plane, F = 1 .. 4, up to 31 x 31"""
    ok = _ok_lines(host_program, "kernels")
    assert len(ok) == 5 * 4
    assert sum("(all zeros)" in line for line in ok) == 5 * 2 + 2      # the constant kinds, and every 1 x 1 kernel


def test_index_strips_and_arguments(host_program):
    ok = _ok_lines(host_program, "index")
    assert len(ok) == 3


def test_launch_shape_and_fused_body(host_program):
    """four maps of images 1 and 2 (two kernels per image; the plane of image 0 is NaN): the whole window (pair stores kept), the
    odd rectangle (3, 5, 271, 271), an aligned block and the last element on the M = 144 configuration, the whole window and a
    rectangle of the 1088-row window on the 1152-point transform; static deal and dynamic queue"""
    ok = _ok_lines(host_program, "shape")
    assert len(ok) == 2 * (4 + 2), ok
    for what in ("T=16 (0, 0, 288, 288)", "T=16 (3, 5, 271, 271)", "short window (0, 0, 1088, 288)", "short window (1001, 9, 87, 21)"):
        mine = [line for line in ok if what in line]
        assert len(mine) == 2 and any(" static " in line for line in mine) and any(" dynamic " in line for line in mine), (what, mine)
    assert all(" wide:" in line for line in ok if "(0, 0, " in line)            # the whole window keeps the pair stores
    assert all(" elementwise:" in line for line in ok if "(3, 5, " in line)


def test_norm_direct_for_every_configuration(host_program):
    """norm_direct reads 1 only with mode 1, norm_store 1, a one-pass plan, fp32 maps, the window or a rectangle and a built
    configuration on the tiled intermediate: 0 for map_format 1 / 2, regions 1-4, plans without a configuration (generic,
    Bluestein, kernel_path 1), the row-major intermediate (kernel_path 2), block-wise plans and M = 544 / 2080"""
    import re
    ok = _ok_lines(host_program, "direct")
    assert len(ok) == 2
    src = open(os.path.join(CSRC, "fast_paths.hpp")).read()
    cols = src[src.index("#define FC_FAST_COL_CONFIGS_G0(X)"):src.index("#define FC_FAST_COL_CONFIGS(X)")]
    nconf = len(re.findall(r"X\(\d+, \d+, \d+, \d+, \d+, \d+\)", cols))
    m = re.search(r"availability: (\d+) configurations, (\d+) built", ok[0])
    assert m and int(m.group(1)) == nconf and int(m.group(2)) <= nconf - 2, ok[0]
    m2 = re.search(r"predicate: (\d+) settings walked, (\d+) read 1", ok[1])
    assert m2 and int(m2.group(1)) == (nconf + 1) * 2 * 2 * 2 * 2 * 3 * 6 and int(m2.group(2)) == 2 * int(m.group(2)), ok[1]


def test_entry_is_exported_and_checks_its_plan(fftconv):
    lib = fftconv.load_library()
    assert "fftconv_plan_set_normalisation" in fftconv.EXPORTED_SYMBOLS
    assert "int fftconv_plan_set_normalisation(fftconv_plan *plan, int mode, int box_h, int box_w);" in \
        open(os.path.join(util.ROOT, "include", "fftconv.h")).read()
    assert lib.fftconv_plan_set_normalisation(None, 1, 3, 3) == -1
    assert "NULL" in lib.fftconv_last_error().decode()
    assert hasattr(fftconv.Plan, "set_normalisation")


def test_fused_kernels_keep_the_register_rule():
    """k_fast_cols_norm in the build's own resource reports: two instantiations (static deal, dynamic queue) per configuration
    that fast_paths.hpp does not list in FC_COLS_NORM_NOT_BUILT, none for the listed ones; no spilled register, no scratch, at
    least 3 waves per SIMD, without exception.  The other families are as many as they were."""
    import re
    from test_output_rect_host import _resource_reports
    rep = _resource_reports()
    assert rep, "no csrc/*.rpt resource reports beside the objects"
    norm = {k: v for k, v in rep.items() if "k_fast_cols_normI" in k}
    rect32 = {k: v for k, v in rep.items() if "k_fast_cols_rectI" in k}
    src = open(os.path.join(CSRC, "fast_paths.hpp")).read()
    cols = src[src.index("#define FC_FAST_COL_CONFIGS_G0(X)"):src.index("#define FC_FAST_COL_CONFIGS(X)")]
    configs = [int(m) for m in re.findall(r"X\((\d+), \d+, \d+, \d+, \d+, \d+\)", cols)]
    not_built = [int(x) for x in re.search(r"FC_COLS_NORM_NOT_BUILT\[\] = \{([^}]*)\}", src).group(1).split(",")]
    assert 544 in not_built and 2080 in not_built and set(not_built) <= set(configs)
    assert len(norm) == 2 * (len(configs) - len(not_built)), (len(norm), len(configs), not_built)
    assert len(rect32) == 2 * (len(configs) - 2)
    for k, v in norm.items():
        assert not any("ColCfgILi%dE" % m in k for m in not_built), k
        assert v["occ"] >= 3 and v["spill"] == 0 and v["scratch"] == 0, (k, v)
    for m in (2112, 576, 144):      # the benchmark's main shapes are fused
        assert sum(1 for k in norm if "ColCfgILi%dE" % m in k) == 2, m
