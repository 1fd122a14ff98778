"""Strided result maps (fftconv_plan_set_output_stride) on the CPU tier.

The specialised output kernel samples in its store (csrc/fast_cols.hpp: the RECT_STRIDE store of fast_cols_body); everything it
cannot serve goes through the fp32 window and the sampling crop (csrc/output_route.hpp).  Checked here without a GPU:
  * the kernel bodies: tests/output_stride_host/output_stride_host.cpp, a stand-alone host program over the product's kernel
    headers (built here with the host compiler), stores the full fp32 window with the unchanged body and then a list of extents at
    a list of strides with the RECT_STRIDE body, through the product's launch decision (fast_paths.hpp:
    fast_cols_stride_launch_shape), static deal and dynamic tile queue; every element must be the window's element bit for bit,
    every element written, nothing else, on exactly the tiles that hold a sampled column;
  * the route table with a stride set, and with stride (1, 1) against the record without the new fields;
  * the argument check (csrc/pipeline.hpp: output_stride_error);
  * the build's resource reports: the new kernels keep the project's register rule, the existing families are all still there;
  * the surface that needs no device: the exported symbol, and the argument check ahead of any device work."""
import os
import re
import subprocess

import pytest

import util
from test_output_rect_host import _resource_reports

CSRC = os.path.join(util.ROOT, "cuda-fft-convolution_amd", "csrc")
HOST_DIR = os.path.join(util.ROOT, "tests", "output_stride_host")
NOT_BUILT = (544, 2080)      # fast_paths.hpp: FC_COLS_STRIDE_NOT_BUILT


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("output_stride_host") / "output_stride_host")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-I", os.path.join(util.ROOT, "tests", "emu"),
                    os.path.join(HOST_DIR, "output_stride_host.cpp"), "-o", exe], check=True)
    return exe


def test_stride_bodies_store_the_sampled_window_elements(host_program):
    """fast_cols_body<..., RECT_STRIDE> for T = 16 (M = 144), 8 (M = 2112) and 4 (M = 2560) on 288-column windows, and for the
    1088-row window of the M = 576 transform.  Six extents each -- whole window, "same", odd offsets with odd sizes, one column, one
    row across a tile boundary, the last element -- at ten strides: (2,1), (1,2), (2,2), (3,5), (4,4), (7,3), (1, T+1) and
    (2, 2T+3), which drop whole tiles, and one stride beyond the extent in each dimension.  Static deal and dynamic queue, aligned
    and only element-aligned buffers.  Two maps per launch with a poisoned band around each; columns of unlaunched tiles are NaN in
    the intermediate; the launch's tile count is the number of distinct window tiles that hold a sampled column."""
    r = subprocess.run([host_program, "bodies"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:]
    lines = r.stdout.splitlines()
    ok = [line for line in lines if line.startswith("ok ")]
    assert "all bit-equal" in r.stdout and not any(line.startswith("FAIL") for line in lines)
    # per configuration: 6 extents x 10 strides x (static aligned, dynamic shifted), and both again on the other alignment for the
    # row-stride-1 cases of the two extents whose rows are whole pairs (whole window, "same": (1,2), (1,T+1), (1, out_w+5))
    assert len(ok) == 4 * (6 * 10 * 2 + 2 * 3 * 2), len(ok)
    pat = re.compile(r"ok   (T=16|T=8|T=4|short window) (.+) \((\d+), (\d+), (\d+), (\d+)\) stride \((\d+), (\d+)\) (static|dynamic) shift (\d) "
                     r"(wide|elementwise): (\d+) x (\d+) maps, (\d+) elements bit-equal on (\d+) tiles")
    tile_w = {"T=16": 16, "T=8": 8, "T=4": 4, "short window": 16}
    for what in tile_w:
        mine = [line for line in ok if line.startswith("ok   %s " % what)]
        assert any(" wide:" in line for line in mine) and any(" elementwise:" in line for line in mine), what
        assert any(" dynamic " in line for line in mine) and any(" static " in line for line in mine), what
    dropped = 0
    for line in ok:
        m = pat.match(line)
        assert m, line
        what, _, off_h, off_w, out_h, out_w, sh, sw, _, shift, store, mh, mw, written, tiles = m.groups()
        off_h, off_w, out_h, out_w, sh, sw, mh, mw, written, tiles = (int(x) for x in (off_h, off_w, out_h, out_w, sh, sw, mh, mw, written, tiles))
        T = tile_w[what]
        assert (mh, mw) == (-(-out_h // sh), -(-out_w // sw)) and written == 2 * mh * mw, line
        # the wide store only with a row stride of 1 where every pair is whole and aligned; element stores otherwise
        even = sh == 1 and off_h % 2 == 0 and out_h % 2 == 0 and shift == "0"
        assert (store == "wide") == even, line
        # the tiles: those of the sampled columns, per map -- fewer than the extent's own range once whole tiles drop out
        want = len({(off_w + j * sw) // T for j in range(mw)})
        assert tiles == 2 * want, line
        dropped += want < (off_w + out_w - 1) // T - off_w // T + 1
    assert dropped > 50, dropped


def test_stride_routes(host_program):
    """output_route.hpp: with a stride, RectStride exactly for stride_store on, a one-pass plan on the tiled intermediate with the
    kernel built, fp32 maps, extent window or rectangle, no plane (scores 0 and 2) -- dense, no crop, staging in OC; everything else
    a crop from the fp32 window in O, staged in OC.  With stride (1, 1) every answer is the one without the new fields."""
    out = subprocess.run([host_program, "routes"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout
    m = re.search(r"routes: (\d+) combinations with a stride, (\d+) RectStride, (\d+) cropped, (\d+) wrong", out.stdout)
    # sinks 3 x host_stream 2 x map sizes 2 x regions 5 (4 is refused) x scores 5 x formats 3 x stride_store 2 x built 2 x plan kinds 4 x strides 3
    assert m and int(m.group(1)) == 3 * 2 * 2 * 5 * 5 * 3 * 2 * 2 * 4 * 3 and int(m.group(4)) == 0, out.stdout
    # RectStride: sinks x host_stream x map sizes x regions {0, 5} x scores {0, 2} x strides, on the one plan kind that has it
    assert int(m.group(2)) == 3 * 2 * 2 * 2 * 2 * 3 and int(m.group(2)) + int(m.group(3)) == int(m.group(1))
    m = re.search(r"unit stride: (\d+) combinations, (\d+) differ", out.stdout)
    assert m and int(m.group(1)) == 3 * 2 * 2 * 6 * 5 * 3 * 2 * 2 * 4 and int(m.group(2)) == 0, out.stdout


def test_stride_validation(host_program):
    """pipeline.hpp: output_stride_error -- strides below 1 are refused; region 4 takes no stride, in both orders (the entry checks
    the new stride against the plan's region, "output_region" checks the new region against the plan's stride: the same function)"""
    out = subprocess.run([host_program, "validate"], check=True, stdout=subprocess.PIPE, text=True).stdout.splitlines()
    res = {tuple(int(x) for x in l.split("|")[0].split()): l.split("|")[1].strip() for l in out}
    for ok in ((1, 1, 0), (2, 3, 0), (1000000, 1, 0), (2, 2, 1), (2, 2, 2), (2, 2, 3), (2, 2, 5), (1, 1, 4)):
        assert res[ok] == "ok", (ok, res[ok])
    for bad in ((0, 1, 0), (1, 0, 0), (-2, 2, 0), (2, -2, 5), (0, 0, 4)):
        assert "at least 1" in res[bad], (bad, res[bad])
    for bad in ((2, 1, 4), (1, 2, 4), (3, 3, 4)):
        assert "output_region 4" in res[bad] and "no stride" in res[bad], (bad, res[bad])
    assert len(res) == 16
    # both orders go through it
    api = open(os.path.join(CSRC, "fftconv_api.cpp")).read()
    assert "output_stride_error(stride_h, stride_w, plan->opt_region)" in api and "output_stride_error(plan->stride_h, plan->stride_w, value)" in api


def test_stride_kernels_keep_the_register_rule():
    """k_fast_cols_stride in the build's own report: two instantiations (static deal, dynamic queue) per built configuration, none
    for a listed one; no spilled vector register, no scratch, at least 3 waves per SIMD, without exception.  The existing families
    are all still there, in the numbers they had."""
    rep = _resource_reports()
    assert rep, "no csrc/*.rpt resource reports beside the objects"
    src = open(os.path.join(CSRC, "fast_paths.hpp")).read()
    cols = src[src.index("#define FC_FAST_COL_CONFIGS_G0(X)"):src.index("#define FC_FAST_COL_CONFIGS(X)")]
    ms = [int(m) for m in re.findall(r"X\((\d+), \d+, \d+, \d+, \d+, \d+\)", cols)]
    nconf = len(ms)
    listed = [int(x) for x in re.search(r"FC_COLS_STRIDE_NOT_BUILT\[\] = \{([^}]*)\}", src).group(1).split(",")]
    assert sorted(listed) == sorted(NOT_BUILT) and all(m in ms for m in listed)
    stride = {k: v for k, v in rep.items() if "k_fast_cols_strideI" in k}
    assert len(stride) == 2 * (nconf - len(listed)), (len(stride), nconf)
    for m in ms:
        mine = {k: v for k, v in stride.items() if "ColCfgILi%dE" % m in k}
        assert len(mine) == (0 if m in listed else 2), (m, sorted(mine))
    for k, v in stride.items():
        assert v["occ"] >= 3 and v["spill"] == 0 and v["scratch"] == 0, (k, v)
    # the other families of the output kernel, counted by the filters their own tests use: none picks up the new kernel
    counts = {name: sum(1 for k in rep if name in k) for name in ("k_fast_colsI", "k_fast_cols16I", "k_fast_cols_rectI", "k_fast_cols_rect16I",
                                                                   "k_fast_cols_normI", "k_fast_cols_sqdiffI")}
    plain = 3 * nconf + sum(1 for m in ms if m <= 1056)
    assert counts == {"k_fast_colsI": plain, "k_fast_cols16I": plain, "k_fast_cols_rectI": 2 * (nconf - 2), "k_fast_cols_rect16I": 2 * (nconf - 2),
                      "k_fast_cols_normI": 2 * (nconf - 2), "k_fast_cols_sqdiffI": 2 * (nconf - 2)}, counts


def test_entry_is_exported_and_checks_its_plan(fftconv):
    lib = fftconv.load_library()
    assert "fftconv_plan_set_output_stride" in fftconv.EXPORTED_SYMBOLS
    assert "int fftconv_plan_set_output_stride(fftconv_plan *plan, int stride_h, int stride_w);" in \
        open(os.path.join(util.ROOT, "include", "fftconv.h")).read()
    assert lib.fftconv_plan_set_output_stride(None, 2, 2) == -1
    assert "NULL" in lib.fftconv_last_error().decode()
    assert hasattr(fftconv.Plan, "set_output_stride")
