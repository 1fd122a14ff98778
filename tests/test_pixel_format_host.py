"""Typed image pixels (fftconv_plan_set_images_typed: uint8 / uint16 / fp16 / bf16 elements, converted in the load) on the CPU tier.

All four conversions to fp32 are exact, so everything here is bit-equality.  Checked without a GPU:
  * the kernel bodies: tests/pixel_format_host/pixel_format_host.cpp, a stand-alone host program over the product's kernel
    headers (built here with the host compiler), runs fast_cols_fwd_body with every pixel type against the fp32 body on the
    converted values, and ncc_column_sums likewise;
  * the fp16 and bf16 conversions of csrc/pixel_format.hpp (the host side: integer arithmetic) over all 65 536 bit patterns
    against NumPy;
  * the load-form decision (a pair of rows in one load only where every pair is aligned) over a table;
  * the surface: the header line, the exported symbol, what is refused without a device;
  * the build's resource reports: every new kernel without spills or scratch at 3 waves per SIMD or more, and the table of
    configurations that are not built says what the reports say."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import util
from test_map_format_host import _resource_reports

CSRC = os.path.join(util.ROOT, "cuda-fft-convolution_amd", "csrc")
HOST_DIR = os.path.join(util.ROOT, "tests", "pixel_format_host")


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pixel_format_host") / "pixel_format_host")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-I", os.path.join(util.ROOT, "tests", "emu"),
                    os.path.join(HOST_DIR, "pixel_format_host.cpp"), "-o", exe], check=True)
    return exe


def _run(host_program, *args):
    r = subprocess.run([host_program] + list(args), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    return r.stdout


def test_typed_bodies_are_bit_equal_to_the_fp32_body(host_program):
    """fast_cols_fwd_body<Cfg, R2, Pixel8 / Pixel16> for a T = 16, a T = 8 and a T = 4 configuration against the fp32 body on the
    converted values: h_in even and odd, pair loads and element loads (chosen by the product's own decision, and forced), ncols
    no multiple of T, three planes, an odd plane stride, an odd base, the dynamic tile queue -- four formats each.  The buffers
    end with the last sample, and the values hold 0, 255, 65535, fp16 / bf16 subnormals, +-0 and 65504."""
    out = _run(host_program, "bodies")
    ok = [line for line in out.splitlines() if line.startswith("ok ")]
    assert len(ok) == 13 * 4 and "all bit-equal" in out
    for what, count in (("T=16", 8), ("T=8", 3), ("T=4", 2), ("dynamic tile queue", 2), ("h_in odd", 5), ("odd plane stride", 1), ("odd base", 1),
                        ("element loads forced", 1)):
        for fmt in (1, 2, 3, 4):
            assert sum(what in line and "format %d " % fmt in line for line in ok) == count, (what, fmt)
    assert sum("(pair loads)" in line for line in ok) == 6 * 4 and sum("(element loads)" in line for line in ok) == 7 * 4


def test_window_statistics_read_typed_pixels(host_program):
    """ncc_column_sums<Pixel8 / Pixel16> against the fp32 text on the converted values: the float64 sums are the same bits"""
    out = _run(host_program, "ncc")
    assert out.count("ok   ncc_column_sums") == 4 and "all bit-equal" in out


def test_conversions_over_every_bit_pattern(host_program, tmp_path):
    """fc_f16_to_f32 / fc_bf16_to_f32 (host side) over all 65 536 patterns against NumPy: non-NaN patterns bit-equal, NaN stays
    NaN.  (The program itself holds them against a reference of its own, and checks the uint8 / uint16 values and the pair loads.)"""
    fout = str(tmp_path / "conv.bin")
    _run(host_program, "convert", fout)
    got = np.fromfile(fout, dtype=np.uint32).reshape(65536, 2)
    bits = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    want16 = bits.view(np.float16).astype(np.float32)
    wantbf = (bits.astype(np.uint32) << 16).view(np.float32)
    for col, want in ((0, want16), (1, wantbf)):
        g = got[:, col].copy().view(np.float32)
        nan = np.isnan(want)
        assert nan.sum() > 0 and np.isnan(g[nan]).all()
        assert np.array_equal(g[~nan].view(np.uint32), want[~nan].view(np.uint32)), col
    # the subnormals are kept: the smallest fp16 subnormal is 2^-24, the smallest bf16 one 2^-133
    assert got[1, 0] == np.float32(2.0 ** -24).view(np.uint32) and got[1, 1] == 0x00010000


def test_load_form_decision(host_program):
    """pixel_pair_load_ok: one load for a pair only where base address, pitch and plane stride are all even in elements (and the
    elements are one or two bytes wide)"""
    rows = [tuple(int(x) for x in line.split()) for line in _run(host_program, "loadform").splitlines()]
    assert len(rows) == 4 * 4 * 4 * 3
    for off, pitch, stride, eb, got in rows:
        want = eb in (1, 2) and off % 2 == 0 and pitch % 2 == 0 and stride % 2 == 0
        assert got == int(want), (off, pitch, stride, eb, got)
    assert sum(r[4] for r in rows) == 2 * 2 * 2 * 2


def test_surface(fftconv):
    hdr = open(os.path.join(util.ROOT, "include", "fftconv.h")).read()
    assert "int fftconv_plan_set_images_typed(fftconv_plan *plan, const void *data, int pixel_format, int n_images, int location);" in hdr
    assert re.search(r"enum \{ FFTCONV_PIXEL_F32 = 0, FFTCONV_PIXEL_U8 = 1, FFTCONV_PIXEL_U16 = 2, FFTCONV_PIXEL_F16 = 3, FFTCONV_PIXEL_BF16 = 4 \};", hdr)
    assert "fftconv_plan_set_images_typed" in fftconv.EXPORTED_SYMBOLS
    assert (fftconv.PIXEL_F32, fftconv.PIXEL_U8, fftconv.PIXEL_U16, fftconv.PIXEL_F16, fftconv.PIXEL_BF16) == (0, 1, 2, 3, 4)
    lib = fftconv.load_library()
    buf = (ctypes.c_ubyte * 16)()
    assert lib.fftconv_plan_set_images_typed(None, buf, 1, 1, 0) == -1                      # NULL plan
    assert lib.fftconv_plan_set_images_typed(None, buf, 9, 1, 0) == -1
    for name in ("set_image_typed", "set_images_typed", "set_images_typed_device"):
        assert callable(getattr(fftconv.Plan, name))
    for name in (b"pixel_store", b"pixel_direct", b"pixel_format"):
        v = ctypes.c_long(0)
        assert lib.fftconv_plan_get_option(None, name, ctypes.byref(v)) == -1


def test_refusals_without_a_device_and_the_route_predicate(host_program, fftconv):
    """argument errors are found before anything touches a device, with set_images' messages; fast_paths.hpp's predicate of the
    direct route reads 1 exactly for "pixel_store" 1 on a one-pass plan with the specialised column pass and a built configuration"""
    lib = fftconv.load_library()
    buf = (ctypes.c_ubyte * 16)()
    assert lib.fftconv_plan_set_images_typed(None, buf, 1, 0, 0) == -1 and b"n_images" in lib.fftconv_last_error()
    assert lib.fftconv_plan_set_images_typed(None, buf, 1, 1, 0) == -1 and b"Invalid data input" in lib.fftconv_last_error()
    out = _run(host_program, "routes")
    assert "ok   direct predicate" in out


def test_new_kernels_do_not_spill_and_the_not_built_table_is_right(host_program):
    """every typed forward-column kernel (one per configuration and element size), the conversion kernel of the staged route and
    the typed window-statistics kernel in the build's own report: no spilled register, no scratch, at least 3 waves per SIMD --
    the bound test_hot_kernels_do_not_spill holds their fp32 siblings to.  A configuration is built exactly if it is not listed in
    FC_COLS_FWD_PX_NOT_BUILT, and a listed one must be absent from the reports."""
    rep = _resource_reports()
    if not rep:
        pytest.skip("no csrc/*.rpt resource reports beside the objects (a library built without csrc/Makefile)")
    out = _run(host_program, "routes").splitlines()
    configs = [int(x) for x in out[0].split()[1:]]
    not_built = [int(x) for x in out[1].split()[1:]]
    assert len(configs) == 32 and set(not_built) <= set(configs)
    px = {k: v for k, v in rep.items() if "k_fast_cols_fwd_pxI" in k}
    for M in configs:
        mine = {k: v for k, v in px.items() if "ColCfgILi%dE" % M in k}
        if M in not_built:
            assert not mine, (M, sorted(mine))
            continue
        assert len(mine) == 2 and sum("Pixel8" in k for k in mine) == 1 and sum("Pixel16" in k for k in mine) == 1, (M, sorted(mine))
        for k, v in mine.items():
            assert v["spill"] == 0 and v["scratch"] == 0 and v["occ"] >= 3, (k, v)
    assert len(px) == 2 * (len(configs) - len(not_built))
    small = {k: v for k, v in rep.items() if "k_pixels_to_f32I" in k or "k_ncc_column_sums_pxI" in k}
    assert len(small) == 4, sorted(small)
    for k, v in small.items():
        assert v["spill"] == 0 and v["scratch"] == 0 and v["occ"] >= 3, (k, v)
