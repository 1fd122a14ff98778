"""Image batches (fftconv_plan_set_images) on the CPU tier.

One plan convolves B images per launch set: the spectral-row kernels take the image as a grid coordinate that their __global__
wrappers resolve (csrc/fast_paths.hpp: rows_walk_3d, rows_walk_flat, rows_shift_to_image; the generic body takes it in its map
slot), and the per-kernel loop cuts the (image, kernel) grid into launches (csrc/pipeline.hpp: cut_launches).  Checked here without
a GPU:
  * tests/image_batch_host/image_batch_host.cpp, a stand-alone host program over the product's headers (built here with the host
    compiler): the index functions, the launch cutting, and the row bodies through the wrappers' own text;
  * the build's resource reports: no spectral-row kernel spills a register or uses scratch;
  * the surface that needs no device: the exported symbol, the argument check ahead of any device work, the size of the options."""
import ctypes
import glob
import os
import re
import subprocess

import pytest

import util

CSRC = os.path.join(util.ROOT, "cuda-fft-convolution_amd", "csrc")
HOST_DIR = os.path.join(util.ROOT, "tests", "image_batch_host")


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("image_batch_host") / "image_batch_host")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-I", os.path.join(util.ROOT, "tests", "emu"),
                    os.path.join(HOST_DIR, "image_batch_host.cpp"), "-o", exe], check=True)
    return exe


def _run(exe, mode):
    r = subprocess.run([exe, mode], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout[-6000:])
    assert r.returncode == 0, r.stdout[-6000:]
    assert not any(line.startswith("FAIL") for line in r.stdout.splitlines())
    return r.stdout


def test_index_functions_visit_every_pair_once(host_program):
    """grids of (B, N, per_wg) with B = 1, N = 1, N = 17 at per_wg = 16 and B x walks no multiple of 8: every (image, row group,
    kernel) is visited exactly once by the 3-D grid (F = 1, generic) and by the flat XCD-aware grid (F > 1), no walk crosses an
    image, and the flat order keeps the walks of an image adjacent within a row group, images ascending"""
    out = _run(host_program, "index")
    assert "index functions ok" in out and " 0 failed" in out


def test_launch_cutting_tiles_the_grid(host_program):
    """(B, N, chunk, batch_maps) including (3, 2, all, 4), (2, 5, all, 3), (3, 5, chunk of 2, auto), (1, N, ...) and chunks that
    hold several launches with several images (the product's kernel_chunk_mb > 0): the rectangles
    tile the (image, kernel) grid exactly once, the maps of a rectangle are consecutive in the output, a rectangle is one image x
    a kernel range or whole images x every kernel of the call, and one image gives the (first, ny) loop of a one-image plan"""
    out = _run(host_program, "cut")
    assert "launch cutting ok" in out and " 0 failed" in out
    assert "B=3 n=2 stride=2 chunk=2 maps=4: [img 0+2 x k 0+2] [img 2+1 x k 0+2]" in out
    # (2, 5, all, 3): one chunk of five kernels, launches of three maps -- the second launch of each image reads the chunk at offset 3
    assert "B=2 n=5 stride=5 chunk=5 maps=3: [img 0+1 x k 0+3] [img 0+1 x k 3+2] [img 1+1 x k 0+3] [img 1+1 x k 3+2]" in out
    # the same with chunks of three kernels: a chunk per launch, each serving both images before the next is produced
    assert "B=2 n=5 stride=5 chunk=3 maps=3: [img 0+1 x k 0+3] [img 1+1 x k 0+3] [img 0+1 x k 3+2] [img 1+1 x k 3+2]" in out
    assert "B=3 n=7 stride=7 chunk=6 maps=2: [img 0+1 x k 0+2] [img 0+1 x k 2+2] [img 0+1 x k 4+2] [img 1+1 x k 0+2]" in out
    assert "B=3 n=2 stride=2 chunk=2 maps=64: [img 0+3 x k 0+2]" in out


def test_row_bodies_through_the_wrappers_pointer_shift(host_program):
    """L = 288 (eight rows per workgroup), F = 1 with B = 3 x 20 kernels in walks of 16, F = 2 and 3 on the flat grid, the
    row-major intermediate, and the generic body (direct and Bluestein rows, F = 1 / 2 / 3): a batch run writes the same bits as
    per-image runs with the same walk length, and nothing outside its B x nk slots"""
    out = _run(host_program, "rows")
    assert "all bit-equal" in out and " 0 failed" in out
    assert len([l for l in out.splitlines() if l.startswith("ok ")]) == 9


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


def test_row_kernels_keep_their_registers():
    """the image coordinate costs scalar arithmetic only: in the build's own reports no F = 1 walk kernel and neither generic
    spectral-row kernel spills a register or uses scratch, and every one keeps at least the 3 waves per SIMD of its launch bounds;
    the F > 1 walk keeps what it had (tests/test_host_logic.py holds its documented spills)"""
    rep = _resource_reports()
    f1 = {k: v for k, v in rep.items() if "k_fast_rows_multiI" in k}
    gen = {k: v for k, v in rep.items() if "k_spectral_rowsI" in k}
    assert len(f1) >= 60 and len(gen) == 2, (len(f1), len(gen))
    for k, v in list(f1.items()) + list(gen.items()):
        assert v["spill"] == 0 and v["scratch"] == 0 and v["occ"] >= 3, (k, v)
    # the small and mid-sized walks hold the waves they held before the image coordinate: 5 per SIMD (<= 96 registers)
    for L in (480, 576, 960, 1280, 1536):
        mine = [v for k, v in f1.items() if "RowCfgILi%dE" % L in k]
        assert mine and all(v["occ"] >= 5 for v in mine), (L, mine)


def test_entry_is_exported_and_checks_its_arguments(fftconv):
    lib = fftconv.load_library()
    assert "fftconv_plan_set_images" in fftconv.EXPORTED_SYMBOLS
    assert "int fftconv_plan_set_images(fftconv_plan *plan, const float *data, int n_images, int location);" in \
        open(os.path.join(util.ROOT, "include", "fftconv.h")).read()
    buf = (ctypes.c_float * 4)()
    for n in (0, -1):       # refused ahead of any device work (no plan, no device needed to say so)
        assert lib.fftconv_plan_set_images(None, ctypes.cast(buf, ctypes.c_void_p), n, fftconv.HOST) == -1
        assert "n_images" in lib.fftconv_last_error().decode()
    assert lib.fftconv_plan_set_images(None, ctypes.cast(buf, ctypes.c_void_p), 2, fftconv.HOST) == -1
    assert "Invalid data input" in lib.fftconv_last_error().decode()
    assert ctypes.sizeof(fftconv.PlanOptions) == 40          # no new creation option
    for name in ("set_images", "set_images_device", "images"):
        assert hasattr(fftconv.Plan, name)
