"""The image-walk spectral-row kernel (plan option "image_walk") on the CPU tier.

With "image_walk" 1 a spectral-row launch of more than one image runs fast_rows_images_body (csrc/fast_rows_images.hpp): a
workgroup transforms its kernel row once, keeps the result in registers and walks over the images of the launch
(csrc/fast_paths.hpp: rows_walk_images).  Checked here without a GPU:
  * tests/image_walk_host/image_walk_host.cpp, a stand-alone host program over the product's headers (built here with the host
    compiler): the index function, and the body through the emulator's contexts and the wrapper's own address arithmetic;
  * the build's resource reports: every image-walk kernel that is built keeps its registers and its three waves per SIMD, and the
    built ones plus the not-built predicate's entries are the 32 row lengths;
  * the surface that needs no device: the option names in the header and the binding, the size of the creation options."""
import ctypes
import glob
import os
import re
import subprocess

import pytest

import util

CSRC = os.path.join(util.ROOT, "cuda-fft-convolution_amd", "csrc")
HOST_DIR = os.path.join(util.ROOT, "tests", "image_walk_host")


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("image_walk_host") / "image_walk_host")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-I", os.path.join(util.ROOT, "tests", "emu"),
                    os.path.join(HOST_DIR, "image_walk_host.cpp"), "-o", exe], check=True)
    return exe


def _run(exe, mode):
    r = subprocess.run([exe, mode], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout[-6000:])
    assert r.returncode == 0, r.stdout[-6000:]
    assert not any(line.startswith("FAIL") for line in r.stdout.splitlines())
    return r.stdout


def test_index_function_visits_every_map_once(host_program):
    """grids of (row groups, N, B, per_wg) with N = 1, B = 1, B = 17 at per_wg = 16 and row groups no multiple of 8: every (row
    group, kernel, image) is visited exactly once, no walk runs past the images of the launch, and within a row group the blocks
    of one image walk are consecutive over kernels"""
    out = _run(host_program, "index")
    assert "index function ok" in out and " 0 failed" in out


def test_body_is_walk_independent_and_as_exact_as_the_kernel_walk(host_program):
    """288 (eight rows per workgroup, two store chains), 384 (six rows, window 304), 2112 (two rows, two chains), 2560 (one row,
    cropped) and 1152 on the row-major intermediate, each the configuration the planner picks: walks of 16 + 1, 3 and 1 images of
    a batch of 17 and a batch of 2 write the same bits, nothing outside the B x nk slots, and every row of the first, a middle
    and the last (partial) row group -- each row slot of a workgroup -- is within 2 x the kernel walk's own error of a float64
    row transform"""
    out = _run(host_program, "rows")
    assert "image walk ok" in out and " 0 failed" in out
    ok = [l for l in out.splitlines() if l.startswith("ok ")]
    assert len(ok) == 5 and all("image walk" in l and "kernel walk" in l for l in ok)


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
            for key, pat in (("vgpr", r" VGPRs: (\d+)"), ("spill", r"VGPRs Spill: (\d+)"), ("sspill", r"SGPRs Spill: (\d+)"),
                             ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("occ", r"Occupancy \[waves/SIMD\]: (\d+)")):
                m = re.search(pat, line)
                if m and cur is not None:
                    cur[key] = int(m.group(1))
    return out


def test_built_kernels_keep_their_registers():
    """every k_fast_rows_images kernel of the build: no spilled register, no scratch, at least the 3 waves per SIMD of its launch
    bounds; one kernel per length, and with the lengths of fast_rows_images_built's list (csrc/fast_paths.hpp) they are the 32 row
    lengths, none in both"""
    rep = {k: v for k, v in _resource_reports().items() if "k_fast_rows_imagesI" in k}
    for k, v in rep.items():
        assert v["spill"] == 0 and v["sspill"] == 0 and v["scratch"] == 0 and v["occ"] >= 3, (k, v)
    built = sorted(int(re.search(r"RowCfgILi(\d+)E", k).group(1)) for k in rep)
    assert len(built) == len(set(built)) == len(rep)
    src = open(os.path.join(CSRC, "fast_paths.hpp")).read()
    m = re.search(r"FC_ROWS_IMAGES_NOT_BUILT\[\] = \{([^}]*)\}", src)
    not_built = [int(x) for x in m.group(1).split(",") if x.strip()]
    listed = sorted({int(x) for x in re.findall(r"^\s+X\((\d+), \d+, \d+, \d+, \d+, \d+, \d+\)", src, re.M)})
    assert len(listed) == 32 and len(built) + len(not_built) == 32 and sorted(built + not_built) == listed, (built, not_built)


def test_surface_without_a_device(fftconv):
    header = open(os.path.join(util.ROOT, "include", "fftconv.h")).read()
    binding = open(os.path.join(util.ROOT, "cuda-fft-convolution_amd", "__init__.py")).read()
    for name in ('"image_walk"', '"image_walk_active"'):
        assert name in header and name in binding, name
    assert "batch_maps" in header[header.index('"image_walk"'):][:2500]      # the interplay with the launch cutting is documented
    assert ctypes.sizeof(fftconv.PlanOptions) == 40          # no new creation option
    lib = fftconv.load_library()
    v = ctypes.c_long(7)
    assert lib.fftconv_plan_set_option(None, b"image_walk", 1) == -1 and lib.fftconv_plan_get_option(None, b"image_walk_active", ctypes.byref(v)) == -1
