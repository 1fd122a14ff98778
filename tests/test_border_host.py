"""Border modes (fftconv_plan_set_border: constant / replicate / symmetric / reflect-101 / circular, mapped in the load) on the CPU tier.

Checked without a GPU:
  * the index function of csrc/border.hpp for every mode, n = 1..40 and every admissible MAXK against numpy.pad (and, inside the
    host program, against a modular-arithmetic reference of its own), with the exact fold limits;
  * border_args_error over a table of refusals;
  * fast_paths.hpp's predicate of the direct route over every configuration and setting, and the not-built table against the
    build's resource reports;
  * the kernel body: tests/border_host/border_host.cpp, a stand-alone host program over the product's kernel headers (built here
    with the host compiler), runs fast_cols_fwd_body with the border against the plain body on the materialised extension --
    bit-equal;
  * accuracy: the maps of a bordered plan through the emulator (the bordered forward pass of the host program, the emulator
    library's per-kernel loop) against float64 within util.BUDGET_DIRECT, for the two specialised shapes of the GPU tier;
  * the surface: the header line, the exported symbol, what is refused without a device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import util
from test_map_format_host import _resource_reports

CSRC = os.path.join(util.ROOT, "cuda-fft-convolution_amd", "csrc")
HOST_DIR = os.path.join(util.ROOT, "tests", "border_host")
PAD_MODES = {1: "constant", 2: "edge", 3: "symmetric", 4: "reflect", 5: "wrap"}


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("border_host") / "border_host")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-I", os.path.join(util.ROOT, "tests", "emu"),
                    os.path.join(HOST_DIR, "border_host.cpp"), "-o", exe], check=True)
    return exe


def _run(host_program, *args):
    r = subprocess.run([host_program] + list(args), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    return r.stdout


def reference_maps(data, ks, mkh, mkw, mode, value=0.0, flip=False):
    """float64 "same" maps of the image extended by numpy.pad: full convolution of the padded image, rows and columns
    [MAXK - 1, MAXK - 1 + DATA)"""
    H, W, F = data.shape
    lh, lw = mkh // 2, mkw // 2
    pad = ((lh, mkh - 1 - lh), (lw, mkw - 1 - lw), (0, 0))
    kw = {"constant_values": value} if mode == 1 else {}
    e = np.pad(data.astype(np.float64), pad, mode=PAD_MODES[mode], **kw)
    fh, fw = e.shape[0] + mkh - 1, e.shape[1] + mkw - 1
    E = np.fft.rfft2(e, s=(fh, fw), axes=(0, 1))
    out = []
    for k in ks:
        k = np.asarray(k, dtype=np.float64)
        if flip:
            k = k[::-1, ::-1, :]
        full = np.fft.irfft2(E * np.fft.rfft2(k, s=(fh, fw), axes=(0, 1)), s=(fh, fw), axes=(0, 1)).sum(axis=2)
        out.append(full[mkh - 1:mkh - 1 + H, mkw - 1:mkw - 1 + W])
    return out


def test_index_function_against_numpy_pad(host_program):
    """every mode, n = 1..40, every MAXK border_args_error admits (modes 1 and 2: up to 2n + 3): the source index of every window
    coordinate is numpy.pad's of arange(n) with (lead, trail) = (MAXK / 2, MAXK - 1 - MAXK / 2); the first refused MAXK is the
    fold limit of the mode"""
    out = _run(host_program, "index")
    assert "FAIL" not in out
    rows, limits = 0, {}
    for line in out.splitlines():
        if line.startswith("limit"):
            _, mode, n, maxk = line.split()
            limits[(int(mode), int(n))] = int(maxk)
            continue
        head, idx = line.split(":")
        mode, n, maxk = (int(x) for x in head.split())
        got = np.array([int(x) for x in idx.split()])
        lead = maxk // 2
        kw = {"constant_values": -1} if mode == 1 else {}
        want = np.pad(np.arange(n), (lead, maxk - 1 - lead), mode=PAD_MODES[mode], **kw)
        assert np.array_equal(got, want), (mode, n, maxk, got, want)
        rows += 1
    assert len(limits) == 5 * 40
    for (mode, n), maxk in limits.items():
        # the smallest MAXK with MAXK / 2 > n (3, 5) or > n - 1 (4); modes 1 and 2 have none (the walk stops beyond 2n + 3)
        want = {1: 2 * n + 4, 2: 2 * n + 4, 3: 2 * n + 2, 4: 2 * n, 5: 2 * n + 2}[mode]
        assert maxk == want, (mode, n, maxk)
    assert rows == sum(limits.values()) - len(limits)


def test_argument_errors(host_program):
    """a mode outside 0..5, a value that is not finite (whatever the mode), and the fold limits in each dimension by itself:
    modes 3 and 5 need MAXK / 2 <= DATA, mode 4 MAXK / 2 <= DATA - 1"""
    got = {}
    for line in _run(host_program, "errors").splitlines():
        key, why = line.split(" -> ")
        got[tuple(key.split())] = why
    ok = lambda *k: got[tuple(str(x) for x in k)] == "ok"
    why = lambda *k: got[tuple(str(x) for x in k)]
    assert "border mode is 0" in why(-1, 0, 8, 8, 3, 3) and "border mode is 0" in why(6, 0, 8, 8, 3, 3)
    assert ok(0, 0, 8, 8, 3, 3) and ok(5, 0, 8, 8, 3, 3) and ok(1, -1.25, 8, 8, 3, 3)
    for v in ("inf", "-inf", "nan"):
        assert "finite" in why(1, v, 8, 8, 3, 3)
    assert "finite" in why(2, "nan", 8, 8, 3, 3)
    for mode in (3, 5):
        assert ok(mode, 0, 4, 9, 9, 3) and ok(mode, 0, 9, 4, 3, 9)
        assert "MAX_KERNEL / 2 <= DATA in" in why(mode, 0, 4, 9, 10, 3) and "MAX_KERNEL / 2 <= DATA in" in why(mode, 0, 9, 4, 3, 10)
    assert ok(4, 0, 4, 9, 7, 3) and ok(4, 0, 9, 4, 3, 7) and ok(4, 0, 1, 1, 1, 1)
    assert "DATA - 1" in why(4, 0, 4, 9, 8, 3) and "DATA - 1" in why(4, 0, 9, 4, 3, 8) and "DATA - 1" in why(4, 0, 1, 1, 2, 1)
    assert ok(3, 0, 1, 1, 3, 3) and "fold an index twice" in why(3, 0, 1, 1, 4, 1)
    assert ok(2, 0, 1, 1, 31, 31) and ok(1, 0, 1, 1, 31, 31)
    assert len(got) == 27


def test_direct_route_predicate(host_program):
    """fast_cols_fwd_border_direct over every configuration (and a length without one) x store x block-wise x fast_fwd: 1 exactly
    for "border_store" 1 on a one-pass plan with the specialised column pass and a built configuration"""
    out = _run(host_program, "routes")
    assert "ok   direct predicate: 264 settings walked" in out and "FAIL" not in out


def test_bordered_body_is_bit_equal_to_the_body_on_the_extension(host_program):
    """fast_cols_fwd_body<Cfg, R2, float, Bordered> on the 288-point configuration (M = 144) against the plain body on the
    extension materialised by the program's own reference: every mode, H odd and even, MAXK odd and even (lead != trail), columns
    no multiple of T, three planes, the dynamic tile queue, a border deeper than the data is wide"""
    out = _run(host_program, "bodies")
    ok = [line for line in out.splitlines() if line.startswith("ok ")]
    assert len(ok) == 6 * 5 and "all bit-equal" in out
    for mode in range(1, 6):
        assert sum("mode %d:" % mode in line for line in ok) == 6
    for what in ("H even, MAXK odd", "H odd, MAXK odd", "H even, MAXK even", "H odd, MAXK even mode", "dynamic tile queue", "deep border"):
        assert sum(what in line for line in ok) == 5, what


@pytest.fixture(scope="module")
def emu():
    lib = ctypes.CDLL(util.build_emu())
    lib.emu_spectrum_elems.restype = ctypes.c_long
    return lib


@pytest.mark.parametrize("shape", [(250, 250, 1, 31, 31, 3), (251, 249, 2, 12, 10, 3)])
def test_accuracy_through_the_emulator(host_program, emu, tmp_path, shape):
    """the maps of a bordered plan -- the forward pass with the border (host program), then the emulator library's per-kernel loop
    on that spectrum -- against float64 on the numpy.pad extension, every mode, within util.BUDGET_DIRECT on the "same" rectangle
    (util.normal_inputs: the second kernel is the ragged cell; CONSTANT with value 0.5)"""
    H, W, F, kh, kw, n = shape
    data, ks = util.normal_inputs(shape, 77 + H)
    d, kk, n, kp, khs, kws = util.Oracle._prep(data, ks)
    fin, fout = str(tmp_path / "img.bin"), str(tmp_path / "spec.bin")
    d.transpose(2, 1, 0).astype(np.float32).tofile(fin)      # [f][w][h]
    nspec = emu.emu_spectrum_elems(H, W, F, kh, kw)
    fh, fw = util.ceil16(H + kh - 1), util.ceil16(W + kw - 1)
    for mode in range(1, 6):
        value = 0.5 if mode == 1 else 0.0
        out = _run(host_program, "spectrum", fin, fout, str(H), str(W), str(F), str(kh), str(kw), str(mode), str(value))
        assert "transform 288 x 288" in out, out
        spec = np.fromfile(fout, dtype=np.float32)
        assert spec.size == 2 * nspec
        outs = [np.full((fh, fw), 7e7, dtype=np.float32, order="F") for _ in range(n)]
        op = (ctypes.c_void_p * n)(*[o.ctypes.data for o in outs])
        assert emu.emu_convolve_spectrum(ctypes.c_void_p(spec.ctypes.data), H, W, F, kh, kw, n, kp, khs, kws, op) == 0
        refs = reference_maps(data, ks, kh, kw, mode, value)
        for j, (o, r) in enumerate(zip(outs, refs)):
            m = util.accuracy(o[kh - 1:kh - 1 + H, kw - 1:kw - 1 + W], r)
            print("shape %s mode %d map %d: max %.2e  L2 %.2e  spectral %.2e" % (shape, mode, j, *m))
            assert all(x < b for x, b in zip(m, util.BUDGET_DIRECT)), (shape, mode, j, m, util.BUDGET_DIRECT)


def test_surface(fftconv):
    hdr = open(os.path.join(util.ROOT, "include", "fftconv.h")).read()
    assert "int fftconv_plan_set_border(fftconv_plan *plan, int mode, float value);" in hdr
    assert re.search(r"enum \{ FFTCONV_BORDER_ZERO = 0, FFTCONV_BORDER_CONSTANT = 1, FFTCONV_BORDER_REPLICATE = 2, FFTCONV_BORDER_SYMMETRIC = 3,\s+"
                     r"FFTCONV_BORDER_REFLECT101 = 4, FFTCONV_BORDER_CIRCULAR = 5 \};", hdr)
    assert "fftconv_plan_set_border" in fftconv.EXPORTED_SYMBOLS
    assert (fftconv.BORDER_ZERO, fftconv.BORDER_CONSTANT, fftconv.BORDER_REPLICATE, fftconv.BORDER_SYMMETRIC, fftconv.BORDER_REFLECT101,
            fftconv.BORDER_CIRCULAR) == (0, 1, 2, 3, 4, 5)
    lib = fftconv.load_library()
    assert lib.fftconv_plan_set_border(None, 3, 0.0) == -1 and b"plan is NULL" in lib.fftconv_last_error()
    assert callable(fftconv.Plan.set_border)
    for name in (b"border_store", b"border_direct", b"border_mode", b"border_lead_h", b"border_lead_w"):
        v = ctypes.c_long(0)
        assert lib.fftconv_plan_get_option(None, name, ctypes.byref(v)) == -1


def test_new_kernels_do_not_spill_and_the_not_built_table_is_right(host_program):
    """every bordered forward-column kernel in the build's own report against its plain sibling (the full variant of the same
    configuration): no spilled register, no scratch, not a wave per SIMD fewer.  A configuration is built exactly if it is not
    listed in FC_COLS_FWD_BORDER_NOT_BUILT, and a listed one must be absent from the reports.  The staged kernel does not spill."""
    rep = _resource_reports()
    if not rep:
        pytest.skip("no csrc/*.rpt resource reports beside the objects (a library built without csrc/Makefile)")
    out = _run(host_program, "routes").splitlines()
    configs = [int(x) for x in out[0].split()[1:]]
    not_built = [int(x) for x in out[1].split()[1:]]
    assert len(configs) == 32 and set(not_built) <= set(configs)
    bd = {k: v for k, v in rep.items() if "k_fast_cols_fwd_borderI" in k}
    for M in configs:
        mine = {k: v for k, v in bd.items() if "ColCfgILi%dE" % M in k}
        if M in not_built:
            assert not mine, (M, sorted(mine))
            continue
        assert len(mine) == 1, (M, sorted(mine))
        (k, v), = mine.items()
        r2 = re.search(r"ColCfgILi%dELi\d+ELi(\d+)E" % M, k).group(1)
        plain = [vv for kk, vv in rep.items() if re.search(r"k_fast_cols_fwdINS_6ColCfgILi%dELi\d+ELi%sELi\d+ELi\d+ELi\d+EEELi%sEE" % (M, r2, r2), kk)]
        assert len(plain) == 1, (M, plain)
        assert v["spill"] == 0 and v["scratch"] == 0 and v["occ"] >= plain[0]["occ"] and v["occ"] >= 3, (k, v, plain[0])
    assert len(bd) == len(configs) - len(not_built)
    small = {k: v for k, v in rep.items() if "k_extend_image" in k}
    assert len(small) == 1, sorted(small)
    for k, v in small.items():
        assert v["spill"] == 0 and v["scratch"] == 0 and v["occ"] >= 3, (k, v)
