"""CPU tier of test_rows_nonarith_gpu.py: the same row-kernel bodies (fast_rows_multi.hpp) through the host emulator, on the
same row lengths with the image height cut to what the emulator does in seconds, and the plans of the GPU cases checked against
the planner (the product's make_geometry, through the emulator) so that each case reaches the path its name says."""
import ctypes

import numpy as np
import pytest

import test_rows_nonarith_gpu as tg
import util

# name: ((H, W, F, kh, kw, n), (path mode, rows group) of emu_set_tuning, transform_w, emu_uses_fast_rows bits);
# path mode 2: tiled intermediate where the output kernel is specialised, 1: row-major intermediate
CASES = {
    "4224-uncropped":          ((12, 4098, 1, 5, 127, 17), (2, 16), 4224, 1),
    "4224-cropped-nz3":        ((12, 4098, 1, 5, 63, 5), (2, 3), 4224, 1),
    "2112-two-chains":         ((12, 2000, 1, 5, 63, 5), (2, 3), 2112, 1),
    "2112-two-chains-tiled":   ((280, 2000, 1, 9, 63, 3), (2, 2), 2112, 3),
    "1152":                    ((12, 1000, 1, 5, 63, 5), (2, 3), 1152, 1),
    "1152-tiled":              ((280, 1000, 1, 9, 63, 3), (2, 2), 1152, 3),
    "4224-F3":                 ((12, 4098, 3, 5, 127, 3), (2, 2), 4224, 1),
    "2112-row-major-cropped":  ((280, 2000, 1, 9, 63, 3), (1, 2), 2112, 3),
    "288-eight-rows-tiled":    ((276, 270, 1, 13, 17, 4), (2, 3), 288, 3),
}


@pytest.fixture(scope="module")
def emu():
    lib = ctypes.CDLL(util.build_emu())
    yield lib
    lib.emu_set_tuning(2, -1)


def plan_lengths(emu, shape):
    H, W, F, kh, kw, n = shape
    lh, lw = ctypes.c_int(0), ctypes.c_int(0)
    assert emu.emu_plan_lengths(H, W, F, kh, kw, ctypes.byref(lh), ctypes.byref(lw)) == 0
    return lh.value, lw.value


@pytest.mark.parametrize("name", list(CASES))
def test_emulated_row_kernel_paths(emu, oracle, name):
    shape, tuning, transform_w, fast = CASES[name]
    H, W, F, kh, kw, n = shape
    emu.emu_set_tuning(*tuning)
    assert plan_lengths(emu, shape)[1] == transform_w
    assert emu.emu_uses_fast_rows(H, W, F, kh, kw) == fast
    data, ks = tg.make_inputs(shape, sum(shape))
    d, kl, n_, kp, khs, kws = util.Oracle._prep(data, ks)
    outs = [np.full((util.ceil16(H + kh - 1), util.ceil16(W + kw - 1)), 7e7, dtype=np.float32, order="F") for _ in range(n)]
    op = (ctypes.c_void_p * n)(*[o.ctypes.data for o in outs])
    assert emu.emu_conv_fft(ctypes.c_void_p(d.ctypes.data), H, W, F, kh, kw, n, kp, khs, kws, op, None, None) == 0
    for i, (g, r) in enumerate(zip(outs, oracle.conv_fft(data, kh, kw, ks))):
        assert util.rel_err(g, r) < 1e-5, (name, i)


@pytest.mark.parametrize("name", list(tg.CASES))
def test_gpu_cases_plan_onto_the_named_kernels(emu, name):
    """the transform length and which kernels are specialised, as the GPU cases assert them of their plans"""
    shape, options, transform_w, fft_w, specialised = tg.CASES[name]
    H, W, F, kh, kw, n = shape
    emu.emu_set_tuning({0: 2, 2: 1}[options.get("kernel_path", 0)], options["rows_group"])
    assert plan_lengths(emu, shape)[1] == transform_w and util.ceil16(W + kw - 1) == fft_w
    assert emu.emu_uses_fast_rows(H, W, F, kh, kw) == specialised


def test_gpu_cases_walk_a_full_group_and_a_remainder():
    """F = 1: 17 maps walked 16 at a time (a full walk and a one-map walk); F = 3: 5 maps walked 2 at a time"""
    for name, (shape, options, *_rest) in tg.CASES.items():
        n, walk = shape[5], options["rows_group"]
        assert n > walk and n % walk == 1, name
