"""The spectral-row kernel after its index, address and twiddle work was moved out of the per-map loop (fast_rows_multi.hpp):
every path that change touched, on small problems, against the float64 oracle and against the generic kernels.

What the cases reach (the image is only 40 rows high, or 276 where the case wants the tiled intermediate of the specialised
output kernel: 288 is the shortest specialised column transform):
  * 4224-point rows (one row per workgroup: no index division, the kernel row loaded through a uniform row address, the
    even powers of the stage-1 twiddle kept in registers), uncropped stores, 17 maps walked 16 at a time: one full walk whose
    maps 2..16 take the stage 1 folded into the previous map's last phase, and a one-map walk with the first-map stage 1 only;
  * the same with kernels 63 wide: the 4160-column window of the 4224 transform (the cropped store burst) and the NZ2 = 3 entry;
  * 2112 = 8.12.22, two rows per workgroup, even and odd outputs in two chains of stores;
  * 1152 (two rows per workgroup, one chain);
  * F = 3: the walk over (map, feature) pairs;
  * the row-major intermediate (kernel_path 2).
Each map is held to 1e-4 of the oracle (the bar of the GPU tier, test_gpu_parity.TOL) and to 1e-5 of the generic kernels
(kernel_path 1: the bar test_fast_paths._specialised_vs_generic and test_any_window_gpu set for that pairing).
test_rows_nonarith_host.py runs the same kernel bodies through the host emulator."""
import numpy as np
import pytest

import util

TOL_ORACLE = 1e-4
TOL_GENERIC = 1e-5

# name: ((H, W, F, kh, kw, n), plan options, transform_w, window columns (fft_w), specialised_kernels bits expected)
CASES = {
    "4224-uncropped":           ((40, 4098, 1, 9, 127, 17), {"rows_group": 16}, 4224, 4224, 1),
    "4224-uncropped-tiled":     ((276, 4098, 1, 13, 127, 17), {"rows_group": 16}, 4224, 4224, 3),
    "4224-cropped-nz3":         ((40, 4098, 1, 9, 63, 17), {"rows_group": 16}, 4224, 4160, 1),
    "4224-cropped-nz3-tiled":   ((276, 4098, 1, 13, 63, 17), {"rows_group": 16}, 4224, 4160, 3),
    "2112-two-chains":          ((40, 2000, 1, 9, 63, 17), {"rows_group": 16}, 2112, 2064, 1),
    "2112-two-chains-tiled":    ((276, 2000, 1, 13, 63, 17), {"rows_group": 16}, 2112, 2064, 3),
    "1152":                     ((40, 1000, 1, 9, 63, 17), {"rows_group": 16}, 1152, 1072, 1),
    "1152-tiled":               ((276, 1000, 1, 13, 63, 17), {"rows_group": 16}, 1152, 1072, 3),
    "4224-F3":                  ((40, 4098, 3, 9, 127, 5), {"rows_group": 2}, 4224, 4224, 1),
    "2112-F3-tiled":            ((276, 2000, 3, 13, 63, 5), {"rows_group": 2}, 2112, 2064, 3),
    "4224-row-major":           ((276, 4098, 1, 13, 127, 17), {"rows_group": 16, "kernel_path": 2}, 4224, 4224, 3),
    "2112-row-major-cropped":   ((276, 2000, 1, 13, 63, 17), {"rows_group": 16, "kernel_path": 2}, 2112, 2064, 3),
}


def make_inputs(shape, seed):
    """n distinct kernels of the full size: the walk runs over the equal-size kernels of a launch"""
    H, W, F, kh, kw, n = shape
    rng = np.random.default_rng(seed)
    data = rng.random((H, W, F), dtype=np.float32)
    return data, [rng.random((kh, kw, F), dtype=np.float32) for _ in range(n)]


_REF = {}


def reference(oracle, shape):
    """the float64 oracle's maps of a shape, computed once (the row-major cases share their tiled twins' shapes)"""
    if shape not in _REF:
        data, ks = make_inputs(shape, sum(shape))
        _REF[shape] = oracle.conv_fft(data, shape[3], shape[4], ks)
    return _REF[shape]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_row_kernel_paths_against_oracle_and_generic_kernels(fftconv, oracle, name):
    shape, options, transform_w, fft_w, specialised = CASES[name]
    H, W, F, kh, kw, n = shape
    data, ks = make_inputs(shape, sum(shape))
    with fftconv.Plan(H, W, F, kh, kw, options=options) as p:
        assert (p.info.transform_w, p.info.fft_w) == (transform_w, fft_w), (p.info.transform_w, p.info.fft_w)
        assert p.get_option("specialised_kernels") == specialised, p.get_option("specialised_kernels")
        p.set_image(data)
        got = p.convolve(ks)
    with fftconv.Plan(H, W, F, kh, kw, options={"kernel_path": 1}) as p:
        assert p.get_option("specialised_kernels") == 0
        p.set_image(data)
        generic = p.convolve(ks)
    assert len(got) == len(generic) == n
    worst = [0.0, 0.0]
    for i, (g, q, r) in enumerate(zip(got, generic, reference(oracle, shape))):
        assert g.shape == r.shape == (util.ceil16(H + kh - 1), fft_w)
        eo, eg = util.rel_err(g, r), util.rel_err(g, q)
        worst = [max(worst[0], eo), max(worst[1], eg)]
        assert eo < TOL_ORACLE and eg < TOL_GENERIC, (name, "map %d" % i, "oracle %.2e  generic %.2e" % (eo, eg))
    print("%s: worst vs oracle %.2e, vs generic kernels %.2e" % (name, worst[0], worst[1]))
