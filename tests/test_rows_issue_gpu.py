"""The spectral-row kernel with its phases at two issue priorities (fast_rows_multi.hpp: FC_ROWS_PRIO_POLICY), on the GPU
against the float64 oracle.

A variant of the kernel reads NZ2 stage-2 inputs, R3 elements of the kernel row apart, and is launched for every kernel width
up to NZ2 * R3; an input past the kernel's width is a zero selected in P2, one of the phases that now run at the raised
priority.  A kernel of (NZ2 - 1) * R3 columns or more reaches into the last input block, a narrower one leaves whole inputs to
the select.  Every configuration runs once on either side of that width:

  configuration                      R3   NZ2   (NZ2 - 1) * R3   kernel widths
  288 = 4.6.12, eight rows, 288^2    12    3         24            17 / 31
  2112 = 8.12.22, two store chains   22    3         44            31 / 63
  4224 = 8.24.22, two maps           22    6        110            95 / 127
  4224, window 4160 (wout < L)       22    3         44            33 / 63

Inputs are zero-mean (no DC bin hides an error) and every kernel has the full width.  The bars are the budgets of the direct
transforms, util.BUDGET_DIRECT, as tests/test_accuracy_gpu.py applies them to these kernels.  (A form of P2 that branched on
that width and read the inner inputs without a select was measured with this test and dropped: DESIGN.md 9.5.)"""
import numpy as np
import pytest

import util

# name: ((H, W, F, kh, kw, n), plan options, transform_w, window columns (fft_w), R3, NZ2 of the variant, at or above (NZ2 - 1) * R3)
CASES = {
    "288-below":          ((276, 270, 1, 13, 17, 3), {"rows_group": 2}, 288, 288, 12, 3, False),
    "288-above":          ((276, 256, 1, 13, 31, 3), {"rows_group": 2}, 288, 288, 12, 3, True),
    "2112-below":         ((40, 2032, 1, 9, 31, 3), {"rows_group": 2}, 2112, 2064, 22, 3, False),
    "2112-above":         ((40, 2000, 1, 9, 63, 3), {"rows_group": 2}, 2112, 2064, 22, 3, True),
    "4224-two-maps-below": ((40, 4130, 1, 9, 95, 2), {}, 4224, 4224, 22, 6, False),
    "4224-two-maps-above": ((40, 4098, 1, 9, 127, 2), {}, 4224, 4224, 22, 6, True),
    "4224-cropped-below": ((40, 4128, 1, 9, 33, 3), {"rows_group": 2}, 4224, 4160, 22, 3, False),
    "4224-cropped-above": ((40, 4098, 1, 9, 63, 3), {"rows_group": 2}, 4224, 4160, 22, 3, True),
}


def make_inputs(shape, seed):
    H, W, F, kh, kw, n = shape
    rng = np.random.default_rng(seed)
    data = np.asfortranarray(rng.standard_normal((H, W, F), dtype=np.float32))
    return data, [np.asfortranarray(rng.standard_normal((kh, kw, F), dtype=np.float32)) for _ in range(n)]


def test_cases_sit_on_the_side_of_the_width_they_name():
    """the variant the dispatcher takes is the first whose NZ2 covers the width: each width needs more than the next smaller
    variant of its length (fast_paths.hpp) and lies on the named side of (NZ2 - 1) * R3"""
    smaller = {(288, 3): 0, (2112, 3): 0, (4224, 3): 0, (4224, 6): 3}
    for name, (shape, _options, transform_w, _fft_w, R3, NZ2, above) in CASES.items():
        kw = shape[4]
        assert smaller[(transform_w, NZ2)] * R3 < kw <= NZ2 * R3, name
        assert (kw >= (NZ2 - 1) * R3) == above, name


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_row_kernel_on_both_sides_of_the_last_input_block(fftconv, oracle, name):
    shape, options, transform_w, fft_w, _R3, _NZ2, _above = CASES[name]
    H, W, F, kh, kw, n = shape
    data, ks = make_inputs(shape, sum(shape))
    with fftconv.Plan(H, W, F, kh, kw, options=options) as p:
        assert (p.info.transform_w, p.info.fft_w) == (transform_w, fft_w), (p.info.transform_w, p.info.fft_w)
        assert p.get_option("specialised_kernels") & 1
        p.set_image(data)
        got = p.convolve(ks)
    ref = oracle.conv_fft(data, kh, kw, ks, f64=True)
    assert len(got) == len(ref) == n
    for i, (g, r) in enumerate(zip(got, ref)):
        assert g.shape == r.shape == (util.ceil16(H + kh - 1), fft_w)
        m = util.accuracy(g, r)
        print("%s map %d: max %.2e  L2 %.2e  spectral %.2e" % ((name, i) + m))
        assert all(x < b for x, b in zip(m, util.BUDGET_DIRECT)), (name, i, m, util.BUDGET_DIRECT)
