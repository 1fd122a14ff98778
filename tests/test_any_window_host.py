"""Exact-window plans for any ceil16 window (CPU tier, through the host emulator of the kernel bodies).

A plan created with exact_window transforms the window itself.  Windows whose length (FFT_W, or FFT_H / 2 for the
real h transform) has a prime factor above 17 run Bluestein (chirp-z) transforms on the generic kernels
(fft_lds.hpp: fft_bluestein); default plans and the direct lengths are untouched."""
import ctypes

import numpy as np
import pytest

import util

WINDOWS = list(range(16, 8448 + 1, 16))     # every ceil16 window up to 8448


@pytest.fixture(scope="module")
def emu():
    lib = ctypes.CDLL(util.build_emu())
    lib.emu_spectrum_elems.restype = ctypes.c_long
    lib.emu_set_tuning(2, -1)
    lib.emu_set_exact_window(1)
    yield lib
    lib.emu_set_exact_window(0)


def plan_lengths(emu, H, W, F, kh, kw):
    lh, lw = ctypes.c_int(0), ctypes.c_int(0)
    rc = emu.emu_plan_lengths(H, W, F, kh, kw, ctypes.byref(lh), ctypes.byref(lw))
    return rc, lh.value, lw.value


def emu_conv(emu, data, mkh, mkw, kernels):
    d, ks, n, kp, kh, kw = util.Oracle._prep(data, kernels)
    H, W, F = d.shape
    outs = [np.full((util.ceil16(H + mkh - 1), util.ceil16(W + mkw - 1)), 7e7, dtype=np.float32, order="F") for _ in range(n)]
    op = (ctypes.c_void_p * n)(*[o.ctypes.data for o in outs])
    rc = emu.emu_conv_fft(ctypes.c_void_p(d.ctypes.data), H, W, F, mkh, mkw, n, kp, kh, kw, op, None, None)
    return rc, outs


def inputs(H, W, F, kh, kw, n, seed):
    rng = np.random.default_rng(seed)
    data = rng.random((H, W, F), dtype=np.float32)
    return data, [rng.random((kh, kw, F), dtype=np.float32) for _ in range(n)]


def largest_prime_factor(n):
    p, big = 2, 1
    while n > 1:
        while n % p == 0:
            n //= p
            big = p
        p += 1
    return big


def test_every_window_has_an_exact_plan(emu):
    """all 528 ceil16 windows up to 8448, along h and along w, F = 1 and 3: the plan exists and transforms the window;
    which lengths transform directly is unchanged (test_host_logic: 19, 23, 38, ... are not direct lengths)"""
    nonfactoring = 0
    for N in WINDOWS:
        for F in (1, 3):
            assert plan_lengths(emu, N - 4, 8, F, 5, 5) == (0, N, 16), (N, F)
            assert plan_lengths(emu, 8, N - 4, F, 5, 5) == (0, 16, N), (N, F)
        direct = emu.emu_length_supported(N)
        assert direct == (largest_prime_factor(N) <= 17)
        nonfactoring += not direct
    assert nonfactoring == 329
    for L in (19, 23, 38, 4222, 1087):
        assert emu.emu_length_supported(L) == 0


@pytest.mark.parametrize("N", [304, 1712, 7184, 8368])
def test_large_feature_counts(emu, N):
    """F up to 8 at windows whose work buffer and feature accumulator do (304, 1712) and do not (7184, 8368) fit the LDS together"""
    for F in (2, 5, 8):
        assert plan_lengths(emu, 8, N - 4, F, 5, 5) == (0, 16, N)


@pytest.mark.parametrize("shape", [
    (282, 282, 1, 23, 23),      # 304 x 304: 152 = 8 x 19 along h, 304 = 16 x 19 along w
    (282, 282, 3, 23, 23),
    (346, 442, 1, 23, 23),      # 368 x 464: 23 and 29
    (346, 442, 3, 23, 23),
    (570, 282, 1, 23, 23),      # 592 x 304: 37 and 19
    (570, 282, 3, 23, 23),
    (282, 4200, 1, 23, 23),     # 304 x 4224: Bluestein columns, specialised 4224-point rows (row-major intermediate)
    (8, 8346, 2, 9, 23),        # w window 8368 = 16 x 523, F = 2: the feature sum accumulates in Y
])
def test_emulated_bluestein_parity(emu, oracle, shape):
    H, W, F, kh, kw = shape
    data, ks = inputs(H, W, F, kh, kw, 2, sum(shape))
    ks[1] = ks[1][: kh - 3, : kw - 5]
    rc, got = emu_conv(emu, data, kh, kw, ks)
    assert rc == 0
    for g, r in zip(got, oracle.conv_fft(data, kh, kw, ks)):
        assert util.rel_err(g, r) < 1e-5


def test_emulated_image_spectrum_is_natural_order(emu):
    """the image spectrum of a 304 x 368 window (both directions Bluestein): rows and columns in natural order, scaled
    by 1 / (FFT_H * FFT_W), equal to numpy.fft.rfft2 of the zero-padded planes"""
    H, W, F, kh, kw = 282, 346, 2, 23, 23
    fh, fw = 304, 368
    data, _ = inputs(H, W, F, kh, kw, 0, 5)
    n = emu.emu_spectrum_elems(H, W, F, kh, kw)
    rows, pitch = fh // 2 + 1, (fw + 7) // 8 * 8
    assert n == F * rows * pitch
    spec = np.zeros(2 * n, dtype=np.float32)
    d = np.asfortranarray(data)
    assert emu.emu_image_spectrum(ctypes.c_void_p(d.ctypes.data), H, W, F, kh, kw, ctypes.c_void_p(spec.ctypes.data)) == 0
    S = spec.view(np.complex64).reshape(F, rows, pitch)[:, :, :fw].astype(np.complex128) * (fh * fw)
    padded = np.zeros((F, fw, fh))
    padded[:, :W, :H] = np.transpose(data, (2, 1, 0))
    want = np.fft.rfft2(padded, axes=(1, 2))                  # [f][x][y]
    got = np.transpose(S, (0, 2, 1))
    assert np.abs(got - want).max() / np.abs(want).max() < 1e-5


def test_emulated_oversize_kernel_wraps_modulo_the_window(emu, oracle):
    """a kernel larger than MAX_KERNEL but inside the 304 x 304 window wraps circularly, as in the reference
    (src/cudaConvolutionFFT.cu:242): the oracle's direct convolution modulo the window"""
    H, W, F = 282, 282, 2
    data, _ = inputs(H, W, F, 23, 23, 0, 11)
    big = np.random.default_rng(12).random((40, 31, F), dtype=np.float32)
    rc, got = emu_conv(emu, data, 23, 23, [big])
    assert rc == 0
    assert util.rel_err(got[0], oracle.conv_direct(data, 23, 23, big)) < 1e-5
