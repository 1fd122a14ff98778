"""Exact-window plans for any ceil16 window on the GPU: windows with a prime factor above 17 run Bluestein (chirp-z)
transforms on the generic kernels, so the reference's two-step protocol (the complex gpuArray spectrum of cudaFFTData,
src/cudaFFTData.cu:72-103,150; cudaConvFFTData recovering FFT_H / FFT_W from it, src/cudaConvFFTData.cu:92-98) and the
circular wrap of kernels beyond MAX_KERNEL (src/cudaConvolutionFFT.cu:242) work at every window size."""
import numpy as np
import pytest

import util
from test_mex_gateway import Mex

pytestmark = pytest.mark.gpu

TIGHT = 1e-5
EXACT = {"exact_window": 1}


def inputs(shape, n=2):
    H, W, F, kh, kw = shape
    rng = np.random.default_rng(sum(shape) + 3)
    data = rng.random((H, W, F), dtype=np.float32)
    ks = [rng.random((kh, kw, F), dtype=np.float32) for _ in range(n)]
    if n > 1:
        ks[1] = ks[1][: kh - 3, : kw - 5]
    return data, ks


def rfft2_of_window(data, fh, fw):
    H, W, F = data.shape
    padded = np.zeros((F, fw, fh), dtype=np.float64)
    padded[:, :W, :H] = np.transpose(data, (2, 1, 0))
    return np.fft.rfft2(padded, axes=(1, 2))          # [f][FFT_W][FFT_H/2+1]: the layout export_spectrum uses


@pytest.mark.parametrize("shape", [
    (282, 282, 1, 23, 23),      # 304 x 304 (19 along both)
    (282, 282, 3, 23, 23),
    (346, 442, 1, 23, 23),      # 368 x 464 (23, 29)
    (346, 442, 3, 23, 23),
    (570, 282, 1, 23, 23),      # 592 x 304 (37, 19)
    (570, 282, 3, 23, 23),
    (282, 4200, 1, 23, 23),     # 304 x 4224: Bluestein columns, specialised rows
    (4200, 282, 1, 23, 23),     # 4224 x 304: specialised columns, Bluestein rows
    (8, 8346, 2, 9, 23),        # w window 8368 = 16 x 523, F = 2: the feature sum accumulates in global memory
])
def test_exact_window_plan_spectrum_and_maps(fftconv, oracle, shape):
    H, W, F, kh, kw = shape
    fh, fw = util.ceil16(H + kh - 1), util.ceil16(W + kw - 1)
    data, ks = inputs(shape)
    want = rfft2_of_window(data, fh, fw)
    ref = oracle.conv_fft(data, kh, kw, ks)
    with fftconv.Plan(H, W, F, kh, kw, options=EXACT) as p:
        assert p.info.exact_window == 1 and (p.info.transform_h, p.info.transform_w) == (fh, fw)
        p.set_image(data)
        spec = p.export_spectrum()
        assert spec.shape == (F, fw, fh // 2 + 1)
        assert np.abs(spec - want).max() / np.abs(want).max() < TIGHT
        for g, r in zip(p.convolve(ks), ref):
            assert g.shape == (fh, fw) and util.rel_err(g, r) < TIGHT
    with fftconv.Plan(H, W, F, kh, kw, options=EXACT) as q:
        q.import_spectrum(want.astype(np.complex64))   # numpy's spectrum in, the plan never saw the image
        for g, r in zip(q.convolve(ks), ref):
            assert util.rel_err(g, r) < TIGHT


def test_oversize_kernel_wraps_modulo_a_bluestein_window(fftconv, oracle):
    """kernels larger than MAX_KERNEL but inside the 304 x 304 window wrap circularly, as in the reference"""
    H, W, F = 282, 282, 2
    data, _ = inputs((H, W, F, 23, 23), 0)
    rng = np.random.default_rng(12)
    big = [rng.random((40, 31, F), dtype=np.float32), rng.random((23, 300, F), dtype=np.float32)]
    with fftconv.Plan(H, W, F, 23, 23, options=EXACT) as p:
        p.set_image(data)
        for g, k in zip(p.convolve(big), big):
            assert util.rel_err(g, oracle.conv_direct(data, 23, 23, k)) < TIGHT


def test_generic_kernel_path_matches_the_default_exact_plan(fftconv, oracle):
    """kernel_path = 1 (generic kernels only) against the default exact plan at 304 x 4224, whose rows are specialised"""
    shape = (282, 4200, 1, 23, 23)
    H, W, F, kh, kw = shape
    data, ks = inputs(shape)
    outs = []
    for opts in (EXACT, dict(EXACT, kernel_path=1)):
        with fftconv.Plan(H, W, F, kh, kw, options=opts) as p:
            assert p.info.exact_window == 1 and (p.info.transform_h, p.info.transform_w) == (304, 4224)
            p.set_image(data)
            outs.append(p.convolve(ks))
    for a, b, r in zip(outs[0], outs[1], oracle.conv_fft(data, kh, kw, ks)):
        assert util.rel_err(a, r) < TIGHT and util.rel_err(b, r) < TIGHT
        assert util.rel_err(b, a) < TIGHT


def test_verbose_names_the_chirp_z_passes(fftconv, capfd):
    with fftconv.Plan(282, 282, 1, 23, 23, options=dict(EXACT, verbose=1)) as p:
        p.set_image(np.ones((282, 282, 1), np.float32))
        p.synchronize()
    err = capfd.readouterr().err
    line = [s for s in err.splitlines() if "FFT size: h=304, w=304" in s]
    assert line and "chirp-z passes: h 152 via" in line[0] and ", w 304 via" in line[0], err


@pytest.fixture(scope="module")
def mex():
    return Mex()


def test_mex_gateways_return_and_take_the_gpuarray_at_a_bluestein_window(mex, oracle):
    """cudaFFTData at window 304 returns the reference's complex single gpuArray (not the handle form), equal to
    fft2(...)[:FFT_H/2+1]; cudaConvFFTData and cudaConvFFTDataStreams convolve from it like the oracle"""
    H, W, F, kh, kw = 282, 282, 2, 23, 23
    fh, fw = 304, 304
    data, ks = inputs((H, W, F, kh, kw), 3)
    raised, out = mex.call("cudaFFTData", [mex.numeric(data), mex.scalar(kh), mex.scalar(kw)])
    assert not raised, out
    fft_data = out[0]
    assert mex.rt.mock_is_gpu(fft_data) and mex.rt.mock_gpu_is_complex(fft_data)
    spec = mex.gpu_to_numpy_complex(fft_data)
    assert spec.shape == (fh // 2 + 1, fw, F)
    padded = np.zeros((fh, fw, F))
    padded[:H, :W, :] = data
    want = np.fft.fft2(padded, axes=(0, 1))[:fh // 2 + 1, :, :]
    assert np.abs(spec - want).max() / np.abs(want).max() < TIGHT
    ref = oracle.conv_fft(data, kh, kw, ks)
    for gw in ("cudaConvFFTData", "cudaConvFFTDataStreams"):
        raised, out = mex.call(gw, [fft_data, mex.cell([mex.numeric(k) for k in ks])])
        assert not raised, (gw, out)
        for g, r in zip(mex.cell_to_list(out[0], len(ks)), ref):
            assert g.shape == (fh, fw) and util.rel_err(g, r) < TIGHT, gw
        assert mex.rt.mock_live_gpu_views() == 0
    mex.rt.mock_free(fft_data)
