"""Accuracy budgets, GPU tier: the HIP kernels through the C ABI against float64 references on zero-mean inputs, with the bars
of util.BUDGET_* (set on the host emulator, tests/test_accuracy_host.py).  Every specialised length once along h and once along
w, the plan variants (path modes, maps per workgroup, the dynamic tile queue, flip_kernels, F = 5, a block-wise plan), the
exported spectrum bin by bin, and full 2-D maps at 4224^2, 6144^2 and 8448^2.  The reference is the float64 oracle (NumPy's
float64 FFTs at the exact windows), except for the full maps: there it is the vendor FFT library on the device in float64
(torch.fft, tests only: the library never links it), one per shape, with the metrics computed on the device.

The cases run in one child process per module (the _case_* functions), which exits at the end: the float64 references, the
8448^2 plans and the FFT library's state go with it, and the device the later tests of the tier see is the one they would
have seen without this file (the plan-cache test of test_gpu_parity.py measures free device memory)."""
import concurrent.futures
import multiprocessing

import numpy as np
import pytest

import util
from test_accuracy_host import COL_LENGTHS, ROW_LENGTHS, one_dim_shape
from test_fast_paths import VARIANTS, plan_options

pytestmark = pytest.mark.gpu

CASE_TIMEOUT_S = 300


class _Child:
    """the module's child process: child("_case_...", args...) runs that function there and returns its result.  A case that times
    out or takes the child down ends the child (killed, queued cases cancelled), and every later case fails at once: nothing
    more starts on the device after trouble."""

    def __init__(self, cases=None):
        """cases: the namespace the case functions are looked up in (a module's globals(); default: this module's)"""
        self.ex = concurrent.futures.ProcessPoolExecutor(max_workers=1, mp_context=multiprocessing.get_context("spawn"))
        self.cases = globals() if cases is None else cases
        self.gone = None

    def __call__(self, name, *args):
        if self.gone:
            pytest.fail("the child process was stopped after %s" % self.gone)
        try:
            return self.ex.submit(self.cases[name], *args).result(timeout=CASE_TIMEOUT_S)
        except (concurrent.futures.TimeoutError, concurrent.futures.process.BrokenProcessPool) as e:
            self.gone = "%s in %s%s" % (type(e).__name__, name, args)
            self.kill()
            raise

    def kill(self):
        procs = list((self.ex._processes or {}).values())
        self.ex.shutdown(wait=False, cancel_futures=True)
        for p in procs:
            p.kill()
        for p in procs:
            p.join(10)


@pytest.fixture(scope="module")
def device():
    child = _Child()
    yield child
    if child.gone:
        child.kill()
    else:
        child.ex.shutdown(wait=True)


def check(budget, metrics, what):
    """metrics: [(max-normalised, L2-relative, spectral)] of each map"""
    for m in metrics:
        print("accuracy %s: max %.2e  L2 %.2e  spectral %.2e" % ((what,) + tuple(m)))
        assert all(x < b for x, b in zip(m, budget)), (what, "max %.2e  L2 %.2e  spectral %.2e" % tuple(m), budget)


# ---- the child's side

def _torch():
    import torch
    return torch


def _device_reference(data, mkh, mkw, kernels):
    """float64 maps [FFT_W][FFT_H] on the device: zero-padded planes, rfft2, product, irfft2, sum over the features"""
    torch = _torch()
    dev = torch.device("cuda", 0)
    H, W, F = data.shape
    fh, fw = util.ceil16(H + mkh - 1), util.ceil16(W + mkw - 1)
    d = torch.zeros((F, fw, fh), dtype=torch.float64, device=dev)
    d[:, :W, :H] = torch.from_numpy(np.ascontiguousarray(np.transpose(data, (2, 1, 0)))).to(dev, torch.float64)
    D = torch.fft.rfft2(d)
    del d
    outs = []
    for k in kernels:
        kh, kw = k.shape[0], k.shape[1]
        kp = torch.zeros((F, fw, fh), dtype=torch.float64, device=dev)
        kp[:, :kw, :kh] = torch.from_numpy(np.ascontiguousarray(np.transpose(k, (2, 1, 0)))).to(dev, torch.float64)
        outs.append(torch.fft.irfft2(D * torch.fft.rfft2(kp), s=(fw, fh)).sum(dim=0))
        del kp
    return outs


def _device_accuracy(out, ref):
    """util.accuracy on the device: out (float32 [FFT_W][FFT_H]) against ref (float64, same layout)"""
    torch = _torch()
    e = out.to(torch.float64) - ref
    nr = float(torch.linalg.vector_norm(ref))
    return (float(e.abs().max()) / float(ref.abs().max()), float(torch.linalg.vector_norm(e)) / nr,
            float(torch.fft.rfft2(e).abs().max()) / nr)


def _case_length(orient, N):
    shape = one_dim_shape(N, orient, 1)
    H, W, F, kh, kw, n = shape
    data, ks = util.normal_inputs(shape, N * 8 + 1 + (orient == "h"))
    with util.load_package().Plan(H, W, F, kh, kw, options={"exact_window": 1}) as p:
        assert (p.info.transform_h, p.info.transform_w) == ((16, N) if orient == "w" else (N, 16))
        assert p.get_option("specialised_kernels") & (1 if orient == "w" else 2)
        p.set_image(data)
        got = p.convolve(ks)
    return [util.accuracy(g, r) for g, r in zip(got, util.Oracle().conv_fft(data, kh, kw, ks, f64=True))]


VARIANT_SHAPE = (1024, 1024, 1, 63, 63, 2)
F5_SHAPE = (540, 500, 5, 37, 40, 2)


def _case_variants():
    """{name: metrics} of one 1152 x 1152 problem under every plan variant, one reference"""
    fc = util.load_package()
    H, W, F, kh, kw, n = VARIANT_SHAPE
    data, ks = util.normal_inputs(VARIANT_SHAPE, 11)
    ref = util.Oracle().conv_fft(data, kh, kw, ks, f64=True)
    flipped = [np.asfortranarray(k[::-1, ::-1, :]) for k in ks]
    runs = [("variant %s" % (v,), plan_options(v), {}, ks) for v in VARIANTS]
    runs += [("dynamic_tiles %d" % d, {}, {"dynamic_tiles": d}, ks) for d in (1, 2)]
    runs += [("flip_kernels", {}, {"flip_kernels": 1}, flipped), ("blockwise", {"max_transform": 576}, {}, ks)]
    res = {}
    for name, opts, settings, kernels in runs:
        with fc.Plan(H, W, F, kh, kw, options=opts) as p:
            if name == "blockwise":
                assert p.get_option("blockwise") > 1 and p.get_option("overlap_save") == 1
            elif opts.get("kernel_path") != 1:
                assert p.get_option("specialised_kernels") == 3, name
            for key, value in settings.items():
                p.set_option(key, value)
            p.set_image(data)
            got = p.convolve(kernels)
        res[name] = [util.accuracy(g, r) for g, r in zip(got, ref)]
    return res


def _case_five_features(group):
    H, W, F, kh, kw, n = F5_SHAPE
    data, ks = util.normal_inputs(F5_SHAPE, 13)
    with util.load_package().Plan(H, W, F, kh, kw, options=plan_options((2, group))) as p:
        assert p.get_option("specialised_kernels") == 3
        p.set_image(data)
        got = p.convolve(ks)
    return [util.accuracy(g, r) for g, r in zip(got, util.Oracle().conv_fft(data, kh, kw, ks, f64=True))]


def _case_spectrum(shape):
    """(per-bin error of the exported spectrum, metrics of the maps) of an exact_window plan"""
    H, W, F, kh, kw = shape
    fh, fw = util.ceil16(H + kh - 1), util.ceil16(W + kw - 1)
    data, ks = util.normal_inputs(shape + (2,), sum(shape))
    padded = np.zeros((F, fw, fh))
    padded[:, :W, :H] = np.transpose(data, (2, 1, 0))
    want = np.fft.rfft2(padded, axes=(1, 2))
    with util.load_package().Plan(H, W, F, kh, kw, options={"exact_window": 1}) as p:
        assert (p.info.transform_h, p.info.transform_w) == (fh, fw)
        p.set_image(data)
        err = util.spectrum_bin_error(p.export_spectrum(), want)
        got = p.convolve(ks)
    ref = util.numpy_fft_conv(data, kh, kw, ks)         # (the oracle takes 11 s at 1712 x 1712)
    return err, [util.accuracy(g, r) for g, r in zip(got, ref)]


_LARGE_REFS = {}


def _case_large(size, k, options, transform):
    torch = _torch()
    shape = (size, size, 1, k, k, 2)
    data, ks = util.normal_inputs(shape, size + k)
    ks[1] = np.asfortranarray(np.pad(ks[1], ((0, k - ks[1].shape[0]), (0, k - ks[1].shape[1]), (0, 0))))   # packed: one size
    if (size, k) not in _LARGE_REFS:      # the two 8192 x 8192 plans share theirs
        _LARGE_REFS.clear()
        _LARGE_REFS[(size, k)] = _device_reference(data, k, k, ks)
    ref = _LARGE_REFS[(size, k)]
    kd = torch.from_numpy(np.ascontiguousarray(np.stack([np.transpose(x, (2, 1, 0)) for x in ks]))).cuda()
    with util.load_package().Plan(size, size, 1, k, k, options=options) as p:
        if transform:
            assert (p.info.transform_h, p.info.transform_w, p.get_option("blockwise")) == (transform, transform, 0)
        else:
            assert p.get_option("blockwise") == 0 or p.get_option("overlap_save") == 1
        p.set_image(data)
        od = torch.empty((2, p.info.fft_w, p.info.fft_h), dtype=torch.float32, device="cuda")
        p.convolve_packed_device(2, kd.data_ptr(), k, k, od.data_ptr())
        p.synchronize()
        return [_device_accuracy(o, r) for o, r in zip(od, ref)]


# ---- the tests

@pytest.mark.parametrize("orient,N", [("w", L) for L in ROW_LENGTHS] + [("h", L) for L in COL_LENGTHS])
def test_every_specialised_length(device, orient, N):
    """the window N as an exact_window plan along h or w (16 along the other), its specialised kernel, a wide and a ragged kernel
    (both stage-2 forms of the row kernel)"""
    check(util.BUDGET_DIRECT, device("_case_length", orient, N), (N, orient))


def test_plan_variants(device):
    """one 1152 x 1152 problem (both kernels specialised), one reference: every VARIANT of test_fast_paths, the dynamic tile
    queue (1: output kernel, 2: the forward column kernels too), flip_kernels (given the flipped kernels) and a block-wise plan
    (overlap-save blocks of 576-point transforms)"""
    for name, metrics in device("_case_variants").items():
        check(util.BUDGET_DIRECT, metrics, name)


@pytest.mark.parametrize("group", [-1, 3])
def test_five_features(device, group):
    """the feature sum of F = 5 (576 x 576), one map per workgroup and three (the multi-map row kernel)"""
    check(util.BUDGET_DIRECT, device("_case_five_features", group), ("F5", group))


@pytest.mark.parametrize("shape,budget", [
    ((282, 346, 2, 23, 23), util.BUDGET_BLUESTEIN),      # 304 x 368: Bluestein both ways
    ((1700, 1700, 1, 13, 13), util.BUDGET_BLUESTEIN),    # 1712 x 1712
    ((12, 8346, 2, 5, 23), util.BUDGET_BLUESTEIN),       # 16 x 8368, F = 2: the feature sum in global memory
    ((8354, 12, 1, 15, 5), util.BUDGET_BLUESTEIN),       # 8368 x 16
    ((282, 4200, 1, 23, 23), util.BUDGET_BLUESTEIN),     # 304 x 4224: Bluestein columns, specialised rows
    ((1030, 1025, 1, 57, 64), util.BUDGET_DIRECT),       # 1088 x 1088 on the native-window kernels
    ((24, 4096, 2, 5, 63), util.BUDGET_DIRECT),          # 32 x 4160
    ((4096, 28, 1, 63, 5), util.BUDGET_DIRECT),          # 4160 x 32
])
def test_exported_spectrum_and_maps(device, shape, budget):
    """exact_window plans: the exported spectrum against numpy.fft.rfft2 in float64 bin by bin, and the maps"""
    err, metrics = device("_case_spectrum", shape)
    print("spectrum %s: per bin %.2e" % (shape, err))
    assert err < util.BUDGET_SPECTRUM_BIN, err
    check(budget, metrics, shape)


@pytest.mark.parametrize("size,k,options,transform", [
    (4096, 127, {}, 4224),
    (6000, 63, {"blockwise": 1}, 6144),
    (8192, 127, {"blockwise": 1}, 8448),
    (8192, 127, {}, None),          # the default plan: overlap-save blocks of a shorter transform where the planner prefers them
])
def test_large_maps(device, size, k, options, transform):
    """full 2-D maps, two kernels (one ragged), device-resident in and out"""
    check(util.BUDGET_LARGE, device("_case_large", size, k, options, transform), (size, k, options))
