"""Test helpers: package import, the CPU oracle (checker only), synthetic inputs."""
import ctypes
import importlib
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_NAME = "cuda-fft-convolution_amd"


def load_package():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    return importlib.import_module(PKG_NAME)


def ceil16(n):
    return (n + 15) // 16 * 16


def _build(path, target_dir, target=None):
    """make -C target_dir, one process at a time (pytest-xdist workers would otherwise run the same make side by side)"""
    import fcntl
    with open(os.path.join(target_dir, ".build.lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            subprocess.run(["make", "-C", target_dir] + ([target] if target else []), check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)
    assert os.path.exists(path), path


def build_emu():
    d = os.path.join(ROOT, "tests", "emu")
    so = os.path.join(d, "libfftconv_emu.so")
    _build(so, d)
    return so


class Oracle:
    """ctypes view of oracle/liboracle.so -- the CPU restatement of the reference path.
    Used by tests / smoke / the bench's cpu_baseline leg only."""

    def __init__(self, native=False):
        """native=True: the same source built -march=native for THIS host (oracle/_native/, made on the spot; the bench's
        cpu_baseline leg only -- the tests check against the portable build)."""
        d = os.path.join(ROOT, "oracle")
        so = os.path.join(d, "_native", "liboracle.so") if native else os.path.join(d, "liboracle.so")
        if native or not os.path.exists(so):
            _build(so, d, "native" if native else None)
        self.lib = ctypes.CDLL(so)
        self.lib.oracle_num_threads.argtypes = [ctypes.c_int]

    def num_threads(self, threads=0):
        return self.lib.oracle_num_threads(threads)

    @staticmethod
    def _prep(data, kernels):
        d = np.asfortranarray(np.asarray(data, dtype=np.float32))
        if d.ndim == 2:
            d = np.asfortranarray(d[:, :, None])
        ks = []
        for k in kernels:
            k = np.asarray(k, dtype=np.float32)
            if k.ndim == 2:
                k = k[:, :, None]
            ks.append(np.asfortranarray(k))
        n = len(ks)
        kp = (ctypes.c_void_p * n)(*[k.ctypes.data for k in ks])
        kh = (ctypes.c_int * n)(*[k.shape[0] for k in ks])
        kw = (ctypes.c_int * n)(*[k.shape[1] for k in ks])
        return d, ks, n, kp, kh, kw

    def conv_fft(self, data, mkh, mkw, kernels, threads=0, f64=False):
        d, ks, n, kp, kh, kw = self._prep(data, kernels)
        H, W, F = d.shape
        fh, fw = ceil16(H + mkh - 1), ceil16(W + mkw - 1)
        dt = np.float64 if f64 else np.float32
        outs = [np.zeros((fh, fw), dtype=dt, order="F") for _ in range(n)]
        op = (ctypes.c_void_p * n)(*[o.ctypes.data for o in outs])
        fn = self.lib.oracle_conv_fft_f64 if f64 else self.lib.oracle_conv_fft
        rc = fn(ctypes.c_void_p(d.ctypes.data), H, W, F, mkh, mkw, n, kp, kh, kw, op, threads)
        if rc != 0:
            raise ValueError("oracle_conv_fft rc=%d" % rc)
        return outs

    def conv_direct(self, data, mkh, mkw, kernel):
        d, ks, n, kp, kh, kw = self._prep(data, [kernel])
        H, W, F = d.shape
        fh, fw = ceil16(H + mkh - 1), ceil16(W + mkw - 1)
        out = np.zeros((fh, fw), dtype=np.float64, order="F")
        rc = self.lib.oracle_conv_direct(ctypes.c_void_p(d.ctypes.data), H, W, F, mkh, mkw,
                                         ctypes.c_void_p(ks[0].ctypes.data), ks[0].shape[0], ks[0].shape[1],
                                         ctypes.c_void_p(out.ctypes.data))
        if rc != 0:
            raise ValueError("oracle_conv_direct rc=%d" % rc)
        return out


class CpuF32:
    """ctypes view of oracle/libcpu_f32.so: the fp32 half-spectrum CPU restatement (second CPU
    baseline of SURVEY.md 8(d)); same contract as Oracle.conv_fft."""

    def __init__(self, native=False):
        d = os.path.join(ROOT, "oracle")
        so = os.path.join(d, "_native", "libcpu_f32.so") if native else os.path.join(d, "libcpu_f32.so")
        if native or not os.path.exists(so):
            _build(so, d, "native" if native else None)
        self.lib = ctypes.CDLL(so)

    def conv_fft(self, data, mkh, mkw, kernels, threads=0):
        d, ks, n, kp, kh, kw = Oracle._prep(data, kernels)
        H, W, F = d.shape
        fh, fw = ceil16(H + mkh - 1), ceil16(W + mkw - 1)
        outs = [np.zeros((fh, fw), dtype=np.float32, order="F") for _ in range(n)]
        op = (ctypes.c_void_p * n)(*[o.ctypes.data for o in outs])
        rc = self.lib.cpu_f32_conv_fft(ctypes.c_void_p(d.ctypes.data), H, W, F, mkh, mkw, n, kp, kh, kw, op, threads)
        if rc != 0:
            raise ValueError("cpu_f32_conv_fft rc=%d" % rc)
        return outs


def numpy_fft_conv(data, mkh, mkw, kernels):
    """Independent float64 statement of demoCudaConvolutionFFT.m:78-102 with NumPy's pocketfft."""
    data = np.asarray(data, dtype=np.float64)
    if data.ndim == 2:
        data = data[:, :, None]
    H, W, F = data.shape
    fh, fw = ceil16(H + mkh - 1), ceil16(W + mkw - 1)
    D = np.fft.fft2(data, s=(fh, fw), axes=(0, 1))
    res = []
    for k in kernels:
        k = np.asarray(k, dtype=np.float64)
        if k.ndim == 2:
            k = k[:, :, None]
        K = np.fft.fft2(k, s=(fh, fw), axes=(0, 1))
        res.append(np.real(np.fft.ifft2(D * K, axes=(0, 1))).sum(axis=2))
    return res


def rel_err(a, b):
    """max|a-b| / max|b| -- the norm-relative parity metric of SURVEY.md 8(d)."""
    b = np.asarray(b, dtype=np.float64)
    return float(np.abs(np.asarray(a, dtype=np.float64) - b).max() / max(np.abs(b).max(), 1e-300))


def synth(cfg_seed, H, W, F, kh, kw, n):
    """Synthetic inputs of SURVEY.md 8(d): image U[0,1) seed 1234+cfg, kernel k U[0,1) seed 5678+cfg+k."""
    img = np.random.default_rng(1234 + cfg_seed).random((H, W, F), dtype=np.float32)
    ks = [np.random.default_rng(5678 + cfg_seed + k).random((kh, kw, F), dtype=np.float32) for k in range(n)]
    return np.asfortranarray(img), [np.asfortranarray(k) for k in ks]


def accuracy(out, ref):
    """(max-normalised, L2-relative, spectral) error of a map against its float64 reference:
    max|e| / max|ref|, ||e||_2 / ||ref||_2 and max_k |FFT(e)_k| / rms_k |FFT(ref)_k|.  The last is the largest error of
    any one frequency bin against a typical bin of the reference (rms_k |FFT(ref)_k| = ||ref||_2 by Parseval): the metric
    that sees a wrong twiddle or a misplaced output bin, which max / L2 norms of a map dilute over all its bins."""
    r = np.asarray(ref, dtype=np.float64)
    e = np.asarray(out, dtype=np.float64) - r
    nr = max(float(np.sqrt(np.sum(r * r))), 1e-300)
    return (float(np.abs(e).max() / max(np.abs(r).max(), 1e-300)),
            float(np.sqrt(np.sum(e * e)) / nr),
            float(np.abs(np.fft.rfft2(e)).max() / nr))


def normal_inputs(shape, seed):
    """zero-mean inputs for the accuracy budgets: image and kernels standard normal, so no DC bin dominates the maps.
    shape = (H, W, F, kh, kw, n); with n > 1 the second kernel is a ragged cell (shorter and narrower than the maximum)."""
    H, W, F, kh, kw, n = shape
    rng = np.random.default_rng(seed)
    data = np.asfortranarray(rng.standard_normal((H, W, F), dtype=np.float32))
    ks = [rng.standard_normal((kh, kw, F), dtype=np.float32) for _ in range(n)]
    if n > 1:
        ks[1] = rng.standard_normal((max(1, kh - 1), max(1, kw // 4), F), dtype=np.float32)
    return data, [np.asfortranarray(k) for k in ks]


# Accuracy budgets: bars for accuracy() = (max-normalised, L2-relative, spectral) of an fp32 map against its float64 reference
# on normal_inputs.  Each bar is at most 4x the worst value of its class measured on the clean tree through the host emulator
# (tests/emu, the kernel bodies under g++); tests/test_accuracy_host.py and test_accuracy_gpu.py apply them, one set for both:
# the MI355X's worst value of each class and metric (test_accuracy_gpu.py, quoted per class below) is at most 1.1x the emulator's.
# Direct transforms (every prime factor <= 17; generic and specialised kernels, every length of fast_paths.hpp along h and w,
# path modes 0 / 1 / 2, F = 1 / 3, 2-D maps up to 2112 x 2112): worst 8.1e-7 max-normalised (16 x 8448 rows, F = 3), 5.0e-7
# L2 and 4.2e-6 spectral (1088 x 1088 on the native-window kernels).  The R1 = 16 row configurations (2560, 3072, 5632, 6144,
# 7680, 8448) sit at about 1.5x the L2 of the R1 = 8 ones (4e-7 against 2.8e-7): their stage-1 power chains reach w^15.
# MI355X: 5.3e-7 max-normalised, 4.9e-7 L2, 3.3e-6 spectral, all at 1088 x 1088.
BUDGET_DIRECT = (3e-6, 1.5e-6, 1.2e-5)
# Bluestein (chirp-z) windows, exact_window plans (304, 592, 1712, 8368 along h and w; 304 x 368, 1712 x 1712): worst 6.0e-7
# max-normalised, 6.0e-7 L2, 4.9e-6 spectral, all at 1712 x 1712.  About 1.2x direct lengths of the same size: the work
# transforms are >= 2N - 1 points long, in fp32.  MI355X: 6.1e-7 / 5.7e-7 / 5.0e-6, at 1712 x 1712.
BUDGET_BLUESTEIN = (2e-6, 1.6e-6, 1.5e-5)
# Full 2-D maps on the long specialised configurations: 4224^2 (4096^2, 127^2 kernels) 4.5e-7 / 3.9e-7 / 3.3e-6, 6144^2
# (6000^2, 63^2) 6.8e-7 / 5.4e-7 / 4.8e-6, 8448^2 (8192^2, 127^2) 6.9e-7 / 5.0e-7 / 5.0e-6.  MI355X: 4224^2 4.5e-7 / 3.7e-7 /
# 3.9e-6, 6144^2 7.1e-7 / 5.3e-7 / 5.2e-6, 8448^2 6.2e-7 / 4.7e-7 / 4.0e-6 (default plan at 8192^2: 6.7e-7 / 5.0e-7 / 4.9e-6).
BUDGET_LARGE = (2.5e-6, 2e-6, 2e-5)
# The image spectrum of an exact_window plan in the reference's order against numpy.fft.rfft2 in float64, per bin:
# max_k |S_k - ref_k| / rms_k |ref_k|.  Worst 1.4e-6 (1088 x 1088 on the native-window kernels), Bluestein 1.3e-6 (1712 x 1712);
# MI355X 1.35e-6 and 1.39e-6.
BUDGET_SPECTRUM_BIN = 5e-6


def spectrum_bin_error(got, want):
    """max_k |got_k - want_k| / rms_k |want_k| over complex spectra: the worst bin against a typical one"""
    want = np.asarray(want, dtype=np.complex128)
    e = np.asarray(got, dtype=np.complex128) - want
    return float(np.abs(e).max() / max(float(np.sqrt(np.mean(np.abs(want) ** 2))), 1e-300))


# ---- a stream that is behind the host (tests/test_async_gpu.py, tests/test_graph_gpu.py)

_LAG = {}


def lag_calibrate(stream):
    """how lag() spins on this device, measured once with an event pair: ("sleep", cycles of torch.cuda._sleep per millisecond)
    or, where torch has no _sleep, ("matmul", 2048 x 2048 fp32 products per millisecond)"""
    import torch
    if "unit" in _LAG:
        return _LAG["kind"], _LAG["unit"]

    def timed(work):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record(stream)
            work()
            e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    if hasattr(torch.cuda, "_sleep"):
        n, ms = 250000, 0.0
        for _ in range(12):                 # grows until one spin takes 5 ms: at most ~40 ms a try, whatever a cycle is
            ms = timed(lambda: torch.cuda._sleep(n))
            if ms >= 5.0:
                break
            n *= 8
        ms = min(ms, timed(lambda: torch.cuda._sleep(n)))      # (clocks settled)
        _LAG["kind"], _LAG["unit"] = "sleep", n / max(ms, 1e-3)
    else:
        with torch.cuda.stream(stream):
            a = torch.ones((2048, 2048), dtype=torch.float32, device=stream.device)
            _LAG["a"] = a
            torch.mm(a, a)
        reps = 64
        ms = timed(lambda: [torch.mm(a, a) for _ in range(reps)])
        _LAG["kind"], _LAG["unit"] = "matmul", reps / max(ms, 1e-3)
    return _LAG["kind"], _LAG["unit"]


def lag(stream, ms=50.0):
    """queues a bounded busy-wait of about `ms` milliseconds on `stream` (a finite spin on the device, never a wait for
    something the host does later) and returns a torch.cuda.Event recorded right behind it: while ev.query() is False the
    stream is behind the host, and whatever was queued after lag() has not started"""
    import torch
    kind, unit = lag_calibrate(stream)
    with torch.cuda.stream(stream):
        if kind == "sleep":
            torch.cuda._sleep(int(ms * unit))
        else:
            a = _LAG["a"]
            for _ in range(max(1, int(ms * unit))):
                torch.mm(a, a)
    ev = torch.cuda.Event()
    ev.record(stream)
    return ev
