"""Accuracy budgets, CPU tier: the kernel bodies through the host emulator (tests/emu) against the float64 oracle on zero-mean
inputs, measured three ways (util.accuracy: max-normalised, L2-relative, spectral) against the bars of util.BUDGET_*.

The parity tests elsewhere compare max|error| / max|reference| on U[0,1) inputs, where a map is mostly its DC bin; a wrong
twiddle, a misplaced output bin or a lost digit in one stage hides under that.  Here every transform length of the
specialised tables runs along h and along w (path modes 0 / 1 / 2, F = 1 / 3), the Bluestein windows and the native 1088 /
4160 windows run as exact_window plans, the plan variants run on 2-D maps, the multi-map row kernel walks distinct kernels at
F = 1, 32 and 256, and the exported spectrum is checked bin by bin."""
import ctypes
import os
import re
import time

import numpy as np
import pytest

import util

CSRC = os.path.join(util.ROOT, "cuda-fft-convolution_amd", "csrc")


def table_lengths():
    """transform lengths of the specialised kernels: X(L, R1, R2, R3, NT, RPW, NZ2) rows (length L along w) and
    X(M, R1, R2, R3, T, NT) output columns (real transform of 2M points along h), read from fast_paths.hpp"""
    src = open(os.path.join(CSRC, "fast_paths.hpp")).read()
    rows = {int(m.group(1)) for m in re.finditer(r"^\s*X\((\d+)(?:,\s*\d+){6}\)", src, re.M)}
    cols = {2 * int(m.group(1)) for m in re.finditer(r"^\s*X\((\d+)(?:,\s*\d+){5}\)", src, re.M)}
    return sorted(rows), sorted(cols)


ROW_LENGTHS, COL_LENGTHS = table_lengths()
BLUESTEIN_WINDOWS = [304, 592, 1712, 8368]      # 16 x 19, 16 x 37, 16 x 107, 16 x 523 (h: 152, 296, 856, 4184 complex points)


def one_dim_shape(N, orient, F):
    """window N along `orient` ("h" or "w"), 16 along the other; wide kernels at F = 1 (the unpruned stage 2 of the row
    kernel), narrow ones at F = 3 (pruned); the second kernel is a ragged cell (util.normal_inputs)"""
    kl = 9 + N // 64 if F == 1 else 5
    return (12, N - kl - 4, F, 5, kl, 2) if orient == "w" else (N - kl - 4, 12, F, kl, 5, 2)


@pytest.fixture(scope="module")
def emu(request):
    lib = ctypes.CDLL(util.build_emu())
    start = time.perf_counter()
    yield lib
    lib.emu_set_tuning(2, -1)
    lib.emu_set_exact_window(0)
    lib.emu_set_dynamic_tiles(0)
    tr = request.config.pluginmanager.get_plugin("terminalreporter")
    if tr is not None:
        tr.ensure_newline()
        tr.write_line("test_accuracy_host.py: %.1f s" % (time.perf_counter() - start))


def emu_conv(emu, data, mkh, mkw, kernels):
    d, ks, n, kp, kh, kw = util.Oracle._prep(data, kernels)
    H, W, F = d.shape
    outs = [np.full((util.ceil16(H + mkh - 1), util.ceil16(W + mkw - 1)), 7e7, dtype=np.float32, order="F") for _ in range(n)]
    op = (ctypes.c_void_p * n)(*[o.ctypes.data for o in outs])
    rc = emu.emu_conv_fft(ctypes.c_void_p(d.ctypes.data), H, W, F, mkh, mkw, n, kp, kh, kw, op, None, None)
    assert rc == 0
    return outs


def plan_lengths(emu, H, W, F, kh, kw):
    lh, lw = ctypes.c_int(0), ctypes.c_int(0)
    assert emu.emu_plan_lengths(H, W, F, kh, kw, ctypes.byref(lh), ctypes.byref(lw)) == 0
    return lh.value, lw.value


def check(budget, got, refs, what):
    for g, r in zip(got, refs):
        m = util.accuracy(g, r)
        assert all(x < b for x, b in zip(m, budget)), (what, "max %.2e  L2 %.2e  spectral %.2e" % m, budget)


def run_one_dim(emu, oracle, N, orient, budget, modes=(0, 1, 2)):
    """window N along `orient` as an exact_window plan, every path mode, F = 1 and 3: one oracle map set per F"""
    emu.emu_set_exact_window(1)
    try:
        for F in (1, 3):
            shape = one_dim_shape(N, orient, F)
            H, W, _, kh, kw, _ = shape
            data, ks = util.normal_inputs(shape, N * 8 + F + (orient == "h"))
            ref = oracle.conv_fft(data, kh, kw, ks, f64=True)
            for mode in modes:
                emu.emu_set_tuning(mode, -1)
                assert plan_lengths(emu, H, W, F, kh, kw) == ((16, N) if orient == "w" else (N, 16))
                fast = emu.emu_uses_fast_rows(H, W, F, kh, kw)
                yield mode, F, fast
                check(budget, emu_conv(emu, data, kh, kw, ks), ref, (N, orient, mode, F))
    finally:
        emu.emu_set_tuning(2, -1)
        emu.emu_set_exact_window(0)


@pytest.mark.parametrize("orient,N", [("w", L) for L in ROW_LENGTHS] + [("h", L) for L in COL_LENGTHS])
def test_every_specialised_length(emu, oracle, orient, N):
    """mode 0 runs the generic kernels at the length, modes 1 and 2 its specialised kernel (rows: bit 1, columns: bit 2)"""
    for mode, F, fast in run_one_dim(emu, oracle, N, orient, util.BUDGET_DIRECT):
        assert fast == (0 if mode == 0 else (1 if orient == "w" else 2)), (mode, F, fast)


@pytest.mark.parametrize("N", BLUESTEIN_WINDOWS)
@pytest.mark.parametrize("orient", ["w", "h"])
def test_bluestein_windows(emu, oracle, orient, N):
    assert emu.emu_length_supported(N if orient == "w" else N // 2) == 0        # no direct transform of the window
    for mode, F, fast in run_one_dim(emu, oracle, N, orient, util.BUDGET_BLUESTEIN):
        assert fast == 0


# 2-D maps with both kernels specialised: the intermediate layouts and maps per workgroup (path mode, rows group), the dynamic tile
# queue, the multi-feature sum (F = 5, also through the multi-map row kernel) and the native 1088 x 1088 window
VARIANT_SHAPE = (1024, 1024, 1, 63, 63, 2)
TWO_DIM_CASES = [
    ("generic", VARIANT_SHAPE, (0, -1), {}),
    ("row-major", VARIANT_SHAPE, (1, -1), {}),
    ("tiled", VARIANT_SHAPE, (2, -1), {}),
    ("one-map-groups", VARIANT_SHAPE, (2, 0), {}),
    ("three-map-groups", VARIANT_SHAPE, (2, 3), {}),
    ("dynamic-tiles", VARIANT_SHAPE, (2, -1), {"dynamic": 1}),
    ("F5", (540, 500, 5, 37, 40, 2), (2, -1), {}),
    ("F5-three-map-groups", (540, 500, 5, 37, 40, 2), (2, 3), {}),
    ("F3-2112", (2000, 2000, 3, 63, 63, 1), (2, -1), {}),
    ("native-1088", (1030, 1025, 1, 57, 64, 2), (2, -1), {"exact": 1}),
]
_REFS = {}


@pytest.mark.parametrize("case", TWO_DIM_CASES, ids=[c[0] for c in TWO_DIM_CASES])
def test_two_dimensional_variants(emu, oracle, case):
    name, shape, (mode, group), opts = case
    H, W, F, kh, kw, n = shape
    data, ks = util.normal_inputs(shape, sum(shape))
    if shape not in _REFS:
        _REFS[shape] = oracle.conv_fft(data, kh, kw, ks, f64=True)
    refs = _REFS[shape]
    if group > 1:     # walks of `group` maps over distinct kernels: three more full-size kernels after the first (4 = 3 + 1)
        rng = np.random.default_rng(sum(shape) + 1)
        extra = [np.asfortranarray(rng.standard_normal((kh, kw, F), dtype=np.float32)) for _ in range(3)]
        if (shape, "walk") not in _REFS:
            _REFS[(shape, "walk")] = oracle.conv_fft(data, kh, kw, extra, f64=True)
        ks = ks[:1] + extra + ks[1:]
        refs = refs[:1] + _REFS[(shape, "walk")] + refs[1:]
    emu.emu_set_tuning(mode, group)
    emu.emu_set_dynamic_tiles(opts.get("dynamic", 0))
    emu.emu_set_exact_window(opts.get("exact", 0))
    try:
        assert emu.emu_uses_fast_rows(H, W, F, kh, kw) == (0 if mode == 0 else 3)
        got = emu_conv(emu, data, kh, kw, ks)
        assert len(got) == len(refs)
        check(util.BUDGET_DIRECT, got, refs, name)
    finally:
        emu.emu_set_tuning(2, -1)
        emu.emu_set_dynamic_tiles(0)
        emu.emu_set_exact_window(0)


# Multi-map walks over DISTINCT kernels: the emulator's row launch walks the equal-size kernels of a group at their real strides
# (a_kernel_stride, y_kernel_stride), as the product's launch does.  Five kernels of one size walked 2 or 3 at a time (the last
# walk partial) and a ragged one, exact_window plans 48 x L; F = 1, 32 and 256 (the feature sum over many planes).
WALK_CASES = [(1, 3, 576), (32, 2, 288), (32, 3, 1152), (256, 3, 288), (256, 2, 384)]


@pytest.mark.parametrize("F,walk,L", WALK_CASES, ids=["F%d-walk%d-L%d" % c for c in WALK_CASES])
def test_walks_over_distinct_kernels(emu, F, walk, L):
    H, W, kh, kw = 40, L - 40 - 3, 5, 40
    rng = np.random.default_rng(F * 1000 + L)
    data = np.asfortranarray(rng.standard_normal((H, W, F), dtype=np.float32))
    ks = [np.asfortranarray(rng.standard_normal(s + (F,), dtype=np.float32)) for s in [(kh, kw)] * 5 + [(kh - 1, kw // 4)]]
    emu.emu_set_exact_window(1)
    emu.emu_set_tuning(2, walk)
    try:
        assert plan_lengths(emu, H, W, F, kh, kw) == (48, L) and emu.emu_uses_fast_rows(H, W, F, kh, kw) & 1
        got = emu_conv(emu, data, kh, kw, ks)
    finally:
        emu.emu_set_tuning(2, -1)
        emu.emu_set_exact_window(0)
    check(util.BUDGET_DIRECT, got, util.numpy_fft_conv(data, kh, kw, ks), (F, walk, L))


@pytest.mark.parametrize("shape", [
    (282, 346, 2, 23, 23),      # 304 x 368: Bluestein both ways
    (570, 282, 1, 23, 23),      # 592 x 304
    (1700, 1700, 1, 13, 13),    # 1712 x 1712 (856 = 8 x 107 along h, 1712 = 16 x 107 along w)
    (12, 8346, 1, 5, 23),       # 16 x 8368
    (8354, 12, 1, 15, 5),       # 8368 x 16
    (282, 4200, 1, 23, 23),     # 304 x 4224: Bluestein columns, specialised rows
    (4200, 282, 1, 23, 23),     # 4224 x 304: specialised columns, Bluestein rows
    (1030, 1025, 1, 57, 64),    # 1088 x 1088 on the native-window kernels
    (1024, 40, 3, 63, 9),       # 1088 x 48
    (24, 4096, 2, 5, 63),       # 32 x 4160
    (4096, 28, 1, 63, 5),       # 4160 x 32
])
def test_exported_spectrum_per_bin(emu, shape):
    """the image spectrum of an exact_window plan in the reference's order (emu_export_spectrum: the plan's natural-order
    tables, as fftconv_plan_export_spectrum applies them) against numpy.fft.rfft2 of the zero-padded planes in float64"""
    H, W, F, kh, kw = shape
    fh, fw = util.ceil16(H + kh - 1), util.ceil16(W + kw - 1)
    data, _ = util.normal_inputs((H, W, F, kh, kw, 0), sum(shape))
    emu.emu_set_exact_window(1)
    try:
        assert plan_lengths(emu, H, W, F, kh, kw) == (fh, fw)
        got = np.zeros((F, fw, fh // 2 + 1), dtype=np.complex64)
        assert emu.emu_export_spectrum(ctypes.c_void_p(data.ctypes.data), H, W, F, kh, kw, ctypes.c_void_p(got.ctypes.data)) == 0
    finally:
        emu.emu_set_exact_window(0)
    padded = np.zeros((F, fw, fh))
    padded[:, :W, :H] = np.transpose(data, (2, 1, 0))
    want = np.fft.rfft2(padded, axes=(1, 2))          # [f][FFT_W][FFT_H/2+1]
    err = util.spectrum_bin_error(got, want)
    assert err < util.BUDGET_SPECTRUM_BIN, err


def test_metrics_see_what_the_max_norm_misses():
    """the three metrics on a known defect: one output bin of a 256 x 256 map off by 1e-4 of a typical bin moves the
    spectral error to ~1e-4, while the max-normalised error of the map stays below 1e-5"""
    rng = np.random.default_rng(3)
    ref = rng.standard_normal((256, 256))
    R = np.fft.rfft2(ref)
    R[17, 40] += 1e-4 * np.sqrt(np.mean(np.abs(np.fft.fft2(ref)) ** 2))
    bad = np.fft.irfft2(R, s=ref.shape)
    mx, l2, spec = util.accuracy(bad, ref)
    assert mx < 1e-5 and l2 < 1e-5
    assert 0.9e-4 < spec < 1.1e-4
    assert util.accuracy(ref, ref) == (0.0, 0.0, 0.0)
