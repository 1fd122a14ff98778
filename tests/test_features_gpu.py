"""Feature sums (F > 1) on the GPU: the HIP kernels against float64 references on zero-mean inputs, with the bars of util.BUDGET_*.

F > 1 has a row kernel of its own (kernels_rows_multi.inc: k_fast_rows_multi_f, one instantiation per row-table entry of
fast_paths.hpp) with its own XCD-aware grid decode, the image row fetched per feature, the feature sum parked in LDS and the
inverse phases run for the last feature only.  Here:
  * every instantiation: one exact_window plan per row length L (window L along w, 144 along h: 73 rows, so every RPW of the
    table has more than 8 row groups and not a multiple of 8), kernels whose widths pick each NZ2 entry of L, five distinct
    kernels per width walked 2 or 3 at a time (every walk partial at its end), F from 2 to 16 (ROW_CASES; test_features_host.py
    checks that they cover the table);
  * every specialised length along h at F = 3;
  * a diagnostic with no transform in its reference: kernels with one non-zero feature plane, and sparse taps across planes;
  * realistic feature counts end to end (HOG-like F = 31 / 32, CNN-like F = 256 / 512, cfg2 and cfg5 geometry);
  * the host choices that depend on F: automatic walk lengths, batching, kernel preparation, flip_kernels, the output
    routes, the exported spectrum, a Bluestein row summing in the intermediate, the single-pass limit and a block-wise plan.
The references are float64: NumPy's FFTs on the host, torch.fft on the device for the large problems (tests only: the library
never links it), or a shift-and-add on the host.  The cases run in a spawned child (test_accuracy_gpu._Child), which exits with the module: later tests see the device
as before."""
import os
import re
import time

import numpy as np
import pytest

import util
from test_accuracy_gpu import _Child, _device_accuracy, _device_reference
from test_accuracy_host import COL_LENGTHS, one_dim_shape

CSRC = os.path.join(util.ROOT, "cuda-fft-convolution_amd", "csrc")


def row_table():
    """{L: [(R1, R2, R3, NT, RPW, NZ2), ...]} of fast_paths.hpp's X(L, R1, R2, R3, NT, RPW, NZ2) rows, in the listed (ascending
    NZ2) order: one k_fast_rows_multi(_f) instantiation each"""
    src = open(os.path.join(CSRC, "fast_paths.hpp")).read()
    table = {}
    for m in re.finditer(r"^\s*X\((\d+(?:,\s*\d+){6})\)", src, re.M):
        L, *rest = (int(x) for x in m.group(1).split(","))
        table.setdefault(L, []).append(tuple(rest))
    return table


ROW_TABLE = row_table()


def row_instantiations():
    return sorted((L, e[5]) for L, entries in ROW_TABLE.items() for e in entries)


def dispatched_nz2(L, kw):
    """the NZ2 entry a launch with kernels kw wide runs: the first listed one with NZ2 >= ceil(kw / R3) (pipeline.hpp:
    fast_rows_nz2, fast_paths.hpp: fast_rows_dispatch_group)"""
    entries = ROW_TABLE[L]
    need = -(-kw // entries[0][2])
    return next(e[5] for e in entries if e[5] >= need)


H_WINDOW = 144                 # 73 spectrum rows: 73 / 37 / 19 / 13 / 10 row groups at RPW 1 / 2 / 4 / 6 / 8
ROW_MAX_KH = 15
KERNELS_PER_WIDTH = 5          # walks of 2: 2 + 2 + 1, walks of 3: 3 + 2
ROW_FEATURES = [2, 3, 4, 5, 8, 9, 16]


def row_cases():
    """(L, F, walk, widths): per row length, the widest kernel each NZ2 entry takes (NZ2 * R3: its column kw - 1 is the last
    stage-2 input the entry reads)"""
    cases = []
    for i, L in enumerate(sorted(ROW_TABLE)):
        R3 = ROW_TABLE[L][0][2]
        widths = [e[5] * R3 for e in ROW_TABLE[L]]
        cases.append((L, ROW_FEATURES[i % len(ROW_FEATURES)], 2 + i % 2, widths))
    return cases


ROW_CASES = row_cases()

# worst (max-normalised, L2, spectral) per class, printed at the end of the module
_WORST = {}


@pytest.fixture(scope="module")
def device(request):
    child = _Child(globals())
    start = time.perf_counter()
    yield child
    if child.gone:
        child.kill()
    else:
        child.ex.shutdown(wait=True)
    capture = request.config.pluginmanager.get_plugin("capturemanager")
    if capture is not None and _WORST:
        with capture.global_and_fixture_disabled():      # (teardown output is captured otherwise)
            print("\ntest_features_gpu.py: %.1f s; worst (max, L2, spectral) per class:" % (time.perf_counter() - start))
            for cls, m in sorted(_WORST.items()):
                print("  %-12s %.2e  %.2e  %.2e" % ((cls,) + tuple(m)))


def check(cls, budget, metrics, what):
    """metrics: [(max-normalised, L2-relative, spectral)] of each map"""
    worst = _WORST.setdefault(cls, (0.0, 0.0, 0.0))
    for i, m in enumerate(metrics):
        worst = tuple(max(a, b) for a, b in zip(worst, m))
        assert all(x < b for x, b in zip(m, budget)), (what, "map %d" % i, "max %.2e  L2 %.2e  spectral %.2e" % tuple(m), budget)
    _WORST[cls] = worst
    print("accuracy %s: max %.2e  L2 %.2e  spectral %.2e" % ((what,) + worst))


# ---- the child's side

def _torch():
    import torch
    return torch


def numpy_reference(data, mkh, mkw, kernels):
    """float64 maps (FFT_H x FFT_W) with NumPy's FFTs: util.numpy_fft_conv with the feature sum taken in the spectrum (one
    inverse transform per map instead of F)"""
    H, W, F = data.shape
    fh, fw = util.ceil16(H + mkh - 1), util.ceil16(W + mkw - 1)
    D = np.fft.rfft2(np.asarray(data, dtype=np.float64), s=(fh, fw), axes=(0, 1))
    return [np.fft.irfft2(np.einsum("ijf,ijf->ij", D, np.fft.rfft2(np.asarray(k, dtype=np.float64), s=(fh, fw), axes=(0, 1))),
                          s=(fh, fw), axes=(0, 1)) for k in kernels]


def _host_metrics(got, data, mkh, mkw, kernels, on_device=False):
    """util.accuracy of host maps (FFT_H x FFT_W) against the float64 reference: NumPy's on the host, or (large problems)
    torch.fft's on the device"""
    if not on_device:
        return [util.accuracy(g, r) for g, r in zip(got, numpy_reference(data, mkh, mkw, kernels))]
    torch = _torch()
    ref = _device_reference(data, mkh, mkw, kernels)
    return [_device_accuracy(torch.from_numpy(np.ascontiguousarray(np.asarray(g).T)).cuda(), r) for g, r in zip(got, ref)]


def _packed(kernels):
    torch = _torch()
    return torch.from_numpy(np.ascontiguousarray(np.stack([np.transpose(k, (2, 1, 0)) for k in kernels]))).cuda()


def _inputs(H, W, F, sizes, seed):
    """standard-normal image and kernels of the given (kh, kw)"""
    rng = np.random.default_rng(seed)
    data = np.asfortranarray(rng.standard_normal((H, W, F), dtype=np.float32))
    return data, [np.asfortranarray(rng.standard_normal((kh, kw, F), dtype=np.float32)) for kh, kw in sizes]


def _case_rows(L, F, walk, widths):
    """one exact_window plan, window H_WINDOW x L; KERNELS_PER_WIDTH kernels of each width (one launch per width), walked
    `walk` maps per workgroup"""
    max_kw = max(widths)
    H, W = H_WINDOW - ROW_MAX_KH - 2, L - max_kw - 3
    sizes = [(ROW_MAX_KH - i, kw) for i, kw in enumerate(widths) for _ in range(KERNELS_PER_WIDTH)]
    data, ks = _inputs(H, W, F, sizes, L + F)
    with util.load_package().Plan(H, W, F, ROW_MAX_KH, max_kw, options={"exact_window": 1, "rows_group": walk}) as p:
        assert (p.info.transform_h, p.info.transform_w) == (H_WINDOW, L)
        assert p.get_option("specialised_kernels") & 1
        p.set_image(data)
        got = p.convolve(ks)
    return _host_metrics(got, data, ROW_MAX_KH, max_kw, ks)


def _case_column_length(N):
    shape = one_dim_shape(N, "h", 3)
    H, W, F, kh, kw, n = shape
    data, ks = util.normal_inputs(shape, N * 8 + 5)
    with util.load_package().Plan(H, W, F, kh, kw, options={"exact_window": 1}) as p:
        assert (p.info.transform_h, p.info.transform_w) == (N, 16)
        assert p.get_option("specialised_kernels") & 2
        p.set_image(data)
        got = p.convolve(ks)
    return _host_metrics(got, data, kh, kw, ks)


# the diagnostic: 288 x 288 windows (both kernels specialised), 7 x 7 kernels, walks of 3 maps
DIAG_K = 7
DIAG_HW = 288 - DIAG_K + 1 - 3


def diagnostic_kernels(F):
    """[(description, kernel)]: one non-zero feature plane each for f in {0, 1, F/2, F-1}, then sparse kernels whose taps sit in
    different planes and include column kw - 1 and row kh - 1"""
    rng = np.random.default_rng(F)
    out = []
    for f in (0, 1, F // 2, F - 1):
        k = np.zeros((DIAG_K, DIAG_K, F), dtype=np.float32)
        k[:, :, f] = rng.standard_normal((DIAG_K, DIAG_K))
        out.append(("plane %d" % f, k))
    e = DIAG_K - 1
    for taps in ([(0, 0, 0), (e, e, F - 1)], [(e, 0, 1), (0, e, F // 2), (3, 2, F - 2)], [(e, e, 0), (2, e, 1), (e, 4, F - 1), (1, 1, F // 3)]):
        k = np.zeros((DIAG_K, DIAG_K, F), dtype=np.float32)
        for i, j, f in taps:
            k[i, j, f] = 1.0 + 0.25 * f / F
        out.append(("taps %s" % (taps,), k))
    return [(d, np.asfortranarray(k)) for d, k in out]


def shift_add(data, k, fh, fw):
    """float64 linear convolution of data (H x W x F) with k (kh x kw x F) summed over the features, zero-padded to fh x fw:
    one shifted copy of a plane per non-zero tap, no transform"""
    H, W, F = data.shape
    out = np.zeros((fh, fw))
    for i, j, f in zip(*np.nonzero(k)):
        out[i:i + H, j:j + W] += float(k[i, j, f]) * data[:, :, f].astype(np.float64)
    return out


def _case_diagnostic(F):
    data = np.asfortranarray(np.random.default_rng(F + 1).standard_normal((DIAG_HW, DIAG_HW, F), dtype=np.float32))
    named = diagnostic_kernels(F)
    ks = [k for _, k in named]
    with util.load_package().Plan(DIAG_HW, DIAG_HW, F, DIAG_K, DIAG_K, options={"exact_window": 1, "rows_group": 3}) as p:
        assert (p.info.transform_h, p.info.transform_w) == (288, 288) and p.get_option("specialised_kernels") == 3
        p.set_image(data)
        got = p.convolve(ks)
    res = []
    for (what, k), g in zip(named, got):
        m = util.accuracy(g, shift_add(data, k, 288, 288))
        hint = ""
        if not all(x < b for x, b in zip(m, util.BUDGET_DIRECT)) and what.startswith("plane"):
            f = int(what.split()[1])      # which plane of the image did the map come from?
            errs = [util.accuracy(g, shift_add(data[:, :, [q]], k[:, :, [f]], 288, 288))[1] for q in range(F)]
            hint = "; the map matches image plane %d best (L2 %.2e)" % (int(np.argmin(errs)), min(errs))
        res.append((what + hint, m))
    return res


def _case_hog(F, route):
    """HOG-like: about 200 x 300 cells, 20 ragged filters of 6-15 cells"""
    rng = np.random.default_rng(F)
    sizes = [(int(rng.integers(6, 16)), int(rng.integers(6, 16))) for _ in range(20)]
    sizes[0], sizes[1] = (15, 15), (15, 15)
    data, ks = _inputs(200, 300, F, sizes, F + 100)
    fc = util.load_package()
    if route == "one_shot":
        got = fc.cudaConvolutionFFT(data, 15, 15, ks)
    else:
        with fc.Plan(200, 300, F, 15, 15) as p:
            assert p.get_option("specialised_kernels") & 1
            p.set_image(data)
            got = p.convolve(ks)
    return _host_metrics(got, data, 15, 15, ks)


def _case_device_packed(H, W, F, k, n, options, expect_specialised):
    """n k x k kernels packed on the device, maps packed on the device (convolve_packed)"""
    torch = _torch()
    data, ks = _inputs(H, W, F, [(k, k)] * n, H * W + F)
    kd = _packed(ks)
    with util.load_package().Plan(H, W, F, k, k, options=options) as p:
        assert bool(p.get_option("specialised_kernels") & 1) == expect_specialised, p.get_option("specialised_kernels")
        p.set_image(data)
        od = torch.empty((n, p.info.fft_w, p.info.fft_h), dtype=torch.float32, device="cuda")
        p.convolve_packed_device(n, kd.data_ptr(), k, k, od.data_ptr())
        p.synchronize()
    ref = _device_reference(data, k, k, ks)
    return [_device_accuracy(o, r) for o, r in zip(od, ref)]


def _case_one_shot(H, W, F, k, n, options):
    data, ks = _inputs(H, W, F, [(k, k)] * (n - 1) + [(k - 2, k // 3)], H + W + F)
    got = util.load_package().cudaConvolutionFFT(data, k, k, ks, options=options)
    return _host_metrics(got, data, k, k, ks, on_device=True)


AUTO_WALK_SHAPE = (2040, 1045, 9, 40)      # exact_window 2048 x 1088 (L = 1088: RPW 1, 1025 row groups), 9 x 40 kernels
AUTO_WALK_MAPS = 17


def auto_walk(F, num_cus=256, slots_per_cu=4):
    """pipeline.hpp: rows_group_for with the automatic choice -- rows_group_auto capped by min(4, 32 / F), at least 2"""
    groups, nmaps = 1025, AUTO_WALK_MAPS
    slots, total = num_cus * max(1, slots_per_cu), groups * nmaps
    if total >= 8 * slots:
        g1 = max(1, min(16, total // (4 * slots), nmaps))
    elif total <= slots:
        g1 = 1
    else:
        g1 = next((w for w in range(2, min(16, nmaps) + 1) if groups * (nmaps // w) <= slots), min(16, nmaps))
    return g1 if F == 1 else min(g1, max(2, min(4, 32 // F)))


def _logged(fn):
    """(fn(), what it wrote to the process's stderr): the plan's "verbose" lines, one per launch with its maps per launch,
    kernels per column-spectrum chunk and maps per workgroup of the row kernel (fftconv_api.cpp: run_group)"""
    import tempfile
    with tempfile.TemporaryFile() as tmp:
        saved = os.dup(2)
        os.dup2(tmp.fileno(), 2)
        try:
            result = fn()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        return result, tmp.read().decode(errors="replace")


def _case_auto_walk(F, walk):
    torch = _torch()
    H, W, kh, kw = AUTO_WALK_SHAPE
    data, ks = _inputs(H, W, F, [(kh, kw)] * AUTO_WALK_MAPS, F * 7)
    with util.load_package().Plan(H, W, F, kh, kw, options={"exact_window": 1}) as p:
        assert (p.info.transform_h, p.info.transform_w) == (2048, 1088) and p.get_option("specialised_kernels") & 1
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        assert auto_walk(F, cus, p.get_option("rows_slots_per_cu")) == walk, (cus, p.get_option("rows_slots_per_cu"))
        p.set_option("verbose", 1)
        p.set_image(data)
        got, log = _logged(lambda: p.convolve(ks))
    # the walk the launch ran: one launch of all 17 maps
    assert re.findall(r"(\d+) maps per workgroup", log) == [str(walk)], log
    return _host_metrics(got, data, kh, kw, ks, on_device=True)


def _case_plan_settings(shape, settings, n, expect):
    """one plan, host kernels and maps; settings applied with set_option before the image; `expect`: a pattern every launch
    line of the plan's verbose log matches"""
    H, W, F, kh, kw = shape
    data, ks = _inputs(H, W, F, [(kh, kw)] * n, H + W + F + n)
    with util.load_package().Plan(H, W, F, kh, kw) as p:
        for key, value in settings.items():
            p.set_option(key, value)
        p.set_option("verbose", 1)
        p.set_image(data)
        got, log = _logged(lambda: p.convolve(ks))
    key = "maps per workgroup" if "workgroup" in expect else "maps per launch"
    lines = [ln for ln in log.splitlines() if key in ln]
    assert lines and all(re.search(expect, ln) for ln in lines), (expect, log)
    return _host_metrics(got, data, kh, kw, ks)


def _case_prepare(defer):
    """prepare_kernels_packed (an image-column launch of na * F planes), deferred into the image's column pass or not"""
    torch = _torch()
    H, W, F, k, n = 500, 520, 16, 31, 6
    data, ks = _inputs(H, W, F, [(k, k)] * n, 77 + defer)
    kd = _packed(ks)
    with util.load_package().Plan(H, W, F, k, k) as p:
        p.set_option("defer_prepare", defer)
        p.prepare_kernels_packed_device(n, kd.data_ptr(), k, k)
        assert p.get_option("prepare_pending") == defer
        p.set_image(data)
        od = torch.empty((n, p.info.fft_w, p.info.fft_h), dtype=torch.float32, device="cuda")
        p.convolve_packed_device(n, kd.data_ptr(), k, k, od.data_ptr())
        p.synchronize()
    ref = _device_reference(data, k, k, ks)
    return [_device_accuracy(o, r) for o, r in zip(od, ref)]


def _case_output_routes(F):
    """the "same" output_region (the crop kernel after the output kernel) and the host_stream ring (pinned, chunks of 64 KB
    over three slots: many wraps) on one plan"""
    H, W, k, n = 500, 520, 31, 5
    data, ks = _inputs(H, W, F, [(k, k)] * n, 19)
    ref = numpy_reference(data, k, k, ks)
    res = []
    with util.load_package().Plan(H, W, F, k, k) as p:
        p.set_image(data)
        p.set_option("output_region", 2)
        assert (p.info.out_h, p.info.out_w) == (H, W)
        h0 = w0 = (k - 1) // 2
        res += [util.accuracy(g, r[h0:h0 + H, w0:w0 + W]) for g, r in zip(p.convolve(ks), ref)]
        p.set_option("output_region", 0)
        for key, value in (("host_stream", 2), ("host_chunk_kb", 64), ("host_slots", 3), ("host_min_kb", 0)):
            p.set_option(key, value)
        res += [util.accuracy(g, r) for g, r in zip(p.convolve(ks), ref)]
    return res


def _case_flip():
    """flip_kernels with 64 x 256 x 9 x 9 = 1.3 M kernel elements (k_flip_planes loops over its grid): the maps of the flipped
    kernels"""
    H, W, F, k, n = 60, 70, 256, 9, 64
    data, ks = _inputs(H, W, F, [(k, k)] * n, 5)
    with util.load_package().Plan(H, W, F, k, k) as p:
        p.set_option("flip_kernels", 1)
        p.set_image(data)
        got = p.convolve(ks)
    flipped = [np.asfortranarray(x[::-1, ::-1, :]) for x in ks]
    return _host_metrics(got, data, k, k, flipped, on_device=True)


def _case_spectrum_exchange():
    """export_spectrum at F = 32 against numpy.fft.rfft2 bin by bin, imported into a fresh plan, and the maps of both plans"""
    H, W, F, kh, kw, n = 270, 272, 32, 13, 11, 3          # 288 x 288, both kernels specialised
    fh, fw = util.ceil16(H + kh - 1), util.ceil16(W + kw - 1)
    data, ks = _inputs(H, W, F, [(kh, kw)] * n, 32)
    padded = np.zeros((F, fw, fh))
    padded[:, :W, :H] = np.transpose(data, (2, 1, 0))
    fc = util.load_package()
    with fc.Plan(H, W, F, kh, kw, options={"exact_window": 1}) as p:
        p.set_image(data)
        spec = p.export_spectrum()
        got = p.convolve(ks)
    err = util.spectrum_bin_error(spec, np.fft.rfft2(padded, axes=(1, 2)))
    with fc.Plan(H, W, F, kh, kw, options={"exact_window": 1}) as q:
        q.import_spectrum(spec)
        got2 = q.convolve(ks)
    return err, _host_metrics(got + got2, data, kh, kw, ks + ks)


def _case_blockwise(shape, n, options, expect, transform_w):
    """a plan the planner makes block-wise (expect 'blockwise') or keeps in one pass ('one pass', on a row transform of
    transform_w points by the generic kernels); host maps"""
    H, W, F, kh, kw = shape
    data, ks = _inputs(H, W, F, [(kh, kw)] * (n - 1) + [(max(1, kh - 2), max(1, kw - 2))], H + W + F)
    with util.load_package().Plan(H, W, F, kh, kw, options=options) as p:
        planned = p.get_option("blockwise")
        overlap_save = p.get_option("overlap_save")
        rows = (p.info.transform_w, p.get_option("specialised_kernels") & 1)
        p.set_image(data)
        got = p.convolve(ks)
    if expect == "one pass":
        assert planned == 0 and rows == (transform_w, 0), (planned, rows)
    else:
        assert planned > 1 and overlap_save == 1, (planned, overlap_save)
    return _host_metrics(got, data, kh, kw, ks)


def _case_mex_two_step(F):
    """fftData = cudaFFTData(data, kH, kW) -> cudaConvFFTData(fftData, kernelCell) through the MEX gateways (tests/mexmock)"""
    from test_mex_gateway import Mex
    mex = Mex()
    H, W, kh, kw, n = 90, 110, 9, 12, 4
    data, ks = _inputs(H, W, F, [(kh, kw)] * (n - 1) + [(5, 7)], 31)
    raised, out = mex.call("cudaFFTData", [mex.numeric(data), mex.scalar(kh), mex.scalar(kw)])
    assert not raised, out
    fft_data = out[0]
    raised, out = mex.call("cudaConvFFTData", [fft_data, mex.cell([mex.numeric(k) for k in ks])])
    assert not raised, out
    got = mex.cell_to_list(out[0], n)
    mex.rt.mock_free(fft_data)
    return _host_metrics(got, data, kh, kw, ks)


# ---- the tests

@pytest.mark.gpu
@pytest.mark.parametrize("L,F,walk,widths", ROW_CASES, ids=["L%d-F%d-walk%d" % c[:3] for c in ROW_CASES])
def test_every_feature_row_kernel(device, L, F, walk, widths):
    """every k_fast_rows_multi_f instantiation of length L: one launch per NZ2 entry, distinct kernels walked `walk` at a time"""
    check("rows", util.BUDGET_DIRECT, device("_case_rows", L, F, walk, widths), (L, F, walk, widths))


@pytest.mark.gpu
@pytest.mark.parametrize("N", COL_LENGTHS)
def test_every_column_length_three_features(device, N):
    check("columns", util.BUDGET_DIRECT, device("_case_column_length", N), (N, "h", 3))


@pytest.mark.gpu
@pytest.mark.parametrize("F", [32, 256])
def test_feature_plane_diagnostic(device, F):
    """no transform in the reference: a map that comes from the wrong feature plane or the wrong kernel of a walk fails with
    the kernel's planes in the message (and, for a one-plane kernel, the image plane the map matches)"""
    for what, m in device("_case_diagnostic", F):
        check("diagnostic", util.BUDGET_DIRECT, [m], (F, what))


@pytest.mark.gpu
@pytest.mark.parametrize("F,route", [(31, "plan"), (32, "one_shot")])
def test_hog_like_features(device, F, route):
    check("hog", util.BUDGET_DIRECT, device("_case_hog", F, route), (F, route))


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,F,k,n,options,spec", [
    (64, 64, 256, 3, 16, {}, False),                   # 66 x 80: the planner's generic lengths
    (96, 128, 512, 7, 8, {}, False),
    (250, 270, 256, 7, 8, {}, True),                   # 288 x 288: both kernels specialised
    (250, 270, 256, 7, 8, {"kernel_path": 1}, False),  # ... and forced onto the generic kernels
], ids=["F256-3x3", "F512-7x7", "F256-specialised", "F256-generic"])
def test_cnn_like_features(device, H, W, F, k, n, options, spec):
    check("cnn", util.BUDGET_DIRECT, device("_case_device_packed", H, W, F, k, n, options, spec), (H, W, F, k, options))


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,F,k,n", [(1024, 1024, 32, 63, 4), (2048, 2048, 16, 63, 6)], ids=["cfg2-F32", "cfg5-F16"])
def test_baseline_geometry_features(device, H, W, F, k, n):
    """cfg2's 1024^2 (63^2 kernels, 1152^2 specialised) at F = 32 and cfg5's 2048^2 (2112^2) at F = 16, one-shot entry"""
    check("baseline", util.BUDGET_DIRECT, device("_case_one_shot", H, W, F, k, n, {}), (H, W, F, k))


@pytest.mark.gpu
@pytest.mark.parametrize("F,walk", [(F, auto_walk(F)) for F in (8, 9, 16, 32)], ids=["F%d-walk%d" % (F, auto_walk(F)) for F in (8, 9, 16, 32)])
def test_automatic_walk_length(device, F, walk):
    """17 maps on 1025 row groups: rows_group_auto alone walks 4, the F cap gives 4 / 3 / 2 / 2 (remainders 1 / 2 / 1 / 1)"""
    check("walks", util.BUDGET_DIRECT, device("_case_auto_walk", F, walk), (F, walk))


@pytest.mark.gpu
@pytest.mark.parametrize("shape,settings,n,expect", [
    ((500, 520, 4, 31, 31), {"rows_group": 2}, 7, r"\b2 maps per workgroup"),
    ((500, 520, 4, 31, 31), {"rows_group": 5}, 7, r"\b5 maps per workgroup"),
    ((300, 400, 16, 21, 21), {"batch_maps": 1}, 5, r"maps per launch 1, kernels per column-spectrum chunk 1,"),
    ((300, 400, 16, 21, 21), {"batch_maps": 3}, 8, r"maps per launch 3, kernels per column-spectrum chunk 3,"),
    ((300, 400, 16, 21, 21), {"batch_maps": 0}, 8, r"maps per launch 8, kernels per column-spectrum chunk 8,"),
    # 384 x 480 plan: 16 x 193 x 24 complex values (593 KB) of column spectra per kernel, three to a 2-MB chunk: one map per
    # launch, three launches per chunk (the row kernel reads its kernels at offsets 1 and 2 inside a chunk)
    ((300, 400, 16, 21, 21), {"batch_maps": 1, "kernel_chunk_mb": 2}, 8, r"maps per launch 1, kernels per column-spectrum chunk 3,"),
], ids=["walk2-F4", "walk5-F4", "batch1", "batch3", "batch-auto", "batch1-chunks-of-3"])
def test_batching_and_walks(device, shape, settings, n, expect):
    check("batching", util.BUDGET_DIRECT, device("_case_plan_settings", shape, settings, n, expect), (shape, settings))


@pytest.mark.gpu
@pytest.mark.parametrize("defer", [0, 1])
def test_prepared_kernels(device, defer):
    check("prepare", util.BUDGET_DIRECT, device("_case_prepare", defer), ("defer_prepare", defer))


@pytest.mark.gpu
def test_output_routes(device):
    check("routes", util.BUDGET_DIRECT, device("_case_output_routes", 16), "output_region same / host_stream ring F16")


@pytest.mark.gpu
def test_flip_kernels_many_planes(device):
    check("flip", util.BUDGET_DIRECT, device("_case_flip"), "flip_kernels F256")


@pytest.mark.gpu
def test_spectrum_export_and_import(device):
    err, metrics = device("_case_spectrum_exchange")
    print("spectrum F32: per bin %.2e" % err)
    assert err < util.BUDGET_SPECTRUM_BIN, err
    check("spectrum", util.BUDGET_DIRECT, metrics, "export / import F32")


# (the row forms -- Bluestein, acc_in_y, no single-pass plan -- of these shapes are checked against the planner on the CPU tier:
#  test_features_host.test_plan_form_cases_take_the_named_path)
BLUESTEIN_ACC_SHAPE = (12, 8346, 16, 5, 23)       # exact_window 16 x 8368: Bluestein row, feature sum in the intermediate
SINGLE_PASS_SHAPE = (12, 10500, 3, 5)             # (H, W, kh, kw): 10648 in one pass at F = 1, no single-pass plan at F = 4


@pytest.mark.gpu
@pytest.mark.parametrize("shape,n,options,expect,transform_w,budget", [
    (BLUESTEIN_ACC_SHAPE, 3, {"exact_window": 1}, "one pass", 8368, util.BUDGET_BLUESTEIN),
    (SINGLE_PASS_SHAPE[:2] + (1,) + SINGLE_PASS_SHAPE[2:], 3, {}, "one pass", 10648, util.BUDGET_DIRECT),
    (SINGLE_PASS_SHAPE[:2] + (4,) + SINGLE_PASS_SHAPE[2:], 3, {}, "blockwise", None, util.BUDGET_DIRECT),
    ((1500, 1400, 16, 63, 63), 4, {"max_transform": 576}, "blockwise", None, util.BUDGET_DIRECT),   # overlap-save blocks
], ids=["bluestein-acc-in-y-F16", "single-pass-F1", "single-pass-limit-F4", "overlap-save-F16"])
def test_plan_forms(device, shape, n, options, expect, transform_w, budget):
    check("plans", budget, device("_case_blockwise", shape, n, options, expect, transform_w), (shape, options, expect))


@pytest.mark.gpu
def test_mex_two_step_thirty_one_features(device):
    check("mex", util.BUDGET_DIRECT, device("_case_mex_two_step", 31), "cudaFFTData -> cudaConvFFTData F31")
