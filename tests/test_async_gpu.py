"""Asynchronous contracts, GPU tier: every entry of include/fftconv.h that may return before its work has run, called while the
plan's stream is BEHIND the host.  The rest of the tier does `call; synchronize; compare`, mostly on the default stream, where
the GPU has caught up whenever a call returns: the guards that only matter otherwise -- PinBuf::mark / wait around the pinned
staging the CPU writes, the stream test on prepared column spectra, flush_pending_prepare, the self-resetting tile-queue
counters, the events of multi_gpu.py -- can be removed there without a test noticing.

Every scenario runs on a non-blocking torch.cuda.Stream (never the default stream) with all torch work on that stream, its
outputs pre-filled with NaN, in three timings on one plan:
    sync   a device-wide synchronisation after every call (the reference run; also the warm-up that sizes the scratch),
    idle   the calls back to back on an idle stream,
    lag    the same calls behind util.lag(): a finite 50 ms spin queued on the stream first (the calls cost about 0.1 ms of host
           time, so the whole scenario is issued while the stream has not started on it),
with no synchronisation between the calls of idle / lag and one at the end.  Assertions: every map of every step against the
float64 oracle under util.BUDGET_DIRECT (no new bar), and -- one-pass and overlap-save plans write every output element once,
without float atomics -- idle and lag bit-identical to sync.  Entries the header promises never to synchronise (set_image(DEVICE),
convolve_packed, prepare_kernels_packed after a warm-up; host set_image / convolve on the pinned small path at the FIRST use of
a pinned buffer) must return while the lag event is still pending: otherwise the case fails as "no lag".  The second fill of a
pinned buffer has to wait for the GPU -- that wait is the guard under test -- and calls that may block (pageable arrays beyond the
pinned sizes, host_pinned = 0, block-wise plans) are exempt: they must merely be right.

The cases run in the module's child process (test_accuracy_gpu._Child): after a crash or a timeout nothing more starts on the
device."""
import importlib
import math
import time

import numpy as np
import pytest

import util
from test_accuracy_gpu import _Child

pytestmark = pytest.mark.gpu

LAG_MS = 50.0
MODES = ("sync", "idle", "lag")


@pytest.fixture(scope="module")
def device():
    child = _Child(globals())
    start = time.perf_counter()
    yield child
    if child.gone:
        child.kill()
    else:
        child.ex.shutdown(wait=True)
    print("test_async_gpu child: %.1f s" % (time.perf_counter() - start))


def judge(r, what, never_sync, identical=True):
    """r: what _outcome() returned in the child"""
    print("async %s: lag pending at the check %s; idle max %.2e L2 %.2e spectral %.2e (bit-identical to sync: %s); "
          "lag max %.2e L2 %.2e spectral %.2e (bit-identical to sync: %s)"
          % ((what, r["pending"]) + tuple(r["worst"]["idle"]) + (r["equal"]["idle"],) + tuple(r["worst"]["lag"]) + (r["equal"]["lag"],)))
    for mode in MODES:
        assert all(x < b for x, b in zip(r["worst"][mode], util.BUDGET_DIRECT)), (what, mode, r["worst"][mode], util.BUDGET_DIRECT)
    if identical:
        assert r["equal"]["idle"] and r["equal"]["lag"], (what, r["equal"])
    if never_sync:
        assert r["pending"] is True, "no lag: the stream had caught up when the calls of %s returned (%r)" % (what, r["pending"])


# ---- the child's side

def _ctx():
    import torch
    return torch, util.load_package(), torch.device("cuda", 0)


_REFS = {}


def _reference(img, mkh, mkw, ks, key):
    """float64 oracle maps, kept per key: the cases of one shape share their inputs"""
    if key not in _REFS:
        _REFS[key] = util.Oracle().conv_fft(img, mkh, mkw, ks, f64=True)
    return _REFS[key]


def _uniform(ks):
    """the cell of util.normal_inputs with its ragged kernel zero-padded to the common size (packed kernels have one size)"""
    kh, kw = max(k.shape[0] for k in ks), max(k.shape[1] for k in ks)
    return [np.asfortranarray(np.pad(k, ((0, kh - k.shape[0]), (0, kw - k.shape[1]), (0, 0)))) for k in ks]


def _kernel(kh, kw, F, seed):
    return util.normal_inputs((1, 1, F, kh, kw, 1), seed)[1][0]


def _image_t(torch, img):
    """host tensor [F][W][H] of a MATLAB H x W x F image"""
    return torch.from_numpy(np.ascontiguousarray(np.transpose(img, (2, 1, 0))))


def _pack_t(torch, ks):
    """host tensor [n][F][kw][kh] of equally sized kernels"""
    return torch.from_numpy(np.ascontiguousarray(np.stack([np.transpose(k, (2, 1, 0)) for k in ks])))


def _poison(arrays):
    for a in arrays:
        a.fill(np.nan)


def _nan_maps(torch, dev, n, w, h):
    return torch.full((n, w, h), float("nan"), dtype=torch.float32, device=dev)


def _ptrs(t):
    return [t[j].data_ptr() for j in range(t.shape[0])]


def judge_maps(outs, refs, crop=None):
    """worst util.accuracy() triple over the maps of outs (host arrays [n][w][h]) against refs (per array the float64 maps,
    h x w, or the windows `crop` cuts out of); a NaN anywhere counts as infinite"""
    w = [0.0, 0.0, 0.0]
    for o, rs in zip(outs, refs):
        assert o.shape[0] == len(rs)
        for j, r in enumerate(rs):
            m = util.accuracy(o[j].T, r if crop is None else r[crop])
            w = [max(a, float("inf") if math.isnan(b) else b) for a, b in zip(w, m)]
    return tuple(w)


class _Timing:
    """one timing of a scenario: lag() queues the spin (lag timing only), between() stands between two calls (sync timing: the
    device catches up; a device-wide wait, which -- unlike fftconv_plan_synchronize -- leaves a deferred preparation pending),
    returned() is where the never-synchronise promise is checked: every spin queued so far must still be running"""

    def __init__(self, torch, mode):
        self.torch, self.mode, self.events, self.pending = torch, mode, [], None

    def lag(self, stream):
        if self.mode == "lag":
            self.events.append(util.lag(stream, LAG_MS))

    def between(self):
        if self.mode == "sync":
            self.torch.cuda.synchronize()

    def returned(self):
        if self.mode == "lag":
            now = all(not ev.query() for ev in self.events)
            self.pending = now if self.pending is None else (self.pending and now)


def _outcome(torch, run, refs, crop=None):
    """run(t) issues the scenario once in the timing t and returns its output tensors ([n][w][h] each); refs: per output tensor
    the float64 maps (h x w).  -> what judge() reads"""
    got, pending = {}, None
    for mode in MODES:
        torch.cuda.synchronize()
        t = _Timing(torch, mode)
        outs = run(t)
        torch.cuda.synchronize()
        got[mode] = [o.cpu().numpy() for o in outs]
        if mode == "lag":
            pending = t.pending
    worst = {mode: judge_maps(got[mode], refs, crop) for mode in MODES}
    equal = {mode: all(np.array_equal(a, b) for a, b in zip(got["sync"], got[mode])) for mode in MODES}     # (a NaN left anywhere: not equal)
    return {"pending": pending, "worst": worst, "equal": equal}


def _case_calibrate():
    """(kind, unit per ms) of util.lag_calibrate and the measured length of one lag(LAG_MS)"""
    torch, fc, dev = _ctx()
    stream = torch.cuda.Stream(dev)
    kind, unit = util.lag_calibrate(stream)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    t0 = time.perf_counter()
    ev = util.lag(stream, LAG_MS)
    host_ms = (time.perf_counter() - t0) * 1e3
    pending = not ev.query()
    e1.record(stream)
    e1.synchronize()
    return kind, unit, e0.elapsed_time(e1), host_ms, pending


# -- a. pinned image reuse

def _case_pinned_image(shape, host_pinned):
    torch, fc, dev = _ctx()
    H, W, F, kh, kw, n = shape
    img1, ks1 = util.normal_inputs(shape, 21)
    img2, ks2 = util.normal_inputs(shape, 22)
    ks1, ks2 = _uniform(ks1), _uniform(ks2)        # one group a call: the check below stands behind the FIRST use of pin_k
    refs = [_reference(img1, kh, kw, ks1, ("a", shape, 21)), _reference(img2, kh, kw, ks2, ("a", shape, 22))]
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream), fc.Plan(H, W, F, kh, kw, stream=stream.cuda_stream) as p:
        p.set_option("host_pinned", host_pinned)
        fh, fw = p.info.fft_h, p.info.fft_w

        def run(t):
            outs = [_nan_maps(torch, dev, n, fw, fh) for _ in range(2)]
            a1, a2 = img1.copy(order="F"), img2.copy(order="F")
            c1, c2 = [k.copy(order="F") for k in ks1], [k.copy(order="F") for k in ks2]
            t.lag(stream)
            p.set_image(a1)
            _poison([a1])                         # consumed when the call returned
            t.between()
            p.convolve_to_device(c1, _ptrs(outs[0]))
            _poison(c1)
            t.returned()
            t.between()
            p.set_image(a2)                       # the second fill of pin_img: waits for the transform of img1
            _poison([a2])
            t.between()
            p.convolve_to_device(c2, _ptrs(outs[1]))
            _poison(c2)
            return outs

        return _outcome(torch, run, refs)


# -- b. pinned kernel reuse

B_IMAGE = (256, 256, 1, 63, 63)


def _case_pinned_kernels(variant):
    torch, fc, dev = _ctx()
    H, W, F, mkh, mkw = B_IMAGE
    img = util.normal_inputs(B_IMAGE + (1,), 31)[0]
    small = lambda seed, kh=31, kw=31: [_kernel(kh, kw, F, seed + j) for j in range(3)]
    first, last = small(100), small(200, 17, 9)
    location = fc.HOST
    if variant == "sets":            # same sizes: the same bytes of pin_k, other values
        middle = small(300)
    elif variant == "ragged":        # four groups in one call: pin_k refilled inside it
        middle = [_kernel(kh, kw, F, 400 + j) for j, (kh, kw) in enumerate([(31, 31), (31, 31), (15, 7), (63, 63), (63, 63), (5, 5)])]
    elif variant == "large":         # 40 x 63 x 63 floats = 620 KiB: beyond the pinned path, staged in K by the runtime's copies
        middle = [_kernel(63, 63, F, 500 + j) for j in range(40)]
    else:                            # "auto": host arrays and device tensors in one cell, two groups
        middle = [_kernel(kh, kw, F, 600 + j) for j, (kh, kw) in enumerate([(31, 31), (31, 31), (31, 31), (15, 15), (15, 15)])]
        location = fc.AUTO
    orc = util.Oracle()
    refs = [orc.conv_fft(img, mkh, mkw, ks, f64=True) for ks in (first, middle, last)]
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream), fc.Plan(H, W, F, mkh, mkw, stream=stream.cuda_stream) as p:
        fh, fw = p.info.fft_h, p.info.fft_w
        img_d = _image_t(torch, img).to(dev)
        on_device = {j: _image_t(torch, middle[j]).to(dev) for j in (1, 3)} if variant == "auto" else {}
        stream.synchronize()

        def run(t):
            outs = [_nan_maps(torch, dev, len(ks), fw, fh) for ks in (first, middle, last)]
            cells = [[k.copy(order="F") for k in ks] for ks in (first, middle, last)]
            host = [list(c) for c in cells]
            for j, d in on_device.items():
                cells[1][j] = (d.data_ptr(), middle[j].shape[0], middle[j].shape[1])
                host[1][j] = None
            t.lag(stream)
            p.set_image_device(img_d.data_ptr())
            t.between()
            for i, loc in enumerate((fc.HOST, location, fc.HOST)):
                p.convolve_to_device(cells[i], _ptrs(outs[i]), loc)
                _poison([a for a in host[i] if a is not None])       # pageable arrays: consumed when the call returned
                if i == 0:
                    t.returned()
                t.between()
            return outs

        return _outcome(torch, run, refs)


# -- c. packed steps back to back

PACKED = {
    "tile queue, three launches": ((1024, 1024, 1, 63, 63, 5), {}, {"batch_maps": 2}),
    "F = 2 walk": ((300, 260, 2, 31, 17, 7), {}, {}),
    "generic kernels": ((300, 260, 2, 31, 17, 3), {"kernel_path": 1}, {}),
    "output_region 2": ((1024, 1024, 1, 63, 63, 3), {}, {"batch_maps": 2, "output_region": 2}),
    "flip_kernels": ((256, 256, 1, 31, 31, 3), {}, {"flip_kernels": 1}),
    "overlap-save blocks": ((1024, 1024, 1, 63, 63, 3), {"max_transform": 576}, {}),
}
PACKED_STEPS = 5


def _case_packed(name):
    torch, fc, dev = _ctx()
    shape, options, settings = PACKED[name]
    H, W, F, kh, kw, n = shape
    orc = util.Oracle()
    steps = []
    for k in range(PACKED_STEPS):
        img, ks = util.normal_inputs(shape, 40 + k)
        ks = _uniform(ks)
        steps.append((img, ks, orc.conv_fft(img, kh, kw, ks, f64=True)))
    refs = [s[2] for s in steps]
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream), fc.Plan(H, W, F, kh, kw, stream=stream.cuda_stream, options=options) as p:
        for key, value in settings.items():
            p.set_option(key, value)
        if name == "overlap-save blocks":
            assert p.get_option("blockwise") > 1 and p.get_option("overlap_save") == 1
        elif name == "tile queue, three launches":
            assert p.get_option("dynamic_tiles") == 1 and p.get_option("blockwise") == 0
        ow, oh = p.info.out_w, p.info.out_h
        crop = None
        if settings.get("output_region") == 2:
            assert (oh, ow) == (H, W)
            crop = (slice((kh - 1) // 2, (kh - 1) // 2 + H), slice((kw - 1) // 2, (kw - 1) // 2 + W))
        flip = settings.get("flip_kernels")            # the plan flips: it is handed the flipped kernels and must give the maps of the originals
        imgs_h = [_image_t(torch, s[0]).pin_memory() for s in steps]
        kers_h = [_pack_t(torch, [np.asfortranarray(k[::-1, ::-1, :]) for k in s[1]] if flip else s[1]).pin_memory() for s in steps]
        img_d = [torch.empty(imgs_h[0].shape, dtype=torch.float32, device=dev) for _ in range(2)]   # two device buffers in turn, refilled on the same stream
        ker_d = [torch.empty(kers_h[0].shape, dtype=torch.float32, device=dev) for _ in range(2)]

        def run(t):
            outs = [_nan_maps(torch, dev, n, ow, oh) for _ in range(PACKED_STEPS)]
            t.lag(stream)
            for k in range(PACKED_STEPS):
                b = k & 1
                img_d[b].copy_(imgs_h[k], non_blocking=True)
                ker_d[b].copy_(kers_h[k], non_blocking=True)
                t.between()
                p.set_image_device(img_d[b].data_ptr())
                t.between()
                p.convolve_packed_device(n, ker_d[b].data_ptr(), kh, kw, outs[k].data_ptr())
                t.between()
            t.returned()
            return outs

        return _outcome(torch, run, refs, crop)


# -- d. prepare / defer / streams

def _case_prepare_orders(shape, defer):
    """the orders of test_gpu_parity.test_deferred_kernel_preparation_in_every_order with nothing between the calls, then
    prepared spectra across a stream change: a consumer stream ordered behind the preparation (5) and one ordered only behind
    what came BEFORE it, while the producer stream lags (6: the spectra count on the stream they were produced on, so they
    are recomputed, never read early)"""
    torch, fc, dev = _ctx()
    H, W, F, kh, kw, n = shape
    img, ks = util.normal_inputs(shape, 51)
    img2, ks2 = util.normal_inputs(shape, 52)
    ks, ks2 = _uniform(ks), _uniform(ks2)
    r11, r21, r22 = (_reference(i, kh, kw, k, ("d", shape, j)) for j, (i, k) in enumerate(((img, ks), (img2, ks), (img2, ks2))))
    refs = [r11, r11, r22, r21, r22, r11]
    X, Y = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    with torch.cuda.stream(X), fc.Plan(H, W, F, kh, kw, stream=X.cuda_stream) as p:
        p.set_option("defer_prepare", defer)
        fh, fw = p.info.fft_h, p.info.fft_w
        img_d, img2_d = _image_t(torch, img).to(dev), _image_t(torch, img2).to(dev)
        k_d, k2_d = _pack_t(torch, ks).to(dev), _pack_t(torch, ks2).to(dev)
        X.synchronize()
        prepare = lambda k: p.prepare_kernels_packed_device(n, k.data_ptr(), kh, kw)
        convolve = lambda k, o: p.convolve_packed_device(n, k.data_ptr(), kh, kw, o.data_ptr())

        def run(t):
            outs = [_nan_maps(torch, dev, n, fw, fh) for _ in range(6)]
            ev = [torch.cuda.Event() for _ in range(5)]
            t.lag(X)
            # 1: prepare -> set_image (deferred: one launch) -> convolve
            prepare(k_d); t.between()
            p.set_image_device(img_d.data_ptr()); t.between()
            convolve(k_d, outs[0]); t.between()
            # 2: prepare -> convolve, the image spectrum reused
            prepare(k_d); t.between()
            convolve(k_d, outs[1]); t.between()
            # 3: prepared for one set of kernels, convolved with another
            prepare(k_d); t.between()
            p.set_image_device(img2_d.data_ptr()); t.between()
            convolve(k2_d, outs[2]); t.between()
            # 4: two preparations, the image transformed on another stream (ordered by the caller both ways), back, convolve
            prepare(k2_d); t.between()
            prepare(k_d); t.between()
            ev[0].record(X); Y.wait_event(ev[0])
            p.set_stream(Y.cuda_stream)
            p.set_image_device(img2_d.data_ptr()); t.between()
            ev[1].record(Y)
            p.set_stream(X.cuda_stream)
            X.wait_event(ev[1])
            convolve(k_d, outs[3]); t.between()
            # 5: prepared on X, consumed on Y, Y ordered behind the preparation
            prepare(k2_d); t.between()
            p.set_stream(Y.cuda_stream)          # (a deferred preparation is launched here, on X)
            ev[2].record(X)
            Y.wait_event(ev[2])
            convolve(k2_d, outs[4]); t.between()
            ev[3].record(Y)
            p.set_stream(X.cuda_stream)
            X.wait_event(ev[3])
            t.returned()
            # 6: X lags again, prepares; Y is ordered behind everything BEFORE that and transforms + convolves at once
            ev[4].record(X)
            t.lag(X)
            prepare(k_d); t.between()
            p.set_stream(Y.cuda_stream)
            Y.wait_event(ev[4])
            p.set_image_device(img_d.data_ptr()); t.between()
            convolve(k_d, outs[5]); t.between()
            p.set_stream(X.cuda_stream)
            t.returned()
            return outs

        return _outcome(torch, run, refs)


# -- e. spectrum hand-over

E_HAND = (300, 260, 2, 31, 17, 3)
E_STEPS = 6


def _case_handover_by_hand():
    """HipPlanEngine's pattern by hand: two caller-owned spectrum buffers, set_image of step k + 1 on a side stream while step k
    convolves on the (lagging) main stream, the events placed as FilterShardedConvolver places them"""
    torch, fc, dev = _ctx()
    H, W, F, kh, kw, n = E_HAND
    orc = util.Oracle()
    ks = _uniform(util.normal_inputs(E_HAND, 60)[1])
    imgs = [util.normal_inputs(E_HAND, 61 + k)[0] for k in range(E_STEPS)]
    refs = [orc.conv_fft(i, kh, kw, ks, f64=True) for i in imgs]
    main, side = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    with torch.cuda.stream(main), fc.Plan(H, W, F, kh, kw, stream=main.cuda_stream) as p:
        fh, fw = p.info.fft_h, p.info.fft_w
        img_d = [_image_t(torch, i).to(dev) for i in imgs]
        k_d = _pack_t(torch, ks).to(dev)
        spec = [torch.empty(p.info.spectrum_bytes, dtype=torch.uint8, device=dev) for _ in range(2)]
        main.synchronize()

        def run(t):
            outs = [_nan_maps(torch, dev, n, fw, fh) for _ in range(E_STEPS)]
            ready, consumed = [torch.cuda.Event() for _ in range(2)], [torch.cuda.Event() for _ in range(2)]

            def submit(k):
                b = k % 2
                side.wait_event(consumed[b])            # never recorded = complete
                p.use_spectrum_buffer(spec[b].data_ptr(), spec[b].numel())
                p.set_stream(side.cuda_stream)
                p.set_image_device(img_d[k].data_ptr())
                p.set_stream(main.cuda_stream)
                ready[b].record(side)
                t.between()

            def convolve(k):
                b = k % 2
                main.wait_event(ready[b])
                p.use_spectrum_buffer(spec[b].data_ptr(), spec[b].numel())
                p.mark_spectrum_valid()
                p.convolve_packed_device(n, k_d.data_ptr(), kh, kw, outs[k].data_ptr())
                consumed[b].record(main)
                t.between()

            t.lag(main)
            submit(0)
            for k in range(E_STEPS):
                if k + 1 < E_STEPS:
                    submit(k + 1)
                convolve(k)
            t.returned()
            return outs

        return _outcome(torch, run, refs)


E_ENGINE = (256, 256, 1, 63, 63, 40)       # 40 x 63 x 63 floats = 620 KiB of kernels: HipPlanEngine's upload stream is live


def _case_handover_convolver(kind):
    """the real orchestration over HipPlanEngine: FilterShardedConvolver(depth = 2) or ImageStreamedConvolver, the kernels
    uploaded inside every step (k_uploaded / k_consumed), on_result copying every step's maps aside on the main stream"""
    torch, fc, dev = _ctx()
    mg = importlib.import_module(fc.__name__ + ".multi_gpu")
    H, W, F, kh, kw, n = E_ENGINE
    ks = [_kernel(kh, kw, F, 700 + j) for j in range(n)]
    imgs = [util.normal_inputs(E_ENGINE[:5] + (1,), 71 + k)[0] for k in range(E_STEPS)]
    refs = [_reference(i, kh, kw, ks, ("e", k)) for k, i in enumerate(imgs)]
    main = torch.cuda.Stream(dev)
    with torch.cuda.stream(main), fc.Plan(H, W, F, kh, kw, stream=main.cuda_stream) as p:
        fh, fw = p.info.fft_h, p.info.fft_w
        kern_pin = _pack_t(torch, ks).pin_memory()
        assert kern_pin.numel() * 4 > (512 << 10)
        img_pin = [_image_t(torch, i).pin_memory() for i in imgs]
        img_d = [i.to(dev) for i in img_pin]
        main.synchronize()

        def run(t):
            aside = [_nan_maps(torch, dev, n, fw, fh) for _ in range(E_STEPS)]
            engine = mg.HipPlanEngine(torch, fc, p, dev, kern_pin.to(dev), kh, kw, main_stream=main, overlap=True,
                                      defer_prepare=(kind == "streamed"), kernels_host=kern_pin)
            assert not engine.zero_copy
            engine.out.fill_(float("nan"))
            seen = []

            def on_result(k, maps):
                aside[k].copy_(maps)             # (the current stream is main)
                seen.append(k)
                t.between()

            if kind == "sharded":
                conv = mg.FilterShardedConvolver(engine, None, 0, 1, n, depth=2)
                images = img_d
            else:
                conv = mg.ImageStreamedConvolver(engine, n)
                images = img_pin
            torch.cuda.synchronize()
            t.lag(main)
            conv.run(images, on_result=on_result)
            t.returned()
            assert seen == list(range(E_STEPS)) and engine.uploads == E_STEPS + 1
            torch.cuda.synchronize()             # (the engine's upload stream included, before its buffers go)
            return aside

        return _outcome(torch, run, refs)


# -- f. two plans, two streams

def _case_two_plans():
    torch, fc, dev = _ctx()
    s1, s2 = (256, 256, 1, 31, 31, 3), (300, 260, 2, 15, 13, 3)
    orc = util.Oracle()
    rounds = []
    for r in range(2):
        i1, k1 = util.normal_inputs(s1, 80 + r)
        i2, k2 = util.normal_inputs(s2, 90 + r)
        rounds.append((i1, _uniform(k1), i2, _uniform(k2)))
    refs = []
    for i1, k1, i2, k2 in rounds:
        refs += [orc.conv_fft(i1, s1[3], s1[4], k1, f64=True), orc.conv_fft(i2, s2[3], s2[4], k2, f64=True)]
    A, B = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    with torch.cuda.stream(A), fc.Plan(*s1[:5], stream=A.cuda_stream) as p1, fc.Plan(*s2[:5], stream=B.cuda_stream) as p2:
        with torch.cuda.stream(B):
            i2_d = [_image_t(torch, r[2]).to(dev) for r in rounds]
            k2_d = [_pack_t(torch, r[3]).to(dev) for r in rounds]
        B.synchronize()

        def run(t):
            outs = []
            for r in range(2):
                outs.append(_nan_maps(torch, dev, s1[5], p1.info.fft_w, p1.info.fft_h))
                with torch.cuda.stream(B):
                    outs.append(_nan_maps(torch, dev, s2[5], p2.info.fft_w, p2.info.fft_h))
            t.lag(A)
            t.lag(B)
            for r, (i1, k1, i2, k2) in enumerate(rounds):
                a, c = i1.copy(order="F"), [k.copy(order="F") for k in k1]
                p1.set_image(a); _poison([a]); t.between()                # host arrays, pinned small path
                p2.set_image_device(i2_d[r].data_ptr()); t.between()
                p1.convolve_to_device(c, _ptrs(outs[2 * r])); _poison(c); t.between()
                p2.convolve_packed_device(s2[5], k2_d[r].data_ptr(), s2[3], s2[4], outs[2 * r + 1].data_ptr()); t.between()
                if r == 0:
                    t.returned()              # (the second round refills p1's pinned buffers: it waits)
            return outs

        return _outcome(torch, run, refs)


# -- g. null-stream set-up next to a non-blocking stream

def _case_null_stream_setup(dynamic_tiles):
    """a plan's tables are uploaded with plain copies and its tile queue is zeroed with a plain memset (at creation; set_option
    "dynamic_tiles" does the same for a plan that has no queue yet): work of the NULL stream, which a non-blocking stream does
    not wait for.  A convolve right behind fftconv_plan_create / set_option on such a stream must find them complete.  No lag;
    three fresh plans."""
    torch, fc, dev = _ctx()
    shape = (256, 256, 1, 31, 31, 3)         # 288-point columns: M = 144 < 432, the static deal by default
    H, W, F, kh, kw, n = shape
    img, ks = util.normal_inputs(shape, 95)
    ks = _uniform(ks)
    ref = util.Oracle().conv_fft(img, kh, kw, ks, f64=True)
    stream = torch.cuda.Stream(dev)
    worst, equal = [0.0, 0.0, 0.0], True
    with torch.cuda.stream(stream):
        img_d, k_d = _image_t(torch, img).to(dev), _pack_t(torch, ks).to(dev)
        outs = [_nan_maps(torch, dev, n, util.ceil16(W + kw - 1), util.ceil16(H + kh - 1)) for _ in range(4)]
        torch.cuda.synchronize()
        for rep in range(3):
            with fc.Plan(H, W, F, kh, kw, stream=stream.cuda_stream) as p:
                assert p.get_option("dynamic_tiles") == 0 and p.get_option("specialised_kernels") == 3
                p.set_image_device(img_d.data_ptr())                      # straight behind fftconv_plan_create
                p.convolve_packed_device(n, k_d.data_ptr(), kh, kw, outs[0].data_ptr())
                for i, d in enumerate(dynamic_tiles):
                    p.set_option("dynamic_tiles", d)
                    p.convolve_packed_device(n, k_d.data_ptr(), kh, kw, outs[1 + i].data_ptr())
                p.synchronize()
                got = [o.cpu().numpy() for o in outs[:1 + len(dynamic_tiles)]]
                p.set_option("dynamic_tiles", 0)
                p.convolve_packed_device(n, k_d.data_ptr(), kh, kw, outs[3].data_ptr())
                p.synchronize()
                again = outs[3].cpu().numpy()
            for g in got:
                equal = equal and np.array_equal(g, again)
                worst = [max(a, b) for a, b in zip(worst, judge_maps([g], [ref]))]
            for o in outs:
                o.fill_(float("nan"))
    return tuple(worst), equal


# ---- the tests

def test_lag_calibration(device):
    """what util.lag() is made of on this device, and that a 50 ms lag is one: long against the ~0.1 ms of a call, still running
    when the call that queued it returns"""
    kind, unit, lag_ms, host_ms, pending = device("_case_calibrate")
    print("lag calibration: %s, %.4g per ms; lag(%g ms) measured %.1f ms on the stream, queued in %.3f ms of host time, "
          "pending on return: %s" % (kind, unit, LAG_MS, lag_ms, host_ms, pending))
    assert pending and 0.5 * LAG_MS <= lag_ms <= 4 * LAG_MS, (lag_ms, pending)


@pytest.mark.parametrize("host_pinned", [1, 0])
@pytest.mark.parametrize("shape", [(256, 256, 1, 31, 31, 3),      # 256 KiB: read in place from pin_img
                                   (300, 260, 2, 15, 13, 3),      # 609 KiB: pinned + one asynchronous copy
                                   (1024, 1024, 1, 63, 63, 2)])   # 4 MiB: pageable, the call may block
def test_pinned_image_reuse(device, shape, host_pinned):
    """a. set_image(img1); convolve; set_image(img2); convolve with host arrays and DEVICE maps, every host array poisoned as
    soon as its call has returned"""
    small = shape[0] * shape[1] * shape[2] * 4 <= (1 << 20)
    judge(device("_case_pinned_image", shape, host_pinned), ("pinned image", shape, host_pinned), never_sync=bool(small and host_pinned))


@pytest.mark.parametrize("variant", ["sets", "ragged", "large", "auto"])
def test_pinned_kernel_reuse(device, variant):
    """b. three fftconv_plan_convolve calls in a row with host kernels and DEVICE maps: a small set (first use of pin_k: must not
    wait), then another small set / a ragged cell / a group beyond 512 KiB / FFTCONV_AUTO over host arrays and device tensors,
    then a small set again; host arrays poisoned after every return"""
    judge(device("_case_pinned_kernels", variant), ("pinned kernels", variant), never_sync=True)


@pytest.mark.parametrize("name", list(PACKED))
def test_packed_steps_back_to_back(device, name):
    """c. five steps of set_image(DEVICE) + convolve_packed, another image and other kernels each, uploaded into two device
    buffers in turn on the same stream, every step's maps kept"""
    judge(device("_case_packed", name), ("packed", name), never_sync=(name != "overlap-save blocks"))


@pytest.mark.parametrize("defer", [0, 1])
@pytest.mark.parametrize("shape", [(256, 256, 1, 31, 31, 3), (300, 260, 2, 15, 13, 5), (1024, 1024, 1, 63, 63, 4)])
def test_prepare_orders_and_streams(device, shape, defer):
    """d. prepare / set_image / convolve in every order with nothing in between, defer_prepare 0 and 1, and prepared column
    spectra across set_stream: recomputed or correctly ordered, never read early (_case_prepare_orders)"""
    judge(device("_case_prepare_orders", shape, defer), ("prepare", shape, defer), never_sync=True)


def test_spectrum_handover_by_hand(device):
    """e. two caller-owned spectrum buffers handed between a side stream (set_image of step k + 1) and the lagging main stream
    (convolve of step k), six steps"""
    judge(device("_case_handover_by_hand"), "hand-over by hand", never_sync=True)


@pytest.mark.parametrize("kind", ["sharded", "streamed"])
def test_spectrum_handover_through_the_convolvers(device, kind):
    """e. FilterShardedConvolver(depth = 2) / ImageStreamedConvolver over HipPlanEngine"""
    judge(device("_case_handover_convolver", kind), ("convolver", kind), never_sync=True)


def test_two_plans_two_streams(device):
    """f. calls of two plans on two lagging streams interleaved from one thread: each plan's maps are its own"""
    judge(device("_case_two_plans"), "two plans", never_sync=True)


@pytest.mark.parametrize("dynamic_tiles", [(1, 2), (2,)])
def test_null_stream_setup_beside_a_non_blocking_stream(device, dynamic_tiles):
    """g. convolve on a non-blocking stream straight behind fftconv_plan_create and behind set_option("dynamic_tiles")"""
    worst, equal = device("_case_null_stream_setup", dynamic_tiles)
    print("async null-stream set-up %s: max %.2e L2 %.2e spectral %.2e, bit-identical to a later run: %s" % ((dynamic_tiles,) + worst + (equal,)))
    assert all(x < b for x, b in zip(worst, util.BUDGET_DIRECT)), worst
    assert equal
