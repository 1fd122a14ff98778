"""Spectral filters (fftconv_plan_set_spectral_filter) on the GPU: phase correlation (mode 1) and Wiener maps (mode 2).

The oracle is NumPy's float64 fft2 over the plan's own transform lengths (info.transform_h x transform_w), written here from the
definition of include/fftconv.h: the window the plan transforms (the zero-padded image, or the bordered extension), the kernel at
the origin after "flip_kernels", the filter per bin, the normalised inverse, the FFT_H x FFT_W window of it.  Parity is
util.rel_err (max-normalised) under the project's bar of 1e-4, on util.synth inputs with three kernels per case and lambda = 1e-3
of the mean |K^|^2; the fp32 arithmetic alone stays two orders of magnitude under that bar at these inputs (numpy complex64 against
complex128: 6e-8 ... 7e-7).  Every case asserts the transform lengths it is about through get_info.

The width case at 2112 runs kernels 3, 33 and 67 columns wide: 3 and 33 both fall to the NZ2 = 3 instantiation of 2112 = 8.12.22
(ceil(33 / 22) = 2 stage-2 inputs), 67 is the narrowest width that reaches the second one (NZ2 = 12).

The cases run in a spawned child (test_accuracy_gpu._Child), which exits with the module."""
import numpy as np
import pytest

import util
from test_accuracy_gpu import _Child

pytestmark = pytest.mark.gpu

BAR = 1e-4
N_KERNELS = 3
# name: (H, W, max_kh, max_kw), kernel sizes, creation options, (transform_h, transform_w), spectral_filter_fast
PARITY = {
    "288": ((270, 270, 19, 19), [(19, 19)] * 3, {}, (288, 288), 1),
    "384 cropped": ((282, 300, 23, 23), [(23, 23)] * 3, {}, (384, 384), 1),
    "2112": ((2000, 2000, 33, 33), [(33, 33)] * 3, {}, (2112, 2112), 1),
    "2560 one row": ((2500, 2500, 40, 40), [(40, 40)] * 3, {}, (2560, 2560), 1),
    "2112 widths 3 33 67": ((2000, 2000, 33, 67), [(33, 3), (33, 33), (33, 67)], {}, (2112, 2112), 1),
    "kernel_path 2 at 1152": ((40, 1100, 9, 31), [(9, 31)] * 3, {"kernel_path": 2}, (48, 1152), 1),
    "kernel_path 1": ((40, 52, 7, 5), [(7, 5)] * 3, {"kernel_path": 1}, (48, 56), 0),
    "exact_window Bluestein 304": ((282, 282, 23, 23), [(23, 23)] * 3, {"exact_window": 1}, (304, 304), 0),
}
SMALL = (270, 270, 19, 19)          # the 288 x 288 window of the composition, state, graph and refusal cases


@pytest.fixture(scope="module")
def device():
    child = _Child(globals())
    yield child
    if child.gone:
        child.kill()
    else:
        child.ex.shutdown(wait=True)


# ---- the oracle

def _inputs(shape, sizes, seed):
    """util.synth image (H x W) and one util.synth kernel per size"""
    H, W, mkh, mkw = shape
    img, _ = util.synth(seed, H, W, 1, 1, 1, 0)
    ks = [util.synth(seed + j, 1, 1, 1, kh, kw, 1)[1][0] for j, (kh, kw) in enumerate(sizes)]
    return img, ks


def _lambda(ks, L):
    """1e-3 of the mean |K^|^2 over the bins of the L[0] x L[1] transform and over the kernels (Parseval: the mean over the bins is
    sum k^2, whatever the lengths)"""
    return float(1e-3 * np.mean([np.sum(np.asarray(k, dtype=np.float64) ** 2) for k in ks]))


def _oracle(window, ks, L, fft, mode, lam, flip=False):
    """float64 maps (fft_h x fft_w) of `window` (2-D, what the plan transforms) under the definition of include/fftconv.h"""
    I = np.fft.fft2(np.asarray(window, dtype=np.float64), s=L)
    out = []
    for k in ks:
        k2 = np.asarray(k, dtype=np.float64)[:, :, 0]
        K = np.fft.fft2(k2[::-1, ::-1] if flip else k2, s=L)
        if mode == 1:
            P = I * K
            mag = np.abs(P)
            X = np.where(mag > 0, P / np.where(mag > 0, mag, 1.0), 0.0)
        elif mode == 2:
            den = np.abs(K) ** 2 + lam
            X = np.where(den > 0, I * np.conj(K) / np.where(den > 0, den, 1.0), 0.0)
        else:
            X = I * K
        r = np.real(np.fft.ifft2(X))
        m = np.zeros(fft, dtype=np.float64)
        h, w = min(fft[0], L[0]), min(fft[1], L[1])
        m[:h, :w] = r[:h, :w]
        out.append(m)
    return out


def _bits_differ(a, b):
    return sum(int((np.ascontiguousarray(x).view(np.uint32 if x.dtype == np.float32 else np.uint16) !=
                    np.ascontiguousarray(y).view(np.uint32 if y.dtype == np.float32 else np.uint16)).sum()) for x, y in zip(a, b))


# ---- the child's side

def _ctx():
    import torch
    return torch, util.load_package(), torch.device("cuda", 0)


def _case_parity(name):
    fc = util.load_package()
    shape, sizes, options, L, fast = PARITY[name]
    H, W, mkh, mkw = shape
    img, ks = _inputs(shape, sizes, 31 + len(name))
    res = {}
    with fc.Plan(H, W, 1, mkh, mkw, options=options) as p:
        i = p.info
        assert (i.transform_h, i.transform_w) == L, (name, i.transform_h, i.transform_w)
        assert p.get_option("spectral_filter") == 0 and p.get_option("spectral_filter_fast") == 0
        fft = (i.fft_h, i.fft_w)
        lam = _lambda(ks, L)
        p.set_image(img)
        for mode in (fc.FILTER_PHASE, fc.FILTER_WIENER):
            p.set_spectral_filter(mode, lam if mode == fc.FILTER_WIENER else 0.0)
            assert p.get_option("spectral_filter") == mode and p.get_option("spectral_filter_fast") == fast, name
            p.set_option("rows_group", 3)                 # one launch walks the three maps ...
            got = p.convolve(ks)
            p.set_option("rows_group", 1)                 # ... another walks one
            one = p.convolve(ks)
            p.set_option("rows_group", 0)
            want = _oracle(img[:, :, 0], ks, L, fft, mode, lam)
            res[mode] = (max(util.rel_err(g, w) for g, w in zip(got, want)), _bits_differ(got, one), int(sum(np.isnan(g).sum() for g in got)))
    return res


def _case_phase_peak(exact):
    """flip_kernels 1, a template cut from the image at (y0, x0): the zero-shift peak lies at (y0 + kh - 1, x0 + kw - 1)"""
    fc = util.load_package()
    H, W, kh, kw = 282, 300, 23, 23
    y0, x0 = 101, 57
    img = np.asfortranarray(np.random.default_rng(77).standard_normal((H, W, 1)).astype(np.float32))
    tpl = np.asfortranarray(img[y0:y0 + kh, x0:x0 + kw, :].copy())
    with fc.Plan(H, W, 1, kh, kw, options={"exact_window": 1} if exact else {}) as p:
        i = p.info
        longer = i.transform_h > i.fft_h and i.transform_w > i.fft_w
        assert longer != bool(exact) and i.exact_window == (1 if exact else 0), (i.transform_h, i.transform_w, i.fft_h, i.fft_w)
        p.set_option("flip_kernels", 1)
        p.set_image(img)
        p.set_spectral_filter(fc.FILTER_PHASE)
        m = p.convolve([tpl])[0]
    peak = np.unravel_index(int(np.argmax(m)), m.shape)
    second = float(np.partition(m.ravel(), -2)[-2])
    return tuple(int(v) for v in peak), (y0 + kh - 1, x0 + kw - 1), float(m[peak]), second


def _case_wiener_peak():
    """an image that is zero except for the kernel itself at (y0, x0) peaks at (y0, x0) with a height in (0, 1]"""
    fc = util.load_package()
    H, W, kh, kw = SMALL
    y0, x0 = 120, 33
    _, ks = _inputs(SMALL, [(kh, kw)], 5)
    img = np.zeros((H, W, 1), dtype=np.float32, order="F")
    img[y0:y0 + kh, x0:x0 + kw, :] = ks[0]
    with fc.Plan(H, W, 1, kh, kw) as p:
        L = (p.info.transform_h, p.info.transform_w)
        p.set_image(img)
        p.set_spectral_filter(fc.FILTER_WIENER, _lambda(ks, L))
        m = p.convolve(ks)[0]
    peak = np.unravel_index(int(np.argmax(m)), m.shape)
    return tuple(int(v) for v in peak), (y0, x0), float(m[peak])


def _case_composition(name):
    fc = util.load_package()
    H, W, kh, kw = SMALL
    img, ks = _inputs(SMALL, [(kh, kw)] * N_KERNELS, 91)
    L = fft = (288, 288)
    lam = _lambda(ks, L)
    out = {}
    with fc.Plan(H, W, 1, kh, kw) as p:
        assert (p.info.transform_h, p.info.transform_w, p.info.fft_h, p.info.fft_w) == L + fft
        for mode in (fc.FILTER_PHASE, fc.FILTER_WIENER):
            param = lam if mode == fc.FILTER_WIENER else 0.0
            p.set_spectral_filter(mode, param)
            p.set_image(img)
            full = p.convolve(ks)
            if name == "fp16":
                p.set_option("map_format", 1)
                got = p.convolve(ks)
                p.set_option("map_format", 0)
                out[mode] = _bits_differ(got, [f.astype(np.float16) for f in full])
            elif name == "rectangle and stride":
                p.set_output_rect(7, 5, 271, 273)
                rect = p.convolve(ks)
                p.set_output_stride(2, 3)
                both = p.convolve(ks)
                p.set_option("output_region", 0)
                win = p.convolve(ks)
                p.set_output_stride(1, 1)
                out[mode] = (_bits_differ(rect, [np.asfortranarray(f[7:278, 5:278]) for f in full]),
                             _bits_differ(both, [np.asfortranarray(f[7:278:2, 5:278:3]) for f in full]),
                             _bits_differ(win, [np.asfortranarray(f[::2, ::3]) for f in full]), p.get_option("spectral_filter"))
            elif name == "image batch":
                imgs = np.asfortranarray(np.stack([util.synth(200 + b, H, W, 1, 1, 1, 0)[0][:, :, 0] for b in range(3)], axis=2))
                singles = []
                for b in range(3):
                    with fc.Plan(H, W, 1, kh, kw) as q:
                        q.set_spectral_filter(mode, param)
                        q.set_image(np.asfortranarray(imgs[:, :, b:b + 1]))
                        singles += q.convolve(ks)
                p.set_option("image_walk", 1)
                p.set_option("batch_maps", 16)                # the three images behind one launch
                p.set_images(imgs)
                active = p.get_option("image_walk_active")
                got = p.convolve(ks)
                p.set_spectral_filter(fc.FILTER_PRODUCT)
                active_off = p.get_option("image_walk_active")
                p.set_option("image_walk", 0)
                p.set_option("batch_maps", 0)
                out[mode] = (len(got), _bits_differ(got, singles), active, active_off)
            elif name == "uint8 image":
                px = np.asfortranarray(np.random.default_rng(6).integers(0, 256, (H, W), dtype=np.uint8))
                p.set_image_typed(px)
                got = p.convolve(ks)
                p.set_image(np.asfortranarray(px.astype(np.float32)[:, :, None]))
                out[mode] = _bits_differ(got, p.convolve(ks))
            elif name == "border replicate":
                p.set_border(fc.BORDER_REPLICATE)
                p.set_image(img)
                got = p.convolve(ks)
                lead_h, lead_w = kh // 2, kw // 2
                ext = np.pad(img[:, :, 0], ((lead_h, kh - 1 - lead_h), (lead_w, kw - 1 - lead_w)), mode="edge")
                want = [w[kh - 1:kh - 1 + H, kw - 1:kw - 1 + W] for w in _oracle(ext, ks, L, fft, mode, lam)]
                out[mode] = (got[0].shape, max(util.rel_err(g, w) for g, w in zip(got, want)))
                p.set_border(fc.BORDER_ZERO)
    return out


def _packed_maps(torch, dev, p, n, ker_d, kh, kw):
    i = p.refresh_info()
    out = torch.full((n, i.out_w, i.out_h), float("nan"), dtype=torch.float32, device=dev)
    p.convolve_packed_device(n, ker_d.data_ptr(), kh, kw, out.data_ptr())
    p.synchronize()
    return out.cpu().numpy()


def _dev_inputs(torch, dev, img, ks):
    img_d = torch.from_numpy(np.ascontiguousarray(np.transpose(img, (2, 1, 0)))).to(dev)
    ker_d = torch.from_numpy(np.ascontiguousarray(np.stack([np.transpose(k, (2, 1, 0)) for k in ks]))).to(dev)
    return img_d, ker_d


def _case_state():
    """one live plan with an image and prepared kernels through modes 0 -> 1 -> 2 -> 0, a convolve after each"""
    torch, fc, dev = _ctx()
    H, W, kh, kw = SMALL
    img, ks = _inputs(SMALL, [(kh, kw)] * N_KERNELS, 17)
    img_d, ker_d = _dev_inputs(torch, dev, img, ks)
    L = fft = (288, 288)
    lam = _lambda(ks, L)
    with fc.Plan(H, W, 1, kh, kw) as q:
        q.set_image_device(img_d.data_ptr())
        fresh = _packed_maps(torch, dev, q, N_KERNELS, ker_d, kh, kw)
    errs, maps = [], []
    with fc.Plan(H, W, 1, kh, kw) as p:
        p.set_option("profile", 1)
        p.set_image_device(img_d.data_ptr())
        p.profile(reset=True)
        for mode in (0, 1, 2, 0):
            p.prepare_kernels_packed_device(N_KERNELS, ker_d.data_ptr(), kh, kw)
            p.set_spectral_filter(mode, lam if mode == 2 else 0.0)          # the image and the prepared kernels survive
            m = _packed_maps(torch, dev, p, N_KERNELS, ker_d, kh, kw)
            maps.append(m)
            if mode:
                want = _oracle(img[:, :, 0], ks, L, fft, mode, lam)
                errs.append(max(util.rel_err(m[k].T, want[k]) for k in range(N_KERNELS)))
        prof = p.profile()
        images = p.get_option("images")
    return (errs, _bits_differ([maps[0]], [fresh]), _bits_differ([maps[3]], [fresh]), prof["kernel_cols"]["launches"], prof["image_cols"]["launches"],
            prof["spectral_rows"]["launches"], images)


def _case_graph():
    """a warm convolve under mode 2 captured into a graph and replayed, as tests/test_graph_gpu.py captures: the plan bound to the
    capturing stream, one eager warm-up with the same arguments, new inputs copied into the captured buffers before the replay"""
    torch, fc, dev = _ctx()
    H, W, kh, kw = SMALL
    sets = [_inputs(SMALL, [(kh, kw)] * N_KERNELS, 300 + k) for k in range(2)]
    lam = _lambda(sets[0][1], (288, 288))
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream), fc.Plan(H, W, 1, kh, kw, stream=stream.cuda_stream) as p:
        p.set_spectral_filter(fc.FILTER_WIENER, lam)
        hosts = [tuple(t.pin_memory() for t in _dev_inputs(torch, torch.device("cpu"), *s)) for s in sets]
        img_d = torch.empty(hosts[0][0].shape, dtype=torch.float32, device=dev)
        ker_d = torch.empty(hosts[0][1].shape, dtype=torch.float32, device=dev)
        out = torch.full((N_KERNELS, p.info.out_w, p.info.out_h), float("nan"), dtype=torch.float32, device=dev)

        def step():
            p.set_image_device(img_d.data_ptr())
            p.convolve_packed_device(N_KERNELS, ker_d.data_ptr(), kh, kw, out.data_ptr())

        img_d.copy_(hosts[0][0], non_blocking=True)
        ker_d.copy_(hosts[0][1], non_blocking=True)
        step()                                   # eager warm-up: nothing allocates from here on
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        cap = torch.cuda.Stream(dev)
        with torch.cuda.graph(graph, stream=cap):
            p.set_stream(torch.cuda.current_stream(dev).cuda_stream)
            step()
        p.set_stream(stream.cuda_stream)
        out.fill_(float("nan"))
        img_d.copy_(hosts[1][0], non_blocking=True)
        ker_d.copy_(hosts[1][1], non_blocking=True)
        graph.replay()
        replayed = out.clone()
        torch.cuda.synchronize()
        out.fill_(float("nan"))
        step()
        torch.cuda.synchronize()
        got, eager = replayed.cpu().numpy(), out.cpu().numpy()
        mode = p.get_option("spectral_filter")
        del graph
    want = _oracle(sets[1][0][:, :, 0], sets[1][1], (288, 288), (288, 288), 2, lam)
    return _bits_differ([got], [eager]), max(util.rel_err(got[k].T, want[k]) for k in range(N_KERNELS)), mode


def _refused(fc, fn, *words):
    try:
        fn()
    except fc.FFTConvError as e:
        return all(w in str(e) for w in words)
    return False


def _case_refusals():
    fc = util.load_package()
    H, W, kh, kw = SMALL
    img, ks = _inputs(SMALL, [(kh, kw)] * N_KERNELS, 23)
    lam = _lambda(ks, (288, 288))
    out = {}
    with fc.Plan(H, W, 1, kh, kw) as p:
        p.set_image(img)
        p.set_spectral_filter(fc.FILTER_WIENER, lam)
        base = p.convolve(ks)
        bad = {"mode 3": (3, 0.0), "mode -1": (-1, 0.0), "nan": (2, float("nan")), "inf": (2, float("inf")), "negative": (2, -1.0), "param in mode 1": (1, 0.5)}
        for what, args in bad.items():
            ok = _refused(fc, lambda a=args: p.set_spectral_filter(*a))
            out[what] = (ok, p.get_option("spectral_filter"), _bits_differ(p.convolve(ks), base))
        # a score while a filter is on: refused, the filter and the image stay
        for what, fn in (("set_match_score", lambda: p.set_match_score(fc.SCORE_CCORR_NORMED, kh, kw)), ("set_normalisation", lambda: p.set_normalisation(1, kh, kw))):
            ok = _refused(fc, fn, "spectral filter")
            out[what] = (ok and p.get_option("match_score") == 0, p.get_option("spectral_filter"), _bits_differ(p.convolve(ks), base))
        p.set_spectral_filter(fc.FILTER_WIENER, lam)              # changes nothing: a no-op
        out["no-op"] = (True, p.get_option("spectral_filter"), _bits_differ(p.convolve(ks), base))
        # a filter while a score is on
        p.set_spectral_filter(fc.FILTER_PRODUCT)
        p.set_match_score(fc.SCORE_CCOEFF, kh, kw)
        p.set_image(img)
        scored = p.convolve(ks)
        for mode in (1, 2):
            ok = _refused(fc, lambda m=mode: p.set_spectral_filter(m, 0.0), "score")
            out["under a score, mode %d" % mode] = (ok and p.get_option("match_score") == 2, p.get_option("spectral_filter"), _bits_differ(p.convolve(ks), scored))
        p.set_normalisation(1, kh, kw)
        p.set_image(img)
        normed = p.convolve(ks)
        ok = _refused(fc, lambda: p.set_spectral_filter(1, 0.0), "score")
        out["under normalisation"] = (ok and p.get_option("normalise") == 1, p.get_option("spectral_filter"), _bits_differ(p.convolve(ks), normed))
    # feature_dim > 1
    img2 = np.asfortranarray(np.random.default_rng(3).random((H, W, 2), dtype=np.float32))
    ks2 = [np.asfortranarray(np.random.default_rng(4 + j).random((kh, kw, 2), dtype=np.float32)) for j in range(2)]
    with fc.Plan(H, W, 2, kh, kw) as p:
        p.set_image(img2)
        base = p.convolve(ks2)
        for mode in (1, 2):
            ok = _refused(fc, lambda m=mode: p.set_spectral_filter(m, 0.0), "feature")
            out["F = 2, mode %d" % mode] = (ok, p.get_option("spectral_filter"), _bits_differ(p.convolve(ks2), base))
    # a block-wise plan
    imgb, ksb = _inputs((600, 600, 9, 9), [(9, 9)] * 2, 29)
    with fc.Plan(600, 600, 1, 9, 9, options={"max_transform": 512}) as p:
        assert p.get_option("blockwise") > 0
        p.set_image(imgb)
        base = p.convolve(ksb)
        ok = _refused(fc, lambda: p.set_spectral_filter(2, 1.0), "block-wise")
        out["block-wise"] = (ok, p.get_option("spectral_filter"), _bits_differ(p.convolve(ksb), base))
    # a specialised row length whose filter kernel is not built (fast_paths.hpp: FC_ROWS_FILTER_NOT_BUILT)
    imgl, ksl = _inputs((16, 7000, 3, 3), [(3, 3)] * 2, 37)
    with fc.Plan(16, 7000, 1, 3, 3) as p:
        assert p.info.transform_w == 7040 and p.get_option("specialised_kernels") & 1
        p.set_image(imgl)
        base = p.convolve(ksl)
        ok = _refused(fc, lambda: p.set_spectral_filter(1, 0.0), "kernel_path", "7040")
        out["not built: 7040"] = (ok, p.get_option("spectral_filter"), _bits_differ(p.convolve(ksl), base))
    with fc.Plan(16, 7000, 1, 3, 3, options={"kernel_path": 1}) as p:       # ... and the way out the message names
        p.set_image(imgl)
        p.set_spectral_filter(1, 0.0)
        got = p.convolve(ksl)
        L, fft = (p.info.transform_h, p.info.transform_w), (p.info.fft_h, p.info.fft_w)
        out["7040 on kernel_path 1"] = max(util.rel_err(g, w) for g, w in zip(got, _oracle(imgl[:, :, 0], ksl, L, fft, 1, 0.0)))
    return out


# ---- the tests

@pytest.mark.parametrize("name", list(PARITY))
def test_parity_with_the_float64_definition(device, name):
    res = device("_case_parity", name)
    for mode, (err, differ, nans) in res.items():
        print("spectral filter parity %s mode %d: rel_err %.3g, walks of 3 and 1 differ in %d elements" % (name, mode, err, differ))
        assert nans == 0 and err < BAR, (name, mode, err)
        assert differ == 0, (name, mode, differ)


@pytest.mark.parametrize("exact", [0, 1], ids=["transform longer than the window", "exact_window"])
def test_phase_peak_of_a_cut_template(device, exact):
    peak, want, height, second = device("_case_phase_peak", exact)
    print("phase peak %s: at %s (want %s), height %.4f, runner-up %.4f" % ("exact_window" if exact else "default plan", peak, want, height, second))
    assert peak == want and height > second


def test_wiener_peak_of_the_kernel_itself(device):
    peak, want, height = device("_case_wiener_peak")
    print("wiener peak at %s (want %s), height %.4f" % (peak, want, height))
    assert peak == want and 0.0 < height <= 1.0


@pytest.mark.parametrize("name", ["fp16", "rectangle and stride", "image batch", "uint8 image", "border replicate"])
def test_composition(device, name):
    out = device("_case_composition", name)
    assert sorted(out) == [1, 2]
    for mode, r in out.items():
        print("spectral filter composition %s mode %d: %s" % (name, mode, r))
        if name in ("fp16", "uint8 image"):
            assert r == 0
        elif name == "rectangle and stride":
            assert r == (0, 0, 0, mode)
        elif name == "image batch":
            assert r == (9, 0, 0, 1)          # nine maps, bit-equal to three one-image plans, no image walk under a mode, back without one
        else:
            assert r[0] == (270, 270) and r[1] < BAR


def test_state_survives_the_setter(device):
    errs, first_differs, last_differs, kernel_cols, image_cols, rows, images = device("_case_state")
    print("spectral filter state: rel_err %s, mode-0 maps differ from a fresh plan's in %d / %d elements, kernel column launches %d" %
          (errs, first_differs, last_differs, kernel_cols))
    assert all(e < BAR for e in errs) and len(errs) == 2
    assert first_differs == 0 and last_differs == 0
    assert kernel_cols == 4 and image_cols == 0 and rows >= 4 and images == 1      # one column pass per prepare, none per convolve, no new image


def test_graph_replay_under_wiener(device):
    differ, err, mode = device("_case_graph")
    print("spectral filter graph replay: %d elements differ from the eager call, rel_err %.3g" % (differ, err))
    assert differ == 0 and err < BAR and mode == 2


def test_refusals_leave_the_plan_untouched(device):
    out = device("_case_refusals")
    for what, r in out.items():
        print("spectral filter refusal %s: %s" % (what, r))
    assert out.pop("7040 on kernel_path 1") < BAR
    assert len(out) == 16
    # (the first plan runs mode 2 throughout its argument cases; every other plan never had a mode)
    mode_2 = ("mode 3", "mode -1", "nan", "inf", "negative", "param in mode 1", "set_match_score", "set_normalisation", "no-op")
    for what, (refused, mode, differ) in out.items():
        assert refused and mode == (2 if what in mode_2 else 0) and differ == 0, (what, refused, mode, differ)
