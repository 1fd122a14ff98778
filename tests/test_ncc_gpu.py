"""Normalised cross-correlation maps (fftconv_plan_set_normalisation) on the GPU.

The yardstick is a NumPy float64 restatement of the definition in include/fftconv.h, written here (ncc_reference): window sums
as direct sums over the box, the floor, centred unit-norm kernels, the map D * (I (*) T'').  Per element

    |got - ref| <= 1e-5 * max_u |raw_k(u)| * D_ref(u) + 4 * 2^-24

raw_k the float64 I (*) T''_k: 1e-5 of a map's maximum is the project's bar for fp32 maps (util.rel_err, tools/fuzz_gpu.py)
carried through the multiply by D; the last term is the fp32 rounding of D and of the product with |ncc| <= 1.  16-bit maps
get half an ulp of their format on top.  Where D_ref is 0 the result must be exactly 0.  Elements whose float64 den2 lies within
a factor 16 of the floor could be left out, and every case asserts that there are none: the inputs are Gaussian noise plus a flat
patch larger than the box.

The scale is one fp32 multiply of the output kernel's fp32 value by D, in the output kernel's store (fast_cols.hpp: NORM) or while
the staged fp32 window is cropped (kernels_ncc.hip): the two routes must agree BIT FOR BIT on every configuration of the
specialised output kernel, and a 16-bit map, a region, a rectangle, a host map and a prepared kernel set must return the rounded
/ cropped fp32 ncc window bit for bit.  The cases run in a spawned child
(test_accuracy_gpu._Child), which exits with the module."""
import numpy as np
import pytest

import util
from test_accuracy_gpu import _Child
from test_features_gpu import _logged
from test_map_format_gpu import _image_t, _pack_t, from_bits, to_bits
from test_output_rect_gpu import _crop, _differ, _guarded, _unguard, col_configs

pytestmark = pytest.mark.gpu

FLOOR = 2.0 ** -30
ROUND = 4 * 2.0 ** -24

# name: (H, W, F, kh, kw), creation options, host arrays (the pinned in-place route) instead of device pointers
KINDS = {
    "specialised, F = 1": ((250, 250, 1, 31, 31), {}, False),
    "specialised, F = 2": ((250, 250, 2, 31, 31), {}, False),
    "generic": ((100, 100, 1, 9, 9), {}, False),
    "Bluestein": ((290, 290, 1, 15, 15), {"exact_window": 1}, False),
    "pinned in-place rows": ((48, 1152, 1, 7, 9), {}, True),
}


@pytest.fixture(scope="module")
def device():
    child = _Child(globals())
    yield child
    if child.gone:
        child.kill()
    else:
        child.ex.shutdown(wait=True)


# ---- the definition, in float64

def window_sums(img, kh, kw, fft_h, fft_w):
    """s1, s2 [F][fft_h][fft_w]: direct sums of the zero-padded image and of its square over the box that ends at each element"""
    H, W, F = img.shape
    z = np.zeros((F, kh - 1 + fft_h, kw - 1 + fft_w))
    z[:, kh - 1:kh - 1 + H, kw - 1:kw - 1 + W] = np.transpose(img.astype(np.float64), (2, 0, 1))
    z2 = z * z
    s1, s2 = np.zeros((F, fft_h, fft_w)), np.zeros((F, fft_h, fft_w))
    for a in range(kh):
        for b in range(kw):
            s1 += z[:, kh - 1 - a:kh - 1 - a + fft_h, kw - 1 - b:kw - 1 - b + fft_w]
            s2 += z2[:, kh - 1 - a:kh - 1 - a + fft_h, kw - 1 - b:kw - 1 - b + fft_w]
    return s1, s2


def scale_plane(img, kh, kw, fft_h, fft_w):
    """(D [fft_h][fft_w], number of elements within a factor 16 of the floor)"""
    s1, s2 = window_sums(img, kh, kw, fft_h, fft_w)
    den2 = (s2 - s1 * s1 / (kh * kw)).sum(axis=0)
    e = s2.sum(axis=0)
    floored = den2 <= FLOOR * e
    near = (e > 0) & (den2 > FLOOR * e / 16) & (den2 < FLOOR * e * 16)
    with np.errstate(divide="ignore", invalid="ignore"):
        D = np.where(floored, 0.0, 1.0 / np.sqrt(np.where(floored, 1.0, den2)))
    return D.astype(np.float32).astype(np.float64), int(near.sum())


def unit_kernel(k):
    """T'': centred per plane, unit joint norm; zeros for a constant kernel"""
    t = k.astype(np.float64)
    t = t - t.mean(axis=(0, 1), keepdims=True)
    norm = np.sqrt((t * t).sum())
    return t / norm if norm > 0 else np.zeros_like(t)


def raw_map(img, t, fft_h, fft_w, flip):
    """float64 I (*) T'' on the window (flip: correlation), summed over the planes; the window holds the whole linear result"""
    H, W, F = img.shape
    if flip:
        t = t[::-1, ::-1, :]
    out = np.zeros((fft_h, fft_w))
    for f in range(F):
        out += np.fft.irfft2(np.fft.rfft2(img[:, :, f].astype(np.float64), (fft_h, fft_w)) * np.fft.rfft2(t[:, :, f], (fft_h, fft_w)), (fft_h, fft_w))
    return out


def ncc_reference(img, ks, fft_h, fft_w, flip):
    """(ref [n][fft_w][fft_h] as the maps lie in memory, bound of the same shape, D [fft_w][fft_h], near-floor count)"""
    kh, kw = ks[0].shape[:2]
    D, near = scale_plane(img, kh, kw, fft_h, fft_w)
    refs, bounds = [], []
    for k in ks:
        raw = raw_map(img, unit_kernel(k), fft_h, fft_w, flip)
        refs.append((raw * D).T)
        bounds.append((1e-5 * np.abs(raw).max() * D + ROUND).T)
    return np.stack(refs), np.stack(bounds), D.T, near


def inputs(shape, n, seed, constant=None):
    """Gaussian noise with a flat patch larger than the box; n noise kernels (number `constant` is a constant one)"""
    H, W, F, kh, kw = shape
    rng = np.random.default_rng(seed)
    img = rng.standard_normal((H, W, F)).astype(np.float32)
    img[H // 4:H // 4 + kh + 6, W // 3:W // 3 + kw + 7, :] = np.float32(0.75)
    ks = [np.asfortranarray((1.0 + 3.0 * j) * rng.standard_normal((kh, kw, F)).astype(np.float32) + np.float32(5.0 * j)) for j in range(n)]
    if constant is not None:
        ks[constant] = np.asfortranarray(np.full((kh, kw, F), 2.5, dtype=np.float32))
    return np.asfortranarray(img), ks


def worst_excess(got, ref, bound):
    """max of |got - ref| / bound (<= 1 passes), and the number of elements that must be exactly 0 and are not"""
    got = np.asarray(got, dtype=np.float64).reshape(ref.shape)
    D0 = bound <= ROUND          # D_ref = 0 there: bound is the rounding term alone
    return float((np.abs(got - ref) / bound).max()), int((got[D0] != 0).sum())


# ---- the child's side

def _ctx():
    import torch
    return torch, util.load_package(), torch.device("cuda", 0)


def _ncc_window(torch, dev, p, n_maps, ker_d, n, kh, kw):
    """the plan's packed fp32 maps of its current region [n_maps][out_w][out_h] (image set, normalisation on)"""
    i = p.refresh_info()
    ne = n_maps * i.out_h * i.out_w
    t, ptr = _guarded(torch, dev, ne, 0)
    p.convolve_packed_device(n, ker_d.data_ptr(), kh, kw, ptr)
    p.synchronize()
    return _unguard(t, ne, 0).reshape(n_maps, i.out_w, i.out_h).copy()


def _case_parity(name, flip):
    torch, fc, dev = _ctx()
    shape, options, host = KINDS[name]
    H, W, F, kh, kw = shape
    n = 3
    img, ks = inputs(shape, n, 11 + len(name) + flip, constant=1)
    with fc.Plan(H, W, F, kh, kw, options=options) as p:
        i = p.info
        p.set_option("flip_kernels", flip)
        p.set_normalisation(1, kh, kw)
        state = (p.get_option("normalise"), p.get_option("norm_box_h"), p.get_option("norm_box_w"), p.get_option("images"))
        ref, bound, D, near = ncc_reference(img, ks, i.fft_h, i.fft_w, flip)
        if host:
            p.set_image(img)
            got = np.stack([np.ascontiguousarray(o.T) for o in p.convolve(ks)])
        else:
            img_d, ker_d = _image_t(torch, img).to(dev), _pack_t(torch, ks).to(dev)
            p.set_image_device(img_d.data_ptr())
            got = _ncc_window(torch, dev, p, n, ker_d, n, kh, kw)
        kinds = (p.get_option("specialised_kernels"), p.info.transform_h, p.info.fft_h)
    excess, nonzero = worst_excess(got, ref, bound)
    return {"state": state, "near": near, "excess": excess, "nonzero": nonzero, "kinds": kinds, "floored": int((D == 0).sum()),
            "constant": float(np.abs(got[1]).max()), "peak": float(np.abs(got).max()), "nan": int(np.isnan(got).sum())}


def _case_properties():
    """correlation with a template cut from the image scores 1 at its position and nowhere more; gain and offset of image and
    kernel do not move the maps"""
    torch, fc, dev = _ctx()
    shape = H, W, F, kh, kw = (250, 250, 2, 31, 31)
    img, ks = inputs(shape, 2, 5)
    y0, x0 = 140, 37
    ks[0] = np.asfortranarray(img[y0:y0 + kh, x0:x0 + kw, :].copy())
    with fc.Plan(H, W, F, kh, kw) as p:
        i = p.info
        p.set_option("flip_kernels", 1)
        p.set_normalisation(1, kh, kw)
        ref, bound, D, near = ncc_reference(img, ks, i.fft_h, i.fft_w, 1)
        ker_d = _pack_t(torch, ks).to(dev)
        img_d = _image_t(torch, img).to(dev)
        p.set_image_device(img_d.data_ptr())
        got = _ncc_window(torch, dev, p, 2, ker_d, 2, kh, kw).astype(np.float64)
        img2 = np.asfortranarray((np.float32(3.7) * img + np.float32(11.0)).astype(np.float32))
        ks2 = [np.asfortranarray((np.float32(0.5) * k - np.float32(2.0)).astype(np.float32)) for k in ks]
        ker2_d, img2_d = _pack_t(torch, ks2).to(dev), _image_t(torch, img2).to(dev)
        p.set_image_device(img2_d.data_ptr())
        got2 = _ncc_window(torch, dev, p, 2, ker2_d, 2, kh, kw).astype(np.float64)
    at = (x0 + kw - 1, y0 + kh - 1)              # [w][h] of the map
    return {"near": near, "peak_err": abs(got[0][at] - 1.0) / bound[0][at], "argmax": tuple(int(v) for v in np.unravel_index(np.argmax(got[0]), got[0].shape)),
            "at": at, "over": float(((got - 1.0) / bound).max()), "under": float(((-1.0 - got) / bound).max()),
            "excess": worst_excess(got, ref, bound),
            # (the padding is zero for both images -- it does not take the offset -- so the property holds where the box lies
            #  wholly inside the data: the "valid" part of the window)
            "invariance": float((np.abs(got2 - got) / (2 * bound))[:, kw - 1:W, kh - 1:H].max()),
            "invariance_border": float((np.abs(got2 - got) / (2 * bound)).max()),
            "raw_would_fail": float(np.abs(img).max())}


def _case_composition():
    """16-bit maps, a region, a rectangle, host maps and prepared kernels against the plan's own fp32 ncc window"""
    torch, fc, dev = _ctx()
    shape = H, W, F, kh, kw = (250, 250, 1, 31, 31)
    n = 3
    img, ks = inputs(shape, n, 23)
    img_d, ker_d = _image_t(torch, img).to(dev), _pack_t(torch, ks).to(dev)
    out = {}
    with fc.Plan(H, W, F, kh, kw) as p:
        p.set_normalisation(1, kh, kw)
        p.set_image_device(img_d.data_ptr())
        win = _ncc_window(torch, dev, p, n, ker_d, n, kh, kw)
        ref, bound, D, near = ncc_reference(img, ks, p.info.fft_h, p.info.fft_w, 0)
        out["near"], out["window"] = near, worst_excess(win, ref, bound)
        for fmt in (1, 2):
            p.set_option("map_format", fmt)
            i = p.refresh_info()
            ne = n * i.out_h * i.out_w
            t, ptr = _guarded(torch, dev, ne, fmt)
            p.convolve_packed_device(n, ker_d.data_ptr(), kh, kw, ptr)
            p.synchronize()
            bits = _unguard(t, ne, fmt)
            out["fmt%d" % fmt] = _differ(bits, win, fmt)
            # ... and against the definition: half an ulp of the format on top of the fp32 bound
            vals = from_bits(bits, fmt).reshape(ref.shape)
            binade = 2.0 ** (np.frexp(np.maximum(np.abs(ref), 2.0 ** -14 if fmt == 1 else 2.0 ** -126))[1] - 1)      # 2^floor(log2 |ref|)
            half_ulp = binade * (2.0 ** -11 if fmt == 1 else 2.0 ** -8)
            out["fmt%d_def" % fmt] = float((np.abs(vals - ref) / (bound + half_ulp)).max())
        p.set_option("map_format", 0)
        p.set_option("output_region", 2)
        i = p.refresh_info()
        same = (i.out_h, i.out_w)
        got = _ncc_window(torch, dev, p, n, ker_d, n, kh, kw)
        out["region2"] = (same, _differ(got, _crop(win, ((kh - 1) // 2, (kw - 1) // 2, H, W)), 0))
        rect = (3, 5, 271, 271)
        p.set_output_rect(*rect)
        direct, fused = p.get_option("rect_direct"), p.get_option("norm_direct")
        p.set_option("verbose", 1)
        got, log = _logged(lambda: _ncc_window(torch, dev, p, n, ker_d, n, kh, kw))
        p.set_option("verbose", 0)
        out["rect"] = (direct, _differ(got, _crop(win, rect), 0), ("normalisation: fused" if fused else "normalisation: staged") in log)
        for fmt in (0, 1):       # host maps through convolve, the rectangle still set
            p.set_option("map_format", fmt)
            outs = p.convolve(ks)
            got = np.stack([np.ascontiguousarray(o.T) for o in outs])
            out["host%d" % fmt] = _differ(got if fmt == 0 else got.view(np.uint16), _crop(win, rect), fmt)
        p.set_option("map_format", 0)
        p.set_option("output_region", 0)
        for defer in (0, 1):
            p.set_option("defer_prepare", defer)
            p.prepare_kernels_packed_device(n, ker_d.data_ptr(), kh, kw)
            pending = p.get_option("prepare_pending")
            if defer:
                p.set_image_device(img_d.data_ptr())       # the deferred column pass rides in the image's
            got = _ncc_window(torch, dev, p, n, ker_d, n, kh, kw)
            out["prepare%d" % defer] = (pending, _differ(got, win, 0))
        p.set_option("defer_prepare", 0)
    return out


def _case_fused(M):
    """an exact_window plan whose transform along h is 2M points on a 288-column window (the shapes of
    test_output_rect_gpu.test_every_configuration_is_bit_equal), two maps: "norm_store" 1 against 0, static deal and dynamic
    queue, the whole window and the odd rectangle"""
    torch, fc, dev = _ctx()
    kh, kw, n = 13, 11, 2
    shape = (2 * M - 18, 272, 1, kh, kw)
    img, ks = inputs(shape, n, 7 + M)
    img_d, ker_d = _image_t(torch, img).to(dev), _pack_t(torch, ks).to(dev)
    out = {}
    with fc.Plan(shape[0], shape[1], 1, kh, kw, options={"exact_window": 1, "blockwise": 1}) as p:
        assert p.get_option("blockwise") == 0 and (p.info.fft_h, p.info.fft_w, p.info.transform_h) == (2 * M, 288, 2 * M)
        assert p.get_option("specialised_kernels") == 3
        p.set_normalisation(1, kh, kw)
        p.set_image_device(img_d.data_ptr())
        for dyn in (0, 1):
            p.set_option("dynamic_tiles", dyn)
            for rect in (None, (3, 5, 2 * M - 17, 271)):
                if rect:
                    p.set_output_rect(*rect)
                else:
                    p.set_option("output_region", 0)
                maps, direct, lines = {}, {}, {}
                for store in (1, 0):
                    p.set_option("norm_store", store)
                    direct[store] = p.get_option("norm_direct")
                    p.set_option("verbose", 1)
                    maps[store], log = _logged(lambda: _ncc_window(torch, dev, p, n, ker_d, n, kh, kw))
                    p.set_option("verbose", 0)
                    lines[store] = ("normalisation: fused" in log, "normalisation: staged" in log)
                out[(dyn, rect is not None)] = (direct[1], direct[0], _differ(maps[1], maps[0], 0), lines[1], lines[0],
                                                int(np.isnan(maps[0]).sum()), float(np.abs(maps[0]).max()))
    return out


def _case_batch(walk):
    """B = 3 images with different statistics (gain, offset, another patch), image-major maps"""
    torch, fc, dev = _ctx()
    shape = H, W, F, kh, kw = (250, 250, 1, 31, 31)
    n, B = 2, 3
    imgs, ks = [], None
    for b in range(B):
        img, k = inputs(shape, n, 31 + b)
        imgs.append(np.asfortranarray((np.float32(1.0 + 2.5 * b) * img + np.float32(7.0 * b)).astype(np.float32)))
        ks = ks or k
    ker_d = _pack_t(torch, ks).to(dev)
    with fc.Plan(H, W, F, kh, kw) as p:
        i = p.info
        p.set_option("image_walk", walk)
        p.set_normalisation(1, kh, kw)
        p.set_images(np.asfortranarray(np.stack([im[:, :, 0] for im in imgs], axis=2)))
        active = p.get_option("image_walk_active")
        p.set_option("norm_store", 0)
        not_fused = p.get_option("norm_direct")
        staged = _ncc_window(torch, dev, p, B * n, ker_d, n, kh, kw)
        p.set_option("norm_store", 1)          # the fused kernel finds each map's image itself
        fused = p.get_option("norm_direct")
        got = _ncc_window(torch, dev, p, B * n, ker_d, n, kh, kw)
        p.set_option("batch_maps", 3)          # launches that cut the image-major grid inside an image
        got3 = _ncc_window(torch, dev, p, B * n, ker_d, n, kh, kw)
        p.set_option("norm_store", 0)
        staged3 = _ncc_window(torch, dev, p, B * n, ker_d, n, kh, kw)
    res = []
    for b in range(B):
        ref, bound, D, near = ncc_reference(imgs[b], ks, i.fft_h, i.fft_w, 0)
        res.append((near, worst_excess(got[b * n:(b + 1) * n], ref, bound), worst_excess(got3[b * n:(b + 1) * n], ref, bound)))
    return {"active": active, "images": res, "fused": (fused, not_fused), "fused_vs_staged": (_differ(got, staged, 0), _differ(got3, staged3, 0))}


def _case_surface():
    torch, fc, dev = _ctx()
    shape = H, W, F, kh, kw = (250, 250, 1, 31, 31)
    n = 2
    img, ks = inputs(shape, n, 43)
    img_d, ker_d = _image_t(torch, img).to(dev), _pack_t(torch, ks).to(dev)
    small_d = torch.zeros((n, 1, 9, 9), dtype=torch.float32, device=dev)
    out = {}

    def refused(fn, word=""):
        try:
            fn()
            return None
        except fc.FFTConvError as e:
            return (e.status, word in str(e))

    def state(p):
        return (p.get_option("normalise"), p.get_option("norm_box_h"), p.get_option("norm_box_w"), p.get_option("images"))

    with fc.Plan(H, W, F, kh, kw) as p:
        p.set_image_device(img_d.data_ptr())
        fresh = _ncc_window(torch, dev, p, n, ker_d, n, kh, kw)          # (normalisation off: the raw maps of a fresh plan)
        out["fresh_state"] = state(p)
        out["bad"] = [refused(lambda a=a: p.set_normalisation(*a)) for a in ((2, 31, 31), (-1, 31, 31), (1, 0, 31), (1, 31, 0), (1, 32, 31), (1, 31, 32))]
        out["after_bad"] = state(p)
        p.set_normalisation(0)                                           # changes nothing: the image stays
        out["noop0"] = state(p)
        p.set_normalisation(1, kh, kw)
        out["on"] = state(p)                                             # the image is gone
        out["no_image"] = refused(lambda: _ncc_window(torch, dev, p, n, ker_d, n, kh, kw))
        p.set_image_device(img_d.data_ptr())
        p.set_normalisation(1, kh, kw)                                   # changes nothing
        out["noop1"] = state(p)
        good = _ncc_window(torch, dev, p, n, ker_d, n, kh, kw)
        i = p.info
        t, ptr = _guarded(torch, dev, n * i.fft_h * i.fft_w, 0)
        out["other_size_packed"] = refused(lambda: p.convolve_packed_device(n, small_d.data_ptr(), 9, 9, ptr), "box")
        out["other_size_prepare"] = refused(lambda: p.prepare_kernels_packed_device(n, small_d.data_ptr(), 9, 9), "box")
        out["ragged"] = refused(lambda: p.convolve([ks[0], np.zeros((9, 9, 1), dtype=np.float32)]), "box")
        out["mark"] = refused(lambda: p.mark_spectrum_valid(), "statistics")
        out["after_refusals"] = state(p)
        again = _ncc_window(torch, dev, p, n, ker_d, n, kh, kw)
        out["still_convolves"] = _differ(again, good, 0)
        ref, bound, D, near = ncc_reference(img, ks, i.fft_h, i.fft_w, 0)
        out["near"], out["good"] = near, worst_excess(good, ref, bound)
        p.set_normalisation(1, kh, kw - 1)                               # another box: the image is dropped
        out["new_box"] = state(p)
        p.set_normalisation(0)
        out["off"] = state(p)
        p.set_image_device(img_d.data_ptr())
        out["off_is_fresh"] = _differ(_ncc_window(torch, dev, p, n, ker_d, n, kh, kw), fresh, 0)
    with fc.Plan(290, 290, 1, 15, 15, options={"exact_window": 1}) as p:   # exact window: a kernel above MAX_KERNEL is refused too
        p.set_normalisation(1, 15, 15)
        p.set_image(np.zeros((290, 290, 1), dtype=np.float32, order="F"))
        out["above_max"] = refused(lambda: p.convolve([np.ones((17, 15, 1), dtype=np.float32)]), "box")
        out["import"] = refused(lambda: p.import_spectrum(np.zeros((1, p.info.fft_w, p.info.fft_h // 2 + 1), dtype=np.complex64)), "statistics")
        out["exact_state"] = state(p)
    with fc.Plan(600, 600, 1, 9, 9, options={"max_transform": 512}) as p:
        out["blockwise"] = (p.get_option("blockwise") > 0, refused(lambda: p.set_normalisation(1, 9, 9), "block-wise"), p.get_option("normalise"))
    return out


def _case_graph():
    """a captured warm set_image(DEVICE) + convolve_packed with normalisation on, replayed with new inputs: bit-equal to the
    eager step on the same inputs (the conditions of tests/test_graph_gpu.py: one eager warm-up, nothing allocates afterwards)"""
    torch, fc, dev = _ctx()
    shape = H, W, F, kh, kw = (840, 270, 1, 13, 11)           # M = 432: the tile queue, whose counters every launch must leave at zero
    n = 3
    sets = [inputs(shape, n, 90 + k) for k in range(3)]
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream), fc.Plan(H, W, F, kh, kw, stream=stream.cuda_stream) as p:
        p.set_normalisation(1, kh, kw)
        i = p.info
        ne = n * i.fft_h * i.fft_w
        imgs_h = [_image_t(torch, s[0]).pin_memory() for s in sets]
        kers_h = [_pack_t(torch, s[1]).pin_memory() for s in sets]
        img_d = torch.empty(imgs_h[0].shape, dtype=torch.float32, device=dev)
        ker_d = torch.empty(kers_h[0].shape, dtype=torch.float32, device=dev)
        out, out_ptr = _guarded(torch, dev, ne, 0)
        replayed = [torch.empty_like(out) for _ in range(2)]
        eager = [torch.empty_like(out) for _ in range(2)]

        def step():
            p.set_image_device(img_d.data_ptr())
            p.convolve_packed_device(n, ker_d.data_ptr(), kh, kw, out_ptr)

        img_d.copy_(imgs_h[0], non_blocking=True)
        ker_d.copy_(kers_h[0], non_blocking=True)
        step()                                   # eager warm-up: sizes the scratch; nothing allocates from here on
        torch.cuda.synchronize()
        ws = p.refresh_info().workspace_bytes
        graph = torch.cuda.CUDAGraph()
        cap = torch.cuda.Stream(dev)
        with torch.cuda.graph(graph, stream=cap):
            p.set_stream(torch.cuda.current_stream(dev).cuda_stream)
            step()
        p.set_stream(stream.cuda_stream)
        for r in range(2):                       # nothing synchronised inside the loop
            out.fill_(float("nan"))
            img_d.copy_(imgs_h[r + 1], non_blocking=True)
            ker_d.copy_(kers_h[r + 1], non_blocking=True)
            graph.replay()
            replayed[r].copy_(out)
        torch.cuda.synchronize()
        for r in range(2):
            out.fill_(float("nan"))
            img_d.copy_(imgs_h[r + 1], non_blocking=True)
            ker_d.copy_(kers_h[r + 1], non_blocking=True)
            step()
            eager[r].copy_(out)
        torch.cuda.synchronize()
        got = [_unguard(t, ne, 0) for t in replayed]
        want = [_unguard(t, ne, 0) for t in eager]
        del graph
        same_ws = p.refresh_info().workspace_bytes == ws
    defs = []
    for r in range(2):
        ref, bound, D, near = ncc_reference(sets[r + 1][0], sets[r + 1][1], i.fft_h, i.fft_w, 0)
        defs.append((near, worst_excess(want[r], ref, bound)))
    return ([_differ(a, b, 0) for a, b in zip(got, want)], defs, bool(np.array_equal(got[0], got[1])), same_ws)


# ---- the tests

@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("name", list(KINDS))
def test_parity_with_the_definition(device, name, flip):
    """three kernels (the second one constant) on every kind of plan, convolution and correlation"""
    res = device("_case_parity", name, flip)
    print(name, "flip_kernels", flip, res)
    shape = KINDS[name][0]
    assert res["state"] == (1, shape[3], shape[4], 0)
    assert res["near"] == 0, "the inputs must keep every window 16 floors from flat"
    assert res["nan"] == 0 and res["floored"] > 0
    assert res["excess"] <= 1.0 and res["nonzero"] == 0, res
    assert res["constant"] == 0.0                         # a constant kernel gives a zero map
    assert 0.05 < res["peak"] <= 1.0 + 1e-4
    spec, lh, fft_h = res["kinds"]
    if name.startswith("specialised"):
        assert spec == 3 and fft_h == 288
    if name == "generic":
        assert spec != 3
    if name == "Bluestein":
        assert spec == 0 and (lh, fft_h) == (304, 304)


def test_properties_a_raw_map_fails(device):
    res = device("_case_properties")
    print(res)
    assert res["near"] == 0
    assert res["excess"][0] <= 1.0 and res["excess"][1] == 0
    assert res["argmax"] == res["at"] and res["peak_err"] <= 1.0      # the template scores 1 where it was cut
    assert res["over"] <= 1.0 and res["under"] <= 1.0                   # nothing leaves [-1, 1] by more than the bound
    assert res["invariance"] <= 1.0                                     # 3.7 I + 11 against 0.5 T - 2: within twice the bound
    # (where the box reaches the zero padding the offset of the image shows: reported as "invariance_border" above, not asserted)


def test_composition(device):
    res = device("_case_composition")
    print(res)
    assert res["near"] == 0 and res["window"][0] <= 1.0 and res["window"][1] == 0
    assert res["fmt1"] == 0 and res["fmt2"] == 0                        # the rounded fp32 ncc, bit for bit
    assert res["fmt1_def"] <= 1.0 and res["fmt2_def"] <= 1.0
    assert res["region2"] == ((250, 250), 0)
    assert res["rect"] == (0, 0, True)
    assert res["host0"] == 0 and res["host1"] == 0
    assert res["prepare0"] == (0, 0) and res["prepare1"] == (1, 0)


def norm_not_built():
    """fast_paths.hpp: FC_COLS_NORM_NOT_BUILT -- the configurations whose fused kernel is not built (staged route)"""
    import os
    import re
    src = open(os.path.join(util.ROOT, "cuda-fft-convolution_amd", "csrc", "fast_paths.hpp")).read()
    return tuple(int(x) for x in re.search(r"FC_COLS_NORM_NOT_BUILT\[\] = \{([^}]*)\}", src).group(1).split(","))


@pytest.mark.parametrize("M", [m for m, _ in col_configs()])
def test_fused_equals_staged_bit_for_bit(device, M):
    """the fused kernels and the staged pair (plain output kernel, then the crop that scales) do the same fp32 multiply on the same
    fp32 value: every built configuration is held to bit-equality, both tile deals, the whole window and an odd rectangle -- a
    compiler that contracts differently fails here.  "norm_direct" reads 1 with "norm_store" 1 except for the configurations
    listed as not built, which read 0 and run the staged route twice."""
    res = device("_case_fused", M)
    print(M, res)
    built = M not in norm_not_built()
    assert set(res) == {(dyn, rect) for dyn in (0, 1) for rect in (False, True)}
    for key, (direct1, direct0, differ, lines1, lines0, nans, peak) in res.items():
        assert (direct1, direct0) == (1 if built else 0, 0), (M, key)
        assert differ == 0 and nans == 0 and 0.05 < peak <= 1.0 + 1e-4, (M, key, differ, nans, peak)
        assert lines1 == ((True, False) if built else (False, True)) and lines0 == (False, True), (M, key, lines1, lines0)


@pytest.mark.parametrize("walk", [0, 1])
def test_image_batch(device, walk):
    res = device("_case_batch", walk)
    print(res)
    assert res["active"] == walk
    assert res["fused"] == (1, 0) and res["fused_vs_staged"] == (0, 0)
    for near, whole, cut in res["images"]:
        assert near == 0
        assert whole[0] <= 1.0 and whole[1] == 0 and cut[0] <= 1.0 and cut[1] == 0, res


def test_surface(device):
    out = device("_case_surface")
    print(out)
    assert out["fresh_state"] == (0, 0, 0, 1)
    assert out["bad"] == [(-1, True)] * 6 and out["after_bad"] == (0, 0, 0, 1)
    assert out["noop0"] == (0, 0, 0, 1)
    assert out["on"] == (1, 31, 31, 0) and out["no_image"] == (-9, True)
    assert out["noop1"] == (1, 31, 31, 1)
    for key in ("other_size_packed", "other_size_prepare", "ragged", "mark", "above_max", "import"):
        assert out[key] == (-1, True), (key, out[key])
    assert out["after_refusals"] == (1, 31, 31, 1) and out["still_convolves"] == 0
    assert out["near"] == 0 and out["good"][0] <= 1.0 and out["good"][1] == 0
    assert out["new_box"] == (1, 31, 30, 0)
    assert out["off"] == (0, 0, 0, 0) and out["off_is_fresh"] == 0      # mode 0 afterwards: the bits of a fresh plan
    assert out["exact_state"] == (1, 15, 15, 1)
    assert out["blockwise"] == (True, (-1, True), 0)


def test_graph_replay(device):
    replay_vs_eager, defs, same_twice, same_ws = device("_case_graph")
    print(replay_vs_eager, defs, same_twice, same_ws)
    assert replay_vs_eager == [0, 0]
    for near, (excess, nonzero) in defs:
        assert near == 0 and excess <= 1.0 and nonzero == 0
    assert not same_twice and same_ws
