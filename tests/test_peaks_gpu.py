"""Peak lists (fftconv_plan_set_peaks) on the GPU: per delivered map the number of its thresholded local maxima and the first max_peaks
of them in memory order, with a sub-pixel offset per dimension, found by a scan of the maps where they lie on the device.

The yardstick in every case: convolve once under peaks, take the maps that SAME convolve returned, and run a NumPy restatement of the
rule over them (numpy_peaks: shifted compares over the (2 rh + 1)(2 rw + 1) offsets).  found, the stored prefix in memory order and
its values, rows and columns must be bit-equal.  d_row and d_col are expected bit-equal too; the bar is 2^-24 absolute, one fp32 ulp at
0.5, in case the device's float64 divide differs in the last place, and the number of offsets that differ at all is printed.
Thresholds come from the returned maps: a high quantile under which every map has between 1 and max_peaks peaks of the reference,
and the median, under which every map overflows max_peaks; both conditions are asserted on the reference.  Without the feature
every case fails at its first set_peaks.  The cases run in a spawned child (test_accuracy_gpu._Child)."""
import numpy as np
import pytest

import test_ncc_gpu as N
import util
from test_accuracy_gpu import _Child
from test_extrema_gpu import SHAPE, values_of
from test_map_format_gpu import _image_t, _pack_t
from test_match_score_gpu import zero_kernel_inputs
from test_output_rect_gpu import _differ, _guarded, _unguard

pytestmark = pytest.mark.gpu

CAP = 256          # max_peaks of the 288 x 288 cases: white noise of this size has 82 peaks of radius 3 at the 99.9 % quantile, 1 694 at -inf
OFFSET_BAR = 2.0 ** -24


@pytest.fixture(scope="module")
def device():
    child = _Child(globals())
    yield child
    if child.gone:
        child.kill()
    else:
        child.ex.shutdown(wait=True)


# ---- the yardstick

def _fit(a, v, b):
    """the three-point parabola in float64 from fp32 values, + - * / alone, rounded to fp32 once"""
    A, V, B = a.astype(np.float64), v.astype(np.float64), b.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        den = (A - V) + (B - V)
        ok = np.isfinite(a) & np.isfinite(v) & np.isfinite(b) & (den != 0)
        d = 0.5 * (A - B) / np.where(ok, den, 1.0)
    d = np.where(ok, np.clip(d, -0.5, 0.5), 0.0)
    return d.astype(np.float32)


def numpy_peaks(vals, mode, threshold, radius, dtype):
    """vals [out_w][out_h] fp32 values of ONE delivered map (memory order: column-major out_h x out_w) -> (found, every record in
    ascending index order)"""
    rh, rw = radius
    ow, oh = vals.shape
    U = -vals if mode == 2 else vals
    thr = np.float32(-threshold if mode == 2 else threshold)
    with np.errstate(invalid="ignore"):
        peak = U >= thr
        for dc in range(-min(rw, ow - 1), min(rw, ow - 1) + 1):
            for dr in range(-min(rh, oh - 1), min(rh, oh - 1) + 1):
                if dc == 0 and dr == 0:
                    continue
                c0, c1, r0, r1 = max(0, -dc), ow - max(0, dc), max(0, -dr), oh - max(0, dr)
                me, other = U[c0:c1, r0:r1], U[c0 + dc:c1 + dc, r0 + dr:r1 + dr]
                earlier = dc < 0 or (dc == 0 and dr < 0)            # the neighbour's index is the smaller one
                peak[c0:c1, r0:r1] &= ~((other > me) | ((other == me) & earlier))
    index = np.flatnonzero(peak.reshape(-1))
    flat = vals.reshape(-1)
    rec = np.zeros(len(index), dtype=dtype)
    rec["value"], rec["row"], rec["col"] = flat[index], index % oh, index // oh
    r, c = rec["row"], rec["col"]
    inner_r, inner_c = (r > 0) & (r < oh - 1) & (rh > 0), (c > 0) & (c < ow - 1) & (rw > 0)
    ir, ic = index[inner_r], index[inner_c]
    rec["d_row"][inner_r] = _fit(flat[ir - 1], flat[ir], flat[ir + 1])
    rec["d_col"][inner_c] = _fit(flat[ic - oh], flat[ic], flat[ic + oh])
    return len(index), rec


def lists_differ(found, lists, maps, fmt, mode, threshold, radius, cap):
    """every map's found and stored prefix against numpy_peaks on `maps` [n][out_w][out_h] as delivered"""
    vals = values_of(maps, fmt)
    out = {"maps": len(vals), "got_maps": len(found), "ref_found": [], "found_bad": 0, "recs": 0, "recs_bad": 0, "off_differ": 0, "off_worst": 0.0}
    for m in range(len(vals)):
        n, ref = numpy_peaks(vals[m], mode, threshold, radius, lists[m].dtype)
        want, got = ref[:cap], lists[m]
        out["ref_found"].append(n)
        out["found_bad"] += int(found[m]) != n
        if len(got) != len(want):
            out["recs_bad"] += max(len(got), len(want))
            continue
        out["recs"] += len(want)
        out["recs_bad"] += int(((got["value"].view(np.uint32) != want["value"].view(np.uint32)) | (got["row"] != want["row"]) | (got["col"] != want["col"])).sum())
        for f in ("d_row", "d_col"):
            out["off_differ"] += int((got[f].view(np.uint32) != want[f].view(np.uint32)).sum())
            if len(want):
                out["off_worst"] = max(out["off_worst"], float(np.abs(got[f].astype(np.float64) - want[f].astype(np.float64)).max()))
    return out


def lists_bytes(found, lists):
    return found.tobytes() + b"".join(l.tobytes() for l in lists)


def exact(r, n_maps, cap):
    """the assertions every comparison makes; prints the offsets that differ at all"""
    print("maps %d, reference found %s, records compared %d, offsets that differ at all %d (worst %.3g)" % (r["maps"], r["ref_found"], r["recs"], r["off_differ"], r["off_worst"]))
    assert r["maps"] == n_maps and r["got_maps"] == n_maps, r                      # every map took part
    assert r["found_bad"] == 0 and r["recs_bad"] == 0, r
    assert r["recs"] == sum(min(f, cap) for f in r["ref_found"]), r
    assert r["off_worst"] <= OFFSET_BAR, r


def few_and_many(res, n_maps, cap, overflow=True):
    exact(res["few"], n_maps, cap)
    exact(res["many"], n_maps, cap)
    assert all(1 <= f <= cap for f in res["few"]["ref_found"]), res["few"]["ref_found"]
    if overflow:
        assert all(f > cap for f in res["many"]["ref_found"]), res["many"]["ref_found"]
    assert res["same_ws"] == [True, True]      # a threshold-only change does not reallocate


# ---- the child's side

def inputs(shape, n, seed, unit=True):
    """Gaussian noise with a flat patch; n noise kernels of unit norm (unit False: of unit variance, the image's), so that the maps of
    one convolve have one scale and ONE threshold can leave every map between 1 and max_peaks peaks"""
    H, W, F, kh, kw = shape
    rng = np.random.default_rng(seed)
    img = rng.standard_normal((H, W, F)).astype(np.float32)
    img[H // 4:H // 4 + kh + 6, W // 3:W // 3 + kw + 7, :] = np.float32(0.75)
    ks = [rng.standard_normal((kh, kw, F)).astype(np.float32) for _ in range(n)]
    if unit:
        ks = [k / np.float32(np.sqrt(np.sum(k.astype(np.float64) ** 2))) for k in ks]
    ks = [np.asfortranarray(k) for k in ks]
    return np.asfortranarray(img), ks


def _packed(torch, dev, p, n_maps, ker_d, n, kh, kw, fmt=0):
    """one convolve into a guarded packed device buffer: (maps [n_maps][out_w][out_h] as delivered, found, lists of that convolve)"""
    i = p.refresh_info()
    ne = n_maps * i.out_h * i.out_w
    t, ptr = _guarded(torch, dev, ne, fmt)
    p.convolve_packed_device(n, ker_d.data_ptr(), kh, kw, ptr)
    found, lists = p.peaks()
    return _unguard(t, ne, fmt).reshape(n_maps, i.out_w, i.out_h).copy(), found, lists


def thresholds_of(maps, fmt, mode, q):
    """from returned maps: the high quantile every map reaches (mode 2: the low one) and the median of all"""
    flat = values_of(maps, fmt).reshape(len(maps), -1).astype(np.float64)
    if mode == 1:
        few = min(np.quantile(f, q) for f in flat)
    else:
        few = max(np.quantile(f, 1.0 - q) for f in flat)
    return float(np.float32(few)), float(np.float32(np.median(flat)))


def _few_and_many(p, run, mode, radius, cap, n_maps, fmt=0, q=0.999, many=None):
    """run() -> (maps, found, lists).  One convolve for the thresholds, then one per threshold, each compared on its own maps."""
    p.set_peaks(mode, n_maps, cap, 0.0, radius)
    few, median = thresholds_of(run()[0], fmt, mode, q)
    ws = p.refresh_info().workspace_bytes      # (behind a convolve: it sizes the plan's own scratch)
    out = {"same_ws": [], "thresholds": (few, median if many is None else many)}
    for name, thr in (("few", few), ("many", median if many is None else many)):
        p.set_peaks(mode, n_maps, cap, thr, radius)
        out["same_ws"].append(p.refresh_info().workspace_bytes == ws)
        maps, found, lists = run()
        out[name] = lists_differ(found, lists, maps, fmt, mode, thr, radius, cap)
    return out


def _case_format(fmt):
    """fp32 / fp16 / bf16 maps of the whole window, radius (3, 3), (0, 0) and (1, 5)"""
    torch, fc, dev = N._ctx()
    H, W, F, kh, kw = SHAPE
    n = 3
    img, ks = inputs(SHAPE, n, 23)
    img_d, ker_d = _image_t(torch, img).to(dev), _pack_t(torch, ks).to(dev)
    out = {}
    with fc.Plan(H, W, F, kh, kw) as p:
        p.set_option("map_format", fmt)
        p.set_image_device(img_d.data_ptr())
        for radius in ((3, 3), (0, 0), (1, 5)):
            out[radius] = _few_and_many(p, lambda: _packed(torch, dev, p, n, ker_d, n, kh, kw, fmt), 1, radius, CAP, n, fmt)
        out["size"] = (p.info.out_h, p.info.out_w)
        out["state"] = tuple(p.get_option(o) for o in ("peaks", "peaks_max_maps", "peaks_max", "peaks_radius_h", "peaks_radius_w", "peaks_maps"))
    return out


EXTENTS = {      # name: (what sets it, (out_h, out_w), max_peaks, the quantile of the high threshold, whether a map can overflow max_peaks)
    "region2": (("region", 2), (250, 250), CAP, 0.999, True),
    "odd rectangle": (("rect", (3, 5, 271, 271)), (271, 271), CAP, 0.999, True),
    "stride": (("stride", (2, 3)), (144, 96), 64, 0.995, True),
    "one column": (("rect", (0, 9, 288, 1)), (288, 1), 8, 0.99, True),      # 288 elements: about 40 peaks of radius 3 among them all
    "one element": (("rect", (100, 100, 1, 1)), (1, 1), 1, 0.5, False),      # one element: found is 1 at both thresholds, nothing can overflow
}


def _case_extent(name):
    torch, fc, dev = N._ctx()
    H, W, F, kh, kw = SHAPE
    n = 3
    img, ks = inputs(SHAPE, n, 27)
    img_d, ker_d = _image_t(torch, img).to(dev), _pack_t(torch, ks).to(dev)
    (kind, arg), size, cap, q, _ = EXTENTS[name]
    with fc.Plan(H, W, F, kh, kw) as p:
        p.set_image_device(img_d.data_ptr())
        if kind == "region":
            p.set_option("output_region", arg)
        elif kind == "rect":
            p.set_output_rect(*arg)
        else:
            p.set_output_stride(*arg)
        # (one column, one element: -inf, every element a candidate -- the median of 288 elements leaves too few to overflow 8)
        out = _few_and_many(p, lambda: _packed(torch, dev, p, n, ker_d, n, kh, kw), 1, (3, 3), cap, n, q=q, many=float("-inf") if size[1] == 1 else None)
        out["size"] = (p.info.out_h, p.info.out_w)
        out["unaligned"] = (size[0] * size[1] * 4) % 16 != 0
    return out


def _case_scores():
    """score 1 with two copies of a template planted in the image; score 4 with mode 2; phase correlation of a template cut from the image"""
    torch, fc, dev = N._ctx()
    H, W, F, kh, kw = SHAPE
    img, ks = inputs(SHAPE, 2, 5, unit=False)
    at = [(140, 37), (20, 190)]
    tpl = np.asfortranarray(img[at[0][0]:at[0][0] + kh, at[0][1]:at[0][1] + kw, :].copy())
    img[at[1][0]:at[1][0] + kh, at[1][1]:at[1][1] + kw, :] = tpl
    ks[0] = tpl
    img_d, ker_d = _image_t(torch, img).to(dev), _pack_t(torch, ks).to(dev)
    out = {"at": [(y + kh - 1, x + kw - 1) for y, x in at]}      # (row, col) of the window
    with fc.Plan(H, W, F, kh, kw) as p:
        p.set_option("flip_kernels", 1)
        for score, mode in ((1, 1), (4, 2)):
            p.set_match_score(score, kh, kw)
            p.set_image_device(img_d.data_ptr())
            res = _few_and_many(p, lambda: _packed(torch, dev, p, 2, ker_d, 2, kh, kw), mode, (3, 3), CAP, 2)
            p.set_peaks(mode, 2, CAP, res["thresholds"][0], (3, 3))
            _, found, lists = _packed(torch, dev, p, 2, ker_d, 2, kh, kw)
            strong = p.peaks(order="strength")[1][0]
            res["planted"] = ([(int(l["row"]), int(l["col"]), float(l["value"])) for l in lists[0] if (int(l["row"]), int(l["col"])) in out["at"]],
                              sorted((int(l["row"]), int(l["col"])) for l in strong[:2]),
                              bool(np.array_equal(np.sort(strong, order=["col", "row"]), np.sort(lists[0], order=["col", "row"]))))
            out[score] = res
        p.set_match_score(0)
        p.set_image_device(img_d.data_ptr())
        p.set_spectral_filter(fc.FILTER_PHASE)
        res = _few_and_many(p, lambda: _packed(torch, dev, p, 2, ker_d, 2, kh, kw), 1, (3, 3), CAP, 2)
        p.set_peaks(1, 2, CAP, res["thresholds"][0], (3, 3))
        _packed(torch, dev, p, 2, ker_d, 2, kh, kw)
        strong = p.peaks(order="strength")[1][0]
        res["strongest"] = sorted((int(l["row"]), int(l["col"])) for l in strong[:2])
        res["offsets"] = [(float(l["d_row"]), float(l["d_col"])) for l in strong[:2]]
        out["phase"] = res
    return out


def _case_zero_and_nan():
    """an all-zero kernel: the map is all zeros; a kernel holding a NaN: no element compares"""
    torch, fc, dev = N._ctx()
    H, W, F, kh, kw = SHAPE
    n = 3
    img, ks = zero_kernel_inputs(SHAPE, n, 61)
    ks[2] = ks[2].copy(order="F")
    ks[2][3, 4, 0] = np.nan
    img_d, ker_d = _image_t(torch, img).to(dev), _pack_t(torch, ks).to(dev)
    out = {}
    with fc.Plan(H, W, F, kh, kw) as p:
        p.set_image_device(img_d.data_ptr())
        i = p.info
        for radius in ((1, 1), (0, 0)):
            p.set_peaks(1, n, CAP, 0.0, radius)
            maps, found, lists = _packed(torch, dev, p, n, ker_d, n, kh, kw)
            cmp = lists_differ(found, lists, maps, 0, 1, 0.0, radius, CAP)
            z = lists[1]
            out[radius] = (cmp, int(np.count_nonzero(maps[1])), int(found[1]), len(z), [(int(r["row"]), int(r["col"])) for r in z[:2]],
                           bool(np.array_equal(z["col"].astype(np.int64) * i.out_h + z["row"], np.arange(len(z)))), bool((z["value"] == 0).all()),
                           bool((z["d_row"] == 0).all() and (z["d_col"] == 0).all()),
                           int(np.isnan(maps[2]).sum()), int(found[2]), len(lists[2]))
        out["elements"] = i.out_h * i.out_w
    return out


def _case_batch(walk):
    """an image batch of 3 x 2 kernels: the lists are image-major, as the maps are; batch_maps 3 cuts a launch inside an image"""
    torch, fc, dev = N._ctx()
    H, W, F, kh, kw = SHAPE
    n, B = 2, 3
    imgs = [inputs(SHAPE, n, 31 + b)[0] for b in range(B)]
    ks = inputs(SHAPE, n, 31)[1]
    ker_d = _pack_t(torch, ks).to(dev)
    out = {}
    with fc.Plan(H, W, F, kh, kw) as p:
        p.set_option("image_walk", walk)
        p.set_images(np.asfortranarray(np.stack([im[:, :, 0] for im in imgs], axis=2)))
        out["active"] = p.get_option("image_walk_active")
        for batch_maps in (0, 3):
            p.set_option("batch_maps", batch_maps)
            p.set_peaks(0)      # (the scratch of a launch is sized for the "batch_maps" of the setter's time)
            out[batch_maps] = _few_and_many(p, lambda: _packed(torch, dev, p, B * n, ker_d, n, kh, kw), 1, (3, 3), CAP, B * n)
        maps = _packed(torch, dev, p, B * n, ker_d, n, kh, kw)[0]
        out["images_differ"] = bool(not np.array_equal(maps[0], maps[n]))
    return out


def _case_sinks():
    """host maps on the pinned, the ring and the plain-copy route against the packed device route: the same lists"""
    torch, fc, dev = N._ctx()
    H, W, F, kh, kw = SHAPE
    n = 3
    img, ks = inputs(SHAPE, n, 29)
    ker_d = _pack_t(torch, ks).to(dev)
    out = {}
    with fc.Plan(H, W, F, kh, kw) as p:
        p.set_image(img)
        p.set_peaks(1, n, CAP, 0.0, (3, 3))
        few, _ = thresholds_of(_packed(torch, dev, p, n, ker_d, n, kh, kw)[0], 0, 1, 0.999)
        p.set_peaks(1, n, CAP, few, (3, 3))
        maps, found, lists = _packed(torch, dev, p, n, ker_d, n, kh, kw)
        out["packed"] = lists_differ(found, lists, maps, 0, 1, few, (3, 3), CAP)
        want = lists_bytes(found, lists)
        for name, options in (("pinned", {"host_stream": 0, "host_pinned": 1}), ("ring", {"host_stream": 2, "host_min_kb": 1}),
                              ("copies", {"host_stream": 0, "host_pinned": 0})):
            for k, v in options.items():
                p.set_option(k, v)
            outs = p.convolve(ks)
            found, lists = p.peaks()
            hmaps = np.stack([np.ascontiguousarray(o.T) for o in outs])
            out[name] = (lists_differ(found, lists, hmaps, 0, 1, few, (3, 3), CAP), lists_bytes(found, lists) == want)
        part = p.peaks(1, 2)
        out["partial_read"] = lists_bytes(*part) == lists_bytes(found[1:3], lists[1:3])
    return out


def _case_with_extrema():
    """both on, a 24 x 20 rectangle, a radius covering the map: the single peak is the extrema record's maximum; mode 2: its minimum"""
    torch, fc, dev = N._ctx()
    H, W, F, kh, kw = SHAPE
    n = 3
    img, ks = inputs(SHAPE, n, 47)
    img_d, ker_d = _image_t(torch, img).to(dev), _pack_t(torch, ks).to(dev)
    out = {}
    with fc.Plan(H, W, F, kh, kw) as p:
        p.set_image_device(img_d.data_ptr())
        p.set_output_rect(3, 5, 24, 20)
        p.set_extrema(1, n)
        for mode, thr, side in ((1, float("-inf"), "max"), (2, float("inf"), "min")):
            p.set_peaks(mode, n, 4, thr, (24, 20))
            maps, found, lists = _packed(torch, dev, p, n, ker_d, n, kh, kw)
            recs = p.extrema()
            out[mode] = (lists_differ(found, lists, maps, 0, mode, thr, (24, 20), 4), [int(f) for f in found],
                         [len(l) == 1 and (int(l[0]["row"]), int(l[0]["col"])) == (int(r[side + "_row"]), int(r[side + "_col"]))
                          and np.float32(l[0]["value"]).view(np.uint32) == np.float32(r[side + "_value"]).view(np.uint32) for l, r in zip(lists, recs)])
        out["state"] = (p.get_option("extrema"), p.get_option("peaks"), (p.info.out_h, p.info.out_w))
    return out


def _case_deals():
    """both tile deals at M = 432 (the dynamic queue's default) and M = 144: identical bytes"""
    torch, fc, dev = N._ctx()
    out = {}
    for shape in ((840, 270, 1, 13, 11), SHAPE):
        H, W, F, kh, kw = shape
        n = 2
        img, ks = inputs(shape, n, 53)
        img_d, ker_d = _image_t(torch, img).to(dev), _pack_t(torch, ks).to(dev)
        with fc.Plan(H, W, F, kh, kw) as p:
            p.set_image_device(img_d.data_ptr())
            p.set_peaks(1, n, CAP, 0.0, (3, 3))
            few, _ = thresholds_of(_packed(torch, dev, p, n, ker_d, n, kh, kw)[0], 0, 1, 0.9995)
            p.set_peaks(1, n, CAP, few, (3, 3))
            res = []
            for dyn in (0, 1):
                p.set_option("dynamic_tiles", dyn)
                maps, found, lists = _packed(torch, dev, p, n, ker_d, n, kh, kw)
                res.append((lists_differ(found, lists, maps, 0, 1, few, (3, 3), CAP), lists_bytes(found, lists)))
            out[shape[0]] = (res[0][0], res[1][0], res[0][1] == res[1][1], p.info.transform_h)
    return out


def _case_graph():
    """set_image_device + convolve_packed under peaks at M = 432, captured once and replayed with other inputs: the lists read through
    peaks_device() equal the eager ones, and the capture allocates nothing"""
    torch, fc, dev = N._ctx()
    shape = H, W, F, kh, kw = (840, 270, 1, 13, 11)
    n, cap, radius = 3, CAP, (3, 3)
    sets = [inputs(shape, n, 90 + k) for k in range(3)]
    stream = torch.cuda.Stream(dev)
    out = {}
    with torch.cuda.stream(stream), fc.Plan(H, W, F, kh, kw, stream=stream.cuda_stream) as p:
        p.set_peaks(1, n, cap, 0.0, radius)
        i = p.info
        ne = n * i.out_h * i.out_w
        imgs_h = [_image_t(torch, s[0]).pin_memory() for s in sets]
        kers_h = [_pack_t(torch, s[1]).pin_memory() for s in sets]
        img_d = torch.empty(imgs_h[0].shape, dtype=torch.float32, device=dev)
        ker_d = torch.empty(kers_h[0].shape, dtype=torch.float32, device=dev)
        maps_t, out_ptr = _guarded(torch, dev, ne, 0)
        fptr, rptr, nbytes = p.peaks_device()
        out["device"] = (fptr != 0 and rptr != 0, nbytes)

        def view(ptr, words):      # a device array of the plan seen as a tensor: copies of it are ordered on the stream like everything else
            class _Array:
                __cuda_array_interface__ = {"shape": (words,), "typestr": "<i4", "data": (ptr, False), "version": 2}
            return torch.as_tensor(_Array(), device=dev)
        found_view, rec_view = view(fptr, n), view(rptr, nbytes // 4)
        snaps = [(torch.empty(n, dtype=torch.int32, device=dev), torch.empty(nbytes // 4, dtype=torch.int32, device=dev)) for _ in range(4)]

        def snapshot(k):
            snaps[k][0].copy_(found_view, non_blocking=True)
            snaps[k][1].copy_(rec_view, non_blocking=True)

        def step():
            p.set_image_device(img_d.data_ptr())
            p.convolve_packed_device(n, ker_d.data_ptr(), kh, kw, out_ptr)

        img_d.copy_(imgs_h[0], non_blocking=True)
        ker_d.copy_(kers_h[0], non_blocking=True)
        step()                                   # eager warm-up: sizes the scratch; the threshold comes from its maps
        torch.cuda.synchronize()
        few, _ = thresholds_of(_unguard(maps_t, ne, 0).reshape(n, i.out_w, i.out_h), 0, 1, 0.9995)
        p.set_peaks(1, n, cap, few, radius)
        step()
        torch.cuda.synchronize()
        ws = p.refresh_info().workspace_bytes
        graph = torch.cuda.CUDAGraph()
        capture = torch.cuda.Stream(dev)
        with torch.cuda.graph(graph, stream=capture):
            p.set_stream(torch.cuda.current_stream(dev).cuda_stream)
            step()
        p.set_stream(stream.cuda_stream)
        maps_seen = []
        for r in range(2):                       # nothing synchronised inside the loop
            img_d.copy_(imgs_h[r + 1], non_blocking=True)
            ker_d.copy_(kers_h[r + 1], non_blocking=True)
            graph.replay()
            snapshot(r)
            maps_seen.append(maps_t.clone())
        torch.cuda.synchronize()
        eager = []
        for r in range(2):
            img_d.copy_(imgs_h[r + 1], non_blocking=True)
            ker_d.copy_(kers_h[r + 1], non_blocking=True)
            step()
            snapshot(2 + r)
            eager.append(p.peaks())
        torch.cuda.synchronize()
        del graph
        out["same_ws"] = p.refresh_info().workspace_bytes == ws

        def read(k):
            found = snaps[k][0].cpu().numpy().copy()
            recs = np.frombuffer(snaps[k][1].cpu().numpy().tobytes(), dtype=eager[0][1][0].dtype).reshape(n, cap)
            return found, [recs[m, :min(int(found[m]), cap)] for m in range(n)]
        got = [read(k) for k in range(4)]
        out["replay_vs_eager"] = [lists_bytes(*got[r]) == lists_bytes(*eager[r]) and lists_bytes(*got[2 + r]) == lists_bytes(*eager[r]) for r in range(2)]
        out["replay_vs_numpy"] = [lists_differ(got[r][0], got[r][1], _unguard(maps_seen[r], ne, 0).reshape(n, i.out_w, i.out_h), 0, 1, few, radius, cap) for r in range(2)]
        out["replays_differ"] = lists_bytes(*got[0]) != lists_bytes(*got[1])
        out["M"] = p.info.transform_h // 2
    return out


def _case_surface():
    torch, fc, dev = N._ctx()
    H, W, F, kh, kw = SHAPE
    n = 2
    img, ks = N.inputs(SHAPE, n + 1, 43)
    img_d, ker_d = _image_t(torch, img).to(dev), _pack_t(torch, ks).to(dev)
    out = {}
    state_names = ("peaks", "peaks_max_maps", "peaks_max", "peaks_radius_h", "peaks_radius_w", "peaks_maps")

    def refused(fn, word=""):
        try:
            fn()
            return None
        except fc.FFTConvError as e:
            return (e.status, word in str(e))

    def state(p):
        return tuple(p.get_option(o) for o in state_names) + p.peaks_device()

    with fc.Plan(H, W, F, kh, kw) as never, fc.Plan(H, W, F, kh, kw) as p:
        never.set_image_device(img_d.data_ptr())
        p.set_image_device(img_d.data_ptr())
        want = N._ncc_window(torch, dev, never, n, ker_d, n, kh, kw)
        out["off_get"] = (refused(lambda: p.peaks(0, 1)), refused(lambda: p.peaks_device()))
        out["off_state"] = tuple(p.get_option(o) for o in state_names)
        p.prepare_kernels_packed_device(n, ker_d.data_ptr(), kh, kw)      # (the setter keeps the image and the prepared kernels)
        ws_off = p.refresh_info().workspace_bytes
        p.set_peaks(1, n, 32, 0.25, (2, 3))
        out["on"] = state(p)[:6]
        ws_on = p.refresh_info().workspace_bytes
        out["workspace"] = ws_on - ws_off      # found + records + the scratch of a launch
        out["before_convolve"] = refused(lambda: p.peaks(0, 1), "no convolve")
        # every refusal leaves the state as it was
        before = state(p)
        bad = [(3, n, 32, 0.25, 2, 3), (-1, n, 32, 0.25, 2, 3), (1, 0, 32, 0.25, 2, 3), (1, n, 0, 0.25, 2, 3), (2, n, -5, 0.25, 2, 3),
               (1, n, 32, float("nan"), 2, 3), (1, n, 32, 0.25, -1, 3), (1, n, 32, 0.25, 2, -1)]
        out["bad_rc"] = [p._lib.fftconv_plan_set_peaks(p._h, *a) for a in bad]
        out["bad_keeps_state"] = state(p) == before and p.refresh_info().workspace_bytes == ws_on
        out["inf_allowed"] = [p._lib.fftconv_plan_set_peaks(p._h, 1, n, 32, t, 2, 3) for t in (float("inf"), float("-inf"))]
        p.set_peaks(1, n, 32, 0.25, (2, 3))
        i = p.info
        t, optr = _guarded(torch, dev, (n + 1) * i.out_h * i.out_w, 0)
        out["too_many"] = refused(lambda: p.convolve_packed_device(n + 1, ker_d.data_ptr(), kh, kw, optr), "max_maps")
        maps, found, lists = _packed(torch, dev, p, n, ker_d, n, kh, kw)                  # the plan is usable afterwards
        out["after_refusal"] = (lists_differ(found, lists, maps, 0, 1, 0.25, (2, 3), 32), _differ(maps, want, 0), p.get_option("peaks_maps"))
        ws_run = p.refresh_info().workspace_bytes      # (behind a convolve: it sizes the plan's own scratch)
        out["beyond"] = refused(lambda: p.peaks(1, 2))
        p.set_peaks(1, n, 32, 0.25, (2, 3))                                               # changes nothing: returns early, the lists stay
        out["noop"] = (state(p) == before[:5] + (n,) + before[6:], lists_bytes(*p.peaks()) == lists_bytes(found, lists))
        # threshold, radius or mode alone: the buffers stay
        p.set_peaks(2, n, 32, -0.5, (1, 0))
        out["rule_only"] = (state(p)[6:] == before[6:], p.refresh_info().workspace_bytes == ws_run, state(p)[:6], refused(lambda: p.peaks(0, 1), "no convolve"))
        p.set_peaks(1, n, 32, 0.25, (2, 3))
        # it survives the other setters
        p.set_output_rect(3, 5, 100, 77)
        p.set_match_score(2, kh, kw)
        p.set_image_device(img_d.data_ptr())
        p.set_option("map_format", 1)
        out["survives"] = (state(p)[:5] == before[:5], state(p)[6:] == before[6:])
        maps, found, lists = _packed(torch, dev, p, n, ker_d, n, kh, kw, 1)
        out["after_setters"] = ((p.info.out_h, p.info.out_w), lists_differ(found, lists, maps, 1, 1, 0.25, (2, 3), 32))
        p.set_option("map_format", 0)
        p.set_match_score(0)
        p.set_option("output_region", 0)
        p.set_image_device(img_d.data_ptr())
        # off -> on -> off leaves the maps bit-equal to a plan that never had it
        res, ws = [], []
        for mode in (0, 1, 0):
            p.set_peaks(mode, n, 32, 0.25, (2, 3))
            res.append(_differ(N._ncc_window(torch, dev, p, n, ker_d, n, kh, kw), want, 0))
            ws.append(p.refresh_info().workspace_bytes)
        out["off_on_off"] = (res, p.get_option("peaks"), refused(lambda: p.peaks(0, 1)), (ws[1] - ws[0], ws[2] - ws[0]))
    # a block-wise plan refuses it with the table's message
    with fc.Plan(600, 600, 1, 9, 9, options={"max_transform": 512}) as big:
        out["blockwise"] = (big.get_option("blockwise"), refused(lambda: big.set_peaks(1, 4, 16, 0.0, (1, 1)), "block-wise plan"), refused(lambda: big.set_peaks(0)),
                            big.get_option("peaks"))
    return out


# ---- the tests

@pytest.mark.parametrize("fmt", [0, 1, 2])
def test_formats_and_radii(device, fmt):
    """250 x 250 (*) 31 x 31, three kernels, the whole 288 x 288 window (331 KB of fp32 per map: 21 units) as fp32, fp16 and bf16 maps,
    radius (3, 3), (0, 0) -- plain thresholding -- and (1, 5), each at a threshold with 1 .. 256 peaks per map and at one that
    overflows 256"""
    res = device("_case_format", fmt)
    assert res.pop("size") == (288, 288)
    assert res.pop("state") == (1, 3, CAP, 1, 5, 3)
    assert sorted(res) == [(0, 0), (1, 5), (3, 3)]
    for radius, r in res.items():
        print(fmt, radius, r["thresholds"])
        few_and_many(r, 3, CAP)


@pytest.mark.parametrize("name", sorted(EXTENTS))
def test_extents(device, name):
    """region 2, the odd rectangle (3, 5, 271, 271) -- 73 441 elements: maps 1 and 2 start off a 16-byte address -- stride (2, 3), one
    column, one element"""
    res = device("_case_extent", name)
    _, size, cap, _, overflow = EXTENTS[name]
    print(name, res["thresholds"])
    assert res["size"] == size
    assert res["unaligned"] == (name in ("odd rectangle", "one element"))
    few_and_many(res, 3, cap, overflow)
    if not overflow:
        assert res["many"]["ref_found"] == [1, 1, 1]


def test_scores_and_phase_correlation(device):
    """score 1 with a template cut from the image and planted in it once more: both positions are in the list, at 1 within the
    score's bound (1e-4, as the extrema's test of the same score), and are the two strongest; score 4 with mode 2: both are the two
    smallest; phase correlation: the strongest peaks sit at the shifts"""
    res = device("_case_scores")
    for key in (1, 4, "phase"):
        print(key, res[key]["thresholds"])
        few_and_many(res[key], 2, CAP)
    at = sorted(res["at"])
    planted, strongest, same_set = res[1]["planted"]
    assert sorted((r, c) for r, c, _ in planted) == at and all(abs(v - 1.0) < 1e-4 for _, _, v in planted), planted
    assert strongest == at and same_set
    planted, strongest, same_set = res[4]["planted"]
    assert sorted((r, c) for r, c, _ in planted) == at and strongest == at and same_set, (planted, strongest)
    assert res["phase"]["strongest"] == at, res["phase"]["strongest"]
    assert all(abs(d) <= 0.5 for pair in res["phase"]["offsets"] for d in pair)


def test_zero_map_and_nan_map(device):
    """an all-zero kernel, threshold 0: radius 1 leaves one peak at (0, 0); radius 0 counts every element and stores the first 256 in
    memory order.  A kernel holding a NaN: its map is all NaN and has no peak."""
    res = device("_case_zero_and_nan")
    print(res)
    elements = res["elements"]
    cmp, nonzero, found, stored, first, in_order, zeros, no_offsets, nans, nan_found, nan_stored = res[(1, 1)]
    exact(cmp, 3, CAP)
    assert nonzero == 0 and found == 1 and stored == 1 and first == [(0, 0)] and zeros and no_offsets
    assert nans == elements and nan_found == 0 and nan_stored == 0
    cmp, nonzero, found, stored, first, in_order, zeros, no_offsets, nans, nan_found, nan_stored = res[(0, 0)]
    exact(cmp, 3, CAP)
    assert nonzero == 0 and found == elements and stored == CAP and first == [(0, 0), (1, 0)] and in_order and zeros and no_offsets
    assert nans == elements and nan_found == 0 and nan_stored == 0


@pytest.mark.parametrize("walk", [0, 1])
def test_image_batches_are_image_major(device, walk):
    res = device("_case_batch", walk)
    assert res["active"] == walk and res["images_differ"]
    for batch_maps in (0, 3):
        few_and_many(res[batch_maps], 6, CAP)


def test_host_delivery_gives_the_same_lists(device):
    res = device("_case_sinks")
    exact(res["packed"], 3, CAP)
    assert all(1 <= f <= CAP for f in res["packed"]["ref_found"])
    for name in ("pinned", "ring", "copies"):
        cmp, same = res[name]
        exact(cmp, 3, CAP)
        assert same, name
    assert res["partial_read"]


def test_with_extrema_on_as_well(device):
    res = device("_case_with_extrema")
    print(res)
    assert res["state"] == (1, 2, (24, 20))
    for mode in (1, 2):
        cmp, found, same = res[mode]
        exact(cmp, 3, 4)
        assert found == [1, 1, 1] and all(same), (mode, found, same)


def test_both_tile_deals_give_identical_bytes(device):
    res = device("_case_deals")
    for H, M in ((840, 432), (250, 144)):
        static, dynamic, same, transform_h = res[H]
        assert transform_h == 2 * M
        exact(static, 2, CAP)
        exact(dynamic, 2, CAP)
        assert all(1 <= f <= CAP for f in static["ref_found"]) and same


def test_graph_replay(device):
    res = device("_case_graph")
    print(res)
    assert res["M"] == 432 and res["device"] == (True, 3 * CAP * 20) and res["same_ws"]
    assert res["replay_vs_eager"] == [True, True]
    for cmp in res["replay_vs_numpy"]:
        exact(cmp, 3, CAP)
        assert all(f >= 1 for f in cmp["ref_found"])
    assert res["replays_differ"]


def test_state_and_surface(device):
    res = device("_case_surface")
    print(res)
    assert res["off_get"][0][0] == -1 and res["off_get"][1][0] == -1 and res["off_state"] == (0, 0, 0, 0, 0, -1)
    assert res["on"] == (1, 2, 32, 2, 3, -1)
    assert res["workspace"] == 2 * 4 + 2 * 32 * 20 + 2 * 2 * 1024 * 4
    assert res["before_convolve"] == (-1, True)
    assert res["bad_rc"] == [-1] * 8 and res["bad_keeps_state"]
    assert res["inf_allowed"] == [0, 0]
    assert res["too_many"] == (-1, True)
    cmp, maps_differ, peaks_maps = res["after_refusal"]
    exact(cmp, 2, 32)
    assert maps_differ == 0 and peaks_maps == 2
    assert res["beyond"] is not None and res["beyond"][0] == -1
    assert res["noop"] == (True, True)
    assert res["rule_only"] == (True, True, (2, 2, 32, 1, 0, -1), (-1, True))
    assert res["survives"] == (True, True)
    size, cmp = res["after_setters"]
    assert size == (100, 77)
    exact(cmp, 2, 32)
    assert res["off_on_off"][0] == [0, 0, 0] and res["off_on_off"][1] == 0 and res["off_on_off"][2][0] == -1
    assert res["off_on_off"][3] == (res["workspace"], 0)      # workspace_bytes counts the lists and their scratch, and off frees them
    blocks, on, off, state = res["blockwise"]
    assert blocks > 0 and on == (-1, True) and off is None and state == 0
