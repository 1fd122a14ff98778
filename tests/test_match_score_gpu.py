"""Template-matching scores (fftconv_plan_set_match_score) on the GPU: CCOEFF (2), CCORR_NORMED (3) and SQDIFF (4).

The yardstick is a NumPy float64 restatement of the table in include/fftconv.h, written here (score_reference) over the helpers of
tests/test_ncc_gpu.py: E the direct sums of I^2 over the box, t2 the kernel's sum of squares, R the raw map.  Per element

    score 2   |got - ref| <= 1e-5 * max |ref|                                         the project's bar for fp32 maps
    score 3   |got - ref| <= 1e-5 * max_u |raw_k| * Dc_ref(u) + 4 * 2^-24, exactly 0 where Dc_ref = 0      (mode 1's bound)
    score 4   |got - ref| <= 1e-5 * max_u |2 R_k| + 4 * 2^-24 * (E_ref(u) + t2_k + |2 R_ref(u)|)
              the bar on the raw map, then the fp32 roundings of Q, c, the two adds and the result

The inputs are test_ncc_gpu.inputs(): Gaussian noise plus a flat 0.75 patch, so no pixel is 0 and E = 0 holds exactly in the slack of
the window (no data under the box) -- every case asserts that, and that every element took part in its comparison.  Score 4 is two
fp32 adds in one fixed order on every route, score 3 one fp32 multiply: the fused store and the staged crop must agree BIT FOR BIT on
every configuration of the specialised output kernel, and 16-bit maps, regions, rectangles, host maps and prepared kernel sets must
return the rounded / cropped fp32 window bit for bit.  The cases run in a spawned child (test_accuracy_gpu._Child)."""
import os
import re

import numpy as np
import pytest

import test_ncc_gpu as N
import util
from test_accuracy_gpu import _Child
from test_features_gpu import _logged
from test_map_format_gpu import _image_t, _pack_t
from test_output_rect_gpu import _crop, _differ, _guarded, _unguard, col_configs

pytestmark = pytest.mark.gpu

ROUND = 4 * 2.0 ** -24
NAMES = {3: "CCORR_NORMED", 4: "SQDIFF"}


@pytest.fixture(scope="module")
def device():
    child = _Child(globals())
    yield child
    if child.gone:
        child.kill()
    else:
        child.ex.shutdown(wait=True)


# ---- the table, in float64

def score_reference(score, img, ks, fft_h, fft_w, flip):
    """(ref [n][fft_w][fft_h] as the maps lie in memory, bound of the same shape, zero mask of the same shape: where the result must
    be exactly 0 (score 3, Dc = 0), whether E = 0 holds exactly where no data lies under the box)"""
    H, W, F = img.shape
    kh, kw = ks[0].shape[:2]
    _, s2 = N.window_sums(img, kh, kw, fft_h, fft_w)
    E = s2.sum(axis=0)
    slack = np.zeros((fft_h, fft_w), dtype=bool)
    slack[H + kh - 1:, :] = True
    slack[:, W + kw - 1:] = True
    slack_ok = bool(np.array_equal(E == 0, slack)) and bool((img != 0).all())
    refs, bounds, zeros = [], [], []
    for k in ks:
        t = k.astype(np.float64)
        t2 = float((t * t).sum())
        if score == 2:
            ref = N.raw_map(img, t - t.mean(axis=(0, 1), keepdims=True), fft_h, fft_w, flip)
            bound = np.full_like(ref, 1e-5 * np.abs(ref).max())
            zero = np.zeros_like(slack)
        elif score == 3:
            with np.errstate(divide="ignore"):
                Dc = np.where(E == 0, 0.0, 1.0 / np.sqrt(np.where(E == 0, 1.0, E))).astype(np.float32).astype(np.float64)
            raw = N.raw_map(img, t / np.sqrt(t2) if t2 > 0 else np.zeros_like(t), fft_h, fft_w, flip)
            ref, bound, zero = raw * Dc, 1e-5 * np.abs(raw).max() * Dc + ROUND, Dc == 0
        else:
            R = N.raw_map(img, t, fft_h, fft_w, flip)
            ref = E - 2 * R + t2
            bound = 1e-5 * np.abs(2 * R).max() + ROUND * (E + t2 + np.abs(2 * R))
            zero = np.zeros_like(slack)
        refs.append(ref.T)
        bounds.append(np.broadcast_to(bound, ref.shape).T)
        zeros.append(zero.T)
    return np.stack(refs), np.stack(bounds), np.stack(zeros), slack_ok


def excess_of(got, ref, bound, zero):
    """(max of |got - ref| / bound over EVERY element -- <= 1 passes, elements that must be exactly 0 and are not, elements compared)"""
    got = np.asarray(got, dtype=np.float64).reshape(ref.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, np.abs(got - ref) / np.where(bound > 0, bound, 1.0), np.where(got == ref, 0.0, np.inf))
    ratio = np.where(np.isfinite(got), ratio, np.inf)
    return float(ratio.max()), int((got[zero] != 0).sum()), int(ratio.size)


def zero_kernel_inputs(shape, n, seed):
    img, ks = N.inputs(shape, n, seed)
    ks[1] = np.asfortranarray(np.zeros_like(ks[1]))
    return img, ks


def sqdiff_not_built():
    src = open(os.path.join(util.ROOT, "cuda-fft-convolution_amd", "csrc", "fast_paths.hpp")).read()
    return tuple(int(x) for x in re.search(r"FC_COLS_SQDIFF_NOT_BUILT\[\] = \{([^}]*)\}", src).group(1).split(","))


# ---- the child's side

def _state(p):
    return (p.get_option("match_score"), p.get_option("normalise"), p.get_option("norm_box_h"), p.get_option("norm_box_w"), p.get_option("images"))


def _case_parity(name, flip):
    torch, fc, dev = N._ctx()
    shape, options, host = N.KINDS[name]
    H, W, F, kh, kw = shape
    n = 3
    img, ks = zero_kernel_inputs(shape, n, 17 + len(name) + flip)
    out = {}
    with fc.Plan(H, W, F, kh, kw, options=options) as p:
        i = p.info
        p.set_option("flip_kernels", flip)
        if not host:
            img_d, ker_d = _image_t(torch, img).to(dev), _pack_t(torch, ks).to(dev)
        for score in (2, 3, 4):
            p.set_match_score(score, kh, kw)
            state = _state(p)
            if host:
                p.set_image(img)
                got = np.stack([np.ascontiguousarray(o.T) for o in p.convolve(ks)])
            else:
                p.set_image_device(img_d.data_ptr())
                got = N._ncc_window(torch, dev, p, n, ker_d, n, kh, kw)
            ref, bound, zero, slack_ok = score_reference(score, img, ks, i.fft_h, i.fft_w, flip)
            out[score] = {"state": state, "slack_ok": slack_ok, "excess": excess_of(got, ref, bound, zero), "size": int(ref.size),
                          "zero_kernel": (float(got[1].min()), float(got[1].max())), "direct": p.get_option("norm_direct"),
                          "q_max": float(ref[1].max())}
        out["kinds"] = (p.get_option("specialised_kernels"), p.info.transform_h, p.info.fft_h)
    return out


def _case_properties():
    """correlation with a template cut from the image: SQDIFF is 0 and least at its position, CCORR_NORMED is 1 and nowhere more,
    CCOEFF is the ncc map times the template's norm over D; gain moves score 4 and not score 3"""
    torch, fc, dev = N._ctx()
    shape = H, W, F, kh, kw = (250, 250, 2, 31, 31)
    img, ks = N.inputs(shape, 2, 5)
    y0, x0 = 140, 37
    ks[0] = np.asfortranarray(img[y0:y0 + kh, x0:x0 + kw, :].copy())
    at = (x0 + kw - 1, y0 + kh - 1)              # [w][h] of the map
    img2 = np.asfortranarray((np.float32(3.7) * img).astype(np.float32))
    ks2 = [np.asfortranarray((np.float32(0.5) * k).astype(np.float32)) for k in ks]
    out = {"at": at}
    with fc.Plan(H, W, F, kh, kw) as p:
        i = p.info
        p.set_option("flip_kernels", 1)
        ker_d, img_d = _pack_t(torch, ks).to(dev), _image_t(torch, img).to(dev)
        ker2_d, img2_d = _pack_t(torch, ks2).to(dev), _image_t(torch, img2).to(dev)
        got, refs = {}, {}
        for score in (1, 2, 3, 4):
            p.set_match_score(score, kh, kw)
            p.set_image_device(img_d.data_ptr())
            got[score] = N._ncc_window(torch, dev, p, 2, ker_d, 2, kh, kw).astype(np.float64)
            if score > 1:
                refs[score] = score_reference(score, img, ks, i.fft_h, i.fft_w, 1)
                out["excess%d" % score] = excess_of(got[score], *refs[score][:3])
                out["slack_ok"] = refs[score][3]
        gain = {}
        for score in (3, 4):
            p.set_match_score(score, kh, kw)
            p.set_image_device(img2_d.data_ptr())
            gain[score] = N._ncc_window(torch, dev, p, 2, ker2_d, 2, kh, kw).astype(np.float64)
    valid = (slice(None), slice(kw - 1, W), slice(kh - 1, H))
    b4, b3 = refs[4][1], refs[3][1]
    v4 = got[4][0][valid[1:]]
    out["sqdiff_at"] = abs(got[4][0][at]) / b4[0][at]
    out["sqdiff_argmin"] = tuple(int(v) + o for v, o in zip(np.unravel_index(np.argmin(v4), v4.shape), (kw - 1, kh - 1)))
    out["sqdiff_below"] = float((-got[4] / b4).max())                   # <= 1: nothing below -bound
    out["ccorr_at"] = abs(got[3][0][at] - 1.0) / b3[0][at]
    out["ccorr_over"] = float(((got[3] - 1.0) / b3).max())
    # score 2 = ncc * ||T - mean T|| / D on the valid part: the bound of score 2 plus mode 1's bound carried through norm / D
    D, near = N.scale_plane(img, kh, kw, i.fft_h, i.fft_w)
    D = D.T
    E = N.window_sums(img, kh, kw, i.fft_h, i.fft_w)[1].sum(axis=0)
    worst, n_flat = 0.0, 0
    for j, k in enumerate(ks):
        t = k.astype(np.float64)
        t = t - t.mean(axis=(0, 1), keepdims=True)
        norm = np.sqrt((t * t).sum())
        raw_unit_max = np.abs(refs[2][0][j]).max() / norm
        Dv, Ev = D[valid[1:]], E.T[valid[1:]]
        on = Dv > 0
        want = got[1][j][valid[1:]][on] * norm / Dv[on]
        bound = refs[2][1][j][valid[1:]][on] + (1e-5 * raw_unit_max * Dv[on] + ROUND) * norm / Dv[on]
        worst = max(worst, float((np.abs(got[2][j][valid[1:]][on] - want) / bound).max()))
        # D = 0: the window is flat to within 2^-15 of its RMS (the box inside the flat patch), so by Cauchy-Schwarz
        # |sum (I - mean I)(T - mean T)| <= sqrt(den2) * norm <= 2^-15 * sqrt(E) * norm
        flat = ~on
        n_flat += int(flat.sum())
        if flat.any():
            worst = max(worst, float((np.abs(got[2][j][valid[1:]][flat]) / (refs[2][1][j][valid[1:]][flat] + 2.0 ** -15 * np.sqrt(Ev[flat]) * norm)).max()))
    out["ccoeff_vs_ncc"], out["near"], out["flat_windows"] = worst, near, n_flat
    out["gain3"] = float((np.abs(gain[3] - got[3]) / (2 * b3)).max())
    out["gain4"] = float((np.abs(gain[4] - got[4]) / (2 * b4)).max())
    return out


def _case_fused(M, score):
    """test_ncc_gpu._case_fused's shapes under a score: "norm_store" 1 against 0, static deal and dynamic queue, the whole window and
    the odd rectangle"""
    torch, fc, dev = N._ctx()
    kh, kw, n = 13, 11, 2
    shape = (2 * M - 18, 272, 1, kh, kw)
    img, ks = N.inputs(shape, n, 7 + M)
    img_d, ker_d = _image_t(torch, img).to(dev), _pack_t(torch, ks).to(dev)
    name = NAMES[score]
    out = {}
    with fc.Plan(shape[0], shape[1], 1, kh, kw, options={"exact_window": 1, "blockwise": 1}) as p:
        assert p.get_option("blockwise") == 0 and (p.info.fft_h, p.info.fft_w, p.info.transform_h) == (2 * M, 288, 2 * M)
        assert p.get_option("specialised_kernels") == 3
        p.set_match_score(score, kh, kw)
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
                    maps[store], log = _logged(lambda: N._ncc_window(torch, dev, p, n, ker_d, n, kh, kw))
                    p.set_option("verbose", 0)
                    lines[store] = ("normalisation: fused " + name in log, "normalisation: staged " + name in log)
                out[(dyn, rect is not None)] = (direct[1], direct[0], _differ(maps[1], maps[0], 0), lines[1], lines[0],
                                                int((~np.isfinite(maps[0])).sum()), float(np.abs(maps[0]).max()))
    return out


def _case_composition(score):
    """16-bit maps, a region, a rectangle, host maps and prepared kernels against the plan's own fp32 window of the score"""
    torch, fc, dev = N._ctx()
    shape = H, W, F, kh, kw = (250, 250, 1, 31, 31)
    n = 3
    img, ks = N.inputs(shape, n, 23)
    img_d, ker_d = _image_t(torch, img).to(dev), _pack_t(torch, ks).to(dev)
    out = {}
    with fc.Plan(H, W, F, kh, kw) as p:
        p.set_match_score(score, kh, kw)
        p.set_image_device(img_d.data_ptr())
        win = N._ncc_window(torch, dev, p, n, ker_d, n, kh, kw)
        ref, bound, zero, out["slack_ok"] = score_reference(score, img, ks, p.info.fft_h, p.info.fft_w, 0)
        out["window"] = excess_of(win, ref, bound, zero)
        out["fp16_overflows"] = bool((np.abs(win) > 65504).any())
        for fmt in (1, 2):
            p.set_option("map_format", fmt)
            i = p.refresh_info()
            ne = n * i.out_h * i.out_w
            t, ptr = _guarded(torch, dev, ne, fmt)
            p.convolve_packed_device(n, ker_d.data_ptr(), kh, kw, ptr)
            p.synchronize()
            bits = _unguard(t, ne, fmt)
            with np.errstate(over="ignore"):
                out["fmt%d" % fmt] = _differ(bits, win, fmt)
            if fmt == 1:
                out["fp16_infs"] = int((bits.view(np.uint16) == 0x7c00).sum())
        p.set_option("map_format", 0)
        p.set_option("output_region", 2)
        i = p.refresh_info()
        got = N._ncc_window(torch, dev, p, n, ker_d, n, kh, kw)
        out["region2"] = ((i.out_h, i.out_w), _differ(got, _crop(win, ((kh - 1) // 2, (kw - 1) // 2, H, W)), 0))
        rect = (3, 5, 271, 271)
        p.set_output_rect(*rect)
        direct, fused = p.get_option("rect_direct"), p.get_option("norm_direct")
        got = N._ncc_window(torch, dev, p, n, ker_d, n, kh, kw)
        out["rect"] = (direct, fused, _differ(got, _crop(win, rect), 0))
        for fmt in (0, 1):       # host maps through convolve, the rectangle still set
            p.set_option("map_format", fmt)
            outs = p.convolve(ks)
            got = np.stack([np.ascontiguousarray(o.T) for o in outs])
            with np.errstate(over="ignore"):
                out["host%d" % fmt] = _differ(got if fmt == 0 else got.view(np.uint16), _crop(win, rect), fmt)
        p.set_option("map_format", 0)
        p.set_option("output_region", 0)
        other_d = _pack_t(torch, [np.asfortranarray(3.0 * k + 1.0).astype(np.float32) for k in ks]).to(dev)
        for defer in (0, 1):
            # another set first, so that the constants of THIS set are the ones the prepared column spectra must find again
            N._ncc_window(torch, dev, p, n, other_d, n, kh, kw)
            p.set_option("defer_prepare", defer)
            p.prepare_kernels_packed_device(n, ker_d.data_ptr(), kh, kw)
            pending = p.get_option("prepare_pending")
            if defer:
                p.set_image_device(img_d.data_ptr())       # the deferred column pass rides in the image's
            got = N._ncc_window(torch, dev, p, n, ker_d, n, kh, kw)
            out["prepare%d" % defer] = (pending, _differ(got, win, 0))
        p.set_option("defer_prepare", 0)
        # score 2 is a kernel preparation and nothing else: its rectangle is stored by the output kernel itself
        p.set_match_score(2, kh, kw)
        p.set_image_device(img_d.data_ptr())
        win2 = N._ncc_window(torch, dev, p, n, ker_d, n, kh, kw)
        p.set_output_rect(*rect)
        p.set_option("verbose", 1)
        got, log = _logged(lambda: N._ncc_window(torch, dev, p, n, ker_d, n, kh, kw))
        p.set_option("verbose", 0)
        out["ccoeff_rect"] = (p.get_option("rect_direct"), p.get_option("norm_direct"), _differ(got, _crop(win2, rect), 0), "normalisation:" in log)
    return out


def _case_batch(walk):
    """B = 3 images of different gain and offset, image-major maps; batch_maps 3 cuts a launch inside an image"""
    torch, fc, dev = N._ctx()
    shape = H, W, F, kh, kw = (250, 250, 1, 31, 31)
    n, B = 2, 3
    imgs, ks = [], None
    for b in range(B):
        img, k = N.inputs(shape, n, 31 + b)
        imgs.append(np.asfortranarray((np.float32(1.0 + 2.5 * b) * img + np.float32(7.0 * b)).astype(np.float32)))
        ks = ks or k
    ker_d = _pack_t(torch, ks).to(dev)
    with fc.Plan(H, W, F, kh, kw) as p:
        i = p.info
        p.set_option("image_walk", walk)
        p.set_match_score(4, kh, kw)
        p.set_images(np.asfortranarray(np.stack([im[:, :, 0] for im in imgs], axis=2)))
        active = p.get_option("image_walk_active")
        p.set_option("norm_store", 0)
        not_fused = p.get_option("norm_direct")
        staged = N._ncc_window(torch, dev, p, B * n, ker_d, n, kh, kw)
        p.set_option("norm_store", 1)
        fused = p.get_option("norm_direct")
        got = N._ncc_window(torch, dev, p, B * n, ker_d, n, kh, kw)
        p.set_option("batch_maps", 3)
        got3 = N._ncc_window(torch, dev, p, B * n, ker_d, n, kh, kw)
        p.set_option("norm_store", 0)
        staged3 = N._ncc_window(torch, dev, p, B * n, ker_d, n, kh, kw)
    res = []
    for b in range(B):
        ref, bound, zero, slack_ok = score_reference(4, imgs[b], ks, i.fft_h, i.fft_w, 0)
        res.append((slack_ok, excess_of(got[b * n:(b + 1) * n], ref, bound, zero), excess_of(got3[b * n:(b + 1) * n], ref, bound, zero)))
    return {"active": active, "images": res, "fused": (fused, not_fused), "fused_vs_staged": (_differ(got, staged, 0), _differ(got3, staged3, 0))}


def _case_surface():
    torch, fc, dev = N._ctx()
    shape = H, W, F, kh, kw = (250, 250, 1, 31, 31)
    n = 2
    img, ks = N.inputs(shape, n, 43)
    img_d, ker_d = _image_t(torch, img).to(dev), _pack_t(torch, ks).to(dev)
    small_d = torch.zeros((n, 1, 9, 9), dtype=torch.float32, device=dev)
    out = {}

    def refused(fn, word=""):
        try:
            fn()
            return None
        except fc.FFTConvError as e:
            return (e.status, word in str(e))

    with fc.Plan(H, W, F, kh, kw) as p:
        p.set_image_device(img_d.data_ptr())
        fresh = N._ncc_window(torch, dev, p, n, ker_d, n, kh, kw)
        out["fresh_state"] = _state(p)
        bad = [(5, 31, 31), (-1, 31, 31)] + [(s,) + box for s in (2, 3, 4) for box in ((0, 31), (31, 0), (32, 31), (31, 32))]
        out["bad"] = [refused(lambda a=a: p.set_match_score(*a)) for a in bad]
        out["bad_normalisation"] = [refused(lambda a=a: p.set_normalisation(*a)) for a in ((2, 31, 31), (3, 31, 31), (4, 31, 31))]
        out["after_bad"] = _state(p)
        p.set_match_score(0)                                             # changes nothing: the image stays
        out["noop0"] = _state(p)
        p.set_normalisation(1, kh, kw)
        p.set_image_device(img_d.data_ptr())
        p.set_match_score(1, kh, kw)                                     # one state: a no-op, the image stays
        out["noop1"] = _state(p)
        ncc = N._ncc_window(torch, dev, p, n, ker_d, n, kh, kw)
        out["ncc_peak"] = float(np.abs(ncc).max())
        states = {}
        for score in (2, 3, 4):
            p.set_match_score(score, kh, kw)
            dropped = _state(p)                                          # a changed score: the image is gone
            no_image = refused(lambda: N._ncc_window(torch, dev, p, n, ker_d, n, kh, kw))
            p.set_image_device(img_d.data_ptr())
            p.set_match_score(score, kh, kw)                             # changes nothing
            i = p.info
            t, ptr = _guarded(torch, dev, n * i.fft_h * i.fft_w, 0)
            states[score] = {
                "dropped": dropped, "no_image": no_image, "kept": _state(p),
                "other_size_packed": refused(lambda: p.convolve_packed_device(n, small_d.data_ptr(), 9, 9, ptr), "box"),
                "other_size_prepare": refused(lambda: p.prepare_kernels_packed_device(n, small_d.data_ptr(), 9, 9), "box"),
                "ragged": refused(lambda: p.convolve([ks[0], np.zeros((9, 9, 1), dtype=np.float32)]), "box"),
                "border": refused(lambda: p.set_border(fc.BORDER_REPLICATE)),
                "mark": refused(lambda: p.mark_spectrum_valid(), "statistics"),
                "after": _state(p)}
        out["scores"] = states
        p.set_match_score(3, kh, kw - 1)                                 # another box: the image is dropped
        out["new_box"] = _state(p)
        p.set_normalisation(0)                                           # the other entry switches the score off
        out["off"] = _state(p)
        p.set_image_device(img_d.data_ptr())
        out["off_is_fresh"] = _differ(N._ncc_window(torch, dev, p, n, ker_d, n, kh, kw), fresh, 0)
        p.set_border(fc.BORDER_REPLICATE)
        out["under_border"] = [refused(lambda s=s: p.set_match_score(s, kh, kw), "border") for s in (2, 3, 4)]
        out["border_state"] = (p.get_option("match_score"), p.get_option("border_mode"))
    with fc.Plan(600, 600, 1, 9, 9, options={"max_transform": 512}) as p:
        out["blockwise"] = (p.get_option("blockwise") > 0, [refused(lambda s=s: p.set_match_score(s, 9, 9), "block-wise") for s in (2, 3, 4)],
                            p.get_option("match_score"))
    return out


def _case_graph():
    """test_ncc_gpu._case_graph under score 4: a captured warm set_image(DEVICE) + convolve_packed replayed with new inputs"""
    torch, fc, dev = N._ctx()
    shape = H, W, F, kh, kw = (840, 270, 1, 13, 11)           # M = 432: the tile queue, whose counters every launch must leave at zero
    n = 3
    sets = [N.inputs(shape, n, 90 + k) for k in range(3)]
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream), fc.Plan(H, W, F, kh, kw, stream=stream.cuda_stream) as p:
        p.set_match_score(4, kh, kw)
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
        direct = p.get_option("norm_direct")
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
        ref, bound, zero, slack_ok = score_reference(4, sets[r + 1][0], sets[r + 1][1], i.fft_h, i.fft_w, 0)
        defs.append((slack_ok, excess_of(want[r], ref, bound, zero)))
    return ([_differ(a, b, 0) for a, b in zip(got, want)], defs, bool(np.array_equal(got[0], got[1])), same_ws, direct)


# ---- the tests

@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("name", list(N.KINDS))
def test_parity_with_the_table(device, name, flip):
    """scores 2, 3 and 4 with three kernels (the second one all zeros) on every kind of plan, convolution and correlation"""
    res = device("_case_parity", name, flip)
    print(name, "flip_kernels", flip, res)
    shape = N.KINDS[name][0]
    for score in (2, 3, 4):
        r = res[score]
        assert r["state"] == (score, 0, shape[3], shape[4], 0)
        assert r["slack_ok"], "E = 0 must hold exactly where no data lies under the box"
        worst, nonzero, compared = r["excess"]
        assert compared == r["size"] and worst <= 1.0 and nonzero == 0, (score, r)
        if score in (2, 3):
            assert r["zero_kernel"] == (0.0, 0.0)                       # a zero kernel gives a zero map
        else:
            assert r["zero_kernel"][0] >= 0.0 and r["zero_kernel"][1] == np.float32(r["q_max"])      # ... and E itself under score 4
        if score == 2:
            assert r["direct"] == 0
    spec, lh, fft_h = res["kinds"]
    if name.startswith("specialised"):
        assert spec == 3 and fft_h == 288 and res[3]["direct"] == 1 and res[4]["direct"] == 1
    if name == "generic":
        assert spec != 3 and res[4]["direct"] == 0
    if name == "Bluestein":
        assert spec == 0 and (lh, fft_h) == (304, 304) and res[4]["direct"] == 0


def test_properties(device):
    res = device("_case_properties")
    print(res)
    assert res["slack_ok"] and res["near"] == 0
    for score in (2, 3, 4):
        worst, nonzero, compared = res["excess%d" % score]
        assert worst <= 1.0 and nonzero == 0 and compared == 2 * 288 * 288
    assert res["sqdiff_at"] <= 1.0 and res["sqdiff_argmin"] == res["at"]      # 0 where the template was cut, and least there
    assert res["sqdiff_below"] <= 1.0                                          # nothing below -bound
    assert res["ccorr_at"] <= 1.0 and res["ccorr_over"] <= 1.0                 # 1 there, nowhere above 1 + bound
    assert res["ccoeff_vs_ncc"] <= 1.0 and res["flat_windows"] > 0      # (every valid element compared: D > 0 through the ncc map, D = 0 against 0)
    assert res["gain3"] <= 1.0                                                 # 3.7 I against 0.5 T: within twice the bound
    print("score 4 under the same gain moves by %.3g times twice its bound: SQDIFF is not invariant to gain" % res["gain4"])
    assert res["gain4"] > 1.0


@pytest.mark.parametrize("M", [m for m, _ in col_configs()])
def test_sqdiff_fused_equals_staged_bit_for_bit(device, M):
    """the fused kernels and the staged pair do the same two fp32 adds in the same order: every configuration is held to
    bit-equality, both tile deals, the whole window and an odd rectangle.  "norm_direct" reads 1 with "norm_store" 1 except for the
    configurations listed as not built, which read 0 and run the staged route twice."""
    res = device("_case_fused", M, 4)
    print(M, res)
    built = M not in sqdiff_not_built()
    assert set(res) == {(dyn, rect) for dyn in (0, 1) for rect in (False, True)}
    for key, (direct1, direct0, differ, lines1, lines0, bad, peak) in res.items():
        assert (direct1, direct0) == (1 if built else 0, 0), (M, key)
        assert differ == 0 and bad == 0 and peak > 1.0, (M, key, differ, bad, peak)
        assert lines1 == ((True, False) if built else (False, True)) and lines0 == (False, True), (M, key, lines1, lines0)


@pytest.mark.parametrize("M", [144, 432])
def test_ccorr_normed_fused_equals_staged_bit_for_bit(device, M):
    """score 3 runs the NORM kernels, already held per configuration: one case on the static default and one on the queue's"""
    res = device("_case_fused", M, 3)
    print(M, res)
    for key, (direct1, direct0, differ, lines1, lines0, bad, peak) in res.items():
        assert (direct1, direct0) == (1, 0) and differ == 0 and bad == 0 and 0.05 < peak <= 1.0 + 1e-4, (M, key, res[key])
        assert lines1 == (True, False) and lines0 == (False, True), (M, key)


@pytest.mark.parametrize("score", [4, 3])
def test_composition(device, score):
    res = device("_case_composition", score)
    print(res)
    worst, nonzero, compared = res["window"]
    assert res["slack_ok"] and worst <= 1.0 and nonzero == 0 and compared == 3 * 288 * 288
    assert res["fmt1"] == 0 and res["fmt2"] == 0                        # the rounded fp32 score, bit for bit
    if score == 4:
        assert res["fp16_overflows"] and res["fp16_infs"] > 0           # +inf where fp16 overflows, on both sides
    assert res["region2"] == ((250, 250), 0)
    assert res["rect"] == (0, 1, 0)
    assert res["host0"] == 0 and res["host1"] == 0
    assert res["prepare0"] == (0, 0) and res["prepare1"] == (1, 0)
    assert res["ccoeff_rect"] == (1, 0, 0, False)


@pytest.mark.parametrize("walk", [0, 1])
def test_image_batch(device, walk):
    res = device("_case_batch", walk)
    print(res)
    assert res["active"] == walk
    assert res["fused"] == (1, 0) and res["fused_vs_staged"] == (0, 0)
    for slack_ok, whole, cut in res["images"]:
        assert slack_ok
        assert whole[0] <= 1.0 and cut[0] <= 1.0 and whole[2] == cut[2] == 2 * 288 * 288, res


def test_surface(device):
    out = device("_case_surface")
    print(out)
    assert out["fresh_state"] == (0, 0, 0, 0, 1)
    assert out["bad"] == [(-1, True)] * 14 and out["bad_normalisation"] == [(-1, True)] * 3 and out["after_bad"] == (0, 0, 0, 0, 1)
    assert out["noop0"] == (0, 0, 0, 0, 1)
    assert out["noop1"] == (1, 1, 31, 31, 1) and 0.05 < out["ncc_peak"] <= 1.0 + 1e-4
    for score, s in out["scores"].items():
        assert s["dropped"] == (score, 0, 31, 31, 0) and s["no_image"] == (-9, True)
        assert s["kept"] == (score, 0, 31, 31, 1) and s["after"] == s["kept"], (score, s)
        for key in ("other_size_packed", "other_size_prepare", "ragged"):
            assert s[key] == (-1, True), (score, key, s[key])
        assert s["border"] == (-1, True)
        assert s["mark"] == (None if score == 2 else (-1, True)), (score, s["mark"])
    assert out["new_box"] == (3, 0, 31, 30, 0)
    assert out["off"] == (0, 0, 0, 0, 0) and out["off_is_fresh"] == 0      # the bits of a fresh plan
    assert out["under_border"] == [(-1, True)] * 3 and out["border_state"][0] == 0 and out["border_state"][1] != 0
    assert out["blockwise"] == (True, [(-1, True)] * 3, 0)


def test_graph_replay(device):
    replay_vs_eager, defs, same_twice, same_ws, direct = device("_case_graph")
    print(replay_vs_eager, defs, same_twice, same_ws, direct)
    assert direct == 1 and replay_vs_eager == [0, 0]
    for slack_ok, (worst, nonzero, compared) in defs:
        assert slack_ok and worst <= 1.0 and nonzero == 0
    assert not same_twice and same_ws
