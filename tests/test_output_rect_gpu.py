"""Result maps of any rectangle of the window (fftconv_plan_set_output_rect) on the GPU.

The yardstick is always the plan's own "output_region" 0 fp32 maps -- the path the rest of the suite pins to the float64 oracle --
cropped in NumPy (16-bit formats: converted by test_map_format_gpu.to_bits).  A rectangle map must equal that BIT FOR BIT: the
output kernel does the same arithmetic and only stores elsewhere, so no tolerance is involved.  One case is also held against the
float64 oracle at the project's 1e-4 bar.

Every case reads from the plan (read-only option "rect_direct") and from its verbose log which route it ran: the output kernel
storing the rectangle itself ("output kernel: tiled rectangle, ..."), or the window staged in fp32 and cropped ("output
rectangle: ... cropped ...").  Every configuration of the specialised output kernel has a case of its own
(test_every_configuration_is_bit_equal).  Device map buffers carry a poisoned guard band in front and behind.  The cases run in a spawned
child (test_accuracy_gpu._Child), which exits with the module."""
import re

import numpy as np
import pytest

import golden_util
import util
from test_accuracy_gpu import _Child
from test_features_gpu import _logged
from test_map_format_gpu import ROUTES, SCALES, _image_t, _inputs, _pack_t, to_bits

pytestmark = pytest.mark.gpu

GUARD = 64                   # elements in front of and behind a device map buffer that must stay untouched
POISON16 = 0x7E5A            # a NaN in both 16-bit formats
FMT_NAMES = {0: "fp32", 1: "fp16", 2: "bf16"}
SHAPE_288 = (270, 272, 1, 13, 11, 5)          # 288 x 288 window, M = 144, T = 16, exact_window


def rect_list(fft_h, T):
    """the rectangles of a 288-column window (off_h, off_w, out_h, out_w); fft_h = 288, T = 16: the list of the 288 x 288 window"""
    return [(0, 0, fft_h, 288),             # whole window
            (6, 5, fft_h - 18, 272),        # "same"
            (12, 10, fft_h - 30, 262),      # "valid"
            (1, 0, fft_h - 1, 288),         # odd offset, odd pitch
            (5, 3, fft_h - 6, 283),         # odd, odd, even pitch, odd width
            (7, T + 1, 33, 1),              # one column
            (3, T - 1, 1, 2),               # one row across a tile boundary
            (0, T, 2, T),                   # exactly one tile, one pair
            (fft_h - 1, 287, 1, 1),         # last element
            (2, 2 * T, 4, 3 * T)]           # all even and tile-aligned: the wide-store case


# name: (H, W, F, kh, kw, maps), creation options, plan options, transform length along h, tile width, "dynamic_tiles", rectangle
# (odd offset, odd pitch)
LAUNCH_SHAPES = {
    "T = 16, dynamic queue": ((840, 270, 1, 13, 11, 3), {}, {}, 864, 16, 1, (7, 3, 831, 271)),
    "window shorter than the transform": ((1060, 270, 1, 20, 11, 3), {}, {}, 1152, 16, 1, (1001, 9, 87, 21)),
    "T = 8, dynamic queue": ((4200, 270, 1, 13, 11, 2), {}, {}, 4224, 8, 1, (5, 3, 4201, 271)),
    "T = 8, static deal": ((4200, 270, 1, 13, 11, 2), {}, {"dynamic_tiles": 0}, 4224, 8, 0, (5, 3, 4201, 271)),
    "T = 4": ((5100, 270, 1, 13, 11, 2), {"blockwise": 1}, {}, 5120, 4, 1, (3, 5, 5101, 269)),
    "F = 3": ((270, 272, 3, 13, 11, 5), {"exact_window": 1}, {}, 288, 16, 0, (1, 2, 281, 283)),
}
# name: shape, creation options, rectangle, formats
FALLBACKS = {
    "kernel_path 1": (SHAPE_288, {"exact_window": 1, "kernel_path": 1}, (5, 3, 281, 283), (0, 1, 2)),
    "kernel_path 2": (SHAPE_288, {"exact_window": 1, "kernel_path": 2}, (5, 3, 281, 283), (0, 1, 2)),
    "Bluestein": ((282, 282, 1, 23, 23, 3), {"exact_window": 1}, (5, 3, 281, 283), (0, 1, 2)),
    "block-wise": ((600, 600, 1, 9, 9, 3), {"max_transform": 512}, (5, 3, 581, 583), (0,)),
}


def col_configs():
    """[(M, T)] of fast_paths.hpp's X(M, R1, R2, R3, T, NT) rows: every configuration of the specialised output kernel"""
    from test_map_format_gpu import col_table
    return sorted(col_table().items())


NOT_BUILT = (544, 2080)      # configurations whose rectangle kernel would spill (fast_paths.hpp: fast_cols_rect_built): staged route


@pytest.fixture(scope="module")
def device():
    child = _Child(globals())
    yield child
    if child.gone:
        child.kill()
    else:
        child.ex.shutdown(wait=True)


# ---- the child's side

def _ctx():
    import torch
    return torch, util.load_package(), torch.device("cuda", 0)


def _guarded(torch, dev, n_elems, fmt, shift=0):
    """(tensor, pointer of the first map): GUARD + shift poisoned elements, n_elems for the maps, GUARD - shift poisoned elements"""
    ne = GUARD + n_elems + GUARD
    if fmt == 0:
        t = torch.full((ne,), float("nan"), dtype=torch.float32, device=dev)
    else:
        t = torch.full((ne,), POISON16, dtype=torch.int16, device=dev)
    return t, t.data_ptr() + (GUARD + shift) * (4 if fmt == 0 else 2)


def _unguard(t, n_elems, fmt, shift=0):
    """the map elements of a _guarded buffer as fp32 values / uint16 bit patterns; both guard bands must be as they were"""
    a = t.cpu().numpy()
    lo, body, hi = a[:GUARD + shift], a[GUARD + shift:GUARD + shift + n_elems], a[GUARD + shift + n_elems:]
    for band in (lo, hi):
        assert np.isnan(band).all() if fmt == 0 else (band == POISON16).all(), "a guard band beside the maps was written"
    return body if fmt == 0 else body.view(np.uint16)


def _crop(ref, rect):
    """ref [n][fft_w][fft_h] -> [n][out_w][out_h]"""
    oh, ow, h, w = rect
    return np.ascontiguousarray(ref[:, ow:ow + w, oh:oh + h])


def _differ(got, ref_crop, fmt):
    want = ref_crop if fmt == 0 else to_bits(ref_crop, fmt)
    got = np.ascontiguousarray(got).reshape(want.shape)
    if fmt == 0:
        return int((got.view(np.uint32) != want.view(np.uint32)).sum())
    return int((got != want).sum())


def _reference(torch, dev, p, n, ker_d, kh, kw):
    """the plan's output_region 0 fp32 maps [n][fft_w][fft_h] (image already set)"""
    p.set_option("output_region", 0)
    p.set_option("map_format", 0)
    i = p.info
    t, ptr = _guarded(torch, dev, n * i.fft_h * i.fft_w, 0)
    p.convolve_packed_device(n, ker_d.data_ptr(), kh, kw, ptr)
    p.synchronize()
    ref = _unguard(t, n * i.fft_h * i.fft_w, 0).reshape(n, i.fft_w, i.fft_h).copy()
    assert not np.isnan(ref).any()
    return ref


def _run_rect(torch, dev, p, n, ker_d, kh, kw, rect, fmt, shift=0):
    """the packed maps of `rect` in format fmt (flat), the verbose log of the call, rect_direct"""
    p.set_option("map_format", fmt)
    p.set_output_rect(*rect)
    i = p.info
    assert (i.out_h, i.out_w, i.out_map_bytes) == (rect[2], rect[3], rect[2] * rect[3] * (4 if fmt == 0 else 2)), (rect, i.out_h, i.out_w)
    assert p.get_option("output_region") == 5 and (p.get_option("rect_off_h"), p.get_option("rect_off_w")) == rect[:2]
    ne = n * rect[2] * rect[3]
    t, ptr = _guarded(torch, dev, ne, fmt, shift)
    direct = p.get_option("rect_direct")
    p.set_option("verbose", 1)

    def run():
        p.convolve_packed_device(n, ker_d.data_ptr(), kh, kw, ptr)
        p.synchronize()
    _, log = _logged(run)
    p.set_option("verbose", 0)
    return _unguard(t, ne, fmt, shift), log, direct


def _route_line(log, rect, fmt, direct):
    """the log line that names the route and the rectangle"""
    span = r"rows \[%d, %d\) of columns \[%d, %d\)" % (rect[0], rect[0] + rect[2], rect[1], rect[1] + rect[3])
    if direct:
        pat = r"output kernel: tiled rectangle, \d+ workgroups, %s elements, %s" % (FMT_NAMES[fmt], span)
    else:
        pat = r"output rectangle: \d+ maps cropped from the fp32 window, %s, into %s maps" % (span, FMT_NAMES[fmt])
    lines = [ln for ln in log.splitlines() if "output " in ln]
    assert any(re.search(pat, ln) for ln in lines), (pat, lines)
    if direct:
        assert not any("cropped" in ln or "output region" in ln for ln in lines), lines
    else:      # ahead of the crop the output kernel stores the fp32 window
        assert any(re.search(r"output kernel: .*fp32 elements", ln) and "rectangle" not in ln for ln in lines), lines


def _case_values(fmt, rect_store):
    torch, fc, dev = _ctx()
    H, W, F, kh, kw, n = SHAPE_288
    data, ks = _inputs(SHAPE_288, 41)
    img_d, ker_d = _image_t(torch, data).to(dev), _pack_t(torch, ks).to(dev)
    out = []
    with fc.Plan(H, W, F, kh, kw, options={"exact_window": 1}) as p:
        assert (p.info.fft_h, p.info.fft_w, p.info.transform_h) == (288, 288, 288) and p.get_option("rect_store") == 1
        p.set_image_device(img_d.data_ptr())
        ref = _reference(torch, dev, p, n, ker_d, kh, kw)
        p.set_option("rect_store", rect_store)
        for k, rect in enumerate(rect_list(288, 16)):
            got, log, direct = _run_rect(torch, dev, p, n, ker_d, kh, kw, rect, fmt, shift=k & 1)    # (every other buffer only element-aligned)
            assert direct == rect_store, (rect, direct)
            _route_line(log, rect, fmt, direct)
            want = _crop(ref, rect)
            bits = to_bits(want, 1) & 0x7FFF
            out.append((rect, _differ(got, want, fmt), int(((bits > 0) & (bits < 0x400)).sum()), int((bits == 0x7C00).sum())))
        oracle = None
        if fmt == 0 and rect_store == 1:       # the "same" rectangle against the float64 oracle
            rect = (6, 5, 270, 272)
            got, _, _ = _run_rect(torch, dev, p, n, ker_d, kh, kw, rect, 0)
            want = np.stack([np.ascontiguousarray(r.T) for r in util.Oracle().conv_fft(data, kh, kw, ks, f64=True)])
            want = _crop(want, rect)
            got = got.reshape(want.shape)
            oracle = max(util.rel_err(g, w) for g, w in zip(got, want))
    return out, oracle


def _case_launch_shape(name):
    torch, fc, dev = _ctx()
    shape, options, settings, want_lh, want_t, want_dyn, rect = LAUNCH_SHAPES[name]
    H, W, F, kh, kw, n = shape
    data, ks = _inputs(shape, 53 + len(name))
    img_d, ker_d = _image_t(torch, data).to(dev), _pack_t(torch, ks).to(dev)
    out = {}
    with fc.Plan(H, W, F, kh, kw, options=options) as p:
        for key, value in settings.items():
            p.set_option(key, value)
        assert p.get_option("blockwise") == 0 and p.info.transform_h == want_lh and p.get_option("dynamic_tiles") == want_dyn
        assert rect[0] % 2 == 1 and rect[2] % 2 == 1 and rect[0] + rect[2] <= p.info.fft_h and rect[1] + rect[3] <= p.info.fft_w
        p.set_image_device(img_d.data_ptr())
        ref = _reference(torch, dev, p, n, ker_d, kh, kw)
        for fmt in (0, 1, 2):
            got, log, direct = _run_rect(torch, dev, p, n, ker_d, kh, kw, rect, fmt, shift=1)
            assert direct == 1
            _route_line(log, rect, fmt, True)
            grid = int(re.search(r"tiled rectangle, (\d+) workgroups", log).group(1))
            tiles = ((rect[1] + rect[3] + want_t - 1) // want_t - rect[1] // want_t) * n
            assert 1 <= grid <= tiles, (grid, tiles)
            out[fmt] = _differ(got, _crop(ref, rect), fmt)
    return out


def _case_configuration(M):
    """an exact_window plan whose transform along h is 2M points on a 288-column window, two maps: an odd-offset, odd-pitch
    rectangle in fp32 and fp16, static deal and dynamic queue, against the plan's own cropped window"""
    torch, fc, dev = _ctx()
    kh, kw, n = 13, 11, 2
    shape = (2 * M - 18, 272, 1, kh, kw, n)
    data, ks = _inputs(shape, 7 + M)
    img_d, ker_d = _image_t(torch, data).to(dev), _pack_t(torch, ks).to(dev)
    rect = (3, 5, 2 * M - 17, 271)
    out = {}
    with fc.Plan(shape[0], shape[1], 1, kh, kw, options={"exact_window": 1, "blockwise": 1}) as p:
        assert p.get_option("blockwise") == 0 and (p.info.fft_h, p.info.fft_w, p.info.transform_h) == (2 * M, 288, 2 * M)
        assert p.get_option("specialised_kernels") == 3
        p.set_image_device(img_d.data_ptr())
        ref = _reference(torch, dev, p, n, ker_d, kh, kw)
        for dyn in (0, 1):
            p.set_option("dynamic_tiles", dyn)
            for fmt in (0, 1):
                got, log, direct = _run_rect(torch, dev, p, n, ker_d, kh, kw, rect, fmt, shift=1)
                _route_line(log, rect, fmt, direct)
                out[(dyn, fmt)] = (direct, _differ(got, _crop(ref, rect), fmt))
    return out


def _case_route(route):
    """every delivery route hands out the bytes of the cropped reference; pointer-per-map destinations are one element off an
    8-byte (fp32) / 4-byte (fp16) boundary"""
    torch, fc, dev = _ctx()
    small = route == "pinned small call"
    if small:
        data, _, _, ks, _ = golden_util.load_case("case_demo")        # 64 x 8 x 5, three 10 x 4 x 5 kernels: 80 x 16 window
        data, ks = np.asfortranarray(data), [np.asfortranarray(k) for k in ks]
        H, W, F = data.shape
        kh, kw, n, options, rect = 10, 4, len(ks), {}, (1, 1, 77, 13)
    else:
        H, W, F, kh, kw, n = shape = SHAPE_288
        data, ks = _inputs(shape, 77)
        options, rect = {"exact_window": 1}, (5, 3, 281, 283)
    res = {}
    with fc.Plan(H, W, F, kh, kw, options=options) as p:
        if route.startswith("host_stream"):
            p.set_option("host_min_kb", 0)
            p.set_option("host_stream", int(route[-1]))
            p.set_option("batch_maps", 2)            # three batches: both staging buffers of the streamed routes are reused
        if route == "host_pinned 0":
            p.set_option("host_pinned", 0)
        p.set_image(data)
        ref = np.stack([np.ascontiguousarray(o.T) for o in p.convolve(ks)])
        assert ref.shape == (n, p.info.fft_w, p.info.fft_h)
        want = _crop(ref, rect)
        ne = rect[2] * rect[3]
        for fmt in (0, 1):
            p.set_option("map_format", fmt)
            p.set_output_rect(*rect)
            res["direct"] = p.get_option("rect_direct")
            if route == "device pointers":
                bufs = [_guarded(torch, dev, ne, fmt, shift=1) for _ in range(n)]
                assert all(ptr % (8 if fmt == 0 else 4) != 0 for _, ptr in bufs)
                p.convolve_to_device(ks, [ptr for _, ptr in bufs])
                p.synchronize()
                got = np.stack([_unguard(t, ne, fmt, shift=1) for t, _ in bufs])
            else:
                outs = p.convolve(ks)
                assert all(o.dtype == fc.MAP_DTYPES[fmt] and o.shape == (rect[2], rect[3]) for o in outs)
                got = np.stack([np.ascontiguousarray(o.T) for o in outs])
                got = got if fmt == 0 else got.view(np.uint16)
            res[fmt] = _differ(got, want, fmt)
    return res


def _case_fallback(name):
    torch, fc, dev = _ctx()
    shape, options, rect, formats = FALLBACKS[name]
    H, W, F, kh, kw, n = shape
    data, ks = _inputs(shape, 61 + len(name))
    img_d, ker_d = _image_t(torch, data).to(dev), _pack_t(torch, ks).to(dev)
    out = {}
    with fc.Plan(H, W, F, kh, kw, options=options) as p:
        assert (p.get_option("blockwise") > 0) == (name == "block-wise")
        p.set_image_device(img_d.data_ptr())
        ref = _reference(torch, dev, p, n, ker_d, kh, kw)
        for fmt in formats:
            got, log, direct = _run_rect(torch, dev, p, n, ker_d, kh, kw, rect, fmt)
            assert direct == 0 and p.get_option("rect_store") == 1
            if name == "block-wise":       # (the blocks' own launches are in the log too)
                assert "output rectangle: %d maps cropped from the fp32 window" % n in log, log
            else:
                _route_line(log, rect, fmt, False)
            assert "tiled rectangle" not in log
            out[fmt] = _differ(got, _crop(ref, rect), fmt)
    return out


def _case_surface():
    torch, fc, dev = _ctx()
    H, W, F, kh, kw, n = shape = (271, 273, 1, 12, 10, 3)       # the shape of the map-format test's named regions: 288 x 288 window
    data, ks = _inputs(shape, 19)
    img_d, ker_d = _image_t(torch, data).to(dev), _pack_t(torch, ks).to(dev)
    out = {}
    with fc.Plan(H, W, F, kh, kw) as p:
        p.set_image_device(img_d.data_ptr())
        out["fresh"] = (p.get_option("output_region"), p.get_option("rect_off_h"), p.get_option("rect_off_w"), p.get_option("rect_direct"), p.get_option("rect_store"))
        p.set_output_rect(7, 9, 33, 21)
        i = p.info
        out["set"] = (i.out_h, i.out_w, i.out_map_bytes, p.get_option("output_region"), p.get_option("rect_off_h"), p.get_option("rect_off_w"), p.get_option("rect_direct"))
        errors = []
        for bad in ((0, 0, 289, 1), (0, 0, 1, 289), (288, 0, 1, 1), (-1, 0, 5, 5), (0, -1, 5, 5), (0, 0, 0, 5), (0, 0, 5, -2), (280, 280, 9, 9)):
            try:
                p.set_output_rect(*bad)
                errors.append(None)
            except fc.FFTConvError as e:
                errors.append((e.status, "288 x 288 window" in str(e)))
        try:
            p.set_option("output_region", 5)
            errors.append(None)
        except fc.FFTConvError as e:
            errors.append((e.status, "fftconv_plan_set_output_rect" in str(e)))
        out["errors"] = errors
        i = p.info
        out["kept"] = (i.out_h, i.out_w, p.get_option("output_region"), p.get_option("rect_off_h"), p.get_option("rect_off_w"))
        p.set_option("map_format", 1)
        out["fp16"] = p.info.out_map_bytes
        p.set_option("map_format", 0)
        p.set_option("rect_store", 0)
        out["store0"] = (p.get_option("rect_store"), p.get_option("rect_direct"))
        p.set_option("rect_store", 1)
        # a named region afterwards is the named region again, with its log line
        p.set_option("output_region", 2)
        i = p.info
        out["region2"] = (i.out_h, i.out_w, p.get_option("output_region"), p.get_option("rect_off_h"), p.get_option("rect_direct"))
        t, ptr = _guarded(torch, dev, n * H * W, 0)
        p.set_option("verbose", 1)

        def run():
            p.convolve_packed_device(n, ker_d.data_ptr(), kh, kw, ptr)
            p.synchronize()
        _, log = _logged(run)
        p.set_option("verbose", 0)
        out["region2_log"] = bool(re.search(r"output region 2: .* cropped .* 271 x 273", log)) and "rectangle" not in log
        same = _unguard(t, n * H * W, 0).reshape(n, W, H).copy()
        # ... and the rectangle that IS "same" returns the same bytes
        got, _, direct = _run_rect(torch, dev, p, n, ker_d, kh, kw, ((kh - 1) // 2, (kw - 1) // 2, H, W), 0)
        out["same_rect"] = (direct, _differ(got, same, 0))
    # workspace: a direct-rectangle plan holds no full-window staging O
    ws = {}
    for store in (1, 0):
        with fc.Plan(H, W, F, kh, kw) as p:
            p.set_image_device(img_d.data_ptr())
            p.set_option("rect_store", store)
            _run_rect(torch, dev, p, n, ker_d, kh, kw, (7, 9, 33, 21), 0)
            i = p.info
            ws[store] = (i.workspace_bytes, n * i.fft_h * i.fft_w * 4)
    out["workspace"] = ws
    return out


def _case_tuning():
    """tune_placement 2 on a direct-rectangle plan: the tuner's probe launches write into the caller's tight buffer"""
    torch, fc, dev = _ctx()
    H, W, F, kh, kw, n = SHAPE_288
    data, ks = _inputs(SHAPE_288, 23)
    img_d, ker_d = _image_t(torch, data).to(dev), _pack_t(torch, ks).to(dev)
    rect = (7, 17, 33, 40)
    with fc.Plan(H, W, F, kh, kw, options={"exact_window": 1}) as p:
        p.set_image_device(img_d.data_ptr())
        ref = _reference(torch, dev, p, n, ker_d, kh, kw)
    res = {}
    for fmt in (0, 1):
        with fc.Plan(H, W, F, kh, kw, options={"exact_window": 1}) as p:      # a fresh intermediate: the tuner runs in the first convolve
            p.set_option("tune_placement", 2)
            p.set_image_device(img_d.data_ptr())
            got, log, direct = _run_rect(torch, dev, p, n, ker_d, kh, kw, rect, fmt, shift=1)
            res[fmt] = (direct, p.get_option("tuned_candidates"), _differ(got, _crop(ref, rect), fmt))
    return res


def _case_graph():
    """set_image(DEVICE) + convolve_packed with a rectangle, captured after one eager warm-up step and replayed with new inputs:
    bit-equal to the eager step on the same inputs"""
    torch, fc, dev = _ctx()
    shape = (840, 270, 1, 13, 11, 3)          # M = 432: the tile queue, whose counters every launch must leave at zero
    H, W, F, kh, kw, n = shape
    rect = (7, 3, 831, 271)
    sets = [_inputs(shape, 90 + k) for k in range(3)]
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream), fc.Plan(H, W, F, kh, kw, stream=stream.cuda_stream) as p:
        p.set_output_rect(*rect)
        assert p.get_option("blockwise") == 0 and p.get_option("dynamic_tiles") == 1 and p.get_option("rect_direct") == 1
        ne = n * rect[2] * rect[3]
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
        ws = p.info.workspace_bytes
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
        same_ws = p.info.workspace_bytes == ws
        # the eager maps against the cropped window of the same plan
        refs = []
        for r in range(2):
            img_d.copy_(imgs_h[r + 1], non_blocking=True)
            ker_d.copy_(kers_h[r + 1], non_blocking=True)
            p.set_image_device(img_d.data_ptr())
            refs.append(_differ(want[r], _crop(_reference(torch, dev, p, n, ker_d, kh, kw), rect), 0))
    return ([_differ(a, b, 0) for a, b in zip(got, want)], refs, bool(np.array_equal(got[0], got[1])), same_ws,
            [int(np.isnan(a).sum()) for a in got])


# ---- the tests

@pytest.mark.parametrize("rect_store", [1, 0])
@pytest.mark.parametrize("fmt", [0, 1, 2])
def test_rectangle_maps_are_the_cropped_window(device, fmt, rect_store):
    """the ten rectangles of the 288 x 288 window, 5 maps whose scales reach both ends of fp16: packed device output, both routes"""
    res, oracle = device("_case_values", fmt, rect_store)
    assert [r[0] for r in res] == rect_list(288, 16)
    for rect, differ, sub, inf in res:
        print("rectangle %s, %s, rect_store %d: %d elements differ (%d fp16-subnormal, %d fp16-inf values in it)" % (rect, FMT_NAMES[fmt], rect_store, differ, sub, inf))
        assert differ == 0, (rect, differ)
    assert res[0][2] > 0 and res[0][3] > 0            # the window really reaches both ends of fp16
    if oracle is not None:
        print("\"same\" rectangle against the float64 oracle: max |out - ref| / max |ref| = %.3g" % oracle)
        assert oracle < 1e-4


@pytest.mark.parametrize("name", list(LAUNCH_SHAPES))
def test_launch_shapes(device, name):
    res = device("_case_launch_shape", name)
    print(name, res)
    assert res == {0: 0, 1: 0, 2: 0}, (name, res)


@pytest.mark.parametrize("M", [m for m, _ in col_configs()])
def test_every_configuration_is_bit_equal(device, M):
    """the rectangle kernels and the plain kernels are separate instantiations, and their arithmetic is only equal if the
    compiler fuses the same multiply-adds in both: every built configuration is held to bit-equality with its plain sibling,
    both variants, fp32 and fp16.  The two configurations that are not built read rect_direct 0 and return the same bytes."""
    res = device("_case_configuration", M)
    print(M, res)
    want = 0 if M in NOT_BUILT else 1
    assert res == {(dyn, fmt): (want, 0) for dyn in (0, 1) for fmt in (0, 1)}, (M, res)


@pytest.mark.parametrize("route", ROUTES)
def test_delivery_routes(device, route):
    res = device("_case_route", route)
    print(route, res)
    assert res[0] == 0 and res[1] == 0, (route, res)
    assert res["direct"] == (0 if route == "pinned small call" else 1)       # (the demo fixture's 80 x 16 window has no specialised kernel)


@pytest.mark.parametrize("name", list(FALLBACKS))
def test_fallbacks_return_the_same_bytes(device, name):
    res = device("_case_fallback", name)
    print(name, res)
    assert res and all(v == 0 for v in res.values()), (name, res)


def test_surface(device):
    out = device("_case_surface")
    print(out)
    assert out["fresh"] == (0, 0, 0, 0, 1)
    assert out["set"] == (33, 21, 33 * 21 * 4, 5, 7, 9, 1)
    assert out["errors"] == [(-1, True)] * 9, out["errors"]
    assert out["kept"] == (33, 21, 5, 7, 9)                       # argument errors left the rectangle in place
    assert out["fp16"] == 33 * 21 * 2
    assert out["store0"] == (0, 0)
    assert out["region2"] == (271, 273, 2, 0, 0) and out["region2_log"]
    assert out["same_rect"] == (1, 0)
    (ws1, o_bytes), (ws0, _) = out["workspace"][1], out["workspace"][0]
    assert ws0 - ws1 >= o_bytes > 0, out["workspace"]


def test_placement_tuning_probes_the_rectangle(device):
    res = device("_case_tuning")
    print(res)
    for fmt in (0, 1):
        direct, candidates, differ = res[fmt]
        assert direct == 1 and candidates == 2 and differ == 0, res


def test_graph_replay(device):
    replay_vs_eager, eager_vs_window, same_twice, same_ws, nans = device("_case_graph")
    assert replay_vs_eager == [0, 0]               # each replay is the eager step on the same inputs, bit for bit
    assert eager_vs_window == [0, 0] and nans == [0, 0]
    assert not same_twice                          # (and the two replays did see different inputs)
    assert same_ws                                 # nothing was allocated after the warm-up step
