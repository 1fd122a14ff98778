"""Strided result maps (fftconv_plan_set_output_stride) on the GPU.

The yardstick for bit-equality is always the same plan's own stride-(1, 1) maps (a twin plan with the same settings where the
sequence of calls on the plan under test must not be disturbed), sliced [::sh, ::sw] in NumPy.  A strided map must equal that BIT FOR
BIT on both routes: the fused store runs the arithmetic of the plain store and only stores fewer elements elsewhere, the staged crop
only copies (or applies the plane in the fixed order it always had).  The fp32 value cases are also held to the project's bar
|got - ref| <= 1e-5 * max |ref| against the float64 oracle's sliced map.  max |ref| is the maximum of the sliced oracle map, except
for the one-element rectangle (287, 287, 1, 1): that element lies in the zero padding of the window (rows and columns 280 .. 287 of
the 288 x 288 window of 250 + 31 - 1 = 280 samples hold no sample of the linear convolution), the oracle's value there is zero up
to its own rounding and is no scale for anything, so the element is held to 1e-5 of the maximum of the map it was taken from.

Every case reads from the plan (read-only option "stride_direct") and from its verbose log which route it ran: the output kernel
sampling in its store ("... stride (sh, sw) fused in the store ...") or the fp32 window sampled by the crop ("output stride (sh,
sw): staged ...").  Device map buffers carry a poisoned guard band in front and behind (test_output_rect_gpu._guarded).  The cases
run in a spawned child (test_accuracy_gpu._Child), which exits with the module."""
import re

import numpy as np
import pytest

import golden_util
import util
from test_accuracy_gpu import _Child
from test_features_gpu import _logged
from test_map_format_gpu import ROUTES, _image_t, _inputs, _pack_t
from test_output_rect_gpu import _ctx, _guarded, _unguard, col_configs

pytestmark = pytest.mark.gpu

SHAPE = (250, 250, 1, 31, 31, 3)              # 288 x 288 window, M = 144, T = 16
STRIDES = [(2, 2), (3, 5), (1, 17), (4, 1)]
# name: how the extent is set, (off_h, off_w, out_h, out_w) of it in the 288 x 288 window, and whether the fused store can serve it
EXTENTS = {
    "window": (("region", 0), (0, 0, 288, 288), True),
    "rectangle": (("rect", (7, 5, 271, 273)), (7, 5, 271, 273), True),
    "last element": (("rect", (287, 287, 1, 1)), (287, 287, 1, 1), True),
    "region 1": (("region", 1), (0, 0, 280, 280), False),
}
NOT_BUILT = (544, 2080)      # fast_paths.hpp: FC_COLS_STRIDE_NOT_BUILT -- the staged route
COMPOSITIONS = ["score 1", "score 2", "score 3", "score 4", "image batch", "typed uint8", "BORDER_REPLICATE", "image_walk", "block-wise"]


@pytest.fixture(scope="module")
def device():
    child = _Child(globals())
    yield child
    if child.gone:
        child.kill()
    else:
        child.ex.shutdown(wait=True)


# ---- the child's side

def _cdiv(a, b):
    return -(-a // b)


def _set_extent(p, how):
    if how[0] == "region":
        p.set_option("output_region", how[1])
    else:
        p.set_output_rect(*how[1])


def _maps(torch, dev, p, nk, ker_d, kh, kw, shift=0):
    """the plan's packed maps as they are delivered: [images * nk][out_w][out_h] (fp32 values or uint16 bit patterns), and the
    verbose log of the call; info must describe the buffer the call fills, and the guards around it must be intact"""
    i = p.info
    fmt = p.get_option("map_format")
    nm = nk * p.images()
    assert i.out_map_bytes == i.out_h * i.out_w * (4 if fmt == 0 else 2), (i.out_h, i.out_w, i.out_map_bytes)
    ne = nm * i.out_h * i.out_w
    t, ptr = _guarded(torch, dev, ne, fmt, shift)
    p.set_option("verbose", 1)

    def run():
        p.convolve_packed_device(nk, ker_d.data_ptr(), kh, kw, ptr)
        p.synchronize()
    _, log = _logged(run)
    p.set_option("verbose", 0)
    return _unguard(t, ne, fmt, shift).reshape(nm, i.out_w, i.out_h).copy(), log


def _slice(ref, sh, sw):
    """[n][w][h] -> every sw-th column and sh-th row"""
    return np.ascontiguousarray(ref[:, ::sw, ::sh])


def _differ(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    bits = np.uint32 if got.dtype == np.float32 else np.uint16
    return int((np.ascontiguousarray(got).view(bits) != np.ascontiguousarray(want).view(bits)).sum())


def _strided(torch, dev, p, nk, ker_d, kh, kw, stride, shift=0):
    """(stride-(1, 1) maps of the plan as it stands, its maps at `stride`, the log of the strided call, stride_direct); the info
    of the strided plan must be the formulas of the issue"""
    p.set_output_stride(1, 1)
    dense, _ = _maps(torch, dev, p, nk, ker_d, kh, kw)
    uh, uw = p.info.out_h, p.info.out_w
    p.set_output_stride(*stride)
    i = p.info
    eb = 4 if p.get_option("map_format") == 0 else 2
    assert (i.out_h, i.out_w, i.out_map_bytes) == (_cdiv(uh, stride[0]), _cdiv(uw, stride[1]), _cdiv(uh, stride[0]) * _cdiv(uw, stride[1]) * eb), (stride, uh, uw)
    assert (p.get_option("stride_h"), p.get_option("stride_w")) == stride
    direct = p.get_option("stride_direct")
    got, log = _maps(torch, dev, p, nk, ker_d, kh, kw, shift)
    return dense, got, log, direct


def _route_named(log, stride, direct):
    """the verbose log names the stride and the route that ran"""
    lines = [ln for ln in log.splitlines() if "stride" in ln]
    fused = "output kernel: tiled rectangle, stride (%d, %d) fused in the store" % stride
    staged = "output stride (%d, %d): staged" % stride
    if direct:
        assert any(fused in ln for ln in lines) and not any("staged" in ln for ln in lines), lines
    else:
        assert any(staged in ln for ln in lines) and not any("fused in the store" in ln for ln in lines), lines


def _case_values(fmt, stride_store):
    torch, fc, dev = _ctx()
    H, W, F, kh, kw, n = SHAPE
    data, ks = _inputs(SHAPE, 141)
    img_d, ker_d = _image_t(torch, data).to(dev), _pack_t(torch, ks).to(dev)
    oracle = None
    if fmt == 0:
        oracle = np.stack([np.ascontiguousarray(r.T) for r in util.Oracle().conv_fft(data, kh, kw, ks, f64=True)])
    out = []
    with fc.Plan(H, W, F, kh, kw) as p:
        assert (p.info.fft_h, p.info.fft_w) == (288, 288) and p.get_option("stride_store") == 1 and p.get_option("stride_direct") == 0
        assert (p.get_option("stride_h"), p.get_option("stride_w")) == (1, 1)
        p.set_image_device(img_d.data_ptr())
        p.set_option("map_format", fmt)
        p.set_option("stride_store", stride_store)
        for k, (name, (how, ext, fusable)) in enumerate(EXTENTS.items()):
            _set_extent(p, how)
            for stride in STRIDES:
                dense, got, log, direct = _strided(torch, dev, p, n, ker_d, kh, kw, stride, shift=k & 1)
                assert dense.shape == (n, ext[3], ext[2])
                assert direct == (1 if fmt == 0 and stride_store == 1 and fusable else 0), (name, stride, direct)
                _route_named(log, stride, direct)
                err = None
                if oracle is not None:      # |got - ref| / max |ref| per map (the one-element extent: of the map it was taken from)
                    want = _slice(oracle[:, ext[1]:ext[1] + ext[3], ext[0]:ext[0] + ext[2]], *stride)
                    scale = oracle if name == "last element" else want
                    err = max(float(np.abs(g.astype(np.float64) - w).max() / np.abs(s).max()) for g, w, s in zip(got, want, scale))
                out.append((name, stride, _differ(got, _slice(dense, *stride)), err))
    return out


def _case_configuration(M, T):
    """an exact_window plan whose transform along h is 2M points on a 288-column window, two maps: strides (2, 3) on an odd
    rectangle and (1, T + 1) on the window, fused and staged, against the plan's own dense maps sliced"""
    torch, fc, dev = _ctx()
    kh, kw, n = 13, 11, 2
    shape = (2 * M - 18, 272, 1, kh, kw, n)
    data, ks = _inputs(shape, 17 + M)
    img_d, ker_d = _image_t(torch, data).to(dev), _pack_t(torch, ks).to(dev)
    out = {}
    with fc.Plan(shape[0], shape[1], 1, kh, kw, options={"exact_window": 1, "blockwise": 1}) as p:
        assert p.get_option("blockwise") == 0 and (p.info.fft_h, p.info.fft_w, p.info.transform_h) == (2 * M, 288, 2 * M)
        assert p.get_option("specialised_kernels") == 3
        p.set_image_device(img_d.data_ptr())
        for how, stride in ((("rect", (3, 5, 2 * M - 17, 271)), (2, 3)), (("region", 0), (1, T + 1))):
            _set_extent(p, how)
            for store in (1, 0):
                p.set_option("stride_store", store)
                dense, got, log, direct = _strided(torch, dev, p, n, ker_d, kh, kw, stride, shift=1)
                _route_named(log, stride, direct)
                out[(stride, store)] = (direct, _differ(got, _slice(dense, *stride)))
    return out


def _case_composition(name):
    torch, fc, dev = _ctx()
    stride = (2, 3)
    shape, options = SHAPE, {}
    if name == "block-wise":
        shape, options = (600, 600, 1, 9, 9, 3), {"max_transform": 512}
    H, W, F, kh, kw, n = shape
    data, ks = _inputs(shape, 171 + len(name))
    ker_d = _pack_t(torch, ks).to(dev)
    want_direct = 1
    with fc.Plan(H, W, F, kh, kw, options=options) as p:
        assert (p.get_option("blockwise") > 0) == (name == "block-wise")
        if name.startswith("score"):
            score = int(name[-1])
            p.set_match_score(score, kh, kw)
            want_direct = 1 if score == 2 else 0          # a plane is combined by the staged crop, at the window coordinate
        if name == "BORDER_REPLICATE":
            p.set_border(fc.BORDER_REPLICATE)
        if name == "image_walk":
            p.set_option("image_walk", 1)
        if name in ("image batch", "image_walk"):
            rng = np.random.default_rng(5)
            p.set_images(np.asfortranarray(rng.standard_normal((H, W, 3), dtype=np.float32)))
            assert p.images() == 3 and (name != "image_walk" or p.get_option("image_walk_active") == 1)
        elif name == "typed uint8":
            p.set_image_typed(np.asfortranarray(np.random.default_rng(6).integers(0, 256, (H, W), dtype=np.uint8)))
        else:
            p.set_image(data)
        if name == "block-wise":
            want_direct = 0
        if name == "BORDER_REPLICATE":
            assert p.get_option("output_region") == 5 and (p.info.out_h, p.info.out_w) == (H, W)
        dense, got, log, direct = _strided(torch, dev, p, n, ker_d, kh, kw, stride, shift=1)
        assert dense.shape[0] == n * p.images()
        if name == "block-wise":
            assert "output stride (2, 3): staged" in log and "fused in the store" not in log, log
        else:
            _route_named(log, stride, direct)
        # the stride left the image alone: the dense maps again, without another set_image
        p.set_output_stride(1, 1)
        again, _ = _maps(torch, dev, p, n, ker_d, kh, kw)
        return direct, want_direct, _differ(got, _slice(dense, *stride)), _differ(again, dense), int(np.isnan(got).sum())


def _case_route(route):
    """every delivery route hands out the bytes of the sliced dense maps; pointer-per-map destinations are one element off an
    8-byte (fp32) / 4-byte (fp16) boundary"""
    torch, fc, dev = _ctx()
    stride = (2, 3)
    small = route == "pinned small call"
    if small:
        data, _, _, ks, _ = golden_util.load_case("case_demo")        # 64 x 8 x 5, three 10 x 4 x 5 kernels: 80 x 16 window
        data, ks = np.asfortranarray(data), [np.asfortranarray(k) for k in ks]
        H, W, F = data.shape
        kh, kw, n, rect = 10, 4, len(ks), (1, 1, 77, 13)
    else:
        H, W, F, kh, kw, n = shape = SHAPE
        data, ks = _inputs(shape, 177)
        rect = (5, 3, 281, 283)
    res = {}
    with fc.Plan(H, W, F, kh, kw) as p:
        if route.startswith("host_stream"):
            p.set_option("host_min_kb", 0)
            p.set_option("host_stream", int(route[-1]))
            p.set_option("batch_maps", 2)            # two batches: both staging buffers of the streamed routes are used
        if route == "host_pinned 0":
            p.set_option("host_pinned", 0)
        p.set_image(data)
        p.set_output_rect(*rect)
        mh, mw = _cdiv(rect[2], stride[0]), _cdiv(rect[3], stride[1])
        ne = mh * mw
        for fmt in (0, 1):
            p.set_option("map_format", fmt)
            p.set_output_stride(1, 1)
            dense = np.stack([np.ascontiguousarray(o.T) for o in p.convolve(ks)])
            assert dense.shape == (n, rect[3], rect[2])
            want = _slice(dense, *stride)
            p.set_output_stride(*stride)
            res["direct"] = p.get_option("stride_direct") if fmt == 0 else res["direct"]
            if route == "device pointers":
                bufs = [_guarded(torch, dev, ne, fmt, shift=1) for _ in range(n)]
                assert all(ptr % (8 if fmt == 0 else 4) != 0 for _, ptr in bufs)
                p.convolve_to_device(ks, [ptr for _, ptr in bufs])
                p.synchronize()
                got = np.stack([_unguard(t, ne, fmt, shift=1) for t, _ in bufs]).reshape(n, mw, mh)
                want = want if fmt == 0 else want.view(np.uint16)
            else:
                outs = p.convolve(ks)
                assert all(o.dtype == fc.MAP_DTYPES[fmt] and o.shape == (mh, mw) for o in outs)
                got = np.stack([np.ascontiguousarray(o.T) for o in outs])
            res[fmt] = _differ(np.ascontiguousarray(got), np.ascontiguousarray(want))
    return res


def _case_state():
    """one live plan through a fixed sequence, a convolve after every step; a twin plan takes the same steps without any stride and
    supplies the dense maps"""
    torch, fc, dev = _ctx()
    H, W, F, kh, kw, n = SHAPE
    data, ks = _inputs(SHAPE, 191)
    img_d, ker_d = _image_t(torch, data).to(dev), _pack_t(torch, ks).to(dev)
    rng = np.random.default_rng(9)
    batch = torch.from_numpy(np.ascontiguousarray(rng.standard_normal((2, 1, W, H), dtype=np.float32))).to(dev)
    other = torch.cuda.Stream(dev)
    steps = [("stride", (2, 3)), ("rect", (7, 5, 271, 273)), ("stride", (1, 1)), ("region", 2), ("stride", (3, 2)), ("format", 1),
             ("images", 2), ("stride", (2, 2)), ("stream", None)]
    out = []
    with fc.Plan(H, W, F, kh, kw) as p, fc.Plan(H, W, F, kh, kw) as twin:
        p.set_image_device(img_d.data_ptr())
        twin.set_image_device(img_d.data_ptr())
        stride = (1, 1)
        for what, arg in steps:
            for q in (p, twin):
                if what == "stride" and q is p:
                    q.set_output_stride(*arg)
                elif what == "rect":
                    q.set_output_rect(*arg)
                elif what == "region":
                    q.set_option("output_region", arg)
                elif what == "format":
                    q.set_option("map_format", arg)
                elif what == "images":
                    q.set_images_device(batch.data_ptr(), arg)
                elif what == "stream" and q is p:
                    torch.cuda.synchronize()
                    q.set_stream(other.cuda_stream)
            if what == "stride":
                stride = arg
            dense, _ = _maps(torch, dev, twin, n, ker_d, kh, kw)
            got, _ = _maps(torch, dev, p, n, ker_d, kh, kw, shift=1)
            i, u = p.info, twin.info
            eb = 4 if p.get_option("map_format") == 0 else 2
            info_ok = (i.out_h, i.out_w, i.out_map_bytes) == (_cdiv(u.out_h, stride[0]), _cdiv(u.out_w, stride[1]),
                                                              _cdiv(u.out_h, stride[0]) * _cdiv(u.out_w, stride[1]) * eb)
            kept = (p.get_option("stride_h"), p.get_option("stride_w")) == stride and p.get_option("images") == twin.get_option("images")
            out.append((what, arg, info_ok, kept, _differ(got, _slice(dense, *stride))))
        torch.cuda.synchronize()
        # region 4 and a stride refuse each other, whichever comes last, and leave the state as it was
        refusals = []
        before = (p.get_option("output_region"), p.info.out_h, p.info.out_w, p.get_option("stride_h"), p.get_option("stride_w"))
        try:
            p.set_option("output_region", 4)
            refusals.append(None)
        except fc.FFTConvError as e:
            refusals.append((e.status, "output_region 4" in str(e)))
        refusals.append(before == (p.get_option("output_region"), p.info.out_h, p.info.out_w, p.get_option("stride_h"), p.get_option("stride_w")))
        p.set_output_stride(1, 1)
        p.set_option("output_region", 4)
        before = (p.get_option("output_region"), p.info.out_h, p.info.out_w, p.get_option("stride_h"), p.get_option("stride_w"))
        try:
            p.set_output_stride(2, 2)
            refusals.append(None)
        except fc.FFTConvError as e:
            refusals.append((e.status, "output_region 4" in str(e)))
        refusals.append(before == (p.get_option("output_region"), p.info.out_h, p.info.out_w, p.get_option("stride_h"), p.get_option("stride_w")))
        for bad in ((0, 1), (1, 0), (-1, 2)):
            try:
                p.set_output_stride(*bad)
                refusals.append(None)
            except fc.FFTConvError as e:
                refusals.append((e.status, "at least 1" in str(e)))
        refusals.append(before[0] == 4 and before[3:] == (1, 1))
    return out, refusals


def _case_tuning():
    """tune_placement 2 on a plan with the fused strided store: the tuner's probe launches are the strided launch into the caller's
    tight buffer"""
    torch, fc, dev = _ctx()
    H, W, F, kh, kw, n = SHAPE
    data, ks = _inputs(SHAPE, 123)
    img_d, ker_d = _image_t(torch, data).to(dev), _pack_t(torch, ks).to(dev)
    stride = (2, 3)
    res = {}
    for name in ("window", "rectangle"):
        how = EXTENTS[name][0] if name == "window" else ("rect", (7, 17, 33, 40))
        with fc.Plan(H, W, F, kh, kw) as p:
            p.set_image_device(img_d.data_ptr())
            _set_extent(p, how)
            dense, _ = _maps(torch, dev, p, n, ker_d, kh, kw)
        with fc.Plan(H, W, F, kh, kw) as p:      # a fresh intermediate: the tuner runs in the first convolve
            p.set_option("tune_placement", 2)
            p.set_image_device(img_d.data_ptr())
            _set_extent(p, how)
            p.set_output_stride(*stride)
            direct = p.get_option("stride_direct")
            got, log = _maps(torch, dev, p, n, ker_d, kh, kw, shift=1)
            _route_named(log, stride, direct)
            res[name] = (direct, p.get_option("tuned_candidates"), _differ(got, _slice(dense, *stride)))
    return res


def _case_graph():
    """set_image(DEVICE) + convolve_packed with a stride, captured after one eager warm-up step and replayed with new inputs:
    bit-equal to the eager step on the same inputs, which is the sliced dense map of the same plan"""
    torch, fc, dev = _ctx()
    shape = (840, 270, 1, 13, 11, 3)          # M = 432: the tile queue, whose counters every launch must leave at zero
    H, W, F, kh, kw, n = shape
    stride = (2, 2)
    sets = [_inputs(shape, 290 + k) for k in range(3)]
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream), fc.Plan(H, W, F, kh, kw, stream=stream.cuda_stream) as p:
        p.set_output_stride(*stride)
        assert p.get_option("blockwise") == 0 and p.get_option("dynamic_tiles") == 1 and p.get_option("stride_direct") == 1
        i = p.info
        ne = n * i.out_h * i.out_w
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
        # the eager maps against the sliced dense maps of the same plan
        refs = []
        for r in range(2):
            img_d.copy_(imgs_h[r + 1], non_blocking=True)
            ker_d.copy_(kers_h[r + 1], non_blocking=True)
            p.set_image_device(img_d.data_ptr())
            p.set_output_stride(1, 1)
            dense, _ = _maps(torch, dev, p, n, ker_d, kh, kw)
            p.set_output_stride(*stride)
            refs.append(_differ(want[r].reshape(n, i.out_w, i.out_h), _slice(dense, *stride)))
    return ([_differ(a, b) for a, b in zip(got, want)], refs, bool(np.array_equal(got[0], got[1])), same_ws,
            [int(np.isnan(a).sum()) for a in got])


# ---- the tests

@pytest.mark.parametrize("stride_store", [1, 0])
@pytest.mark.parametrize("fmt", [0, 1, 2])
def test_strided_maps_are_the_sliced_maps(device, fmt, stride_store):
    """250 x 250 (x) 31 x 31, 3 maps, 288 x 288 window: four strides on four extents, packed device output, both routes"""
    res = device("_case_values", fmt, stride_store)
    assert [(r[0], r[1]) for r in res] == [(name, s) for name in EXTENTS for s in STRIDES]
    for name, stride, differ, err in res:
        print("%s, stride %s, format %d, stride_store %d: %d elements differ from the slice%s" %
              (name, stride, fmt, stride_store, differ, "" if err is None else "; max |got - oracle| / max |oracle| = %.3g" % err))
    for name, stride, differ, err in res:
        assert differ == 0, (name, stride, differ)
        assert (err is not None) == (fmt == 0)
        if err is not None:
            assert err <= 1e-5, (name, stride, err)


@pytest.mark.parametrize("M,T", col_configs())
def test_every_configuration_is_bit_equal(device, M, T):
    """the strided kernels are instantiations of their own: every built configuration is held to bit-equality with the slice of its
    plain sibling's maps, fused and staged.  The listed configurations read stride_direct 0 and return the same bytes."""
    res = device("_case_configuration", M, T)
    print(M, T, res)
    built = 0 if M in NOT_BUILT else 1
    assert res == {(s, store): (built if store else 0, 0) for s in ((2, 3), (1, T + 1)) for store in (1, 0)}, (M, res)


@pytest.mark.parametrize("name", COMPOSITIONS)
def test_compositions(device, name):
    direct, want_direct, differ, image_kept, nans = device("_case_composition", name)
    print(name, direct, differ, image_kept, nans)
    assert direct == want_direct and differ == 0 and image_kept == 0 and nans == 0, (name, direct, differ, image_kept, nans)


@pytest.mark.parametrize("route", ROUTES)
def test_delivery_routes(device, route):
    res = device("_case_route", route)
    print(route, res)
    assert res[0] == 0 and res[1] == 0, (route, res)
    assert res["direct"] == (0 if route == "pinned small call" else 1)       # (the demo fixture's 80 x 16 window has no specialised kernel)


def test_state(device):
    steps, refusals = device("_case_state")
    for s in steps:
        print(s)
    assert len(steps) == 9
    for what, arg, info_ok, kept, differ in steps:
        assert info_ok and kept and differ == 0, (what, arg, info_ok, kept, differ)
    print(refusals)
    assert refusals == [(-1, True), True, (-1, True), True, (-1, True), (-1, True), (-1, True), True], refusals


def test_placement_tuning_probes_the_strided_launch(device):
    res = device("_case_tuning")
    print(res)
    for name in ("window", "rectangle"):
        direct, candidates, differ = res[name]
        assert direct == 1 and candidates == 2 and differ == 0, res


def test_graph_replay(device):
    replay_vs_eager, eager_vs_slice, same_twice, same_ws, nans = device("_case_graph")
    assert replay_vs_eager == [0, 0]               # each replay is the eager step on the same inputs, bit for bit
    assert eager_vs_slice == [0, 0] and nans == [0, 0]
    assert not same_twice                          # (and the two replays did see different inputs)
    assert same_ws                                 # nothing was allocated after the warm-up step
