"""16-bit result maps on the GPU: plan option "map_format" (1 = IEEE fp16, 2 = bfloat16) against the library's own fp32 maps.

The yardstick is the fp32 path, which the rest of the suite pins to the float64 oracle: the same plan, image and kernels are run
with map_format 0, and the fp32 maps converted in NumPy (fp16: astype(np.float16); bf16: round to nearest even on the bit
pattern).  The 16-bit maps must equal that conversion BIT FOR BIT -- the kernels do the same arithmetic and convert the same
fp32 value once, in the store, so no tolerance is involved.  One case (the demo fixture) is also held against the float64
oracle: the project's bar plus half an ulp of the format.

Every output-kernel variant has a case of the smallest shape that reaches it, and every case reads from the plan (transform
lengths, "specialised_kernels", "dynamic_tiles") and from its verbose log ("output kernel: ...") that it ran the variant it
names.  The kernels of a case differ in scale by ten orders of magnitude, so fp16 subnormals and overflows to inf are in the
maps.  Then the delivery routes (host copies blocking / by threads / through the pinned ring, the pinned small-call path,
device pointers, the packed buffer, the cached one-shot entry) and a captured graph.  The cases run in a spawned child
(test_accuracy_gpu._Child), which exits with the module."""
import os
import re

import numpy as np
import pytest

import golden_util
import util
from test_accuracy_gpu import _Child
from test_features_gpu import _logged

pytestmark = pytest.mark.gpu

CSRC = os.path.join(util.ROOT, "cuda-fft-convolution_amd", "csrc")
FORMATS = {1: "fp16", 2: "bf16"}
GUARD = 64                   # elements behind a device map buffer that must stay untouched
SCALES = (1.0, 2e-6, 1e4, 1e-3, 30.0)      # of the kernels of a case: maps in the fp16 subnormal range, and beyond 65504


def col_table():
    """{M: T} of fast_paths.hpp's X(M, R1, R2, R3, T, NT) rows"""
    src = open(os.path.join(CSRC, "fast_paths.hpp")).read()
    cols = src[src.index("#define FC_FAST_COL_CONFIGS_G0(X)"):src.index("#define FC_FAST_COL_CONFIGS(X)")]
    return {int(m.group(1)): int(m.group(2)) for m in re.finditer(r"X\((\d+), \d+, \d+, \d+, (\d+), \d+\)", cols)}


# name: (H, W, F, kh, kw, maps), creation options, plan options, then what the plan must say about itself: transform length
# along h (None: not checked), tile width T of its output kernel (0: the generic kernel), "dynamic_tiles", and the pattern its
# "output kernel:" log lines match
VARIANTS = {
    "T = 16, static, small transform": ((270, 272, 1, 13, 11, 5), {"exact_window": 1}, {}, 288, 16, 0, r"output kernel: tiled intermediate"),
    "row-major intermediate": ((270, 272, 1, 13, 11, 5), {"exact_window": 1, "kernel_path": 2}, {}, 288, 16, 0, r"output kernel: row-major intermediate"),
    "forced generic": ((270, 272, 1, 13, 11, 5), {"exact_window": 1, "kernel_path": 1}, {}, 288, 0, 0, r"output kernel: generic,"),
    "small generic": ((64, 64, 1, 3, 3, 5), {}, {}, None, 0, 0, r"output kernel: generic,"),
    "Bluestein": ((282, 282, 1, 23, 23, 3), {"exact_window": 1}, {}, 304, 0, 0, r"output kernel: generic \(chirp-z\),"),
    # (3 maps are 54 tiles on 256 workgroups: less than one round, nothing to slice -- the queue deals them; the next case has the tail round)
    "window shorter than the transform": ((1060, 270, 1, 20, 11, 3), {}, {}, 1152, 16, 1, r"output kernel: tiled, dynamic tile queue"),
    "sliced tail round": ((1060, 270, 1, 20, 11, 15), {}, {}, 1152, 16, 1, r"output kernel: tiled, sliced tail round"),
    "dynamic tile queue": ((840, 270, 1, 13, 11, 3), {}, {}, 864, 16, 1, r"output kernel: tiled, dynamic tile queue"),
    "T = 8, cfg3's configuration": ((4200, 270, 1, 13, 11, 2), {}, {}, 4224, 8, 1, r"output kernel: tiled, dynamic tile queue"),
    "T = 8, static deal": ((4200, 270, 1, 13, 11, 2), {}, {"dynamic_tiles": 0}, 4224, 8, 0, r"output kernel: tiled intermediate"),
    "T = 4": ((5100, 270, 1, 13, 11, 2), {"blockwise": 1}, {}, 5120, 4, 1, r"output kernel: tiled, dynamic tile queue"),
    "F = 3": ((270, 272, 3, 13, 11, 5), {"exact_window": 1}, {}, 288, 16, 0, r"output kernel: tiled intermediate"),
    "output_region 1": ((271, 273, 1, 12, 10, 3), {}, {"output_region": 1}, None, None, None, r"output region 1: .* cropped .* 282 x 282"),
    "output_region 2": ((271, 273, 1, 12, 10, 3), {}, {"output_region": 2}, None, None, None, r"output region 2: .* cropped .* 271 x 273"),
    "output_region 3": ((271, 273, 1, 12, 10, 3), {}, {"output_region": 3}, None, None, None, r"output region 3: .* cropped .* 260 x 264"),
    "output_region 4": ((271, 273, 1, 12, 10, 3), {}, {"output_region": 4}, None, None, None, r"output region 4: .* padded .* 512 x 512"),
}
# (default host route: maps of 162 KB come back several per copy through the plan's pinned buffer; host_pinned 0: one blocking copy per map)
ROUTES = ["host_stream 0", "host_stream 1", "host_stream 2", "pinned small call", "device pointers", "default host route", "host_pinned 0"]


@pytest.fixture(scope="module")
def device():
    child = _Child(globals())
    yield child
    if child.gone:
        child.kill()
    else:
        child.ex.shutdown(wait=True)


# ---- shared by both sides

def to_bits(a32, fmt):
    """uint16 bit patterns of fp32 values rounded to nearest even into format fmt: the reference conversion"""
    a32 = np.ascontiguousarray(a32, dtype=np.float32)
    if fmt == 1:
        with np.errstate(over="ignore"):
            return a32.astype(np.float16).view(np.uint16)
    u = a32.view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def from_bits(bits, fmt):
    """float64 values of uint16 bit patterns"""
    bits = np.ascontiguousarray(bits, dtype=np.uint16)
    if fmt == 1:
        return bits.view(np.float16).astype(np.float64)
    return (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def compare(got_bits, ref32, fmt):
    """{elements, differing, subnormal / inf results among them}: 16-bit maps against the converted fp32 maps"""
    want = to_bits(ref32, fmt)
    got = np.ascontiguousarray(got_bits).view(np.uint16).reshape(want.shape)
    mag = want & 0x7FFF
    if fmt == 1:
        sub, inf = int(((mag > 0) & (mag < 0x400)).sum()), int((mag == 0x7C00).sum())
    else:
        sub, inf = int(((mag > 0) & (mag < 0x80)).sum()), int((mag == 0x7F80).sum())
    return {"elements": int(want.size), "differ": int((got != want).sum()), "subnormal": sub, "inf": inf,
            "nan_ref": int(np.isnan(np.asarray(ref32)).sum())}


# ---- the child's side

def _ctx():
    import torch
    return torch, util.load_package(), torch.device("cuda", 0)


def _inputs(shape, seed):
    H, W, F, kh, kw, n = shape
    rng = np.random.default_rng(seed)
    data = np.asfortranarray(rng.standard_normal((H, W, F), dtype=np.float32))
    ks = [np.asfortranarray(np.float32(SCALES[j % len(SCALES)]) * rng.standard_normal((kh, kw, F), dtype=np.float32)) for j in range(n)]
    return data, ks


def _image_t(torch, img):
    return torch.from_numpy(np.ascontiguousarray(np.transpose(img, (2, 1, 0))))


def _pack_t(torch, ks):
    return torch.from_numpy(np.ascontiguousarray(np.stack([np.transpose(k, (2, 1, 0)) for k in ks])))


def _map_buffer(torch, dev, p, n, fmt):
    """device buffer for n packed maps of the plan's current format plus GUARD elements, all poisoned"""
    i = p.info
    assert i.out_map_bytes == i.out_h * i.out_w * (4 if fmt == 0 else 2), (fmt, i.out_map_bytes)
    ne = n * i.out_h * i.out_w + GUARD
    if fmt == 0:
        return torch.full((ne,), float("nan"), dtype=torch.float32, device=dev)
    return torch.full((ne,), 0x7E5A, dtype=torch.int16, device=dev)        # (a NaN in both formats)


def _maps_of(buf, p, n, fmt):
    """host maps [n][out_w][out_h] out of a buffer of _map_buffer; the guard must be as it was"""
    i = p.info
    a = buf.cpu().numpy()
    body, guard = a[:a.size - GUARD], a[a.size - GUARD:]
    assert np.isnan(guard).all() if fmt == 0 else (guard == 0x7E5A).all(), "the guard behind the maps was written"
    return body.reshape(n, i.out_w, i.out_h) if fmt == 0 else body.view(np.uint16).reshape(n, i.out_w, i.out_h)


def _case_variant(name):
    torch, fc, dev = _ctx()
    shape, options, settings, want_lh, want_t, want_dyn, pattern = VARIANTS[name]
    H, W, F, kh, kw, n = shape
    data, ks = _inputs(shape, 31 + len(name))
    img_d, ker_d = _image_t(torch, data).to(dev), _pack_t(torch, ks).to(dev)
    res = {}
    with fc.Plan(H, W, F, kh, kw, options=options) as p:
        for key, value in settings.items():
            p.set_option(key, value)
        assert p.get_option("blockwise") == 0 and p.get_option("map_format") == 0
        if want_lh is not None:
            assert p.info.transform_h == want_lh, (name, p.info.transform_h)
        if want_t is not None:
            spec = p.get_option("specialised_kernels")
            assert (spec & 2 != 0) == (want_t > 0), (name, spec)
            if want_t:
                assert col_table()[p.info.transform_h // 2] == want_t
            assert p.get_option("dynamic_tiles") == want_dyn
        p.set_option("verbose", 1)
        p.set_image_device(img_d.data_ptr())
        maps, logs = {}, {}
        for fmt in (0, 1, 2):
            p.set_option("map_format", fmt)
            assert p.get_option("map_format") == fmt
            buf = _map_buffer(torch, dev, p, n, fmt)

            def run():
                p.convolve_packed_device(n, ker_d.data_ptr(), kh, kw, buf.data_ptr())
                p.synchronize()
            _, logs[fmt] = _logged(run)
            maps[fmt] = _maps_of(buf, p, n, fmt)
        p.set_option("verbose", 0)
    assert not np.isnan(maps[0]).any()
    for fmt, fname in FORMATS.items():
        lines = [ln for ln in logs[fmt].splitlines() if re.search(r"output (kernel|region)", ln)]
        assert lines and any(re.search(pattern, ln) for ln in lines), (name, pattern, logs[fmt])
        # the kernel that stores the caller's maps stores this format (ahead of a crop: fp32 into the window the crop reads)
        cropped = "output_region" in settings
        assert all((fname if not cropped or "region" in ln else "fp32") in ln for ln in lines), (name, lines)
        res[fmt] = compare(maps[fmt], maps[0], fmt)
    res["log"] = [ln for ln in logs[1].splitlines() if "output " in ln][:3]
    return res


def _case_route(route):
    """host and device delivery of 16-bit maps: every route hands out the bytes the packed path computes"""
    torch, fc, dev = _ctx()
    small = route == "pinned small call"
    if small:
        data, _, _, ks, _ = golden_util.load_case("case_demo")        # 64 x 8 x 5, three 10 x 4 x 5 kernels: 80 x 16 maps
        data, ks = np.asfortranarray(data), [np.asfortranarray(k) for k in ks]
        H, W, F = data.shape
        kh, kw, n, options = 10, 4, len(ks), {}
    else:
        H, W, F, kh, kw, n = shape = (270, 272, 1, 13, 11, 5)
        data, ks = _inputs(shape, 77)
        options = {"exact_window": 1}
    res = {}
    with fc.Plan(H, W, F, kh, kw, options=options) as p:
        if route.startswith("host_stream"):
            p.set_option("host_min_kb", 0)
            p.set_option("host_stream", int(route[-1]))
            p.set_option("batch_maps", 2)            # three batches: both staging buffers of the streamed routes are reused
        if route == "host_pinned 0":
            p.set_option("host_pinned", 0)
        p.set_image(data)
        got = {}
        for fmt in (0, 1, 2):
            p.set_option("map_format", fmt)
            if route == "device pointers":
                i = p.info
                bufs = [_map_buffer(torch, dev, p, 1, fmt) for _ in range(n)]
                p.convolve_to_device(ks, [b.data_ptr() for b in bufs])
                p.synchronize()
                got[fmt] = np.stack([_maps_of(b, p, 1, fmt)[0] for b in bufs])
            else:
                outs = p.convolve(ks)
                assert all(o.dtype == fc.MAP_DTYPES[fmt] and o.shape == (p.info.out_h, p.info.out_w) for o in outs)
                got[fmt] = np.stack([np.ascontiguousarray(o.T) for o in outs])
        for fmt in FORMATS:
            res[fmt] = compare(got[fmt], got[0], fmt)
    return res


def _case_one_shot():
    """the cached one-shot entry with the options field: format 1 twice (the second call finds the plan), then format 0, which
    must MISS the cache and return fp32 maps"""
    torch, fc, dev = _ctx()
    shape = (270, 272, 1, 13, 11, 5)
    data, ks = _inputs(shape, 78)
    fc.cache_clear()
    a = fc.cudaConvolutionFFT(data, 13, 11, ks, options={"map_format": 1})
    hit_a = fc.last_call_timing()["cache_hit"]
    b = fc.cudaConvolutionFFT(data, 13, 11, ks, options=fc.PlanOptions(map_format=1))
    hit_b = fc.last_call_timing()["cache_hit"]
    c = fc.cudaConvolutionFFT(data, 13, 11, ks, options={"map_format": 0})
    hit_c = fc.last_call_timing()["cache_hit"]
    d = fc.cudaConvolutionFFT(data, 13, 11, ks)
    hit_d = fc.last_call_timing()["cache_hit"]
    e = fc.cudaConvolutionFFT(data, 13, 11, ks, options={"map_format": 2})
    plans = fc.cache_stats()["plans"]
    fc.cache_clear()
    assert all(x.dtype == np.float16 for x in a + b) and all(x.dtype == np.float32 for x in c + d) and all(x.dtype == np.uint16 for x in e)
    return {"hits": (hit_a, hit_b, hit_c, hit_d), "plans": plans,
            "a": compare(np.stack(a), np.stack(c), 1), "b": compare(np.stack(b), np.stack(c), 1), "e": compare(np.stack(e), np.stack(c), 2),
            "c_equals_d": all(np.array_equal(x, y) for x, y in zip(c, d))}


def _case_oracle():
    """the demo fixture against its float64 oracle maps: |out - ref| <= 1e-4 max|ref| + half an ulp of the format at ref"""
    torch, fc, dev = _ctx()
    data, mkh, mkw, ks, expect = golden_util.load_case("case_demo")
    worst = {}
    with fc.Plan(data.shape[0], data.shape[1], data.shape[2], mkh, mkw) as p:
        p.set_image(data)
        for fmt in (1, 2):
            p.set_option("map_format", fmt)
            outs = p.convolve(ks)
            w = 0.0
            for o, r in zip(outs, expect):
                bound = 1e-4 * np.abs(r).max() + (2.0 ** -11 if fmt == 1 else 2.0 ** -8) * np.abs(r)
                err = np.abs(from_bits(o.view(np.uint16), fmt) - r)
                w = max(w, float((err / bound).max()))
            worst[fmt] = w
    return worst


def _case_option_on_plans():
    """the option on real plans: round trip, the bytes plan_info reports, and the refusal on a block-wise plan"""
    torch, fc, dev = _ctx()
    out = {}
    with fc.Plan(64, 64, 1, 3, 3, options=fc.PlanOptions(map_format=2)) as p:
        out["created"] = (p.get_option("map_format"), p.info.map_bytes, p.info.out_map_bytes, p.info.fft_h * p.info.fft_w)
        trip = []
        for v in (1, 0, 2):
            p.set_option("map_format", v)
            trip.append((p.get_option("map_format"), p.info.out_map_bytes))
        out["trip"] = trip
        try:
            p.set_option("map_format", 3)
            out["range"] = None
        except fc.FFTConvError as e:
            out["range"] = (e.status, p.get_option("map_format"))
        p.set_option("output_region", 3)
        out["valid"] = (p.info.out_h, p.info.out_w, p.info.out_map_bytes)
    with fc.Plan(600, 600, 1, 9, 9, options={"max_transform": 512}) as p:
        blocks = p.get_option("blockwise")
        p.set_option("map_format", 0)
        try:
            p.set_option("map_format", 1)
            out["blockwise"] = (blocks, None, "")
        except fc.FFTConvError as e:
            out["blockwise"] = (blocks, e.status, str(e))
        out["blockwise_after"] = (p.get_option("map_format"), p.info.map_bytes == p.info.fft_h * p.info.fft_w * 4)
    try:
        fc.Plan(600, 600, 1, 9, 9, options={"max_transform": 512, "map_format": 1})
        out["create_blockwise"] = None
    except fc.FFTConvError as e:
        out["create_blockwise"] = (e.status, str(e))
    return out


def _case_graph():
    """set_image(DEVICE) + convolve_packed with fp16 maps captured after one eager warm-up step, replayed twice with new inputs in
    the captured buffers: bit-equal to the eager calls on the same inputs (and those to the converted fp32 maps)"""
    torch, fc, dev = _ctx()
    shape = (840, 270, 1, 13, 11, 3)          # M = 432: the tile queue, whose counters every launch must leave at zero
    H, W, F, kh, kw, n = shape
    sets = [_inputs(shape, 90 + k) for k in range(3)]
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream), fc.Plan(H, W, F, kh, kw, stream=stream.cuda_stream, options={"map_format": 1}) as p:
        assert p.get_option("blockwise") == 0 and p.get_option("dynamic_tiles") == 1 and p.get_option("map_format") == 1
        i = p.info
        imgs_h = [_image_t(torch, s[0]).pin_memory() for s in sets]
        kers_h = [_pack_t(torch, s[1]).pin_memory() for s in sets]
        img_d = torch.empty(imgs_h[0].shape, dtype=torch.float32, device=dev)
        ker_d = torch.empty(kers_h[0].shape, dtype=torch.float32, device=dev)
        out = _map_buffer(torch, dev, p, n, 1)
        replayed = [torch.empty_like(out) for _ in range(2)]
        eager = [torch.empty_like(out) for _ in range(2)]

        def step():
            p.set_image_device(img_d.data_ptr())
            p.convolve_packed_device(n, ker_d.data_ptr(), kh, kw, out.data_ptr())

        img_d.copy_(imgs_h[0], non_blocking=True)
        ker_d.copy_(kers_h[0], non_blocking=True)
        step()                                   # eager warm-up: sizes the scratch; nothing allocates from here on
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        cap = torch.cuda.Stream(dev)
        with torch.cuda.graph(graph, stream=cap):
            p.set_stream(torch.cuda.current_stream(dev).cuda_stream)
            step()
        p.set_stream(stream.cuda_stream)
        for r in range(2):                       # nothing synchronised inside the loop
            out.fill_(0x7E5A)
            img_d.copy_(imgs_h[r + 1], non_blocking=True)
            ker_d.copy_(kers_h[r + 1], non_blocking=True)
            graph.replay()
            replayed[r].copy_(out)
        torch.cuda.synchronize()
        for r in range(2):
            out.fill_(0x7E5A)
            img_d.copy_(imgs_h[r + 1], non_blocking=True)
            ker_d.copy_(kers_h[r + 1], non_blocking=True)
            step()
            eager[r].copy_(out)
        torch.cuda.synchronize()
        got = [_maps_of(t, p, n, 1) for t in replayed]
        want = [_maps_of(t, p, n, 1) for t in eager]
        del graph
        # the yardstick for the eager maps: the same plan in fp32
        p.set_option("map_format", 0)
        ref = []
        for r in range(2):
            buf = _map_buffer(torch, dev, p, n, 0)
            img_d.copy_(imgs_h[r + 1], non_blocking=True)
            ker_d.copy_(kers_h[r + 1], non_blocking=True)
            p.set_image_device(img_d.data_ptr())
            p.convolve_packed_device(n, ker_d.data_ptr(), kh, kw, buf.data_ptr())
            p.synchronize()
            ref.append(_maps_of(buf, p, n, 0))
    return ([bool(np.array_equal(a, b)) for a, b in zip(got, want)], [compare(w, r, 1) for w, r in zip(want, ref)],
            bool(np.array_equal(got[0], got[1])))


# ---- the tests

def _bit_equal(res, what, want_extremes=False):
    for fmt, fname in FORMATS.items():
        r = res[fmt]
        print("%s, %s: %d elements, %d differ; %d subnormal and %d inf results among them" % (what, fname, r["elements"], r["differ"], r["subnormal"], r["inf"]))
        assert r["nan_ref"] == 0 and r["elements"] > 0
        assert r["differ"] == 0, (what, fname, r)
        if want_extremes and fmt == 1:
            assert r["subnormal"] > 0 and r["inf"] > 0, (what, r)      # the case really reaches both ends of fp16


@pytest.mark.parametrize("name", list(VARIANTS))
def test_16_bit_maps_are_the_rounded_fp32_maps(device, name):
    res = device("_case_variant", name)
    print("\n".join(res["log"]))
    _bit_equal(res, name, want_extremes=VARIANTS[name][0][5] >= 3)


@pytest.mark.parametrize("route", ROUTES)
def test_delivery_routes(device, route):
    _bit_equal(device("_case_route", route), route)


def test_cached_one_shot_entry(device):
    res = device("_case_one_shot")
    # the format is part of the cache key: the second fp16 call finds the first's plan, the fp32 call after them does not (and
    # is the plan a call without options finds); three plans in the end
    assert res["hits"] == (0, 1, 0, 1) and res["plans"] == 3, res
    assert res["c_equals_d"]
    for k in ("a", "b", "e"):
        assert res[k]["differ"] == 0 and res[k]["elements"] == 5 * 288 * 288, (k, res[k])


def test_demo_fixture_within_the_oracle_bound(device):
    worst = device("_case_oracle")
    print("demo fixture, worst |out - ref| / (1e-4 max|ref| + half ulp |ref|): fp16 %.3f, bf16 %.3f" % (worst[1], worst[2]))
    assert worst[1] <= 1.0 and worst[2] <= 1.0, worst


def test_option_on_plans(device):
    out = device("_case_option_on_plans")
    ne = 80 * 80
    assert out["created"] == (2, 2 * ne, 2 * ne, ne)
    assert out["trip"] == [(1, 2 * ne), (0, 4 * ne), (2, 2 * ne)]
    assert out["range"] == (-1, 2)                                 # refused, the value kept
    assert out["valid"] == (62, 62, 2 * 62 * 62)
    blocks, status, msg = out["blockwise"]
    assert blocks > 0 and status == -1 and "block-wise" in msg and "map_format" in msg, out["blockwise"]
    assert out["blockwise_after"] == (0, True)
    assert out["create_blockwise"] is not None and out["create_blockwise"][0] == -1 and "block-wise" in out["create_blockwise"][1]


def test_graph_replay_with_fp16_maps(device):
    equal, against_fp32, same_twice = device("_case_graph")
    assert equal == [True, True], equal                            # each replay is the eager step on the same inputs, bit for bit
    assert not same_twice                                          # (and the two replays did see different inputs)
    for r in against_fp32:
        assert r["differ"] == 0 and r["nan_ref"] == 0, r
