"""Border modes (fftconv_plan_set_border), GPU tier: the HIP kernels through the C ABI.

  1. every mode against float64 on the numpy.pad extension, within util.BUDGET_DIRECT / BUDGET_BLUESTEIN on the "same" rectangle;
  2. every configuration of the column table: the direct route (the bordered column kernel) against the staged one, bit-equal,
     with "border_direct" and the verbose line naming the route taken;
  3. image batches: every image's maps bit-equal to the plan holding that image alone;
  4. composition: typed pixels, 16-bit maps, a caller's rectangle, host maps, a pending deferred preparation;
  5. state and refusals;
  6. a captured warm step replayed with new inputs, bit-equal to the eager step.

Every case runs in the module's child process (test_accuracy_gpu._Child)."""
import numpy as np
import pytest

import util
from test_accuracy_gpu import _Child
from test_border_host import reference_maps
from test_features_gpu import _logged
from test_map_format_gpu import _image_t, _pack_t, col_table, to_bits

pytestmark = pytest.mark.gpu

SHAPES = {
    "288 x 288, odd MAXK": ((250, 250, 1, 31, 31, 3), {}, util.BUDGET_DIRECT, 1),
    "even MAXK, odd H, F = 2": ((251, 249, 2, 12, 10, 3), {}, util.BUDGET_DIRECT, 1),
    "Bluestein 304 x 368": ((282, 346, 2, 23, 23, 2), {"exact_window": 1}, util.BUDGET_BLUESTEIN, 0),
}
NOT_BUILT = (544, 1280, 1536, 1680, 2304)      # fast_paths.hpp: FC_COLS_FWD_BORDER_NOT_BUILT -- the staged route
DIRECT_LINE = "border (mode %d): direct -- mapped in the column kernel's load"
STAGED_LINE = "border (mode %d): staged -- "


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


def _same(a, b):
    """two lists of maps hold the same bytes"""
    return len(a) == len(b) and all(x.shape == y.shape and x.dtype == y.dtype and x.tobytes(order="F") == y.tobytes(order="F") for x, y in zip(a, b))


def _case_modes(name, flip):
    """{mode: [metrics per map]} on the "same" rectangle; the route the plan took"""
    torch, fc, dev = _ctx()
    shape, options, _, want_direct = SHAPES[name]
    H, W, F, kh, kw, n = shape
    data, ks = util.normal_inputs(shape, 31 + H)
    out = {}
    with fc.Plan(H, W, F, kh, kw, options=options) as p:
        p.set_option("border_store", 1)
        if flip:
            p.set_option("flip_kernels", 1)
        for mode in ((4,) if flip else (1, 2, 3, 4, 5)):
            value = 0.5 if mode == 1 else 0.0
            p.set_border(mode, value)
            assert (p.info.out_h, p.info.out_w) == (H, W) and p.get_option("output_region") == 5
            assert (p.get_option("rect_off_h"), p.get_option("rect_off_w")) == (kh - 1, kw - 1)
            assert (p.get_option("border_mode"), p.get_option("border_lead_h"), p.get_option("border_lead_w")) == (mode, kh // 2, kw // 2)
            assert p.get_option("border_direct") == want_direct, (name, p.get_option("border_direct"))
            p.set_image(data)
            got = p.convolve(ks)
            refs = reference_maps(data, ks, kh, kw, mode, value, flip=bool(flip))
            out[mode] = [util.accuracy(g, r) for g, r in zip(got, refs)]
    return out


def _case_configuration(M):
    """an exact_window plan whose transform along h is 2M points on a 288-column window, two maps, device-resident image: modes 3
    and 1, static deal and the tile queues (dynamic_tiles 0, 1 and 2: the forward kernels take theirs from the queue at 2),
    "border_store" 1 against 0.  {(mode, dyn): (border_direct, the verbose line names the route taken, maps differ)}"""
    torch, fc, dev = _ctx()
    kh, kw, n = 13, 11, 2
    H, W = 2 * M - 18, 272
    data, ks = util.normal_inputs((H, W, 1, kh, kw, n), 7 + M)
    img_d = _image_t(torch, data).to(dev)
    out = {}
    with fc.Plan(H, W, 1, kh, kw, options={"exact_window": 1, "blockwise": 1}) as p:
        assert p.get_option("blockwise") == 0 and (p.info.fft_h, p.info.fft_w, p.info.transform_h) == (2 * M, 288, 2 * M)
        assert p.get_option("specialised_kernels") == 3
        for mode, value in ((3, 0.0), (1, -1.25)):
            p.set_border(mode, value)
            for dyn in (0, 1, 2):
                p.set_option("dynamic_tiles", dyn)
                maps = {}
                for store in (1, 0):
                    p.set_option("border_store", store)
                    direct = p.get_option("border_direct")
                    p.set_option("verbose", 1)
                    _, log = _logged(lambda: (p.set_image_device(img_d.data_ptr()), p.synchronize()))
                    p.set_option("verbose", 0)
                    line_ok = ((DIRECT_LINE % mode) in log) if direct else ((STAGED_LINE % mode) in log and "extended into the fp32 image staging" in log)
                    assert store == 1 or direct == 0
                    maps[store] = (direct, line_ok, p.convolve(ks))
                out[(mode, dyn)] = (maps[1][0], maps[1][1] and maps[0][1], 0 if _same(maps[1][2], maps[0][2]) else 1)
    return out


def _case_batches():
    """B = 3 different images: image_walk 0 and 1, batch_maps 3, direct and staged -- each image's maps against the plan holding
    that image alone.  {setting: maps differ}"""
    torch, fc, dev = _ctx()
    H, W, F, kh, kw, n = 250, 250, 1, 31, 31, 2
    B = 3
    _, ks = util.normal_inputs((H, W, F, kh, kw, n), 5)
    ks = [ks[0], np.asfortranarray(ks[0][::-1].copy())]      # (one size: a batch is convolved with the kernels of one call)
    imgs = [util.normal_inputs((H, W, F, kh, kw, 1), 50 + b)[0] for b in range(B)]
    batch = np.asfortranarray(np.stack(imgs, axis=3))
    out = {}
    with fc.Plan(H, W, F, kh, kw) as p:
        p.set_border(2)
        p.set_option("border_store", 1)
        assert p.get_option("border_direct") == 1
        alone = []
        for b in range(B):
            p.set_image(imgs[b])
            alone += p.convolve(ks)
        for setting in ({"image_walk": 0}, {"image_walk": 1}, {"batch_maps": 3}, {"border_store": 0}):
            for key, value in setting.items():
                p.set_option(key, value)
            p.set_images(batch)
            assert p.get_option("images") == B
            got = p.convolve(ks)
            out[str(setting)] = 0 if _same(got, alone) else 1
    return out


def _case_composition():
    torch, fc, dev = _ctx()
    shape = (250, 250, 1, 31, 31, 3)
    H, W, F, kh, kw, n = shape
    data, ks = util.normal_inputs(shape, 91)
    u8 = np.asfortranarray(np.random.default_rng(3).integers(0, 256, (H, W, F), dtype=np.uint8))
    out = {}
    with fc.Plan(H, W, F, kh, kw) as p:
        p.set_option("border_store", 1)
        p.set_border(3)
        # typed pixels: staged conversion, then the fp32 border route
        assert p.get_option("pixel_direct") == 0 and p.get_option("border_direct") == 1
        p.set_image(u8.astype(np.float32))
        want = p.convolve(ks)
        p.set_image_typed(u8)
        assert p.get_option("pixel_format") == fc.PIXEL_U8
        out["typed"] = 0 if _same(p.convolve(ks), want) else 1
        # host maps through convolve are what the packed device entry stores
        p.set_image(data)
        base = p.convolve(ks)
        ks_same = [ks[0], ks[2]]
        ker_d = _pack_t(torch, ks_same).to(dev)
        maps_d = torch.full((2, W, H), float("nan"), dtype=torch.float32, device=dev)
        p.convolve_packed_device(2, ker_d.data_ptr(), kh, kw, maps_d.data_ptr())
        p.synchronize()
        got = maps_d.cpu().numpy()
        out["host maps"] = 0 if all(np.array_equal(got[j].T, b) for j, b in enumerate((base[0], base[2]))) else 1
        # map_format 1: the rounded fp32 maps
        p.set_option("map_format", 1)
        half = p.convolve(ks)
        out["map_format"] = 0 if all(h.dtype == np.float16 and np.array_equal(h.view(np.uint16), to_bits(b, 1)) for h, b in zip(half, base)) else 1
        p.set_option("map_format", 0)
        # a caller's rectangle inside the "same" rectangle: odd offset, odd height -- the crop
        oh, ow, rh, rw = 7, 4, 101, 33
        p.set_output_rect(kh - 1 + oh, kw - 1 + ow, rh, rw)
        assert p.get_option("border_mode") == 3 and p.get_option("images") == 1
        roi = p.convolve(ks)
        out["rectangle"] = 0 if all(np.array_equal(r, b[oh:oh + rh, ow:ow + rw]) for r, b in zip(roi, base)) else 1
        p.set_output_rect(kh - 1, kw - 1, H, W)
        # a pending deferred preparation: the kernels' column pass is launched by itself ahead of the bordered image
        p.set_option("defer_prepare", 1)
        p.prepare_kernels_packed_device(2, ker_d.data_ptr(), kh, kw)
        pending = p.get_option("prepare_pending")
        img_d = _image_t(torch, data).to(dev)
        p.set_image_device(img_d.data_ptr())
        after = p.get_option("prepare_pending")
        maps_d.fill_(float("nan"))
        p.convolve_packed_device(2, ker_d.data_ptr(), kh, kw, maps_d.data_ptr())
        p.synchronize()
        out["defer_prepare"] = (pending, after, 0 if np.array_equal(maps_d.cpu().numpy(), got) else 1)
        ws = p.refresh_info().workspace_bytes
        p.set_option("border_store", 0)
        p.set_image(data)
        out["staged"] = 0 if _same(p.convolve(ks), base) else 1
        out["workspace"] = p.refresh_info().workspace_bytes - ws      # the staging of the extended image is counted
    return out


def _raises(fc, fn):
    try:
        fn()
    except fc.FFTConvError as e:
        return e.status, str(e)
    return 0, ""


def _case_state():
    torch, fc, dev = _ctx()
    shape = (250, 250, 1, 31, 31, 2)
    H, W, F, kh, kw, n = shape
    data, ks = util.normal_inputs(shape, 17)
    out = {}

    def state(p):
        return tuple(p.get_option(k) for k in ("border_mode", "output_region", "images", "normalise")) + (p.info.out_h, p.info.out_w)

    with fc.Plan(H, W, F, kh, kw, options={"exact_window": 1}) as p:
        p.set_image(data)
        fresh = p.convolve(ks)
        fresh_state = state(p)
        out["fresh state"] = fresh_state
        errs = {}
        errs["mode -1"] = _raises(fc, lambda: p.set_border(-1))
        errs["mode 6"] = _raises(fc, lambda: p.set_border(6))
        errs["inf"] = _raises(fc, lambda: p.set_border(1, float("inf")))
        errs["nan"] = _raises(fc, lambda: p.set_border(1, float("nan")))
        out["kept after bad arguments"] = state(p) == fresh_state and _same(p.convolve(ks), fresh)
        # a change of mode drops the image; a no-op keeps it; a change of value drops it
        p.set_border(1, 0.5)
        out["after a change"] = (p.get_option("images"), _raises(fc, lambda: p.convolve(ks))[0])
        p.set_image(data)
        a = p.convolve(ks)
        p.set_border(1, 0.5)
        out["no-op keeps"] = (p.get_option("images"), _same(p.convolve(ks), a))
        p.set_border(1, 0.25)
        out["after a new value"] = (p.get_option("images"), _raises(fc, lambda: p.convolve(ks))[0])
        p.set_border(4)
        bordered = state(p)
        # refusals while a border is on
        errs["normalisation"] = _raises(fc, lambda: p.set_normalisation(1, kh, kw))
        errs["import"] = _raises(fc, lambda: p.import_spectrum(np.zeros((F, p.info.fft_w, p.info.fft_h // 2 + 1), dtype=np.complex64)))
        errs["mark valid"] = _raises(fc, lambda: p.mark_spectrum_valid())
        out["kept after refusals"] = state(p) == bordered
        # back to zero: the bits of a fresh plan
        p.set_border(0)
        out["zero state"] = state(p)
        p.set_image(data)
        out["zero again"] = _same(p.convolve(ks), fresh)
        # a plan with normalisation on refuses a border
        p.set_normalisation(1, kh, kw)
        errs["border on a normalised plan"] = _raises(fc, lambda: p.set_border(2))
        out["normalised kept"] = (p.get_option("normalise"), p.get_option("border_mode"))
    # the fold limits, exactly
    with fc.Plan(8, 20, 1, 17, 5) as p:       # MAXK_H / 2 = 8 = DATA_H
        errs["fold 3 ok"] = _raises(fc, lambda: p.set_border(3))
        errs["fold 5 ok"] = _raises(fc, lambda: p.set_border(5))
        errs["fold 4"] = _raises(fc, lambda: p.set_border(4))
        out["fold kept"] = p.get_option("border_mode")
    with fc.Plan(20, 8, 1, 5, 18) as p:       # MAXK_W / 2 = 9 > DATA_W
        errs["fold 3 w"] = _raises(fc, lambda: p.set_border(3))
        errs["fold 5 w"] = _raises(fc, lambda: p.set_border(5))
        errs["fold 2 w ok"] = _raises(fc, lambda: p.set_border(2))
    with fc.Plan(9, 20, 1, 17, 5) as p:       # MAXK_H / 2 = 8 = DATA_H - 1
        errs["fold 4 ok"] = _raises(fc, lambda: p.set_border(4))
    with fc.Plan(600, 600, 1, 9, 9, options={"max_transform": 512}) as p:
        assert p.get_option("blockwise") > 0
        errs["block-wise"] = _raises(fc, lambda: p.set_border(2))
        out["block-wise kept"] = (p.get_option("border_mode"), p.get_option("border_direct"))
    out["errors"] = errs
    return out


def _case_graph():
    """test_graph_gpu's conditions: one eager warm-up step, one captured step on a single stream, replays with new inputs copied into
    the captured buffers, nothing synchronised in between; mode 4 at M = 432, the forward kernels on the tile queue"""
    torch, fc, dev = _ctx()
    shape = (840, 270, 1, 13, 11, 3)
    H, W, F, kh, kw, n = shape
    REPLAYS = 3
    sets = []
    for k in range(REPLAYS + 1):
        img, ks = util.normal_inputs(shape, 240 + k)
        ks = [ks[0], ks[2], np.asfortranarray(ks[0][::-1].copy())]
        sets.append((img, ks))
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream), fc.Plan(H, W, F, kh, kw, stream=stream.cuda_stream) as p:
        assert p.info.transform_h == 864 and p.get_option("dynamic_tiles") == 1
        p.set_option("dynamic_tiles", 2)
        p.set_option("border_store", 1)
        p.set_border(4)
        assert p.get_option("border_direct") == 1
        imgs_h = [_image_t(torch, s[0]).pin_memory() for s in sets]
        kers_h = [_pack_t(torch, s[1]).pin_memory() for s in sets]
        img_d = torch.empty(imgs_h[0].shape, dtype=torch.float32, device=dev)
        ker_d = torch.empty(kers_h[0].shape, dtype=torch.float32, device=dev)
        out = torch.full((n, W, H), float("nan"), dtype=torch.float32, device=dev)
        replayed = [torch.empty_like(out) for _ in range(REPLAYS)]
        eager = [torch.empty_like(out) for _ in range(REPLAYS)]

        def step():
            p.set_image_device(img_d.data_ptr())
            p.convolve_packed_device(n, ker_d.data_ptr(), kh, kw, out.data_ptr())

        img_d.copy_(imgs_h[0], non_blocking=True)
        ker_d.copy_(kers_h[0], non_blocking=True)
        step()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        cap = torch.cuda.Stream(dev)
        with torch.cuda.graph(graph, stream=cap):
            p.set_stream(torch.cuda.current_stream(dev).cuda_stream)
            step()
        p.set_stream(stream.cuda_stream)
        out.fill_(float("nan"))
        for r in range(REPLAYS):
            img_d.copy_(imgs_h[r + 1], non_blocking=True)
            ker_d.copy_(kers_h[r + 1], non_blocking=True)
            graph.replay()
            replayed[r].copy_(out)
        torch.cuda.synchronize()
        out.fill_(float("nan"))
        for r in range(REPLAYS):
            img_d.copy_(imgs_h[r + 1], non_blocking=True)
            ker_d.copy_(kers_h[r + 1], non_blocking=True)
            step()
            eager[r].copy_(out)
        torch.cuda.synchronize()
        got, want = [t.cpu().numpy() for t in replayed], [t.cpu().numpy() for t in eager]
        del graph
    worst = (0.0, 0.0, 0.0)
    for r in range(REPLAYS):
        refs = reference_maps(sets[r + 1][0], sets[r + 1][1], kh, kw, 4)
        for j in range(n):
            worst = tuple(max(a, b) for a, b in zip(worst, util.accuracy(got[r][j].T, refs[j])))
    return worst, all(np.array_equal(a, b) for a, b in zip(got, want)) and not any(np.isnan(a).any() for a in got)


# ---- the tests

@pytest.mark.parametrize("name", list(SHAPES))
def test_modes_against_float64(device, name):
    """every mode 1-5 (CONSTANT: 0.5) against numpy.pad + a float64 full convolution, on rows and columns [MAXK - 1, MAXK - 1 + DATA):
    the two specialised shapes on the direct route within BUDGET_DIRECT, the Bluestein window (staged) within BUDGET_BLUESTEIN"""
    budget = SHAPES[name][2]
    res = device("_case_modes", name, 0)
    assert sorted(res) == [1, 2, 3, 4, 5]
    for mode, metrics in sorted(res.items()):
        for j, m in enumerate(metrics):
            print("border %s mode %d map %d: max %.2e  L2 %.2e  spectral %.2e" % ((name, mode, j) + tuple(m)))
    for mode, metrics in res.items():
        for m in metrics:
            assert all(x < b for x, b in zip(m, budget)), (name, mode, m, budget)


def test_flipped_kernels(device):
    """flip_kernels 1 with mode 4: the reference convolves with the kernels flipped inside their own kh x kw"""
    name = "even MAXK, odd H, F = 2"
    res = device("_case_modes", name, 1)
    for m in res[4]:
        print("border flip mode 4: max %.2e  L2 %.2e  spectral %.2e" % tuple(m))
        assert all(x < b for x, b in zip(m, SHAPES[name][2])), (m, SHAPES[name][2])


@pytest.mark.parametrize("M", sorted(col_table()))
def test_every_configuration_direct_against_staged(device, M):
    """the bordered kernels and the plain kernels are separate instantiations: every built configuration is held to bit-equality
    with the staged route (the plain kernel on the materialised extension).  The configurations that are not built read
    border_direct 0 and take the staged route; the verbose line names the route actually taken."""
    res = device("_case_configuration", M)
    print(M, res)
    want = 0 if M in NOT_BUILT else 1
    assert res == {(mode, dyn): (want, True, 0) for mode in (3, 1) for dyn in (0, 1, 2)}, (M, res)


def test_batches(device):
    res = device("_case_batches")
    print(res)
    assert len(res) == 4 and all(v == 0 for v in res.values()), res


def test_composition(device):
    res = device("_case_composition")
    print(res)
    assert res["typed"] == 0 and res["host maps"] == 0 and res["map_format"] == 0 and res["rectangle"] == 0 and res["staged"] == 0
    assert res["defer_prepare"] == (1, 0, 0)
    assert res["workspace"] >= (250 + 30) * (250 + 30) * 4


def test_state_and_refusals(device):
    res = device("_case_state")
    print(res)
    e = res["errors"]
    for key, text in (("mode -1", "border mode is 0"), ("mode 6", "border mode is 0"), ("inf", "finite"), ("nan", "finite"),
                      ("normalisation", "a border is on"), ("import", "carries no border"), ("mark valid", "carries no border"),
                      ("border on a normalised plan", "normalisation is on"), ("fold 4", "DATA - 1"), ("fold 3 w", "fold an index twice"),
                      ("fold 5 w", "fold an index twice"), ("block-wise", "block-wise plan")):
        assert e[key][0] == -1 and text in e[key][1], (key, e[key])
    for key in ("fold 3 ok", "fold 5 ok", "fold 2 w ok", "fold 4 ok"):
        assert e[key][0] == 0, (key, e[key])
    assert res["fresh state"] == (0, 0, 1, 0, 288, 288)
    assert res["kept after bad arguments"] is True
    assert res["after a change"] == (0, -9) and res["after a new value"] == (0, -9)
    assert res["no-op keeps"] == (1, True)
    assert res["kept after refusals"] is True
    assert res["zero state"] == (0, 0, 0, 0, 288, 288) and res["zero again"] is True
    assert res["normalised kept"] == (1, 0)
    assert res["fold kept"] == 5 and res["block-wise kept"] == (0, 0)


def test_graph_replay(device):
    worst, equal = device("_case_graph")
    print("border graph: replays max %.2e L2 %.2e spectral %.2e, bit-identical to eager: %s" % (worst + (equal,)))
    assert all(x < b for x, b in zip(worst, util.BUDGET_DIRECT)), (worst, util.BUDGET_DIRECT)
    assert equal
