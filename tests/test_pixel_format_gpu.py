"""Typed image pixels (fftconv_plan_set_images_typed: uint8 / uint16 / fp16 / bf16, converted in the load) on the GPU.

All four conversions to fp32 are exact, so the yardstick is BIT-EQUALITY: the reference for a typed call is always the same
plan given set_images of the exact fp32 values, and maps are compared as bytes -- the direct route (the column kernel converts
in its load), the staged route (plan option "pixel_store" 0, and every plan without the typed column kernel: a small kernel
writes the fp32 image first) and the fp32 call must all return the same maps.  One case is also held against the float64 oracle
at the project's bar for fp32 maps.  The cases run in a spawned child (test_accuracy_gpu._Child), which exits with the module."""
import ctypes

import numpy as np
import pytest

import util
from plan_walk import KINDS
from test_accuracy_gpu import _Child
from test_map_format_gpu import _pack_t, col_table

pytestmark = pytest.mark.gpu

U8, U16, F16, BF16 = 1, 2, 3, 4
DTYPES = {U8: np.uint8, U16: np.uint16, F16: np.float16, BF16: np.uint16}
NOT_BUILT = ()               # fast_paths.hpp: FC_COLS_FWD_PX_NOT_BUILT -- configurations whose typed column kernel is not built
PIN_INPLACE, PIN_IMAGE = 512 << 10, 1 << 20        # plan_internal.hpp: FC_PIN_INPLACE_BYTES, FC_PIN_IMAGE_BYTES


@pytest.fixture(scope="module")
def device():
    child = _Child(globals())
    yield child
    if child.gone:
        child.kill()
    else:
        child.ex.shutdown(wait=True)


# ---- both sides

def pixels(fmt, shape, seed):
    """a Fortran-ordered H x W x F x B array of format fmt: the values every format has to get right first (0, 255, 65535, fp16
    and bf16 subnormals, +-0, 65504), then random bit patterns without Inf / NaN"""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    if fmt == U8:
        a = rng.integers(0, 256, n, dtype=np.uint16).astype(np.uint8)
        a[:3] = (0, 255, 1)
    elif fmt == U16:
        a = rng.integers(0, 65536, n, dtype=np.uint32).astype(np.uint16)
        a[:4] = (0, 65535, 255, 256)
    else:
        a = rng.integers(0, 65536, n, dtype=np.uint32).astype(np.uint16)
        emask, eshift, mmask = (0x1F, 10, 0x83FF) if fmt == F16 else (0xFF, 7, 0x807F)
        special = ((a >> eshift) & emask) == emask
        a[special] &= np.uint16(0xBFFF)                  # no Inf / NaN
        sub = rng.random(n) < 0.1
        a[sub] &= np.uint16(mmask)                       # a share of subnormals (and zeros of both signs)
        if fmt == BF16:
            a &= np.uint16(0xBFFF)                       # |x| < 2: bf16 has fp32's range, and sums of 1e38 overflow the transform itself
        # +-0, the smallest and the largest subnormal of both signs' formats, +-65504 (bf16: 65280, its largest value below), 1
        a[:8] = (0x0000, 0x8000, 0x0001, 0x8001, 0x03FF, 0x7BFF, 0xFBFF, 0x3C00) if fmt == F16 else (0x0000, 0x8000, 0x0001, 0x8001, 0x007F, 0x477F, 0xC77F, 0x3F80)
        if fmt == F16:
            a = a.view(np.float16)
    return np.asfortranarray(a.reshape(shape, order="F"))


def exact_f32(a, fmt):
    """the exact float32 value of every element"""
    if fmt == BF16:
        return (a.astype(np.uint32) << 16).view(np.float32)
    return a.astype(np.float32)


# ---- the child's side

def _ctx():
    import torch
    return torch, util.load_package(), torch.device("cuda", 0)


def _kernels(torch, dev, F, kh, kw, n, seed):
    rng = np.random.default_rng(seed)
    ks = [np.asfortranarray(rng.standard_normal((kh, kw, F), dtype=np.float32)) for _ in range(n)]
    return ks, _pack_t(torch, ks).to(dev)


def _dev_image(torch, dev, a, odd_base=False):
    """the H x W x F x B array in device memory as the library reads it ([b][f][w][h]); odd_base: one element into its buffer"""
    flat = np.ascontiguousarray(np.transpose(a, (3, 2, 1, 0))).reshape(-1)
    raw = flat.view(np.int16) if flat.dtype.itemsize == 2 else flat
    t = torch.zeros(raw.size + 2, dtype=torch.from_numpy(raw[:1]).dtype, device=dev)
    off = 1 if odd_base else 0
    t[off:off + raw.size] = torch.from_numpy(raw).to(dev)
    return t, t.data_ptr() + off * flat.dtype.itemsize


def _maps(torch, dev, p, ker_d, n, kh, kw):
    """the packed maps of the images the plan holds, as bytes"""
    i = p.info
    out = torch.full((p.images() * n * i.out_h * i.out_w,), float("nan"), dtype=torch.float32, device=dev)
    p.convolve_packed_device(n, ker_d.data_ptr(), kh, kw, out.data_ptr())
    p.synchronize()
    return out.cpu().numpy().view(np.uint32)


def _three_ways(torch, dev, p, a, fmt, ker_d, n, kh, kw, odd_base=False, host=False):
    """(elements of the direct / default-route maps that differ from the fp32 path's, of the staged maps, pixel_direct, formats read back)"""
    B = a.shape[3]
    ref32 = np.asfortranarray(exact_f32(a, fmt))
    p.set_images(ref32)
    want = _maps(torch, dev, p, ker_d, n, kh, kw)
    fmts = [p.get_option("pixel_format")]
    assert not np.isnan(want.view(np.float32)).any()
    res = []
    for store in (1, 0):
        p.set_option("pixel_store", store)
        if host:
            p.set_images_typed(a, fmt)
        else:
            t, ptr = _dev_image(torch, dev, a, odd_base)
            p.set_images_typed_device(ptr, fmt, B)
        fmts.append(p.get_option("pixel_format"))
        res.append(int((_maps(torch, dev, p, ker_d, n, kh, kw) != want).sum()))
    p.set_option("pixel_store", 1)
    return res[0], res[1], p.get_option("pixel_direct"), fmts


def _case_configuration(M):
    """exact_window plans whose transform along h is 2M points on a 288-column window, one map: uint8 and fp16, an even and an odd
    H, direct == staged == fp32"""
    torch, fc, dev = _ctx()
    kh, kw, n = 13, 11, 1
    out = {}
    for H in (2 * M - 18, 2 * M - 19):
        _, ker_d = _kernels(torch, dev, 1, kh, kw, n, M)
        with fc.Plan(H, 272, 1, kh, kw, options={"exact_window": 1, "blockwise": 1}) as p:
            assert p.get_option("blockwise") == 0 and (p.info.fft_h, p.info.fft_w, p.info.transform_h) == (2 * M, 288, 2 * M)
            assert p.get_option("specialised_kernels") == 3
            for fmt in (U8, F16):
                d, s, direct, _ = _three_ways(torch, dev, p, pixels(fmt, (H, 272, 1, 1), M + fmt), fmt, ker_d, n, kh, kw)
                out[(H % 2, fmt)] = (direct, d, s)
    return out


def _case_formats(fmt, layout):
    """the smallest specialised plan (288 x 288 window), F = 2, B = 3; layout: H even (pair loads), H odd (odd pitch and plane
    stride), or a device pointer one element into its buffer"""
    torch, fc, dev = _ctx()
    kh, kw, n, F, B = 13, 11, 2, 2, 3
    H = 275 if layout == "odd" else 276
    _, ker_d = _kernels(torch, dev, F, kh, kw, n, 5)
    with fc.Plan(H, 272, F, kh, kw, options={"exact_window": 1}) as p:
        assert (p.info.fft_h, p.info.fft_w) == (288, 288) and p.get_option("specialised_kernels") == 3
        return _three_ways(torch, dev, p, pixels(fmt, (H, 272, F, B), 11 * fmt), fmt, ker_d, n, kh, kw, odd_base=layout == "base")


def _case_oracle():
    torch, fc, dev = _ctx()
    H, W, F, kh, kw, n = 276, 272, 2, 13, 11, 2
    a = pixels(U8, (H, W, F, 1), 3)
    ks, _ = _kernels(torch, dev, F, kh, kw, n, 9)
    with fc.Plan(H, W, F, kh, kw, options={"exact_window": 1}) as p:
        p.set_image_typed(a[:, :, :, 0])
        assert p.get_option("pixel_direct") == 1 and p.get_option("pixel_format") == U8
        got = p.convolve(ks)
    ref = util.Oracle().conv_fft(np.asfortranarray(a[:, :, :, 0].astype(np.float32)), kh, kw, ks)
    return [util.rel_err(g, r) for g, r in zip(got, ref)]


def _case_staged(kind):
    """plans without the typed column kernel: the generic column pass, a Bluestein window, overlap-save and overlap-add blocks"""
    torch, fc, dev = _ctx()
    H, W, F, kh, kw, options = KINDS[kind]
    n = 2
    _, ker_d = _kernels(torch, dev, F, kh, kw, n, 21)
    with fc.Plan(H, W, F, kh, kw, options=options) as p:
        facts = (p.get_option("blockwise") > 0, p.get_option("specialised_kernels") & 2, p.info.fft_h)
        a = pixels(U8, (H, W, F, 1), 31)
        res = [_three_ways(torch, dev, p, a, U8, ker_d, n, kh, kw), _three_ways(torch, dev, p, a, U8, ker_d, n, kh, kw, host=True)]
        refused = None
        if facts[0]:      # B > 1 on a block-wise plan: refused, the image stays
            before = _maps(torch, dev, p, ker_d, n, kh, kw)
            with pytest.raises(fc.FFTConvError) as e:
                p.set_images_typed(pixels(U8, (H, W, F, 2), 1))
            refused = (e.value.status, int((_maps(torch, dev, p, ker_d, n, kh, kw) != before).sum()), p.get_option("pixel_format"))
    return facts, res, refused


def _case_normalised(rect):
    torch, fc, dev = _ctx()
    H, W, F, kh, kw, n, B = 276, 272, 2, 13, 11, 2, 2
    _, ker_d = _kernels(torch, dev, F, kh, kw, n, 41)
    with fc.Plan(H, W, F, kh, kw, options={"exact_window": 1}) as p:
        p.set_normalisation(1, kh, kw)
        if rect:
            p.set_output_rect(5, 3, 271, 273)
        nd = p.get_option("norm_direct")
        return _three_ways(torch, dev, p, pixels(U8, (H, W, F, B), 43), U8, ker_d, n, kh, kw), nd


def _case_deferred():
    """defer_prepare with a preparation pending, then a typed image: the maps of the fp32 sequence"""
    torch, fc, dev = _ctx()
    H, W, F, kh, kw, n = 276, 272, 1, 13, 11, 3
    _, ker_d = _kernels(torch, dev, F, kh, kw, n, 51)
    a = pixels(F16, (H, W, F, 1), 53)
    t, ptr = _dev_image(torch, dev, a)
    t32, ptr32 = _dev_image(torch, dev, np.asfortranarray(exact_f32(a, F16)))
    out = []
    with fc.Plan(H, W, F, kh, kw, options={"exact_window": 1}) as p:
        p.set_option("defer_prepare", 1)
        for typed in (0, 1):
            p.prepare_kernels_packed_device(n, ker_d.data_ptr(), kh, kw)
            pending = p.get_option("prepare_pending")
            if typed:
                p.set_images_typed_device(ptr, F16, 1)
            else:
                p.set_images_device(ptr32, 1)
            out.append((pending, p.get_option("prepare_pending"), _maps(torch, dev, p, ker_d, n, kh, kw)))
    return out[0][:2], out[1][:2], int((out[0][2] != out[1][2]).sum())


def _case_host_routes(pinned):
    """typed host images below FC_PIN_INPLACE_BYTES, between it and FC_PIN_IMAGE_BYTES and above it -- in TYPED bytes: the fp32
    copies of the first two are beyond the limits they are within"""
    torch, fc, dev = _ctx()
    H, W, F, kh, kw, n = 276, 272, 1, 13, 11, 1
    _, ker_d = _kernels(torch, dev, F, kh, kw, n, 61)
    out = {}
    with fc.Plan(H, W, F, kh, kw, options={"exact_window": 1}) as p:
        p.set_option("host_pinned", pinned)
        for B in (6, 10, 15):
            nbytes = H * W * F * B
            assert (nbytes <= PIN_INPLACE, nbytes <= PIN_IMAGE) == {6: (True, True), 10: (False, True), 15: (False, False)}[B]
            assert 4 * nbytes > PIN_IMAGE
            a = pixels(U8, (H, W, F, B), 60 + B)
            d, s, direct, _ = _three_ways(torch, dev, p, a, U8, ker_d, n, kh, kw, host=True)
            a[...] = 0                                    # the caller's array was consumed on return
            out[B] = (direct, d, s)
        a16 = pixels(F16, (H, W, F, 2), 7)
        out["f16"] = _three_ways(torch, dev, p, a16, F16, ker_d, n, kh, kw, host=True)[:3]
    return out


def _case_state():
    torch, fc, dev = _ctx()
    H, W, F, kh, kw, n = 276, 272, 1, 13, 11, 2
    _, ker_d = _kernels(torch, dev, F, kh, kw, n, 71)
    a = pixels(U16, (H, W, F, 2), 73)
    lib = fc.load_library()
    out = {}
    with fc.Plan(H, W, F, kh, kw, options={"exact_window": 1}) as p:
        out["fresh"] = (p.get_option("pixel_format"), p.get_option("pixel_direct"), p.get_option("pixel_store"))
        p.set_images_typed(a)
        out["typed"] = (p.get_option("pixel_format"), p.get_option("images"))
        before = _maps(torch, dev, p, ker_d, n, kh, kw)
        t, ptr = _dev_image(torch, dev, a)
        errors = []
        for args in ((None, U16, 2, 0), (ptr, 5, 2, 1), (ptr, -1, 2, 1), (ptr, U16, 0, 1), (ptr, U16, 2, 7)):
            rc = lib.fftconv_plan_set_images_typed(p._h, ctypes.c_void_p(args[0]), args[1], args[2], args[3])
            errors.append(rc)
        sb = p.info.spectrum_bytes                                     # a caller's spectrum buffer that holds one image, not two
        big = torch.zeros(sb // 4, dtype=torch.float32, device=dev)
        out["errors"] = errors
        out["kept"] = (int((_maps(torch, dev, p, ker_d, n, kh, kw) != before).sum()), p.get_option("pixel_format"), p.get_option("images"))
        with pytest.raises(fc.FFTConvError):
            p.set_images_typed(np.zeros((H, W, 2), np.float32))
        with pytest.raises(fc.FFTConvError):
            p.set_images_typed(np.zeros((H, W, 2), np.uint16), pixel_format=F16)
        p.use_spectrum_buffer(big.data_ptr(), sb)
        out["one_image_buffer"] = (lib.fftconv_plan_set_images_typed(p._h, ctypes.c_void_p(ptr), U16, 2, 1), p.get_option("images"))
        p.use_spectrum_buffer(0, 0)
        out["store0"] = (p.set_option("pixel_store", 0), p.get_option("pixel_direct"), p.get_option("pixel_store"))
        p.set_option("pixel_store", 1)
        # fp32 again: the format reads 0 and the maps are the fp32 path's
        f32 = np.asfortranarray(exact_f32(a, U16)[:, :, :, 0])
        p.set_image(f32)
        out["after_set_image"] = (p.get_option("pixel_format"), p.get_option("images"))
        m32 = _maps(torch, dev, p, ker_d, n, kh, kw)
        p.set_image_typed(a[:, :, :, 0])
        out["single"] = (p.get_option("pixel_format"), int((_maps(torch, dev, p, ker_d, n, kh, kw) != m32).sum()))
        # format 0 through the typed entry is set_images itself
        rc = lib.fftconv_plan_set_images_typed(p._h, ctypes.c_void_p(f32.ctypes.data), 0, 1, 0)
        out["format0"] = (rc, p.get_option("pixel_format"), int((_maps(torch, dev, p, ker_d, n, kh, kw) != m32).sum()))
    return out


def _case_graph():
    """set_images_typed (device) + convolve_packed captured on a warm plan, replayed with new pixel contents"""
    torch, fc, dev = _ctx()
    H, W, F, kh, kw, n, B = 276, 272, 1, 13, 11, 2, 2
    _, ker_d = _kernels(torch, dev, F, kh, kw, n, 81)
    imgs = [pixels(U8, (H, W, F, B), 83 + j) for j in range(3)]
    flat = [torch.from_numpy(np.ascontiguousarray(np.transpose(a, (3, 2, 1, 0))).reshape(-1)).to(dev) for a in imgs]
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream), fc.Plan(H, W, F, kh, kw, stream=stream.cuda_stream, options={"exact_window": 1}) as p:
        i = p.info
        buf = flat[0].clone()
        out = torch.zeros(B * n * i.out_h * i.out_w, dtype=torch.float32, device=dev)
        replayed = [torch.empty_like(out) for _ in range(2)]
        eager = [torch.empty_like(out) for _ in range(2)]

        def step():
            p.set_images_typed_device(buf.data_ptr(), U8, B)
            p.convolve_packed_device(n, ker_d.data_ptr(), kh, kw, out.data_ptr())

        step()                                   # eager warm-up: sizes the scratch; nothing allocates from here on
        torch.cuda.synchronize()
        p.set_option("verbose", 0)               # (refreshes p.info)
        ws = p.info.workspace_bytes
        graph = torch.cuda.CUDAGraph()
        cap = torch.cuda.Stream(dev)
        with torch.cuda.graph(graph, stream=cap):
            p.set_stream(torch.cuda.current_stream(dev).cuda_stream)
            step()
        p.set_stream(stream.cuda_stream)
        for r in range(2):                       # nothing synchronised inside the loop
            out.fill_(float("nan"))
            buf.copy_(flat[r + 1], non_blocking=True)
            graph.replay()
            replayed[r].copy_(out)
        torch.cuda.synchronize()
        for r in range(2):
            out.fill_(float("nan"))
            buf.copy_(flat[r + 1], non_blocking=True)
            step()
            eager[r].copy_(out)
        torch.cuda.synchronize()
        p.set_option("verbose", 0)               # (refreshes p.info)
        same_ws = ws > 0 and p.info.workspace_bytes == ws
        direct = p.get_option("pixel_direct")
        got = [t.cpu().numpy().view(np.uint32) for t in replayed]
        want = [t.cpu().numpy().view(np.uint32) for t in eager]
    nans = [int(np.isnan(g.view(np.float32)).sum()) for g in got]
    return [int((g != w).sum()) for g, w in zip(got, want)], bool(np.array_equal(got[0], got[1])), direct, same_ws, nans


# ---- the tests

@pytest.mark.parametrize("M", sorted(col_table()))
def test_every_configuration_is_bit_equal(device, M):
    """every built configuration of the forward column kernel: uint8 and fp16, even and odd H, direct == staged == fp32;
    pixel_direct reads 1, or 0 exactly for the configurations listed as not built"""
    res = device("_case_configuration", M)
    print(M, res)
    want = 0 if M in NOT_BUILT else 1
    assert res == {(odd, fmt): (want, 0, 0) for odd in (0, 1) for fmt in (U8, F16)}, (M, res)


@pytest.mark.parametrize("layout", ["even", "odd", "base"])
@pytest.mark.parametrize("fmt", [U8, U16, F16, BF16])
def test_formats_and_alignment(device, fmt, layout):
    direct_differs, staged_differs, direct, fmts = device("_case_formats", fmt, layout)
    print(fmt, layout, direct_differs, staged_differs, direct, fmts)
    assert (direct_differs, staged_differs, direct) == (0, 0, 1)
    assert fmts == [0, fmt, fmt]


def test_against_the_float64_oracle(device):
    errs = device("_case_oracle")
    print("uint8 image, direct route, against the float64 oracle: max |out - ref| / max |ref| =", errs)
    assert all(e <= 1e-5 for e in errs), errs


@pytest.mark.parametrize("kind", ["generic", "bluestein", "save_blocks", "add_blocks"])
def test_staged_kinds(device, kind):
    facts, res, refused = device("_case_staged", kind)
    print(kind, facts, res, refused)
    blockwise = kind in ("save_blocks", "add_blocks")
    assert facts[0] == blockwise
    if kind == "generic":
        assert facts[1] == 0
    if kind == "bluestein":
        assert facts[2] == 304
    for d, s, direct, fmts in res:
        assert (d, s, direct) == (0, 0, 0) and fmts == [0, 1, 1], res
    if blockwise:
        assert refused == (-1, 0, 1), refused


@pytest.mark.parametrize("rect", [0, 1])
def test_normalised_maps(device, rect):
    (d, s, direct, fmts), norm_direct = device("_case_normalised", rect)
    print(rect, d, s, direct, fmts, norm_direct)
    assert (d, s, direct, norm_direct) == (0, 0, 1, 1) and fmts == [0, 1, 1]


def test_deferred_preparation(device):
    fp32, typed, differ = device("_case_deferred")
    print(fp32, typed, differ)
    assert fp32 == (1, 0) and typed == (1, 0) and differ == 0


@pytest.mark.parametrize("pinned", [1, 0])
def test_host_routes(device, pinned):
    res = device("_case_host_routes", pinned)
    print(pinned, res)
    assert res == {6: (1, 0, 0), 10: (1, 0, 0), 15: (1, 0, 0), "f16": (0, 0, 1)}, res


def test_state(device):
    out = device("_case_state")
    print(out)
    assert out["fresh"] == (0, 1, 1)
    assert out["typed"] == (U16, 2)
    assert out["errors"] == [-1] * 5
    assert out["kept"] == (0, U16, 2)
    assert out["one_image_buffer"] == (-1, 0)       # (use_spectrum_buffer itself left the plan without an image)
    assert out["store0"] == (None, 0, 0)
    assert out["after_set_image"] == (0, 1)
    assert out["single"] == (U16, 0)
    assert out["format0"] == (0, 0, 0)


def test_graph_replay(device):
    replay_vs_eager, same_twice, direct, same_ws, nans = device("_case_graph")
    print(replay_vs_eager, same_twice, direct, same_ws, nans)
    assert replay_vs_eager == [0, 0] and nans == [0, 0]      # each replay is the eager step on the same pixels, bit for bit
    assert not same_twice                                    # (and the two replays did see different pixels)
    assert direct == 1 and same_ws                           # nothing was allocated after the warm-up step
