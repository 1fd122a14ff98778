"""Image batches on the GPU: one plan convolves B images per launch set (fftconv_plan_set_images), through the C ABI.

Every fp32 map is held to the float64 oracle within 1e-5 of the map's own maximum (util.rel_err: the bar of tools/fuzz_gpu.py and
tests/plan_walk.py); a 16-bit map gets the same bar plus half an ulp of its format at the element; a rectangle is measured against
its window's maximum.  The shapes are the smallest at which each spectral-row kernel family exists: 288-point specialised rows
(F = 1 walk, F = 2 walk over (image, walk) pairs), 1152-point specialised rows over generic columns with pinned in-place inputs,
the generic kernels (kernel_path 1, F = 1 and 3) and Bluestein rows (window 304).  The oracle's maps are computed once per shape."""
import numpy as np
import pytest

import util

pytestmark = pytest.mark.gpu
BAR = 1e-5

S288 = (270, 270, 1, 19, 19)          # 288-point transforms both ways, specialised kernels
_REFS = {}


@pytest.fixture(scope="module")
def fc(fftconv):
    assert fftconv.device_count() >= 1, "GPU tests need a GPU (no CPU fallback exists)"
    return fftconv


@pytest.fixture(scope="module")
def torch_dev():
    torch = pytest.importorskip("torch")
    return torch, torch.device("cuda", 0)


def _inputs(shape, B, n, seed=0, ragged=False):
    """images H x W x F x B (Fortran order), n kernels kh x kw x F (ragged: the second one smaller)"""
    H, W, F, kh, kw = shape
    rng = np.random.default_rng(4000 + seed)
    imgs = np.asfortranarray(rng.random((H, W, F, B), dtype=np.float32))
    ks = [np.asfortranarray(rng.random((kh, kw, F), dtype=np.float32)) for _ in range(n)]
    if ragged:
        ks[1] = np.asfortranarray(rng.random((max(1, kh - 4), max(1, kw // 3), F), dtype=np.float32))
    return imgs, ks


def _refs(oracle, shape, B, n, seed=0, ragged=False, flip=False):
    """the float64 oracle's maps, image-major: map b * n + k = image b (x) kernel k; computed once per case and left unchanged"""
    key = (shape, B, n, seed, ragged, flip)
    if key not in _REFS:
        imgs, ks = _inputs(shape, B, n, seed, ragged)
        kk = [np.asfortranarray(k[::-1, ::-1, :]) for k in ks] if flip else ks
        out = []
        for b in range(B):
            out += oracle.conv_fft(np.asfortranarray(imgs[:, :, :, b]), shape[3], shape[4], kk, f64=True)
        for o in out:
            o.setflags(write=False)
        _REFS[key] = out
    return _REFS[key]


def _check32(got, refs, what=""):
    assert len(got) == len(refs), (len(got), len(refs))
    for j, (g, r) in enumerate(zip(got, refs)):
        g = np.asarray(g)
        assert g.shape == r.shape, (what, j, g.shape, r.shape)
        err = util.rel_err(g, r)
        assert err < BAR, "%s map %d: %.3g of the map's maximum" % (what, j, err)


def _half_ulp(v, fmt):
    """half an ulp of the 16-bit format at |v| (fp16: 11 significant bits, subnormals below 2^-14; bf16: 8 bits)"""
    a = np.maximum(np.abs(v), 1e-300)
    e = np.floor(np.log2(a))
    if fmt == 1:
        e = np.maximum(e, -14)
        return np.ldexp(1.0, (e - 11).astype(np.int64))
    return np.ldexp(1.0, (e - 8).astype(np.int64))


def _as_f64(a, fmt):
    a = np.asarray(a)
    if fmt == 2:
        return (a.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    return a.astype(np.float64)


def _check16(got, refs, fmt, what=""):
    assert len(got) == len(refs)
    for j, (g, r) in enumerate(zip(got, refs)):
        g = _as_f64(g, fmt)
        assert g.shape == r.shape and np.isfinite(g).all()
        bound = BAR * np.abs(r).max() + _half_ulp(np.maximum(np.abs(g), np.abs(r)), fmt)
        worst = float((np.abs(g - r) - bound).max())
        assert worst <= 0, "%s map %d: %.3g beyond the bar plus half an ulp" % (what, j, worst)


def _packed(torch, dev, p, imgs, ks, B, images_on_device=True):
    """set_images + convolve_packed on device-resident data; returns the B * n maps (numpy, H-major as the oracle's)"""
    H, W, F = imgs.shape[:3]
    n, kh, kw = len(ks), ks[0].shape[0], ks[0].shape[1]
    k_d = torch.from_numpy(np.ascontiguousarray(np.stack([np.transpose(k, (2, 1, 0)) for k in ks]))).to(dev)
    if images_on_device:
        i_d = torch.from_numpy(np.ascontiguousarray(np.transpose(imgs, (3, 2, 1, 0)))).to(dev)      # [b][f][w][h]
        p.set_images_device(i_d.data_ptr(), B)
    else:
        p.set_images(imgs)
    p.refresh_info()
    oh, ow = p.info.out_h, p.info.out_w
    out = torch.full((B * n, ow, oh), float("nan"), dtype=torch.float32, device=dev)
    p.convolve_packed_device(n, k_d.data_ptr(), kh, kw, out.data_ptr())
    p.synchronize()
    got = out.cpu().numpy()
    return [got[j].T for j in range(B * n)]


# ---- the kernel families

@pytest.mark.parametrize("B,n,batch_maps,chunk_mb", [(3, 20, 0, 0), (3, 2, 4, 0), (2, 5, 3, 0), (2, 5, 3, 512), (3, 7, 2, 512)],
                         ids=["one launch: walk boundary at 16 and image boundaries", "whole-image launches 2 + 1", "kernel ranges of one image",
                              "one chunk of 5 kernels, launches of 3: offsets into the chunk, per image", "one chunk of 7 kernels, launches of 2"])
def test_specialised_f1(fc, oracle, torch_dev, B, n, batch_maps, chunk_mb):
    torch, dev = torch_dev
    imgs, ks = _inputs(S288, B, n)
    with fc.Plan(*S288) as p:
        assert p.get_option("specialised_kernels") == 3 and (p.info.transform_h, p.info.transform_w) == (288, 288)
        assert p.get_option("images") == 0
        p.set_option("batch_maps", batch_maps)
        p.set_option("kernel_chunk_mb", chunk_mb)       # > 0: a column-spectrum chunk holds several launches' worth of kernels
        p.set_option("profile", 1)
        got = _packed(torch, dev, p, imgs, ks, B)
        assert p.get_option("images") == B
        _check32(got, _refs(oracle, S288, B, n), "F = 1")
        pr = p.profile()
        if chunk_mb:        # the chunk's column spectra are produced once and serve every launch of every image
            assert pr["kernel_cols"]["launches"] == 1 and pr["kernel_cols"]["units"] == n, pr
            assert pr["spectral_rows"]["launches"] == B * -(-n // batch_maps) and pr["spectral_rows"]["units"] == B * n, pr


def test_specialised_f2_walks_over_image_walk_pairs(fc, oracle, torch_dev):
    torch, dev = torch_dev
    shape, B, n = (270, 270, 2, 19, 19), 2, 3
    imgs, ks = _inputs(shape, B, n)
    with fc.Plan(*shape) as p:
        assert p.get_option("specialised_kernels") == 3
        _check32(_packed(torch, dev, p, imgs, ks, B), _refs(oracle, shape, B, n), "F = 2")
        p.set_option("rows_group", 2)          # two walks per image: (image, walk) pairs on the flat grid
        _check32(_packed(torch, dev, p, imgs, ks, B), _refs(oracle, shape, B, n), "F = 2, walks of 2")


def test_specialised_rows_with_pinned_in_place_inputs(fc, oracle):
    """48 x 1152 transform: specialised rows over generic columns; the host batch (344 KiB) and the host kernels are read in
    place from the plan's pinned buffers"""
    shape, B, n = (40, 1100, 1, 9, 40), 2, 2
    imgs, ks = _inputs(shape, B, n)
    with fc.Plan(*shape) as p:
        assert p.get_option("specialised_kernels") & 1 and (p.info.transform_h, p.info.transform_w) == (48, 1152)
        p.set_images(imgs)
        _check32(p.convolve(ks), _refs(oracle, shape, B, n), "48 x 1152")


@pytest.mark.parametrize("F", [1, 3])
def test_generic_kernels(fc, oracle, torch_dev, F):
    torch, dev = torch_dev
    shape, B, n = (40, 56, F, 5, 7), 3, 2
    imgs, ks = _inputs(shape, B, n)
    with fc.Plan(*shape, options={"kernel_path": 1}) as p:
        assert p.get_option("specialised_kernels") == 0
        _check32(_packed(torch, dev, p, imgs, ks, B), _refs(oracle, shape, B, n), "generic F = %d" % F)
        p.set_images(imgs)
        _check32(p.convolve(ks), _refs(oracle, shape, B, n), "generic F = %d, host" % F)


def test_bluestein_rows(fc, oracle, torch_dev):
    torch, dev = torch_dev
    shape, B, n = (290, 290, 1, 15, 15), 2, 2
    imgs, ks = _inputs(shape, B, n)
    with fc.Plan(*shape, options={"exact_window": 1}) as p:
        assert p.info.exact_window == 1 and (p.info.fft_h, p.info.fft_w) == (304, 304) and p.get_option("specialised_kernels") == 0
        _check32(_packed(torch, dev, p, imgs, ks, B), _refs(oracle, shape, B, n), "Bluestein")


# ---- entries and routes

def test_host_routes(fc, oracle):
    """fftconv_plan_convolve to host arrays: the pinned small-map route, then the copy threads and the pinned ring (host_stream 1
    and 2 with host_min_kb 0, the smallest value that selects them for 324-KiB maps)"""
    B, n = 3, 2
    imgs, ks = _inputs(S288, B, n)
    refs = _refs(oracle, S288, B, n)
    with fc.Plan(*S288) as p:
        p.set_images(imgs)
        _check32(p.convolve(ks), refs, "pinned route")
        for hs in (1, 2):
            p.set_option("host_min_kb", 0)
            p.set_option("host_stream", hs)
            p.set_option("batch_maps", 4)          # two batches: the copy-out of one overlaps the next
            _check32(p.convolve(ks), refs, "host_stream %d" % hs)
        p.set_option("host_stream", 0)
        p.set_option("host_pinned", 0)
        _check32(p.convolve(ks), refs, "blocking copies")


def test_device_pointers_and_ragged_cells(fc, oracle, torch_dev):
    torch, dev = torch_dev
    B, n = 2, 4
    imgs, ks = _inputs(S288, B, n, seed=1, ragged=True)
    refs = _refs(oracle, S288, B, n, seed=1, ragged=True)
    with fc.Plan(*S288) as p:
        p.set_images(imgs)
        _check32(p.convolve(ks), refs, "ragged, host")       # groups {0}, {1}, {2, 3}: out[b * 4 + k]
        outs = [torch.full((p.info.fft_w, p.info.fft_h), float("nan"), dtype=torch.float32, device=dev) for _ in range(B * n)]
        p.convolve_to_device(ks, [o.data_ptr() for o in outs])
        p.synchronize()
        _check32([o.cpu().numpy().T for o in outs], refs, "ragged, device pointers")
        with pytest.raises(fc.FFTConvError):
            p.convolve_to_device(ks, [o.data_ptr() for o in outs[:n]])       # B * n pointers are needed


@pytest.mark.parametrize("defer", [0, 1])
def test_prepared_kernels_survive_set_images(fc, oracle, torch_dev, defer):
    torch, dev = torch_dev
    B, n = 2, 3
    imgs, ks = _inputs(S288, B, n)
    refs = _refs(oracle, S288, B, n)
    kh, kw = ks[0].shape[:2]
    k_d = torch.from_numpy(np.ascontiguousarray(np.stack([np.transpose(k, (2, 1, 0)) for k in ks]))).to(dev)
    i_d = torch.from_numpy(np.ascontiguousarray(np.transpose(imgs, (3, 2, 1, 0)))).to(dev)
    with fc.Plan(*S288) as p:
        p.set_option("defer_prepare", defer)
        out = torch.full((B * n, p.info.fft_w, p.info.fft_h), float("nan"), dtype=torch.float32, device=dev)
        for _ in range(2):        # (the second round runs on warm buffers)
            p.set_option("profile", 0)       # (a profiled plan times the kernels' column pass apart and does not defer it)
            p.prepare_kernels_packed_device(n, k_d.data_ptr(), kh, kw)
            assert p.get_option("prepare_pending") == defer
            p.set_images_device(i_d.data_ptr(), B)
            assert p.get_option("prepare_pending") == 0
            p.set_option("profile", 1)
            p.profile()
            p.convolve_packed_device(n, k_d.data_ptr(), kh, kw, out.data_ptr())
            p.synchronize()
            assert p.profile()["kernel_cols"]["launches"] == 0       # the prepared column spectra were used
            got = out.cpu().numpy()
            _check32([got[j].T for j in range(B * n)], refs, "prepared, defer %d" % defer)


# ---- output options on a batch

def test_output_options(fc, oracle, torch_dev):
    torch, dev = torch_dev
    B, n = 2, 2
    H, W, F, kh, kw = S288
    imgs, ks = _inputs(S288, B, n)
    refs = _refs(oracle, S288, B, n)
    with fc.Plan(*S288) as p:
        p.set_images(imgs)
        for fmt in (1, 2):
            p.set_option("map_format", fmt)
            _check16(p.convolve(ks), refs, fmt, "map_format %d" % fmt)
        p.set_option("map_format", 0)
        rect = (5, 3, 281, 283)             # odd offsets, odd sizes
        crops = [r[rect[0]:rect[0] + rect[2], rect[1]:rect[1] + rect[3]] for r in refs]
        for store in (1, 0):
            p.set_option("rect_store", store)
            p.set_output_rect(*rect)
            assert p.get_option("rect_direct") == store
            _check32(_packed(torch, dev, p, imgs, ks, B), crops, "rectangle, rect_store %d" % store)
            _check32(p.convolve(ks), crops, "rectangle, rect_store %d, host" % store)
        p.set_option("rect_store", 1)
        p.set_option("output_region", 2)
        same = [r[(kh - 1) // 2:(kh - 1) // 2 + H, (kw - 1) // 2:(kw - 1) // 2 + W] for r in refs]
        _check32(_packed(torch, dev, p, imgs, ks, B), same, "output_region 2")
        p.set_option("output_region", 0)
        p.set_option("flip_kernels", 1)
        _check32(_packed(torch, dev, p, imgs, ks, B), _refs(oracle, S288, B, n, flip=True), "flip_kernels")


# ---- isolation, launch counts, state

def test_images_are_isolated(fc, torch_dev):
    torch, dev = torch_dev
    B, n = 3, 2
    imgs, ks = _inputs(S288, B, n)
    with fc.Plan(*S288) as p:
        a = _packed(torch, dev, p, imgs, ks, B)
        other = imgs.copy(order="F")
        other[:, :, :, 1] = _inputs(S288, 1, 1, seed=9)[0][:, :, :, 0]
        b = _packed(torch, dev, p, other, ks, B)
    for img in (0, 2):
        for k in range(n):
            assert np.array_equal(a[img * n + k].view(np.uint32), b[img * n + k].view(np.uint32)), (img, k)
    for k in range(n):
        assert not np.array_equal(a[n + k], b[n + k])


def test_launch_counts(fc, torch_dev):
    """B = 3, N = 2 within one launch's capacity: one spectral-row launch and one output launch for the six maps, and the image
    transform takes the launches of a single image"""
    torch, dev = torch_dev
    B, n = 3, 2
    imgs, ks = _inputs(S288, B, n)
    with fc.Plan(*S288) as p:
        p.set_option("profile", 1)
        p.set_image(np.asfortranarray(imgs[:, :, :, 0]))
        p.synchronize()
        one = p.profile()
        _packed(torch, dev, p, imgs, ks, B)
        pr = p.profile()
        assert pr["spectral_rows"]["launches"] == 1 and pr["spectral_rows"]["units"] == B * n, pr
        assert pr["cols_c2r"]["launches"] == 1 and pr["cols_c2r"]["units"] == B * n, pr
        assert pr["kernel_cols"]["launches"] == 1 and pr["kernel_cols"]["units"] == n, pr
        for kind in ("image_cols", "image_rows"):
            assert pr[kind]["launches"] == one[kind]["launches"] == 1, (kind, pr, one)
            assert pr[kind]["units"] == B * one[kind]["units"], (kind, pr, one)


def test_state(fc, oracle, torch_dev):
    torch, dev = torch_dev
    n = 2
    imgs, ks = _inputs(S288, 3, n)
    refs = _refs(oracle, S288, 3, n)
    with fc.Plan(*S288) as p:
        sb = p.info.spectrum_bytes
        p.set_images(imgs)
        assert p.get_option("images") == 3 and p.spectrum()[1] == 3 * sb and p.refresh_info().spectrum_bytes == sb
        p.set_image(np.asfortranarray(imgs[:, :, :, 1]))
        assert p.get_option("images") == 1 and p.spectrum()[1] == sb
        _check32(p.convolve(ks), refs[n:2 * n], "set_image after set_images(3)")
        p.set_images(imgs)
        p.set_images(np.asfortranarray(imgs[:, :, :, :2]))
        assert p.get_option("images") == 2 and p.spectrum()[1] == 2 * sb
        got = p.convolve(ks)
        assert len(got) == 2 * n
        _check32(got, refs[:2 * n], "set_images(2) after set_images(3)")
        # a spectrum of the batch in a one-image plan: slot 2 of a caller-owned buffer the batch was transformed into
        buf = torch.zeros(3 * sb, dtype=torch.uint8, device=dev)
        p.use_spectrum_buffer(buf.data_ptr(), 3 * sb)
        assert p.get_option("images") == 0
        p.set_images(imgs)
        p.synchronize()
        with fc.Plan(*S288) as q:
            q.use_spectrum_buffer(buf.data_ptr() + 2 * sb, sb)
            q.mark_spectrum_valid()
            assert q.get_option("images") == 1
            _check32(q.convolve(ks), refs[2 * n:], "slot 2 of the batch's spectra")
        p.use_spectrum_buffer(0, 0)


def test_refusals(fc, oracle, torch_dev):
    torch, dev = torch_dev
    n = 2
    # a block-wise plan holds one image
    shape = (100, 100, 1, 9, 9)
    imgs, ks = _inputs(shape, 2, n)
    with fc.Plan(*shape, options={"max_transform": 64}) as p:
        assert p.get_option("blockwise") > 0
        p.set_image(np.asfortranarray(imgs[:, :, :, 0]))
        with pytest.raises(fc.FFTConvError) as e:
            p.set_images(imgs)
        assert e.value.status == -1 and "block-wise" in str(e.value)
        assert p.get_option("images") == 1
        _check32(p.convolve(ks), _refs(oracle, shape, 2, n)[:n], "block-wise plan after the refusal")
        p.set_images(np.asfortranarray(imgs[:, :, :, 1:]))          # a batch of one is one image
        _check32(p.convolve(ks), _refs(oracle, shape, 2, n)[n:], "block-wise plan, batch of one")
    # the spectrum in the reference's order is exchanged for one image
    shape = (274, 274, 1, 15, 15)
    imgs, ks = _inputs(shape, 2, n)
    with fc.Plan(*shape, options={"exact_window": 1}) as p:
        p.set_images(imgs)
        with pytest.raises(fc.FFTConvError) as e:
            p.export_spectrum()
        assert e.value.status == -1 and "2 images" in str(e.value)
        spec = np.zeros((1, p.info.fft_w, p.info.fft_h // 2 + 1), dtype=np.complex64)
        with pytest.raises(fc.FFTConvError) as e:
            p.import_spectrum(spec)
        assert e.value.status == -1 and "2 images" in str(e.value)
        assert p.get_option("images") == 2
        _check32(p.convolve(ks), _refs(oracle, shape, 2, n), "exact_window plan after the refusals")
        p.set_image(np.asfortranarray(imgs[:, :, :, 0]))
        assert p.export_spectrum().shape == spec.shape
    # a caller's spectrum buffer must hold the batch
    imgs, ks = _inputs(S288, 2, n)
    with fc.Plan(*S288) as p:
        sb = p.info.spectrum_bytes
        buf = torch.zeros(2 * sb, dtype=torch.uint8, device=dev)
        p.use_spectrum_buffer(buf.data_ptr(), sb)
        p.set_image(np.asfortranarray(imgs[:, :, :, 1]))
        with pytest.raises(fc.FFTConvError) as e:
            p.set_images(imgs)
        assert e.value.status == -1 and "spectrum buffer" in str(e.value)
        assert p.get_option("images") == 1
        _check32(p.convolve(ks), _refs(oracle, S288, 2, n)[n:], "after the too-small buffer")
        p.use_spectrum_buffer(buf.data_ptr(), 2 * sb)
        p.set_images(imgs)
        _check32(p.convolve(ks), _refs(oracle, S288, 2, n), "a buffer that holds the batch")
        p.use_spectrum_buffer(0, 0)
    with fc.Plan(*S288) as p:
        with pytest.raises(fc.FFTConvError) as e:
            p.set_images_device(1 << 20, 0)
        assert e.value.status == -1 and "n_images" in str(e.value)
