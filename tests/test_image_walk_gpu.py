"""The image-walk spectral-row kernel on the GPU (plan option "image_walk", csrc/fast_rows_images.hpp), through the C ABI.

With "image_walk" 1 a spectral-row launch of more than one image keeps the transformed kernel row in registers and walks over the
images of the launch.  Every fp32 map is held to the float64 oracle within 1e-5 of the map's own maximum (util.rel_err: the bar of
tests/test_image_batch_gpu.py); where a claim is "the same bytes" the maps are compared as bits.  Each case reads from the plan
(read-only option "image_walk_active") and from its verbose log which walk ran and how long.  Transform sizes are what the
planner gives (asserted from plan.info); the oracle's maps are computed once per shape and shared."""
import concurrent.futures
import os
import re

import numpy as np
import pytest

import util
from test_features_gpu import _logged
from test_image_batch_gpu import _check16, _check32, _packed

pytestmark = pytest.mark.gpu
BAR = 1e-5

# image H x W (*) kernel kh x kw -> transform (h, w)
SHAPES = {
    "288: RPW 8, two chains": ((250, 250, 1, 31, 31), (288, 288)),
    "384: RPW 6, cropped store": ((270, 270, 1, 31, 31), (384, 384)),
    "2560: RPW 1, R1 = 16, cropped": ((250, 2500, 1, 9, 41), (288, 2560)),
    "2816: RPW 1, R3 = 22": ((250, 2700, 1, 9, 41), (288, 2816)),
    "2112: RPW 2, two chains at R3 = 22": ((250, 2100, 1, 9, 13), (288, 2112)),
    "1152: row-major intermediate": ((40, 1100, 1, 9, 31), (48, 1152)),
}
S288 = SHAPES["288: RPW 8, two chains"][0]


def _built_lengths():
    """the row lengths whose image-walk kernel is built: the lengths of csrc/fast_paths.hpp's configuration list less the entries of
    fast_rows_images_built's list, read from the header so that the sweep follows it"""
    src = open(os.path.join(util.ROOT, "cuda-fft-convolution_amd", "csrc", "fast_paths.hpp")).read()
    listed = {int(x) for x in re.findall(r"^\s+X\((\d+), \d+, \d+, \d+, \d+, \d+, \d+\)", src, re.M)}
    not_built = {int(x) for x in re.search(r"FC_ROWS_IMAGES_NOT_BUILT\[\] = \{([^}]*)\}", src).group(1).split(",") if x.strip()}
    assert len(listed) == 32 and not_built <= listed, (sorted(listed), sorted(not_built))
    return sorted(listed - not_built, reverse=True)


BUILT = _built_lengths()
_REFS = {}
WALK_LINE = re.compile(r"spectral rows \(specialised, \d+ rows x \d+ points, image walk: (\d+) images per workgroup\)")


@pytest.fixture(scope="module")
def fc(fftconv):
    assert fftconv.device_count() >= 1, "GPU tests need a GPU (no CPU fallback exists)"
    return fftconv


@pytest.fixture(scope="module")
def torch_dev():
    torch = pytest.importorskip("torch")
    return torch, torch.device("cuda", 0)


def _inputs(shape, B, n, seed=0):
    H, W, F, kh, kw = shape
    rng = np.random.default_rng(7000 + seed)
    imgs = np.asfortranarray(rng.random((H, W, F, B), dtype=np.float32))
    ks = [np.asfortranarray(rng.random((kh, kw, F), dtype=np.float32)) for _ in range(n)]
    return imgs, ks


def _refs(oracle, shape, B, n, seed=0, flip=False):
    """float64 oracle maps, image-major (map b * n + k), computed once per case and left unchanged"""
    key = (shape, B, n, seed, flip)
    if key not in _REFS:
        imgs, ks = _inputs(shape, B, n, seed)
        kk = [np.asfortranarray(k[::-1, ::-1, :]) for k in ks] if flip else ks
        # (the oracle threads over the kernels of a call and keeps no state between calls: the images run side by side)
        with concurrent.futures.ThreadPoolExecutor(max_workers=4) as ex:
            per_image = list(ex.map(lambda b: oracle.conv_fft(np.asfortranarray(imgs[:, :, :, b]), shape[3], shape[4], kk, f64=True), range(B)))
        out = [o for maps in per_image for o in maps]
        for o in out:
            o.setflags(write=False)
        _REFS[key] = out
    return _REFS[key]


def _walks(log):
    """images per workgroup of every image-walk launch the verbose log names"""
    return [int(m.group(1)) for m in map(WALK_LINE.search, log.splitlines()) if m]


def _run(torch, dev, p, imgs, ks, B):
    """(maps, image walks of the call) of set_images + convolve_packed with the verbose log on"""
    p.set_option("verbose", 1)
    got, log = _logged(lambda: _packed(torch, dev, p, imgs, ks, B))
    p.set_option("verbose", 0)
    assert len([l for l in log.splitlines() if "spectral rows (" in l]) >= 1, log
    return got, _walks(log)


def _dev_inputs(torch, dev, imgs, ks):
    """device tensors [b][f][w][h] of the images and [n][f][kw][kh] of the kernels"""
    i_d = torch.from_numpy(np.ascontiguousarray(np.transpose(imgs, (3, 2, 1, 0)))).to(dev)
    k_d = torch.from_numpy(np.ascontiguousarray(np.stack([np.transpose(k, (2, 1, 0)) for k in ks]))).to(dev)
    return i_d, k_d


def _run_t(torch, dev, p, i_d, k_d, log=True):
    """(maps as a device tensor [B * n][w][h], image walks of the call) of set_images + convolve_packed.  The large shapes are
    judged on the device: the same figure as util.rel_err, in float64, without 57 maps crossing to the host per run"""
    B, n, kw, kh = i_d.shape[0], k_d.shape[0], k_d.shape[2], k_d.shape[3]
    p.set_images_device(i_d.data_ptr(), B)
    p.refresh_info()
    out = torch.full((B * n, p.info.out_w, p.info.out_h), float("nan"), dtype=torch.float32, device=dev)

    def run():
        p.convolve_packed_device(n, k_d.data_ptr(), kh, kw, out.data_ptr())
        p.synchronize()
    if not log:
        run()
        return out, None
    p.set_option("verbose", 1)
    _, text = _logged(run)
    p.set_option("verbose", 0)
    assert len([l for l in text.splitlines() if "spectral rows (" in l]) >= 1, text
    return out, _walks(text)


def _refs_t(torch, dev, refs):
    return torch.from_numpy(np.ascontiguousarray(np.stack([r.T for r in refs]))).to(dev)        # float64 [maps][w][h]


def _check_t(got, want, what):
    """every map within BAR of its own maximum (util.rel_err: max |a - b| / max |b|, in float64; a NaN fails)"""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = (got.double() - want).abs().amax(dim=(1, 2)) / want.abs().amax(dim=(1, 2))
    assert bool((err < BAR).all()), "%s: worst map %.3g of its maximum" % (what, float(err.nan_to_num(nan=float("inf")).max()))


def _same_bits_t(torch, a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _same_bits(a, b):
    return len(a) == len(b) and all(np.array_equal(np.asarray(x).view(np.uint32), np.asarray(y).view(np.uint32)) for x, y in zip(a, b))


def _walk_plan(fc, shape, transform, **options):
    p = fc.Plan(*shape, options=options or None)
    assert (p.info.transform_h, p.info.transform_w) == transform, (p.info.transform_h, p.info.transform_w)
    assert p.get_option("image_walk") == 0 and p.get_option("image_walk_active") == 0
    p.set_option("image_walk", 1)
    assert p.get_option("image_walk") == 1 and p.get_option("image_walk_active") == 1
    return p


# ---- correctness against the oracle

@pytest.mark.parametrize("name", list(SHAPES))
def test_matches_oracle(fc, oracle, torch_dev, name):
    """(B, N) = (19, 3) and (5, 1) -- the first five images and the first kernel of the same inputs -- with "batch_maps" such that
    a launch holds 19, 4 and 1 images: walks of 16 + 3 ("rows_group" 16), walks of 4 with a launch of the remainder, and the
    launches of one image, which run the kernel walk and return the bytes of "image_walk" 0"""
    torch, dev = torch_dev
    shape, transform = SHAPES[name]
    i_d, k_d = _dev_inputs(torch, dev, *_inputs(shape, 19, 3))
    refs = _refs_t(torch, dev, _refs(oracle, shape, 19, 3))
    with _walk_plan(fc, shape, transform, rows_group=16) as p:
        for B, n in ((19, 3), (5, 1)):
            im, kk = i_d[:B], k_d[:n]
            want = refs[[b * 3 + k for b in range(B) for k in range(n)]]
            for per_launch in (19, 4, 1):
                p.set_option("batch_maps", per_launch * n)
                got, walks = _run_t(torch, dev, p, im, kk)
                _check_t(got, want, "%s, B %d N %d, %d images per launch" % (name, B, n, per_launch))
                if per_launch == 19:
                    assert walks == [min(16, B)], walks
                elif per_launch == 4:
                    assert walks == [4] * (B // 4) + ([B % 4] if B % 4 > 1 else []), walks       # (a last launch of one image: the kernel walk)
                else:
                    assert walks == []
                    p.set_option("image_walk", 0)
                    assert p.get_option("image_walk_active") == 0
                    zero, _ = _run_t(torch, dev, p, im, kk, log=False)
                    assert _same_bits_t(torch, got, zero), "one image per launch: not the bytes of image_walk 0"
                    p.set_option("image_walk", 1)
        # the automatic walk length (rows_group -1): whatever it is, the same bytes
        p.set_option("batch_maps", 57)
        fixed, _ = _run_t(torch, dev, p, i_d, k_d, log=False)
        p.set_option("rows_group", -1)
        auto, walks = _run_t(torch, dev, p, i_d, k_d)
        assert len(walks) == 1 and 1 <= walks[0] <= 16 and _same_bits_t(torch, auto, fixed), walks


@pytest.mark.parametrize("name", ["288: RPW 8, two chains", "2560: RPW 1, R1 = 16, cropped"])
def test_same_bytes_whatever_the_walk(fc, torch_dev, name):
    """ "rows_group" 1, 4 and 16 under "image_walk" 1, 19 images in one launch: identical bytes"""
    torch, dev = torch_dev
    shape, transform = SHAPES[name]
    i_d, k_d = _dev_inputs(torch, dev, *_inputs(shape, 19, 3))
    got = {}
    with _walk_plan(fc, shape, transform) as p:
        p.set_option("batch_maps", 57)
        for rg in (1, 4, 16):
            p.set_option("rows_group", rg)
            got[rg], walks = _run_t(torch, dev, p, i_d, k_d)
            assert walks == [rg], (rg, walks)
    assert not bool(torch.isnan(got[1]).any())
    assert _same_bits_t(torch, got[1], got[4]) and _same_bits_t(torch, got[1], got[16])


def test_walk_isolation(fc, torch_dev):
    """changing one image of the batch changes that image's maps only, bit for bit"""
    torch, dev = torch_dev
    B, n = 5, 2
    imgs, ks = _inputs(S288, B, n)
    with _walk_plan(fc, S288, (288, 288), rows_group=16) as p:
        a, walks = _run(torch, dev, p, imgs, ks, B)
        assert walks == [5]
        other = imgs.copy(order="F")
        other[:, :, :, 2] = _inputs(S288, 1, 1, seed=9)[0][:, :, :, 0]
        b = _packed(torch, dev, p, other, ks, B)
    for img in (0, 1, 3, 4):
        assert _same_bits(a[img * n:(img + 1) * n], b[img * n:(img + 1) * n]), img
    for k in range(n):
        assert not np.array_equal(a[2 * n + k], b[2 * n + k])


# ---- every built length once

@pytest.mark.parametrize("L", BUILT)
def test_every_built_length(fc, oracle, torch_dev, L):
    """image 250 x (L - 60) (*) 9 x 41, h-transform 288, B = 3, N = 2 (above 4608 points B = 2, N = 1: the float64 oracle of these
    windows is what takes the time -- 9 s of the 7680-point case, whose window 7664 = 16 x 479), one launch, one walk (1088: the window's own kernel, which only an exact_window plan runs --
    image 250 x 1040, window 272 x 1088, beside the generic output kernel)"""
    torch, dev = torch_dev
    B, n = (3, 2) if L <= 4608 else (2, 1)
    shape, transform, options = (250, L - 60, 1, 9, 41), (288, L), {"rows_group": 16}
    if L == 1088:
        shape, transform, options = (250, 1040, 1, 9, 41), (272, 1088), {"rows_group": 16, "exact_window": 1}
    i_d, k_d = _dev_inputs(torch, dev, *_inputs(shape, B, n, seed=L))
    with _walk_plan(fc, shape, transform, **options) as p:
        got, walks = _run_t(torch, dev, p, i_d, k_d)
        assert walks == [B], walks
        _check_t(got, _refs_t(torch, dev, _refs(oracle, shape, B, n, seed=L)), "L = %d" % L)


# ---- fallbacks

FALLBACKS = {
    "F = 2": ((250, 250, 2, 31, 31), {}, 2),
    "generic plan": ((100, 100, 1, 9, 9), {}, 2),
    "generic kernels only": ((250, 250, 1, 31, 31), {"kernel_path": 1}, 2),
    "Bluestein rows": ((290, 290, 1, 15, 15), {"exact_window": 1}, 2),
    "block-wise": ((100, 100, 1, 9, 9), {"max_transform": 64}, 1),           # (a block-wise plan holds one image)
    "kernel not built": ((250, 1860, 1, 9, 41), {}, 2),                       # 1920 points: fast_rows_images_built
}


@pytest.mark.parametrize("name", list(FALLBACKS))
def test_fallbacks_keep_the_kernel_walk(fc, torch_dev, name):
    """ "image_walk" can be set, "image_walk_active" reads 0, and the maps are the bytes of "image_walk" 0"""
    torch, dev = torch_dev
    shape, options, B = FALLBACKS[name]
    n = 2
    imgs, ks = _inputs(shape, B, n)
    with fc.Plan(*shape, options=options or None) as p:
        if name == "F = 2":
            assert p.get_option("specialised_kernels") == 3 and (p.info.transform_h, p.info.transform_w) == (288, 288)
        elif name == "block-wise":
            assert p.get_option("blockwise") > 0
        elif name == "kernel not built":
            assert p.get_option("specialised_kernels") == 3 and p.info.transform_w == 1920
        else:
            assert p.get_option("specialised_kernels") & 1 == 0
        zero = _packed(torch, dev, p, imgs, ks, B)
        p.set_option("image_walk", 1)
        assert p.get_option("image_walk") == 1 and p.get_option("image_walk_active") == 0
        one, walks = _run(torch, dev, p, imgs, ks, B)
        assert walks == [] and not np.isnan(np.asarray(one)).any() and _same_bits(zero, one)


# ---- composition with the output-side options (routing checks: the output side sees maps only)

def test_option_composition(fc, oracle, torch_dev):
    torch, dev = torch_dev
    B, n = 5, 3
    H, W, F, kh, kw = S288
    imgs, ks = _inputs(S288, B, n)
    refs = _refs(oracle, S288, B, n)
    k_d = torch.from_numpy(np.ascontiguousarray(np.stack([np.transpose(k, (2, 1, 0)) for k in ks]))).to(dev)
    i_d = torch.from_numpy(np.ascontiguousarray(np.transpose(imgs, (3, 2, 1, 0)))).to(dev)
    with _walk_plan(fc, S288, (288, 288), rows_group=16) as p:
        out = torch.full((B * n, p.info.fft_w, p.info.fft_h), float("nan"), dtype=torch.float32, device=dev)
        p.set_images(imgs)
        p.set_option("map_format", 1)
        p.set_option("verbose", 1)
        got, log = _logged(lambda: p.convolve(ks))
        p.set_option("verbose", 0)
        assert _walks(log) == [5], log
        _check16(got, refs, 1, "map_format 1")
        p.set_option("map_format", 0)
        rect = (5, 3, 261, 263)             # odd offsets, odd sizes
        p.set_output_rect(*rect)
        assert p.get_option("rect_direct") == 1
        got, walks = _run(torch, dev, p, imgs, ks, B)
        assert walks == [5]
        _check32(got, [r[rect[0]:rect[0] + rect[2], rect[1]:rect[1] + rect[3]] for r in refs], "rectangle")
        p.set_option("output_region", 0)
        p.set_option("flip_kernels", 1)
        got, walks = _run(torch, dev, p, imgs, ks, B)
        assert walks == [5]
        _check32(got, _refs(oracle, S288, B, n, flip=True), "flip_kernels")
        p.set_option("flip_kernels", 0)
        for dyn in (1, 0):
            p.set_option("dynamic_tiles", dyn)
            got, walks = _run(torch, dev, p, imgs, ks, B)
            assert walks == [5]
            _check32(got, refs, "dynamic_tiles %d" % dyn)
        for defer in (0, 1):
            p.set_option("defer_prepare", defer)
            p.prepare_kernels_packed_device(n, k_d.data_ptr(), kh, kw)
            assert p.get_option("prepare_pending") == defer
            p.set_option("image_walk", 0)       # nothing prepared depends on the walk: the preparation survives both changes
            p.set_option("image_walk", 1)
            assert p.get_option("prepare_pending") == defer
            p.set_images_device(i_d.data_ptr(), B)
            assert p.get_option("prepare_pending") == 0
            p.set_option("profile", 1)
            p.profile()
            p.set_option("verbose", 1)
            _, log = _logged(lambda: (p.convolve_packed_device(n, k_d.data_ptr(), kh, kw, out.data_ptr()), p.synchronize()))
            p.set_option("verbose", 0)
            assert _walks(log) == [5], log
            assert p.profile()["kernel_cols"]["launches"] == 0       # the prepared column spectra were used
            p.set_option("profile", 0)
            got = out.cpu().numpy()
            _check32([got[j].T for j in range(B * n)], refs, "prepared kernels, defer_prepare %d" % defer)


# ---- graph capture

def test_graph_capture(fc, oracle, torch_dev):
    """a warm set_images + convolve_packed under "image_walk" 1 allocates nothing: it is captured into a graph on the plan's stream
    and replayed once with NEW images in the captured buffer; the replay matches the oracle and the eager step bit for bit"""
    torch, dev = torch_dev
    B, n = 5, 2
    H, W, F, kh, kw = S288
    imgs0, ks = _inputs(S288, B, n)
    imgs1, _ = _inputs(S288, B, n, seed=3)
    refs = []
    for b in range(B):
        refs += oracle.conv_fft(np.asfortranarray(imgs1[:, :, :, b]), kh, kw, ks, f64=True)
    to_t = lambda im: torch.from_numpy(np.ascontiguousarray(np.transpose(im, (3, 2, 1, 0)))).pin_memory()
    h0, h1 = to_t(imgs0), to_t(imgs1)
    k_d = torch.from_numpy(np.ascontiguousarray(np.stack([np.transpose(k, (2, 1, 0)) for k in ks]))).to(dev)
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream), fc.Plan(*S288, stream=stream.cuda_stream, options={"rows_group": 16}) as p:
        p.set_option("image_walk", 1)
        assert p.get_option("image_walk_active") == 1
        img_d = torch.empty(h0.shape, dtype=torch.float32, device=dev)
        out = torch.full((B * n, p.info.fft_w, p.info.fft_h), float("nan"), dtype=torch.float32, device=dev)

        def step():
            p.set_images_device(img_d.data_ptr(), B)
            p.convolve_packed_device(n, k_d.data_ptr(), kh, kw, out.data_ptr())

        img_d.copy_(h0, non_blocking=True)
        p.set_option("verbose", 1)
        _, log = _logged(lambda: (step(), torch.cuda.synchronize()))      # eager warm-up: the scratch buffers are sized
        p.set_option("verbose", 0)
        assert _walks(log) == [5], log
        graph = torch.cuda.CUDAGraph()
        cap = torch.cuda.Stream(dev)
        with torch.cuda.graph(graph, stream=cap):
            p.set_stream(torch.cuda.current_stream(dev).cuda_stream)
            step()                                   # (an allocation or a synchronisation in here fails the capture)
        p.set_stream(stream.cuda_stream)
        out.fill_(float("nan"))
        img_d.copy_(h1, non_blocking=True)
        graph.replay()
        replayed = out.clone()
        torch.cuda.synchronize()
        out.fill_(float("nan"))
        step()
        torch.cuda.synchronize()
        got, eager = replayed.cpu().numpy(), out.cpu().numpy()
        del graph
    _check32([got[j].T for j in range(B * n)], refs, "graph replay")
    assert np.array_equal(got.view(np.uint32), eager.view(np.uint32))
