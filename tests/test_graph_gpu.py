"""HIP graph replay against the oracle, GPU tier.  include/fftconv.h promises that, after one warm-up call with the same
arguments, fftconv_plan_set_image(DEVICE), fftconv_plan_prepare_kernels_packed and fftconv_plan_convolve_packed allocate
nothing and never synchronise, so that a step can be recorded into a graph; bench.py --graph times such replays and checks the
last one, for one shape with default options.  Here the capture is made exactly as bench.py makes it -- the plan bound to the
capturing stream with set_stream, one step captured after one eager warm-up step with the same arguments, a single stream, no
fork or join inside the capture -- and the graph is replayed three times with a NEW image and new kernels copied into the
captured buffers on the same stream before each replay and the maps copied aside after it, nothing synchronised in between.
Every replay must match the float64 oracle under util.BUDGET_DIRECT and equal the eager step on the same inputs bit for bit
(self-resetting tile-queue counters, scratch reuse and launch arguments frozen at capture time are what could differ).

Block-wise plans are not captured: they synchronise between chunks (include/fftconv.h, fftconv_plan_set_stream)."""
import numpy as np
import pytest

import util
from test_accuracy_gpu import _Child
from test_async_gpu import _ctx, _image_t, _nan_maps, _pack_t, _uniform, judge_maps

pytestmark = pytest.mark.gpu

REPLAYS = 3
GRAPHS = {
    "tile queue, batch_maps 2": ((1024, 1024, 1, 63, 63, 5), {}, {"batch_maps": 2}),
    "static deal": ((256, 256, 1, 31, 31, 3), {}, {}),
    "F = 2": ((300, 260, 2, 31, 17, 7), {}, {}),
    "defer_prepare": ((256, 256, 1, 31, 31, 3), {}, {"defer_prepare": 1}),
    "output_region 2": ((1024, 1024, 1, 63, 63, 3), {}, {"batch_maps": 2, "output_region": 2}),
    "flip_kernels": ((256, 256, 1, 31, 31, 3), {}, {"flip_kernels": 1}),
    "generic kernels": ((300, 260, 2, 31, 17, 3), {"kernel_path": 1}, {"tune_placement": 0}),
}


@pytest.fixture(scope="module")
def device():
    child = _Child(globals())
    yield child
    if child.gone:
        child.kill()
    else:
        child.ex.shutdown(wait=True)


def _case_graph(name):
    torch, fc, dev = _ctx()
    shape, options, settings = GRAPHS[name]
    H, W, F, kh, kw, n = shape
    orc = util.Oracle()
    sets = []                               # inputs 0: warm-up and capture; 1..REPLAYS: the replays
    for k in range(REPLAYS + 1):
        img, ks = util.normal_inputs(shape, 140 + k)
        ks = _uniform(ks)
        sets.append((img, ks, orc.conv_fft(img, kh, kw, ks, f64=True) if k else None))
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream), fc.Plan(H, W, F, kh, kw, stream=stream.cuda_stream, options=options) as p:
        for key, value in settings.items():
            p.set_option(key, value)
        assert p.get_option("blockwise") == 0
        if name == "tile queue, batch_maps 2":
            assert p.get_option("dynamic_tiles") == 1
        elif name == "static deal":
            assert p.get_option("dynamic_tiles") == 0
        ow, oh = p.info.out_w, p.info.out_h
        crop = None
        if settings.get("output_region") == 2:
            crop = (slice((kh - 1) // 2, (kh - 1) // 2 + H), slice((kw - 1) // 2, (kw - 1) // 2 + W))
        flip = settings.get("flip_kernels")
        imgs_h = [_image_t(torch, s[0]).pin_memory() for s in sets]
        kers_h = [_pack_t(torch, [np.asfortranarray(k[::-1, ::-1, :]) for k in s[1]] if flip else s[1]).pin_memory() for s in sets]
        img_d = torch.empty(imgs_h[0].shape, dtype=torch.float32, device=dev)       # the captured buffers
        ker_d = torch.empty(kers_h[0].shape, dtype=torch.float32, device=dev)
        out = _nan_maps(torch, dev, n, ow, oh)
        replayed = [_nan_maps(torch, dev, n, ow, oh) for _ in range(REPLAYS)]
        eager = [_nan_maps(torch, dev, n, ow, oh) for _ in range(REPLAYS)]

        def step():
            if settings.get("defer_prepare"):
                p.prepare_kernels_packed_device(n, ker_d.data_ptr(), kh, kw)
            p.set_image_device(img_d.data_ptr())
            p.convolve_packed_device(n, ker_d.data_ptr(), kh, kw, out.data_ptr())

        img_d.copy_(imgs_h[0], non_blocking=True)
        ker_d.copy_(kers_h[0], non_blocking=True)
        step()                                   # eager warm-up: the scratch buffers are sized, nothing allocates from here on
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        cap = torch.cuda.Stream(dev)
        with torch.cuda.graph(graph, stream=cap):
            p.set_stream(torch.cuda.current_stream(dev).cuda_stream)
            step()
        p.set_stream(stream.cuda_stream)
        out.fill_(float("nan"))
        for r in range(REPLAYS):                 # nothing synchronised from here to the end of the loop
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
    refs = [s[2] for s in sets[1:]]
    return judge_maps(got, refs, crop), judge_maps(want, refs, crop), all(np.array_equal(a, b) for a, b in zip(got, want))


@pytest.mark.parametrize("name", list(GRAPHS))
def test_graph_replay_matches_oracle_and_eager(device, name):
    worst, worst_eager, equal = device("_case_graph", name)
    print("graph %s: replays max %.2e L2 %.2e spectral %.2e, eager max %.2e L2 %.2e spectral %.2e, replays bit-identical to eager: %s"
          % ((name,) + worst + worst_eager + (equal,)))
    assert all(x < b for x, b in zip(worst, util.BUDGET_DIRECT)), (name, worst, util.BUDGET_DIRECT)
    assert all(x < b for x, b in zip(worst_eager, util.BUDGET_DIRECT)), (name, worst_eager, util.BUDGET_DIRECT)
    assert equal, name
