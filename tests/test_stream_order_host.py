"""Happens-before check of the pipelined orchestration of multi_gpu.py (FilterShardedConvolver, ImageStreamedConvolver) on the
CPU.  The other CPU tests drive it with NullSync, which orders nothing; here a trace engine implements the engine protocol
over two logical streams with vector clocks: `record` stores the stream's clock in the event, `wait` joins it into the waiting
stream's, an event that was never recorded is complete, `side()` switches the current stream.  Every buffer (spectra, image
buffers, the map buffer) logs each access as (stream, clock, read / write), and any two accesses to one buffer of which at
least one writes must be ordered by program order on a stream plus record -> wait edges.

Mutation check (each a one-line deletion in multi_gpu.py, never committed; violations summed over the cases of this module,
0 on the orchestration as it stands):
    s.wait(self.consumed[b], side=True) in FilterShardedConvolver.submit     212   test_filter_sharded, test_submit_convolve_by_hand fail
    s.wait(self.consumed[b], side=True) in ImageStreamedConvolver._upload     53   test_image_streamed fails
    s.wait(self.ready[b]) in FilterShardedConvolver.convolve                 314   test_filter_sharded, test_submit_convolve_by_hand fail
    s.wait(self.copied[b]) in ImageStreamedConvolver.run                      83   test_image_streamed fails
"""
import contextlib

import pytest

import util

STREAMS = ("main", "side")


class TraceSync:
    """the sync protocol of multi_gpu.py over two logical streams with vector clocks"""

    def __init__(self):
        self.clock = {s: dict.fromkeys(STREAMS, 0) for s in STREAMS}
        self.cur = "main"

    def event(self):
        return {"clock": None}            # never recorded: complete

    @contextlib.contextmanager
    def side(self):
        prev, self.cur = self.cur, "side"
        try:
            yield
        finally:
            self.cur = prev

    def record(self, ev, side=False):
        ev["clock"] = dict(self.clock["side" if side else "main"])

    def wait(self, ev, side=False):
        if ev["clock"] is not None:
            mine = self.clock["side" if side else "main"]
            for s in STREAMS:
                mine[s] = max(mine[s], ev["clock"][s])

    def access(self):
        """one more operation on the current stream: (stream, its clock after the operation)"""
        self.clock[self.cur][self.cur] += 1
        return self.cur, dict(self.clock[self.cur])


class Buf:
    def __init__(self, sync, name):
        self.sync, self.name, self.log, self.content = sync, name, [], None

    def touch(self, write):
        stream, clock = self.sync.access()
        self.log.append((stream, clock, write))

    def violations(self):
        """pairs of accesses, at least one a write, that neither program order nor the events order"""
        def before(a, b):       # a happened before b: b's stream knows of a's stream at least up to a
            return a[1][a[0]] <= b[1][a[0]]
        n = 0
        for i, a in enumerate(self.log):
            for b in self.log[i + 1:]:
                if (a[2] or b[2]) and not before(a, b) and not before(b, a):
                    n += 1
        return n


class TraceEngine:
    """the engine protocol of multi_gpu.py: nothing is computed, every buffer access is logged on the current stream.  A buffer's
    `content` is the image whose data the host last queued into it (program order), which is what reaches on_result."""

    def __init__(self):
        self.sync = TraceSync()
        self.bufs = []
        self.out = self._buf("maps")

    def _buf(self, name):
        b = Buf(self.sync, "%s%d" % (name, len(self.bufs)))
        self.bufs.append(b)
        return b

    def new_spectrum(self):
        return self._buf("spectrum")

    def new_image_buffer(self):
        return self._buf("image")

    def upload(self, buf, host_image):
        buf.touch(True)
        buf.content = host_image

    def compute_spectrum(self, spec, image):
        if isinstance(image, Buf):
            image.touch(False)
            image = image.content
        spec.touch(True)
        spec.content = image

    def prepare_kernels(self, first, count):
        pass

    def convolve(self, spec, first, count):
        assert self.sync.cur == "main"
        spec.touch(False)
        self.out.touch(True)
        self.out.content = spec.content
        return self.out

    def violations(self):
        return sum(b.violations() for b in self.bufs)


@pytest.fixture(scope="module")
def mg():
    util.load_package()
    import importlib
    return importlib.import_module(util.PKG_NAME + ".multi_gpu")


def _collector(engine, seen):
    def on_result(k, maps):
        assert engine.sync.cur == "main"
        maps.touch(False)             # the caller copies the maps aside on the main stream
        seen.append(maps.content)
    return on_result


def test_trace_engine_sees_a_missing_edge():
    """the checker itself: a write on the side stream and a read on the main stream are unordered without an event, ordered
    with record -> wait, and an event that was never recorded orders nothing"""
    for edge, want in ((None, 1), ("recorded", 0), ("never recorded", 1)):
        e = TraceEngine()
        s, b, ev = e.sync, e.new_spectrum(), e.sync.event()
        with s.side():
            b.touch(True)
            if edge == "recorded":
                s.record(ev, side=True)
        if edge:
            s.wait(ev)
        b.touch(False)
        assert e.violations() == want, edge


@pytest.mark.parametrize("depth", [1, 2, 3])
def test_filter_sharded(mg, depth):
    """run() three times over (the buffers and events are reused across calls), 1 to 4 images a call"""
    for n_img in (1, 2, 3, 4):
        e = TraceEngine()
        conv = mg.FilterShardedConvolver(e, None, 0, 1, 8, depth=depth)
        seen, want = [], []
        for call in range(3):
            images = [("img", call, i) for i in range(n_img)]
            want += images
            conv.run(images, on_result=_collector(e, seen))
        assert seen == want
        assert e.violations() == 0, (depth, n_img)
        assert sum(len(b.log) for b in e.bufs) == 3 * n_img * 4      # spectrum write + read, maps write + read per image


@pytest.mark.parametrize("n_img", [1, 2, 3, 4])
def test_image_streamed(mg, n_img):
    e = TraceEngine()
    conv = mg.ImageStreamedConvolver(e, 8)
    seen, want = [], []
    for call in range(3):
        images = [("img", call, i) for i in range(n_img)]
        want += images
        conv.run(images, on_result=_collector(e, seen))
    assert seen == want
    assert e.violations() == 0, n_img
    assert sum(len(b.log) for b in e.bufs) == 3 * n_img * 6          # image write + read, spectrum write + read, maps write + read


@pytest.mark.parametrize("depth", [2, 3])
def test_submit_convolve_by_hand(mg, depth):
    """submit / submit / convolve / convolve, three rounds: both spectra in flight before the first convolve"""
    e = TraceEngine()
    conv = mg.FilterShardedConvolver(e, None, 0, 1, 8, depth=depth)
    seen = []
    for r in range(3):
        conv.submit(("img", r, 0))
        conv.submit(("img", r, 1))
        for _ in range(2):
            out = conv.convolve()
            out.touch(False)
            seen.append(out.content)
    assert seen == [("img", r, i) for r in range(3) for i in range(2)]
    assert e.violations() == 0
    if depth == 2:
        with pytest.raises(RuntimeError):
            conv.submit(0), conv.submit(1), conv.submit(2)
