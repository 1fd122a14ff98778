"""The plan's setters against one another on the GPU: every ordered pair of nine settings on one live plan.

csrc/plan_rules.hpp holds two tables: which setter is refused while which other state holds, and what a changed value
invalidates (the stream wait, the host-output ring, the prepared kernel column spectra, the images held).  tests/plan_rules_host
holds the tables against the conditions they replaced; this file pins what a caller sees of them.  A live plan that holds an
image and prepared kernels gets setting A, a convolve, then setting B:

  B refused    the status is FFTCONV_ERR_INVALID_ARG, the read-only options (STATE) read as before, and a convolve returns the bits
               it returned before;
  B accepted   the maps equal, bit for bit, those of a fresh plan given A then B before its first image;

and once B and A are back at their defaults the maps equal a fresh default plan's bit for bit.  Wherever "images" reads 0 after a
setter, the image is set again, as include/fftconv.h asks of the caller; the kernels are prepared again ahead of every setter call (a
convolve consumes what was prepared), so each setter meets column spectra it has to forget or may keep: without that the walk passed on
a library whose apply step forgot no column spectra at all; with it that library fails at the third pair ("region then norm: not the
maps of a fresh plan") and stops at the fourth, where a launch is refused.  The pairs that are refused are the literal REFUSED_PAIRS.
A block-wise plan refuses five of the nine outright (REFUSED_BLOCKWISE); the rest are held to the same two comparisons, one
setting at a time.

Plans: the smallest at which every setter's state exists -- 270 x 270 with MAX_KERNEL 15 x 13 is the 288 x 288 window (row length 288
and M = 144, both specialised, the filter kernel built), 60 x 44 with 7 x 5 on kernel_path 1 the generic kernels, 200 x 170 with 9 x 9
and max_transform 96 a block-wise plan.  Every convolve runs two kernels of the MAX_KERNEL size (util.normal_inputs).

The cases run in a spawned child (test_accuracy_gpu._Child), which exits with the module."""
import itertools

import numpy as np
import pytest

import util
from test_accuracy_gpu import _Child

pytestmark = pytest.mark.gpu

INVALID_ARG = -1
# name: (H, W, max_kh, max_kw), creation options, the rectangle (off_h, off_w, out_h, out_w: odd, and inside the "same" map of a border)
PLANS = {
    "specialised": ((270, 270, 15, 13), {}, (15, 13, 101, 77)),
    "generic": ((60, 44, 7, 5), {"kernel_path": 1}, (7, 5, 41, 31)),
    "blockwise": ((200, 170, 9, 9), {"max_transform": 96}, (9, 11, 41, 31)),
}
SETTINGS = ("region", "rect", "stride", "norm", "score", "border", "filter", "format", "flip")
STATE = ("output_region", "images", "match_score", "border_mode", "spectral_filter", "stride_h", "stride_w", "map_format")
# score x border and score x filter, both ways, for both entries of the score
REFUSED_PAIRS = {(a, b) for a in ("norm", "score") for b in ("border", "filter")} | {(b, a) for a in ("norm", "score") for b in ("border", "filter")}
REFUSED_BLOCKWISE = {"norm", "score", "border", "filter", "format"}


@pytest.fixture(scope="module")
def device():
    child = _Child(globals())
    yield child
    if child.gone:
        child.kill()
    else:
        child.ex.shutdown(wait=True)


# ---- the child's side

def _apply(fc, p, name, on, shape, rect, lam):
    """setting `name` at its non-default value (on) or back at its default"""
    kh, kw = shape[2], shape[3]
    if name == "region": p.set_option("output_region", 2 if on else 0)
    elif name == "rect":
        if on: p.set_output_rect(*rect)
        else: p.set_option("output_region", 0)
    elif name == "stride": p.set_output_stride(*((2, 3) if on else (1, 1)))
    elif name == "norm": p.set_normalisation(1 if on else 0, kh, kw)
    elif name == "score": p.set_match_score(fc.SCORE_SQDIFF if on else fc.SCORE_NONE, kh, kw)
    elif name == "border": p.set_border(fc.BORDER_REPLICATE if on else fc.BORDER_ZERO)
    elif name == "filter": p.set_spectral_filter(fc.FILTER_WIENER if on else fc.FILTER_PRODUCT, lam if on else 0.0)
    elif name == "format": p.set_option("map_format", 2 if on else 0)
    elif name == "flip": p.set_option("flip_kernels", 1 if on else 0)
    else: raise KeyError(name)


def _state(p):
    i = p.refresh_info()
    return tuple(p.get_option(n) for n in STATE) + (i.out_h, i.out_w)


class _Bench:
    """the inputs of one plan kind on the device, and the calls of the protocol"""

    def __init__(self, kind):
        import torch
        self.torch, self.fc, self.dev = torch, util.load_package(), torch.device("cuda", 0)
        self.shape, self.options, self.rect = PLANS[kind]
        H, W, kh, kw = self.shape
        img, ks = util.normal_inputs((H, W, 1, kh, kw, 3), 41)
        ks = [ks[0], ks[2]]             # (the second of normal_inputs' kernels is a ragged cell: both here have the MAX_KERNEL size)
        self.lam = float(1e-3 * np.mean([np.sum(k.astype(np.float64) ** 2) for k in ks]))
        self.img_d = torch.from_numpy(np.ascontiguousarray(np.transpose(img, (2, 1, 0)))).to(self.dev)
        self.ker_d = torch.from_numpy(np.ascontiguousarray(np.stack([np.transpose(k, (2, 1, 0)) for k in ks]))).to(self.dev)

    def plan(self):
        H, W, kh, kw = self.shape
        return self.fc.Plan(H, W, 1, kh, kw, options=self.options)

    def apply(self, p, name, on, prepared=False):
        """prepared: the plan holds prepared kernels when the setter runs (a convolve consumes them) -- one-pass plans only"""
        if prepared:
            p.prepare_kernels_packed_device(self.ker_d.shape[0], self.ker_d.data_ptr(), self.shape[2], self.shape[3])
        _apply(self.fc, p, name, on, self.shape, self.rect, self.lam)

    def refused(self, p, name, prepared=False):
        """None if the setting was accepted, else the status of the refusal"""
        try:
            self.apply(p, name, True, prepared)
        except self.fc.FFTConvError as e:
            return e.status
        return None

    def image(self, p, always=False):
        if always or p.get_option("images") == 0:
            p.set_image_device(self.img_d.data_ptr())

    def maps(self, p):
        """the bytes of the two maps of a packed convolve, behind a poisoned buffer"""
        n = self.ker_d.shape[0]
        out = self.torch.full((n * p.refresh_info().out_map_bytes,), 0xA5, dtype=self.torch.uint8, device=self.dev)
        p.convolve_packed_device(n, self.ker_d.data_ptr(), self.shape[2], self.shape[3], out.data_ptr())
        p.synchronize()
        got = out.cpu().numpy()
        assert (got.reshape(n, -1) != 0xA5).any(axis=1).all(), "a map was not written"
        return got

    def fresh(self, *names):
        with self.plan() as q:
            for name in names:
                self.apply(q, name, True)
            self.image(q, always=True)
            return self.maps(q)


def _same(a, b):
    return a.shape == b.shape and bool((a == b).all())


def _case_pairs(kind):
    """every ordered pair on ONE live plan; returns the refused pairs and what went wrong, as text"""
    b = _Bench(kind)
    default = b.fresh()
    refused, wrong = [], []
    with b.plan() as p:
        assert p.get_option("blockwise") == 0 and p.get_option("specialised_kernels") == (3 if kind == "specialised" else 0), kind
        b.image(p, always=True)
        try:
            for A, B in itertools.permutations(SETTINGS, 2):
                b.apply(p, A, True, prepared=True)
                b.image(p)
                before, state = b.maps(p), _state(p)
                if _same(before, default): wrong.append("%s: the maps of the default plan (the setting does nothing here)" % A)
                status = b.refused(p, B, prepared=True)
                if status is not None:
                    refused.append((A, B))
                    if status != INVALID_ARG: wrong.append("%s then %s: status %d" % (A, B, status))
                    if _state(p) != state: wrong.append("%s then %s refused: state %s became %s" % (A, B, state, _state(p)))
                    if not _same(b.maps(p), before): wrong.append("%s then %s refused: the maps changed" % (A, B))
                else:
                    b.image(p)
                    if not _same(b.maps(p), b.fresh(A, B)): wrong.append("%s then %s: not the maps of a fresh plan" % (A, B))
                    b.apply(p, B, False, prepared=True)
                b.apply(p, A, False, prepared=True)
                b.image(p)
                if not _same(b.maps(p), default): wrong.append("%s then %s, both back at their defaults: not the maps of a fresh default plan" % (A, B))
        except b.fc.FFTConvError as e:      # (as text: the exception does not cross the process boundary)
            wrong.append("%s then %s: a call that must pass was refused: %s" % (A, B, e))
    return refused, wrong


def _case_blockwise():
    """one setting at a time on a live block-wise plan"""
    b = _Bench("blockwise")
    default = b.fresh()
    refused, wrong = [], []
    with b.plan() as p:
        assert p.get_option("blockwise") > 1
        b.image(p, always=True)
        for B in SETTINGS:
            before, state = b.maps(p), _state(p)
            status = b.refused(p, B)
            if status is not None:
                refused.append(B)
                if status != INVALID_ARG: wrong.append("%s: status %d" % (B, status))
                if _state(p) != state: wrong.append("%s refused: state %s became %s" % (B, state, _state(p)))
                if not _same(b.maps(p), before): wrong.append("%s refused: the maps changed" % B)
            else:
                b.image(p)
                got = b.maps(p)
                if not _same(got, b.fresh(B)): wrong.append("%s: not the maps of a fresh plan" % B)
                if _same(got, default): wrong.append("%s: the maps of the default plan (the setting does nothing here)" % B)
                b.apply(p, B, False)
            b.image(p)
            if not _same(b.maps(p), default): wrong.append("%s, back at its default: not the maps of a fresh default plan" % B)
    return refused, wrong


# ---- the tests

@pytest.mark.parametrize("kind", ["specialised", "generic"])
def test_every_ordered_pair_of_settings(device, kind):
    refused, wrong = device("_case_pairs", kind)
    print("plan setters %s: %d pairs refused: %s" % (kind, len(refused), sorted(refused)))
    for w in wrong:
        print("plan setters %s: %s" % (kind, w))
    assert not wrong
    assert len(refused) == len(set(refused)) and set(refused) == REFUSED_PAIRS


def test_blockwise_refusals(device):
    refused, wrong = device("_case_blockwise")
    print("plan setters block-wise: refused %s" % sorted(refused))
    for w in wrong:
        print("plan setters block-wise: %s" % w)
    assert not wrong
    assert set(refused) == REFUSED_BLOCKWISE
