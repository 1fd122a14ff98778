"""Model-based random walks of ONE live plan: every map of every convolve checked against the float64 oracle.

A plan is a large mutable object (prepared / deferred kernel column spectra, the host-output ring, pinned buffers read in
place, tile-queue counters, the tuned placement, region / rectangle, map format, stream, batch sizes, flip) whose consistency
rests on the invalidations that csrc/plan_rules.hpp tabulates (kSetterEffects, and the FX_* column of kLongOptions in
csrc/fftconv_api.cpp; the refusals: kPlanRules).  A missed one faults nothing: it returns 0 and a wrong map.  The
walk draws a sequence of calls on one plan (draw_walk), a pure-Python model of include/fftconv.h says what every convolve must
return and which calls must be refused (Model), and run_walk drives the plan on the GPU and compares.

Shared by tests/test_plan_walk_gpu.py (committed seeds, in a child process), tests/test_plan_walk_host.py (the generator, the
model's cutting code and the tolerances, no GPU) and tools/plan_walk.py (soak runs and shrinking).  Nothing here imports
torch or touches the GPU at import.

The bars.  fp32 maps: max |got - ref| < 1e-5 x max |ref|, util.rel_err of the returned map, the bar of tools/fuzz_gpu.py (its
worst over 8 000 cases was 7.4e-7).  For the named regions 0-4 the maximum is the returned map's own.  A rectangle
(set_output_rect) is the one departure: it may be a single element or lie wholly in the zero padding and has no magnitude of
its own, so its maximum is taken over the window map it was cut from -- fp32 FFT error is relative to the window's magnitude.
16-bit maps: |got - ref| <= 1e-5 x that maximum + half an ulp of the format at max(|got|, |ref|): the fp32 value is within the
first term, the store rounds it once to nearest, and the rounded value's ulp is never smaller than that of the value rounded.
The condition on the inputs is NOT the one first asked for, that every map VALUE be a normal fp16 number: a convolution of
zero-mean data crosses zero, so no choice of inputs meets it.  It is relaxed to a condition on each map's PEAK (normal_range_ok,
checked on the CPU for every pool entry): the peak is a normal number of the format and, with the first term on top, below its
largest finite value, i.e. nothing overflows and no map is subnormal as a whole.  The values near zero that the relaxed
condition lets through are covered by the bound itself: below the smallest normal number ulp16 is the format's subnormal spacing.

The epilogue of every walk puts every option back to its default, the stream to 0, and runs set_image_device(image 0) +
convolve_packed_device(set 1): the maps must equal those of a fresh plan of the same kind BIT FOR BIT, for every kind (no kind
needed the fall-back to the relative bar: placement tuning and batch sizes change where buffers live, not the arithmetic).

Kinds (KINDS): one per transform path and block-wise scheme, each the smallest shape at which every part of that path's state
exists (create_plan asserts the plan is what its kind names), plus "generic_thin", a data array shorter than its kernels: the one shape at which
"output_region" 3 is empty and must be refused.  The refusal "kernel larger than MAX_KERNEL" is drawn as a kernel taller than
the window (FFTCONV_ERR_KERNEL_SHAPE on every kind): whether MAX_KERNEL + 1 rows are refused depends on whether the planner's
transform happens to be the window, which the generator cannot know without a device.
"""
import numpy as np

import util
from test_map_format_gpu import _image_t, from_bits
from test_output_rect_gpu import GUARD, POISON16, _guarded, _unguard

# name: (H, W, F, kh, kw, creation options)
KINDS = {
    "specialised": (270, 270, 2, 15, 13, {}),
    "specialised_f1_wide": (40, 1100, 1, 9, 40, {}),
    "generic": (60, 44, 3, 7, 5, {"kernel_path": 1}),
    "exact": (274, 274, 1, 15, 15, {"exact_window": 1}),
    "bluestein": (282, 346, 2, 23, 23, {"exact_window": 1}),
    "save_blocks": (500, 420, 1, 15, 13, {"max_transform": 288}),
    "add_blocks": (200, 170, 2, 9, 9, {"max_transform": 96}),
    "generic_thin": (6, 50, 2, 7, 5, {"kernel_path": 1}),
}
KIND_NAMES = list(KINDS)
BLOCKWISE = ("save_blocks", "add_blocks")
EXACT = ("exact", "bluestein")

ENTRIES = ("convolve", "convolve_out", "convolve_to_device", "convolve_packed")
FAMILIES = ("image", "prepare", "forgetting", "ring", "region", "rectangle", "format", "stream", "refusal")
N_IMAGES, N_SETS = 3, 3
HOST, DEVICE = 0, 1

# option name: the values drawn; the plan's default (None: read from the fresh plan)
OPTIONS = {
    "flip_kernels": ((0, 1), 0),
    "batch_maps": ((0, 1, 2, 5), 0),
    "kernel_chunk_mb": ((0, 1), 0),
    "rows_group": ((0, 1, 2, 3, 5), 0),
    "dynamic_tiles": ((0, 1, 2), None),
    "defer_prepare": ((0, 1), 0),
    "host_pinned": ((0, 1), 1),
    "host_min_kb": ((0, 1024), 1024),
    "host_stream": ((0, 1, 2), 1),
    "host_chunk_kb": ((0, 16, 64), 0),
    "host_slots": ((0, 2, 3), 0),
    "host_threads": ((0, 1, 2), 0),
    "map_format": ((0, 1, 2), 0),
    "output_region": ((0, 1, 2, 3, 4), 0),
    "rect_store": ((0, 1), 1),
    "profile": ((0, 1), 0),
    "tune_placement": ((0, 2), -1),
}
FORGETTING = ("flip_kernels", "batch_maps", "kernel_chunk_mb")
RING = ("host_stream", "host_threads", "host_chunk_kb", "host_slots")
RECT_STYLES = ("whole", "one_row", "one_column", "odd", "even", "random")

TOL = 1e-5
FMT_DTYPES = {0: np.dtype(np.float32), 1: np.dtype(np.float16), 2: np.dtype(np.uint16)}
# fp16 / bfloat16: mantissa bits, exponent of the smallest normal number, largest finite value
FMT_SHAPE = {1: (10, -14, 65504.0), 2: (7, -126, float(np.finfo(np.float32).max))}


# ---------------------------------------------------------------------------------------------------------------------
# the model

def pow2_window(n):
    """fftconv_fft_size_pow2: up to a multiple of 16, then up to the next power of two"""
    n16, p = util.ceil16(n), 1
    while p < n16:
        p *= 2
    return p


class Model:
    """the documented state of a plan of one kind that decides what a convolve returns (include/fftconv.h)"""

    def __init__(self, kind):
        self.kind = kind
        self.H, self.W, self.F, self.kh, self.kw, self.options = KINDS[kind]
        self.fft_h, self.fft_w = util.ceil16(self.H + self.kh - 1), util.ceil16(self.W + self.kw - 1)
        self.blockwise = kind in BLOCKWISE
        self.exact = kind in EXACT
        self.image = None          # pool index of the current image
        self.flip = 0
        self.region = 0
        self.rect = (0, 0, self.fft_h, self.fft_w)      # (off_h, off_w, out_h, out_w) of the current region
        self.fmt = 0
        self.stream = 0

    def state(self):
        return dict(kind=self.kind, image=self.image, flip=self.flip, region=self.region, rect=self.rect, fmt=self.fmt, stream=self.stream)

    # -- what the kind supports
    def formats(self):
        return (0,) if self.blockwise else (0, 1, 2)

    def region_rect(self, region):
        """(off_h, off_w, out_h, out_w) of a named region; out sizes < 1: the region is empty and refused"""
        H, W, kh, kw = self.H, self.W, self.kh, self.kw
        if region == 0:
            return (0, 0, self.fft_h, self.fft_w)
        if region == 1:
            return (0, 0, H + kh - 1, W + kw - 1)
        if region == 2:
            return ((kh - 1) // 2, (kw - 1) // 2, H, W)
        if region == 3:
            return (kh - 1, kw - 1, H - kh + 1, W - kw + 1)
        if region == 4:
            return (0, 0, pow2_window(H + kh - 1), pow2_window(W + kw - 1))
        raise ValueError(region)

    def region_empty(self, region):
        r = self.region_rect(region)
        return r[2] < 1 or r[3] < 1

    def rect_valid(self, rect):
        oh, ow, h, w = rect
        return oh >= 0 and ow >= 0 and h >= 1 and w >= 1 and oh + h <= self.fft_h and ow + w <= self.fft_w

    def families(self):
        return tuple(f for f in FAMILIES if not (f == "format" and self.blockwise))

    def alphabet(self):
        """every op item this kind supports (what the coverage conditions count)"""
        items = ["set_image", "set_image_device", "prepare", "set_output_rect", "set_stream", "synchronize", "profile_read"]
        items += ["set_option:" + n for n in OPTIONS if not (n == "map_format" and self.blockwise)]
        items += ["refuse:output_region_5", "refuse:dynamic_tiles_3", "refuse:rect_outside", "refuse:kernel_features", "refuse:kernel_oversize"]
        if self.blockwise:
            items.append("refuse:map_format_blockwise")
        if self.region_empty(3):
            items.append("refuse:output_region_3_empty")
        if self.exact:
            items.append("spectrum")
        return items

    # -- transitions
    def apply(self, op):
        """follows an op; returns the status the call must return (0, or the documented refusal)"""
        name = op[0]
        if name == "refuse":
            return op[-1]
        if name in ("set_image", "set_image_device", "spectrum"):
            self.image = op[1]
        elif name == "set_option":
            _, opt, value = op
            if opt == "flip_kernels":
                self.flip = int(value != 0)
            elif opt == "map_format":
                assert value in self.formats()
                self.fmt = value
            elif opt == "output_region":
                assert not self.region_empty(value)
                self.region, self.rect = value, self.region_rect(value)
        elif name == "set_output_rect":
            assert self.rect_valid(op[1:])
            self.region, self.rect = 5, tuple(op[1:])
        elif name == "set_stream":
            self.stream = op[1]
        return 0

    def out_shape(self):
        return (self.rect[2], self.rect[3])

    def cut(self, window):
        """the result map of the current region out of a full (fft_h, fft_w) window map"""
        return cut(window, self.region, self.rect)


def cut(window, region, rect):
    """regions 0-3 and 5 crop rows [off_h, off_h + out_h) of columns [off_w, off_w + out_w); 4 zero-pads to the pow2 window"""
    off_h, off_w, out_h, out_w = rect
    if region == 4:
        out = np.zeros((out_h, out_w), dtype=window.dtype)
        out[:window.shape[0], :window.shape[1]] = window
        return out
    return window[off_h:off_h + out_h, off_w:off_w + out_w]


def op_item(op):
    """the alphabet item of an op"""
    if op[0] == "set_option":
        return "set_option:" + op[1]
    if op[0] == "refuse":
        return "refuse:" + op[1]
    return op[0]


def op_family(op):
    """the state-changing family of an op (None: a convolve, or an op of no family)"""
    name = op[0]
    if name in ("set_image", "set_image_device", "spectrum"):
        return "image"
    if name == "prepare":
        return "prepare"
    if name == "set_option":
        if op[1] in FORGETTING:
            return "forgetting"
        if op[1] in RING:
            return "ring"
        return {"output_region": "region", "map_format": "format"}.get(op[1])
    return {"set_output_rect": "rectangle", "set_stream": "stream", "refuse": "refusal"}.get(name)


def is_convolve(op):
    return op[0] in ENTRIES


# ---------------------------------------------------------------------------------------------------------------------
# the generator

class _Draw:
    def __init__(self, kind, seed):
        self.m = Model(kind)
        self.rng = np.random.default_rng([seed, KIND_NAMES.index(kind)])
        self.bags = {}
        self.current = {}          # option values as the walk has set them
        self.rect_k, self.region_k = 2 * seed, 3 * seed

    def pick(self, bag, values):
        """the next of a shuffled cycle through `values`: every value comes up before any comes up again"""
        left = self.bags.get(bag)
        if not left:
            left = [values[i] for i in self.rng.permutation(len(values))]
            self.bags[bag] = left
        return left.pop()

    def rectangle(self):
        m, rng = self.m, self.rng
        fh, fw = m.fft_h, m.fft_w
        style = RECT_STYLES[self.rect_k % len(RECT_STYLES)]      # two a walk at least: consecutive seeds deal every style
        self.rect_k += 1
        if style == "whole":
            return (0, 0, fh, fw)
        if style == "one_row":
            ow = int(rng.integers(0, fw - 1))
            return (int(rng.integers(0, fh)), ow, 1, int(rng.integers(2, fw - ow + 1)))
        if style == "one_column":
            oh = int(rng.integers(0, fh - 1))
            return (oh, int(rng.integers(0, fw)), int(rng.integers(2, fh - oh + 1)), 1)
        if style in ("odd", "even"):           # odd offsets and an odd pitch / all even
            bit = 1 if style == "odd" else 0
            oh, ow = int(rng.integers(0, (fh - 3) // 2)) * 2 + bit, int(rng.integers(0, (fw - 3) // 2)) * 2 + bit
            h, w = int(rng.integers(1, (fh - oh) // 2 + 1)) * 2 - bit, int(rng.integers(1, (fw - ow) // 2 + 1)) * 2 - bit
            return (oh, ow, h, w)
        oh, ow = int(rng.integers(0, fh)), int(rng.integers(0, fw))
        return (oh, ow, int(rng.integers(1, fh - oh + 1)), int(rng.integers(1, fw - ow + 1)))

    def rectangle_outside(self):
        m = self.m
        fh, fw = m.fft_h, m.fft_w
        return self.pick("rect_outside", [(0, 0, fh + 1, 1), (0, 0, 1, fw + 1), (fh, 0, 1, 1), (-1, 0, 5, 5), (0, -1, 5, 5), (0, 0, 0, 5),
                                          (fh - 4, fw - 4, 5, 5)])

    def entry_for_refusal(self, entries):
        return self.pick("refusal_entry:" + ",".join(entries), list(entries))

    def item(self, item):
        """an op of an alphabet item"""
        m, rng = self.m, self.rng
        if item in ("set_image", "set_image_device", "spectrum"):
            return (item, int(self.pick("image", list(range(N_IMAGES)))))
        if item == "prepare":
            return ("prepare", int(self.pick("prepare_set", [1, 2])))
        if item == "set_output_rect":
            self.current["output_region"] = 5
            return ("set_output_rect",) + self.rectangle()
        if item == "set_stream":
            return ("set_stream", int(self.pick("stream", [0, 1])))
        if item in ("synchronize", "profile_read"):
            return (item,)
        if item.startswith("set_option:"):
            name = item.split(":", 1)[1]
            values = list(OPTIONS[name][0])
            if name == "output_region":
                values = [v for v in values if not m.region_empty(v)]
                self.region_k += 1                   # two a walk at least: consecutive seeds deal every region
                self.current[name] = values[self.region_k % len(values)]
                return ("set_option", name, self.current[name])
            current = self.current.get(name, OPTIONS[name][1])
            for _ in range(2 * len(values)):        # a value the option does not hold already, where there is one
                value = int(self.pick(name, values))
                if value != current:
                    break
            self.current[name] = value
            return ("set_option", name, value)
        what = item.split(":", 1)[1]
        if what == "output_region_5":
            return ("refuse", what, "output_region", 5, -1)
        if what == "output_region_3_empty":
            return ("refuse", what, "output_region", 3, -1)
        if what == "dynamic_tiles_3":
            return ("refuse", what, "dynamic_tiles", 3, -1)
        if what == "map_format_blockwise":
            return ("refuse", what, "map_format", int(self.pick("refused_format", [1, 2])), -1)
        if what == "rect_outside":
            return ("refuse", what) + self.rectangle_outside() + (-1,)
        if what == "kernel_features":
            return ("refuse", what, self.entry_for_refusal(("convolve", "convolve_to_device")), -3)
        if what == "kernel_oversize":
            return ("refuse", what, self.entry_for_refusal(ENTRIES), -3)
        raise ValueError(item)

    def family(self, fam, conv_set):
        m, rng = self.m, self.rng
        if fam == "image":
            return self.item(self.pick("image_item", ["set_image", "set_image_device"] + (["spectrum"] if m.exact else [])))
        if fam == "prepare":           # of the set the convolve will use, or of the other one
            s = conv_set if conv_set in (1, 2) and rng.random() < 0.5 else int(self.pick("prepare_set", [1, 2]))
            return ("prepare", s)
        if fam == "forgetting":
            return self.item("set_option:" + self.pick("forgetting", list(FORGETTING)))
        if fam == "ring":
            return self.item("set_option:" + self.pick("ring", list(RING)))
        if fam == "region":
            return self.item("set_option:output_region")
        if fam == "rectangle":
            return self.item("set_output_rect")
        if fam == "format":
            return self.item("set_option:map_format")
        if fam == "stream":
            return self.item("set_stream")
        if fam == "refusal":
            return self.item(self.pick("refusal", [i for i in m.alphabet() if i.startswith("refuse:")]))
        raise ValueError(fam)


def combos(kind):
    """every (convolve entry, family) pair of a kind in a fixed shuffled order: walk `seed` forces the pairs from
    (seed x rounds) on, so consecutive seeds deal the whole list"""
    m = Model(kind)
    pairs = [(e, f) for e in ENTRIES for f in m.families()]
    order = np.random.default_rng([4242, KIND_NAMES.index(kind)]).permutation(len(pairs))
    return [pairs[i] for i in order]


def draw_walk(kind, seed, length=70):
    """a list of ops (plain tuples) for one plan of `kind`, deterministic from (seed, kind).  The walk starts with a convolve that
    must be refused (no image yet) and an image; then rounds of two ops off a shuffled cycle through the kind's whole alphabet, one
    op of a forced family, and a convolve through a forced entry.  Ahead of a packed convolve there is, more often than not, also
    a prepare of the very set that convolve will use: the op of the forced family then meets prepared column spectra."""
    d = _Draw(kind, seed)
    m, rng = d.m, d.rng
    ops = [("refuse", "no_image", str(rng.choice(ENTRIES)), -9), d.item(str(rng.choice(["set_image", "set_image_device"])))]
    for op in ops:
        m.apply(op)
    rounds = max(15, (length - 2) // 4)
    forced = combos(kind)
    last_packed = int(rng.integers(1, 3))
    for r in range(rounds):
        entry, fam = forced[(seed * rounds + r) % len(forced)]
        if entry == "convolve_packed":
            s = last_packed if rng.random() < 0.6 else 3 - last_packed
            last_packed = s
        else:
            s = int(d.pick("set", list(range(N_SETS))))
        bag = m.alphabet() + ["set_output_rect", "set_option:output_region"]
        fillers = [d.item(d.pick("alphabet", bag)), d.item(d.pick("alphabet", bag))]
        if entry == "convolve_packed" and rng.random() < 0.6:
            fillers.append(("prepare", s))
        conv = (entry, s, int(rng.integers(0, 2))) if entry == "convolve_to_device" else (entry, s)
        for op in fillers + [d.family(fam, s), conv]:
            m.apply(op)
            ops.append(op)
    return ops


# ---------------------------------------------------------------------------------------------------------------------
# inputs, the oracle and the tolerances (CPU)

class Pool:
    """the inputs of a kind: 3 standard-normal images; kernel set 0 ragged, sets 1 and 2 of one size and count (nothing but
    their contents and addresses tells those two apart); the float64 oracle maps of every (image, set, flipped), computed once"""

    def __init__(self, kind):
        self.kind = kind
        H, W, F, kh, kw, _ = KINDS[kind]
        rng = np.random.default_rng([77, KIND_NAMES.index(kind)])
        self.images = [np.asfortranarray(rng.standard_normal((H, W, F), dtype=np.float32)) for _ in range(N_IMAGES)]
        ragged = [(kh, kw), (kh, kw), (max(1, kh - 1), max(1, kw // 4)), (max(1, kh // 2), kw)]
        sizes = [ragged, [(kh, kw)] * 3, [(kh, kw)] * 3]
        self.sets = [[np.asfortranarray(rng.standard_normal((a, b, F), dtype=np.float32)) for a, b in sz] for sz in sizes]
        self.mk = (kh, kw)
        self._oracle = None
        self._maps = {}

    def windows(self, image, kset, flip):
        """float64 window maps [(fft_h, fft_w)] of one pool entry"""
        key = (image, kset, flip)
        if key not in self._maps:
            if self._oracle is None:
                self._oracle = util.Oracle()
            ks = self.sets[kset]
            if flip:
                ks = [np.asfortranarray(k[::-1, ::-1, :]) for k in ks]
            maps = self._oracle.conv_fft(self.images[image], self.mk[0], self.mk[1], ks, f64=True)
            for a in maps:
                a.setflags(write=False)
            self._maps[key] = maps
        return self._maps[key]

    def entries(self):
        return [(i, s, f) for i in range(N_IMAGES) for s in range(N_SETS) for f in (0, 1)]


def normal_range_ok(window, fmt):
    """the condition on the inputs of the 16-bit bound: the map's maximum is a normal number of the format and, with the fp32
    error bar on top, below its largest finite value"""
    _, e_min, top = FMT_SHAPE[fmt]
    peak = float(np.abs(window).max())
    return 2.0 ** e_min <= peak and peak * (1 + TOL) < top


def ulp16(x, fmt):
    """spacing of format fmt at |x| (float64 array): 2^(e - mantissa bits), e clamped at the smallest normal exponent"""
    mant, e_min, _ = FMT_SHAPE[fmt]
    ax = np.abs(np.asarray(x, dtype=np.float64))
    e = np.floor(np.log2(np.maximum(ax, 2.0 ** e_min)))
    return 2.0 ** (np.maximum(e, e_min) - mant)


def map_error(got, ref, scale, fmt):
    """(error, bound exceeded) of one map.  got: fp32 values or uint16 bit patterns; ref: the float64 map; scale: its maximum (a rectangle: the window's).
    fp32: error = max |got - ref| / scale against TOL.  16-bit: the worst of (|got - ref| - half an ulp) / scale against TOL."""
    ref = np.asarray(ref, dtype=np.float64)
    if fmt == 0:
        g = np.asarray(got, dtype=np.float64)
        err = float(np.abs(g - ref).max() / scale) if g.size else 0.0
        return err, not err < TOL
    g = from_bits(got, fmt)
    if not np.isfinite(g).all():
        return float("inf"), True
    excess = np.abs(g - ref) - 0.5 * ulp16(np.maximum(np.abs(g), np.abs(ref)), fmt)
    err = float(max(excess.max(), 0.0) / scale) if g.size else 0.0
    return err, not err <= TOL


class WalkFailure(AssertionError):
    """a check of a walk failed numerically: wrong values, a wrong shape, a written guard band or an unexpected status"""


# ---------------------------------------------------------------------------------------------------------------------
# the GPU side

_CTX = {}


def _ctx():
    if not _CTX:
        import torch
        _CTX.update(torch=torch, fc=util.load_package(), dev=torch.device("cuda", 0), pools={}, fresh={})
    return _CTX


def _poisoned_host(shape, fmt):
    a = np.empty(shape, dtype=FMT_DTYPES[fmt], order="F")
    if fmt == 0:
        a.fill(np.nan)
    else:
        a.view(np.uint16).fill(POISON16)
    return a


class DevicePool:
    """a Pool with its device copies (never modified during a walk)"""

    def __init__(self, kind):
        c = _ctx()
        torch, dev = c["torch"], c["dev"]
        self.pool = Pool(kind)
        self.images_d = [_image_t(torch, a).to(dev) for a in self.pool.images]
        # every kernel on its own ([F][kw][kh]) and, sets 1 and 2, packed ([n][F][kw][kh])
        self.kernels_d = [[_image_t(torch, k).to(dev) for k in ks] for ks in self.pool.sets]
        self.packed_d = [None] + [torch.stack([_image_t(torch, k) for k in ks]).contiguous().to(dev) for ks in self.pool.sets[1:]]
        H, W, F, kh, kw, _ = KINDS[kind]
        fh = util.ceil16(H + kh - 1)
        rng = np.random.default_rng(5)
        self.oversize = np.asfortranarray(rng.standard_normal((fh + 1, kw, F), dtype=np.float32))
        self.oversize_d = _image_t(torch, self.oversize).to(dev)
        self.wrong_f = np.asfortranarray(rng.standard_normal((kh, kw, F + 1), dtype=np.float32))
        torch.cuda.synchronize()


def device_pool(kind):
    pools = _ctx()["pools"]
    if kind not in pools:
        pools[kind] = DevicePool(kind)
    return pools[kind]


def create_plan(kind):
    """a fresh plan of the kind, asserted to be the plan the kind names"""
    fc = _ctx()["fc"]
    H, W, F, kh, kw, options = KINDS[kind]
    p = fc.Plan(H, W, F, kh, kw, options=dict(options))
    try:
        i = p.info
        facts = dict(specialised=p.get_option("specialised_kernels"), blockwise=p.get_option("blockwise"), overlap_save=p.get_option("overlap_save"),
                     transform=(i.transform_h, i.transform_w), window=(i.fft_h, i.fft_w), exact=i.exact_window)
        p.set_output_rect(0, 0, 1, 1)
        facts["rect_direct"] = p.get_option("rect_direct")
        p.set_option("output_region", 0)
        m = Model(kind)
        assert facts["window"] == (m.fft_h, m.fft_w), facts
        if kind == "specialised":
            assert facts["specialised"] == 3 and facts["blockwise"] == 0 and facts["transform"] == (288, 288) and facts["rect_direct"] == 1, facts
        elif kind == "specialised_f1_wide":
            # (bit 0: the specialised row kernel, what the kind is for; a 48-point column transform has only generic kernels)
            assert facts["specialised"] & 1 and facts["blockwise"] == 0 and facts["transform"] == (48, 1152), facts
        elif kind in ("generic", "generic_thin"):
            assert facts["specialised"] == 0 and facts["blockwise"] == 0 and facts["rect_direct"] == 0, facts
        elif kind == "exact":
            assert facts["exact"] == 1 and facts["specialised"] == 3 and facts["blockwise"] == 0 and facts["transform"] == (288, 288), facts
        elif kind == "bluestein":
            assert facts["exact"] == 1 and facts["specialised"] == 0 and facts["blockwise"] == 0 and facts["transform"] == (304, 368), facts
        elif kind == "save_blocks":
            assert facts["blockwise"] > 1 and facts["overlap_save"] == 1 and max(facts["transform"]) <= 288, facts
        elif kind == "add_blocks":
            assert facts["blockwise"] > 1 and facts["overlap_save"] == 0 and max(facts["transform"]) <= 96, facts
    except BaseException:
        p.destroy()
        raise
    return p


class _Run:
    """one walk on one plan"""

    def __init__(self, kind):
        c = _ctx()
        self.torch, self.fc, self.dev = c["torch"], c["fc"], c["dev"]
        self.kind = kind
        self.dp = device_pool(kind)
        self.pool = self.dp.pool
        self.m = Model(kind)
        self.stats = dict(ops=0, convolves=0, maps=0, refusals=0, worst=0.0, worst16=0.0)
        self.side = None
        self.defaults = {}
        self.index = 0

    def fail(self, what):
        raise WalkFailure(what)

    # -- outputs
    def sync_all(self):
        self.torch.cuda.synchronize()

    def unguard(self, t, n_elems, fmt, shift, what):
        """the map elements of a _guarded buffer; a written guard band fails the walk"""
        try:
            return _unguard(t, n_elems, fmt, shift)
        except AssertionError as e:
            self.fail("%s: %s" % (what, e))

    def check_maps(self, maps, windows, what):
        """maps: one (out_h, out_w) array per kernel, fp32 values or uint16 bit patterns"""
        m = self.m
        if len(maps) != len(windows):
            self.fail("%s: %d maps for %d kernels" % (what, len(maps), len(windows)))
        for j, (g, w) in enumerate(zip(maps, windows)):
            if tuple(g.shape) != m.out_shape():
                self.fail("%s: map %d has shape %s, the model says %s" % (what, j, tuple(g.shape), m.out_shape()))
            if m.fmt and not normal_range_ok(w, m.fmt):
                self.fail("%s: the oracle map %d leaves the normal range of format %d" % (what, j, m.fmt))
            ref = m.cut(w)
            # util.rel_err's norm: the maximum of the map itself; a rectangle may hold one element or nothing but padding,
            # and is held against the maximum of the window it was cut from
            scale = float(np.abs(w if m.region == 5 else ref).max())
            err, bad = map_error(g, ref, scale, m.fmt)
            key = "worst16" if m.fmt else "worst"
            if bad:
                self.fail("%s: map %d is off by %.3g of the %s maximum (bar %.0e, map_format %d)"
                          % (what, j, err, "window's" if m.region == 5 else "map's", TOL, m.fmt))
            self.stats[key] = max(self.stats[key], err)
            self.stats["maps"] += 1

    def kernels_host(self, s):
        return [k.copy(order="F") for k in self.pool.sets[s]]

    def convolve(self, p, op):
        m, dp, torch = self.m, self.dp, self.torch
        entry, s = op[0], op[1]
        n = len(self.pool.sets[s])
        oh, ow = m.out_shape()
        ne, fmt = oh * ow, m.fmt
        what = "op %d %r" % (self.index, op)
        if entry in ("convolve", "convolve_out"):
            ks = self.kernels_host(s)
            outs = [_poisoned_host((oh, ow), fmt) for _ in range(n)] if entry == "convolve_out" else None
            got = p.convolve(ks, out=outs)
            for k in ks:
                k.fill(np.nan)
            if outs is not None and any(g is not o for g, o in zip(got, outs)):
                self.fail("%s: convolve(out=) returned other arrays" % what)
            for g in got:
                if g.dtype != FMT_DTYPES[fmt]:
                    self.fail("%s: map dtype %s for map_format %d" % (what, g.dtype, fmt))
            maps = [g if fmt == 0 else g.view(np.uint16) for g in got]
            for j, g in enumerate(maps):
                if (np.isnan(g).any() if fmt == 0 else (g == POISON16).any()):
                    self.fail("%s: map %d still holds the poison it was filled with" % (what, j))
        elif entry == "convolve_to_device":
            loc = op[2]
            bufs = [_guarded(torch, self.dev, ne, fmt, shift=(self.index + j) & 1) for j in range(n)]
            self.sync_all()
            if loc == HOST:
                ks = self.kernels_host(s)
                p.convolve_to_device(ks, [ptr for _, ptr in bufs], HOST)
                for k in ks:           # consumed when the call returns, whatever the output location
                    k.fill(np.nan)
            else:
                cell = [(t.data_ptr(), k.shape[0], k.shape[1]) for t, k in zip(dp.kernels_d[s], self.pool.sets[s])]
                p.convolve_to_device(cell, [ptr for _, ptr in bufs], DEVICE)
            p.synchronize()
            maps = []
            for j, (t, _) in enumerate(bufs):
                body = self.unguard(t, ne, fmt, (self.index + j) & 1, "%s, map %d" % (what, j))
                maps.append(body.reshape(ow, oh).T)
        else:
            shift = self.index & 1
            t, ptr = _guarded(torch, self.dev, n * ne, fmt, shift)
            self.sync_all()
            k0 = self.pool.sets[s][0]
            p.convolve_packed_device(n, dp.packed_d[s].data_ptr(), k0.shape[0], k0.shape[1], ptr)
            p.synchronize()
            body = self.unguard(t, n * ne, fmt, shift, what)
            maps = [a.T for a in body.reshape(n, ow, oh)]
        self.check_maps(maps, self.pool.windows(m.image, s, m.flip), what)
        self.stats["convolves"] += 1

    # -- refusals
    def refusal(self, p, op):
        m, dp, fc, torch = self.m, self.dp, self.fc, self.torch
        what, status = op[1], op[-1]
        oh, ow = m.out_shape()
        ne, fmt = oh * ow, m.fmt
        guards = []

        def device_outs(n):
            bufs = [_guarded(torch, self.dev, ne, fmt) for _ in range(n)]
            guards.extend(bufs)
            self.sync_all()
            return [ptr for _, ptr in bufs]

        def call():
            if what in ("output_region_5", "output_region_3_empty", "dynamic_tiles_3", "map_format_blockwise"):
                return p.set_option(op[2], op[3])
            if what == "rect_outside":
                return p.set_output_rect(*op[2:6])
            entry = op[2]
            if what == "kernel_features":
                if entry == "convolve":
                    return p.convolve([dp.wrong_f.copy(order="F")])
                return p.convolve_to_device([dp.wrong_f.copy(order="F")], device_outs(1), HOST)
            if what == "kernel_oversize":
                big = dp.oversize
                if entry == "convolve":
                    return p.convolve([big.copy(order="F")])
                if entry == "convolve_out":
                    return p.convolve([big.copy(order="F")], out=[_poisoned_host((oh, ow), fmt)])
                if entry == "convolve_to_device":
                    return p.convolve_to_device([(dp.oversize_d.data_ptr(), big.shape[0], big.shape[1])], device_outs(1), DEVICE)
                return p.convolve_packed_device(1, dp.oversize_d.data_ptr(), big.shape[0], big.shape[1], device_outs(1)[0])
            if what == "no_image":
                s = 1
                k0 = self.pool.sets[s][0]
                n = len(self.pool.sets[s])
                if entry == "convolve":
                    return p.convolve(self.kernels_host(s))
                if entry == "convolve_out":
                    return p.convolve(self.kernels_host(s), out=[_poisoned_host((oh, ow), fmt) for _ in range(n)])
                if entry == "convolve_to_device":
                    return p.convolve_to_device(self.kernels_host(s), device_outs(n), HOST)
                t, ptr = _guarded(torch, self.dev, n * ne, fmt)
                guards.append((t, ptr))
                self.sync_all()
                return p.convolve_packed_device(n, dp.packed_d[s].data_ptr(), k0.shape[0], k0.shape[1], ptr)
            raise ValueError(op)

        try:
            call()
        except fc.FFTConvError as e:
            if e.status != status:
                self.fail("op %d %r: refused with status %d, the header documents %d (%s)" % (self.index, op, e.status, status, e))
        else:
            self.fail("op %d %r: accepted, the header documents status %d" % (self.index, op, status))
        if guards:
            p.synchronize()
            for t, _ in guards:
                a = t.cpu().numpy()
                if not (np.isnan(a).all() if fmt == 0 else (a == POISON16).all()):
                    self.fail("op %d %r: a refused call wrote into its output buffer" % (self.index, op))
        self.stats["refusals"] += 1

    def check_state(self, p, op):
        """what the plan reports equals the model"""
        m = self.m
        i = p.refresh_info()           # (a refused call has not refreshed it)
        eb = 4 if m.fmt == 0 else 2
        got = (i.out_h, i.out_w, i.out_map_bytes, p.get_option("output_region"), p.get_option("map_format"), p.get_option("flip_kernels"))
        want = m.out_shape() + (m.rect[2] * m.rect[3] * eb, m.region, m.fmt, m.flip)
        if got != want:
            self.fail("op %d %r: the plan reports (out_h, out_w, out_map_bytes, output_region, map_format, flip_kernels) = %s, the model says %s"
                      % (self.index, op, got, want))
        if m.region == 5 and (p.get_option("rect_off_h"), p.get_option("rect_off_w")) != m.rect[:2]:
            self.fail("op %d %r: rectangle offsets differ from the model's %s" % (self.index, op, m.rect[:2]))

    # -- one op
    def step(self, p, op):
        m, dp, torch = self.m, self.dp, self.torch
        name = op[0]
        if is_convolve(op):
            self.convolve(p, op)
        elif name == "refuse":
            self.refusal(p, op)
            self.check_state(p, op)
        elif name == "set_image":
            a = self.pool.images[op[1]].copy(order="F")
            p.set_image(a)
            a.fill(np.nan)             # consumed when the call returns
        elif name == "set_image_device":
            p.set_image_device(dp.images_d[op[1]].data_ptr())
        elif name == "spectrum":       # the spectrum of image op[1], exported, then imported over another image
            p.set_image(self.pool.images[op[1]])
            spec = p.export_spectrum()
            p.set_image_device(dp.images_d[(op[1] + 1) % N_IMAGES].data_ptr())
            p.import_spectrum(spec)
        elif name == "prepare":
            k0 = self.pool.sets[op[1]][0]
            p.prepare_kernels_packed_device(len(self.pool.sets[op[1]]), dp.packed_d[op[1]].data_ptr(), k0.shape[0], k0.shape[1])
        elif name == "set_option":
            p.set_option(op[1], op[2])
        elif name == "set_output_rect":
            p.set_output_rect(*op[1:])
        elif name == "set_stream":     # the caller orders the two streams: everything queued so far is over before the switch
            self.sync_all()
            if op[1] and self.side is None:
                self.side = torch.cuda.Stream(self.dev)
            p.set_stream(self.side.cuda_stream if op[1] else 0)
        elif name == "synchronize":
            p.synchronize()
        elif name == "profile_read":
            first, again = p.profile(reset=True), p.profile(reset=True)
            if any(v["launches"] < 0 or v["units"] < 0 for v in first.values()) or any(v["launches"] or v["units"] for v in again.values()):
                self.fail("op %d %r: profile read %s, then %s after the reset" % (self.index, op, first, again))
        else:
            raise ValueError(op)
        status = m.apply(op)
        if name in ("set_option", "set_output_rect"):
            assert status == 0
            self.check_state(p, op)

    def epilogue(self, p):
        """every option back to its default, stream 0; image 0 and set 1 through the packed entry: the bits of a fresh plan"""
        for name, (_, default) in OPTIONS.items():
            if name == "map_format" and self.m.blockwise:
                continue
            self.step(p, ("set_option", name, self.defaults[name] if default is None else default))
        self.step(p, ("set_stream", 0))
        return packed_bits(self, p)


def packed_bits(run, p):
    """set_image_device(image 0) + convolve_packed_device(set 1) on a plan with default settings: the fp32 maps, checked"""
    run.step(p, ("set_image_device", 0))
    m, dp, torch = run.m, run.dp, run.torch
    n = len(run.pool.sets[1])
    ne = m.fft_h * m.fft_w
    t, ptr = _guarded(torch, run.dev, n * ne, 0)
    run.sync_all()
    k0 = run.pool.sets[1][0]
    p.convolve_packed_device(n, dp.packed_d[1].data_ptr(), k0.shape[0], k0.shape[1], ptr)
    p.synchronize()
    body = run.unguard(t, n * ne, 0, 0, "epilogue")
    run.check_maps([a.T for a in body.reshape(n, m.fft_w, m.fft_h)], run.pool.windows(0, 1, 0), "epilogue")
    return body.copy()


def fresh_bits(kind):
    """the maps of a fresh plan of the kind given only set_image_device(image 0) and convolve_packed_device(set 1), once per kind"""
    fresh = _ctx()["fresh"]
    if kind not in fresh:
        run = _Run(kind)
        p = create_plan(kind)
        try:
            fresh[kind] = packed_bits(run, p)
        finally:
            p.destroy()
    return fresh[kind]


def run_walk(kind, ops, seed=None, upto=None, epilogue=True):
    """runs the ops (a prefix: upto) on a fresh plan of the kind; returns the walk's figures or raises WalkFailure with the
    replayable report.  An FFTConvError nobody expected is a failure of the walk."""
    fc = _ctx()["fc"]
    ops = list(ops if upto is None else ops[:upto + 1])
    run = _Run(kind)
    want = fresh_bits(kind) if epilogue else None
    p = create_plan(kind)
    try:
        run.defaults = {name: p.get_option(name) for name, (_, default) in OPTIONS.items() if default is None}
        try:
            for run.index, op in enumerate(ops):
                run.step(p, op)
                run.stats["ops"] += 1
            run.index = len(ops)
            if epilogue:
                got = run.epilogue(p)
                differ = int((got.view(np.uint32) != want.view(np.uint32)).sum())
                if differ:
                    run.fail("epilogue: %d of %d elements differ from the maps of a fresh plan" % (differ, got.size))
        except fc.FFTConvError as e:
            raise WalkFailure(report(kind, seed, run, ops, "unexpected %s" % e)) from None
        except WalkFailure as e:
            raise WalkFailure(report(kind, seed, run, ops, str(e))) from None
    finally:
        run.torch.cuda.synchronize()
        p.destroy()
    return run.stats


def report(kind, seed, run, ops, what):
    upto = min(run.index, len(ops) - 1)
    return ("plan walk failed: kind %s, seed %s, op index %d: %s\nmodel state: %s\nops up to and including the failing one:\n%r"
            % (kind, seed, run.index, what, run.m.state(), ops[:upto + 1]))


def valid_walk(kind, ops):
    """whether the model can follow the ops (what a shrink candidate must still be): images before convolves, the no-image
    refusal only while there is none, regions and rectangles the kind has"""
    m = Model(kind)
    for op in ops:
        if is_convolve(op) or (op[0] == "refuse" and op[1] in ("kernel_features", "kernel_oversize")):
            if m.image is None:
                return False
        if op[0] == "refuse" and op[1] == "no_image" and m.image is not None:
            return False
        try:
            m.apply(op)
        except AssertionError:
            return False
    return True


# ---------------------------------------------------------------------------------------------------------------------
# the one-shot and two-step entries over the plan cache

CACHE_SHAPES = [(100, 90, 1, 9, 7), (130, 70, 2, 7, 9), (64, 150, 1, 5, 5), (90, 90, 3, 8, 8)]      # H, W, F, kh, kw
CACHE_OPTIONS = [None, {"kernel_path": 1}, {"map_format": 1}, {"max_transform": 64}]
CACHE_LIMIT = 2


def draw_cache_walk(seed, length=40):
    """calls of the one-shot entry (shape x options x image x kernel set, fresh arrays or out=), the two-step pair, refused calls
    (feature mismatch: before the cache is touched; a kernel taller than the window: with the plan taken and put back),
    cache_clear and cache_configure(0) / (2).  Half of the one-shot calls return to one of the last three keys."""
    rng = np.random.default_rng([seed, 1 << 20])
    ops, recent = [], []
    while len(ops) < length:
        u = rng.random()
        if u < 0.62 or not recent:
            if recent and rng.random() < 0.5:
                si, oi = recent[-int(rng.integers(1, min(3, len(recent)) + 1))]
            else:
                si, oi = int(rng.integers(0, len(CACHE_SHAPES))), int(rng.integers(0, len(CACHE_OPTIONS)))
            recent.append((si, oi))
            ops.append(("one_shot", si, oi, int(rng.integers(0, 2)), int(rng.integers(0, 3)), int(rng.integers(0, 2))))    # image, kernel set, out=
        elif u < 0.72:
            ops.append(("two_step", int(rng.integers(0, len(CACHE_SHAPES))), int(rng.integers(0, 2)), int(rng.integers(0, 3))))
        elif u < 0.80:
            ops.append(("refuse_features",) + recent[-1] + (-3,))
        elif u < 0.88:
            ops.append(("refuse_oversize",) + recent[-1] + (-3,))
        elif u < 0.93:
            ops.append(("cache_clear",))
        else:
            ops.append(("cache_configure", 0 if rng.random() < 0.5 else CACHE_LIMIT))
    return ops


class CacheModel:
    """which keys the cache holds: least recently used out first, at most `limit` plans; a taken plan is a hit"""

    def __init__(self, limit=CACHE_LIMIT):
        self.limit, self.keys = limit, []

    def take(self, key):
        hit = key in self.keys
        if hit:
            self.keys.remove(key)
        return hit

    def put(self, key):
        if self.limit > 0:
            self.keys.append(key)
            del self.keys[:max(0, len(self.keys) - self.limit)]

    def configure(self, limit):
        self.limit = limit
        del self.keys[:max(0, len(self.keys) - limit)]

    def clear(self):
        self.keys = []


class CachePool:
    """per shape: 2 images; kernel sets 0 and 1 of one size and count, set 2 ragged; float64 oracle maps computed once"""

    def __init__(self):
        self.images, self.sets, self._maps, self._oracle = [], [], {}, None
        for si, (H, W, F, kh, kw) in enumerate(CACHE_SHAPES):
            rng = np.random.default_rng([91, si])
            self.images.append([np.asfortranarray(rng.standard_normal((H, W, F), dtype=np.float32)) for _ in range(2)])
            sizes = [[(kh, kw)] * 3, [(kh, kw)] * 3, [(kh, kw), (max(1, kh - 2), kw), (kh, max(1, kw // 2))]]
            self.sets.append([[np.asfortranarray(rng.standard_normal((a, b, F), dtype=np.float32)) for a, b in sz] for sz in sizes])

    def windows(self, si, image, kset):
        key = (si, image, kset)
        if key not in self._maps:
            if self._oracle is None:
                self._oracle = util.Oracle()
            _, _, _, kh, kw = CACHE_SHAPES[si]
            self._maps[key] = self._oracle.conv_fft(self.images[si][image], kh, kw, self.sets[si][kset], f64=True)
        return self._maps[key]


def run_cache_walk(ops, seed=None):
    """runs the calls; every returned map against the oracle, dtype and shape against the options of THIS call, the cache's
    statistics and last_call_timing against the model after every call.  Leaves the cache at its default, empty."""
    c = _ctx()
    fc = c["fc"]
    pool = c.setdefault("cache_pool", CachePool())
    stats = dict(ops=0, convolves=0, maps=0, refusals=0, worst=0.0, worst16=0.0, hits=0)
    index, model = 0, CacheModel()

    def fail(what):
        raise WalkFailure("cache walk failed: seed %s, op index %d: %s\nmodel: limit %d, resident %s\nops up to and including the failing one:\n%r"
                          % (seed, index, what, model.limit, model.keys, ops[:index + 1]))

    def check(maps, si, image, kset, fmt):
        H, W, F, kh, kw = CACHE_SHAPES[si]
        shape = (util.ceil16(H + kh - 1), util.ceil16(W + kw - 1))
        wins = pool.windows(si, image, kset)
        if len(maps) != len(wins):
            fail("%d maps for %d kernels" % (len(maps), len(wins)))
        for j, (g, w) in enumerate(zip(maps, wins)):
            if g.dtype != FMT_DTYPES[fmt] or tuple(g.shape) != shape:
                fail("map %d is %s %s, this call's options ask for %s %s" % (j, g.dtype, tuple(g.shape), FMT_DTYPES[fmt], shape))
            if fmt and not normal_range_ok(w, fmt):
                fail("the oracle map %d leaves the normal range of format %d" % (j, fmt))
            err, bad = map_error(g if fmt == 0 else g.view(np.uint16), w, float(np.abs(w).max()), fmt)
            if bad:
                fail("map %d is off by %.3g of the window's maximum (bar %.0e, map_format %d)" % (j, err, TOL, fmt))
            key = "worst16" if fmt else "worst"
            stats[key] = max(stats[key], err)
            stats["maps"] += 1

    def expect_refusal(call, status):
        try:
            call()
        except fc.FFTConvError as e:
            if e.status != status:
                fail("refused with status %d, the header documents %d (%s)" % (e.status, status, e))
        else:
            fail("accepted, the header documents status %d" % status)
        stats["refusals"] += 1

    try:
        # the forced block-wise options really make block-wise plans, the others one-pass plans
        for si, (H, W, F, kh, kw) in enumerate(CACHE_SHAPES if "cache_plans_checked" not in c else ()):
            for oi, options in enumerate(CACHE_OPTIONS):
                with fc.Plan(H, W, F, kh, kw, options=options) as p:
                    assert (p.get_option("blockwise") > 1) == (oi == 3), (si, oi, p.get_option("blockwise"))
        c["cache_plans_checked"] = True
        fc.cache_configure(CACHE_LIMIT)
        fc.cache_clear()
        for index, op in enumerate(ops):
            before = fc.cache_stats()
            calls, hit = 0, None
            name = op[0]
            if name == "one_shot":
                _, si, oi, image, kset, use_out = op
                H, W, F, kh, kw = CACHE_SHAPES[si]
                options = CACHE_OPTIONS[oi]
                fmt = (options or {}).get("map_format", 0)
                data, ks = pool.images[si][image].copy(order="F"), [k.copy(order="F") for k in pool.sets[si][kset]]
                outs = None
                if use_out:
                    outs = [_poisoned_host((util.ceil16(H + kh - 1), util.ceil16(W + kw - 1)), fmt) for _ in ks]
                got = fc.cudaConvolutionFFT(data, kh, kw, ks, options=options, out=outs)
                data.fill(np.nan)
                for k in ks:
                    k.fill(np.nan)
                hit = model.take((si, oi))
                model.put((si, oi))
                calls = 1
                check(got, si, image, kset, fmt)
                if bool(fc.last_call_timing()["cache_hit"]) != hit:
                    fail("last_call_timing says cache_hit %d, the model %d" % (fc.last_call_timing()["cache_hit"], hit))
                stats["convolves"] += 1
                stats["hits"] += int(hit)
            elif name == "two_step":
                _, si, image, kset = op
                H, W, F, kh, kw = CACHE_SHAPES[si]
                data = pool.images[si][image].copy(order="F")
                h = fc.cudaFFTData(data, kh, kw)
                try:
                    data.fill(np.nan)
                    got = fc.cudaConvFFTData(h, [k.copy(order="F") for k in pool.sets[si][kset]])
                finally:
                    h.destroy()
                check(got, si, image, kset, 0)
                stats["convolves"] += 1
            elif name == "refuse_features":
                _, si, oi, status = op
                H, W, F, kh, kw = CACHE_SHAPES[si]
                bad = np.asfortranarray(np.ones((kh, kw, F + 1), dtype=np.float32))
                expect_refusal(lambda: fc.cudaConvolutionFFT(pool.images[si][0], kh, kw, [bad], options=CACHE_OPTIONS[oi]), status)
            elif name == "refuse_oversize":
                _, si, oi, status = op
                H, W, F, kh, kw = CACHE_SHAPES[si]
                bad = np.asfortranarray(np.ones((util.ceil16(H + kh - 1) + 1, kw, F), dtype=np.float32))
                expect_refusal(lambda: fc.cudaConvolutionFFT(pool.images[si][0], kh, kw, [bad], options=CACHE_OPTIONS[oi]), status)
                model.take((si, oi))       # the plan was taken (or built) for the call and goes back: argument errors leave it usable
                model.put((si, oi))
                calls = 1
            elif name == "cache_clear":
                fc.cache_clear()
                model.clear()
            elif name == "cache_configure":
                fc.cache_configure(op[1])
                model.configure(op[1])
            else:
                raise ValueError(op)
            after = fc.cache_stats()
            if after["plans"] > model.limit or after["plans"] != len(model.keys):
                fail("the cache holds %d plans, the model %d (limit %d)" % (after["plans"], len(model.keys), model.limit))
            if after["hits"] + after["misses"] - before["hits"] - before["misses"] != calls:
                fail("hits + misses grew by %d over a step with %d cache look-ups" % (after["hits"] + after["misses"] - before["hits"] - before["misses"], calls))
            if hit is not None and after["hits"] - before["hits"] != int(hit):
                fail("hits grew by %d, the model says %d" % (after["hits"] - before["hits"], int(hit)))
            stats["ops"] += 1
    except fc.FFTConvError as e:
        fail("unexpected %s" % e)
    finally:                       # the cache as every other test expects it
        fc.cache_configure(4)
        fc.cache_clear()
    return stats
