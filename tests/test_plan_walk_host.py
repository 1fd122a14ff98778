"""Guards of the plan walk itself (tests/plan_walk.py), no GPU: the generator is deterministic and its committed seeds meet the
coverage conditions, the model cuts windows as plain slicing and padding do, the 16-bit tolerance agrees with the reference
conversion, and the oracle maps of every pool entry lie in the range the 16-bit bound is stated for."""
import collections

import numpy as np
import pytest

import plan_walk as pw
from test_map_format_gpu import from_bits, to_bits
from test_map_format_host import conversion_inputs, numpy_bf16
from test_plan_walk_gpu import CACHE_SEEDS, SEEDS, WALK_LENGTH

KINDS = pw.KIND_NAMES


def walks(kind):
    return [pw.draw_walk(kind, seed, WALK_LENGTH) for seed in SEEDS]


@pytest.mark.parametrize("kind", KINDS)
def test_draw_is_deterministic(kind):
    for seed in SEEDS:
        a, b = pw.draw_walk(kind, seed, WALK_LENGTH), pw.draw_walk(kind, seed, WALK_LENGTH)
        assert a == b and repr(a) == repr(b)
        assert eval(repr(a)) == a                                  # plain tuples: a printed walk can be replayed
        assert pw.valid_walk(kind, a)
    assert pw.draw_walk(kind, SEEDS[0], WALK_LENGTH) != pw.draw_walk(kind, SEEDS[1], WALK_LENGTH)
    assert pw.draw_walk(kind, 1, WALK_LENGTH) != pw.draw_walk(KINDS[(KINDS.index(kind) + 1) % len(KINDS)], 1, WALK_LENGTH)
    assert pw.draw_cache_walk(CACHE_SEEDS[0]) == pw.draw_cache_walk(CACHE_SEEDS[0])


@pytest.mark.parametrize("kind", KINDS)
def test_every_op_of_the_alphabet_occurs(kind):
    count = collections.Counter(pw.op_item(op) for ops in walks(kind) for op in ops)
    m = pw.Model(kind)
    assert set(count) - set(pw.ENTRIES) - {"refuse:no_image"} <= set(m.alphabet())       # nothing the kind does not support is drawn
    rare = {item: count[item] for item in list(m.alphabet()) + list(pw.ENTRIES) + ["refuse:no_image"] if count[item] < 3}
    assert not rare, rare
    if m.blockwise:
        assert count["set_option:map_format"] == 0 and count["refuse:map_format_blockwise"] >= 3
    assert (count["spectrum"] > 0) == m.exact
    # every value of the options that decide what a map holds, a value other than the default of every other; every style of rectangle
    values = collections.defaultdict(set)
    for ops in walks(kind):
        for op in ops:
            if op[0] == "set_option":
                values[op[1]].add(op[2])
    for name, (drawn, default) in pw.OPTIONS.items():
        if name == "map_format" and m.blockwise:
            continue
        want = {v for v in drawn if not (name == "output_region" and m.region_empty(v))}
        assert values[name] <= want and values[name] - {default}, (name, values[name])
        if name in ("flip_kernels", "map_format", "output_region"):
            assert values[name] == want, (name, values[name])
    rects = [op[1:] for ops in walks(kind) for op in ops if op[0] == "set_output_rect"]
    assert any(r == (0, 0, m.fft_h, m.fft_w) for r in rects) and any(r[2] == 1 and r[3] > 1 for r in rects) and any(r[3] == 1 and r[2] > 1 for r in rects)
    assert any(r[0] % 2 and r[1] % 2 and r[2] % 2 for r in rects) and any(not (r[0] % 2 or r[1] % 2 or r[2] % 2 or r[3] % 2) for r in rects)
    assert all(m.rect_valid(r) for r in rects)
    assert all(not m.rect_valid(op[2:6]) for ops in walks(kind) for op in ops if op[0] == "refuse" and op[1] == "rect_outside")


@pytest.mark.parametrize("kind", KINDS)
def test_every_family_comes_right_before_every_entry(kind):
    m = pw.Model(kind)
    seen = set()
    for ops in walks(kind):
        assert sum(pw.is_convolve(op) for op in ops) >= 15
        for i, op in enumerate(ops):
            if pw.is_convolve(op):
                seen.update((op[0], pw.op_family(prev)) for prev in ops[max(0, i - 2):i])
    want = {(entry, fam) for entry in pw.ENTRIES for fam in m.families()}
    assert want <= seen, sorted(want - seen)
    # a prepare of the very set a packed convolve then uses, with another op in between
    assert any(ops[i][0] == "prepare" and ops[i + 2][0] == "convolve_packed" and ops[i][1] == ops[i + 2][1] and ops[i + 1][0] != "prepare"
               for ops in walks(kind) for i in range(len(ops) - 2))
    # ... and of the other set, and a convolve with the other set
    assert any(ops[i][0] == "prepare" and pw.is_convolve(ops[j]) and ops[j][1] != ops[i][1] for ops in walks(kind) for i in range(len(ops) - 2)
               for j in (i + 1, i + 2))


@pytest.mark.parametrize("kind", KINDS)
def test_convolves_under_every_format_and_region(kind):
    m0 = pw.Model(kind)
    formats, regions, flips, streams = set(), set(), set(), set()
    for ops in walks(kind):
        m = pw.Model(kind)
        for op in ops:
            if pw.is_convolve(op):
                assert m.image is not None
                formats.add(m.fmt), regions.add(m.region), flips.add(m.flip), streams.add(m.stream)
            m.apply(op)
    assert formats == set(m0.formats())
    assert regions == {r for r in range(6) if r == 5 or not m0.region_empty(r)}
    assert flips == {0, 1} and streams == {0, 1}
    assert m0.region_empty(3) == (kind == "generic_thin")


def test_cutting_against_plain_slicing():
    for kind in KINDS:
        m = pw.Model(kind)
        H, W, F, kh, kw, _ = pw.KINDS[kind]
        fh, fw = (H + kh - 1 + 15) // 16 * 16, (W + kw - 1 + 15) // 16 * 16
        assert (m.fft_h, m.fft_w) == (fh, fw)
        win = np.arange(fh * fw, dtype=np.float64).reshape(fh, fw) + 1.0          # entry (y, x) = y * fw + x + 1
        assert m.cut(win) is not None and np.array_equal(m.cut(win), win)
        m.apply(("set_option", "output_region", 1))
        assert np.array_equal(m.cut(win), win[:H + kh - 1, :W + kw - 1]) and m.out_shape() == (H + kh - 1, W + kw - 1)
        m.apply(("set_option", "output_region", 2))
        y0, x0 = (kh - 1) // 2, (kw - 1) // 2
        assert np.array_equal(m.cut(win), win[y0:y0 + H, x0:x0 + W]) and m.out_shape() == (H, W)
        if H >= kh and W >= kw:
            m.apply(("set_option", "output_region", 3))
            assert np.array_equal(m.cut(win), win[kh - 1:H, kw - 1:W]) and m.out_shape() == (H - kh + 1, W - kw + 1)
        m.apply(("set_option", "output_region", 4))
        ph = 1 << int(np.ceil(np.log2(fh)))
        pw_ = 1 << int(np.ceil(np.log2(fw)))
        want = np.pad(win, ((0, ph - fh), (0, pw_ - fw)))
        assert m.out_shape() == (ph, pw_) and np.array_equal(m.cut(win), want)
        for rect in [(0, 0, fh, fw), (1, 3, fh - 1, 5), (fh - 1, fw - 1, 1, 1), (2, 0, 1, fw), (0, 7, fh, 1)]:
            m.apply(("set_output_rect",) + rect)
            oh, ow, h, w = rect
            want = np.array([[(oh + y) * fw + (ow + x) + 1.0 for x in range(w)] for y in range(h)])
            assert m.region == 5 and np.array_equal(m.cut(win), want)
        # a refusal changes nothing
        before = m.state()
        assert m.apply(("refuse", "rect_outside", 0, 0, fh + 1, 1, -1)) == -1 and m.state() == before
    assert [pw.pow2_window(n) for n in (1, 16, 17, 32, 33, 100, 284, 1139)] == [16, 16, 32, 32, 64, 128, 512, 2048]


@pytest.mark.parametrize("fmt", [1, 2])
def test_16_bit_tolerance_against_the_reference_conversion(fmt):
    """a value converted by the reference conversion is within half an ulp (the helper's) of itself, one ulp off is not"""
    x = conversion_inputs()
    mant, e_min, top = pw.FMT_SHAPE[fmt]
    x = x[np.isfinite(x) & (np.abs(x) < top * (1 - 2.0 ** -(mant + 2)))]            # no overflow: the bound is stated for the normal range
    bits = to_bits(x, fmt)
    if fmt == 2:
        assert np.array_equal(bits, numpy_bf16(x))
    assert pw.from_bits is from_bits                               # decoded as the map-format tests decode
    back = from_bits(bits, fmt)
    ref = x.astype(np.float64)
    assert np.all(np.abs(back - ref) <= 0.5 * pw.ulp16(np.maximum(np.abs(back), np.abs(ref)), fmt))
    # the ulp helper is the spacing of the format: the next pattern up is exactly one ulp away (finite, non-negative patterns)
    pats = np.arange(0, (0x7BFF if fmt == 1 else 0x7F7F), dtype=np.uint16)
    v0, v1 = pw.from_bits(pats, fmt), pw.from_bits(pats + 1, fmt)
    assert np.array_equal(v1 - v0, pw.ulp16(v0, fmt))
    # map_error: exact conversions pass with no excess, a pattern one step off fails, a NaN pattern fails
    sel = np.abs(ref) > 2.0 ** e_min
    scale = 1.0
    err, bad = pw.map_error(bits[sel], ref[sel], scale, fmt)
    assert err == 0.0 and not bad
    off = bits[sel].copy()
    off[0] += 2
    assert pw.map_error(off, ref[sel], 1e-300 + float(np.abs(ref[sel][0])), fmt)[1]
    off = bits[sel].copy()
    off[5] = pw.POISON16
    assert pw.map_error(off, ref[sel], scale, fmt)[1]
    # fp32: the bar itself
    r = np.array([1.0, -2.0, 0.5])
    assert not pw.map_error(np.float32(r), r, 2.0, 0)[1] and pw.map_error(np.float32(r + [0, 0, 3e-5]), r, 2.0, 0)[1]


@pytest.mark.parametrize("kind", KINDS)
def test_oracle_maps_lie_in_the_normal_range(kind, oracle):
    pool = pw.Pool(kind)
    assert len(pool.entries()) == 18
    for entry in pool.entries():
        maps = pool.windows(*entry)
        assert len(maps) == len(pool.sets[entry[1]])
        for w in maps:
            assert w.dtype == np.float64 and w.shape == (pw.Model(kind).fft_h, pw.Model(kind).fft_w)
            assert pw.normal_range_ok(w, 1) and pw.normal_range_ok(w, 2), (kind, entry, float(np.abs(w).max()))
    # the two sets of one size differ in nothing but their contents; flipping matters
    assert [k.shape for k in pool.sets[1]] == [k.shape for k in pool.sets[2]] and len({k.shape for k in pool.sets[0]}) > 1
    assert not np.allclose(pool.windows(0, 1, 0)[0], pool.windows(0, 1, 1)[0])


def test_cache_walk_inputs(oracle):
    pool = pw.CachePool()
    for si in range(len(pw.CACHE_SHAPES)):
        for image in range(2):
            for kset in range(3):
                assert all(pw.normal_range_ok(w, 1) for w in pool.windows(si, image, kset))
    for seed in CACHE_SEEDS:
        ops = pw.draw_cache_walk(seed)
        names = collections.Counter(op[0] for op in ops)
        assert len(ops) == 40 and all(names[n] > 0 for n in ("one_shot", "two_step", "refuse_features", "refuse_oversize", "cache_clear", "cache_configure"))
    every = [op for seed in CACHE_SEEDS for op in pw.draw_cache_walk(seed)]
    assert {op[2] for op in every if op[0] == "one_shot"} == set(range(len(pw.CACHE_OPTIONS)))
    assert {op[1] for op in every if op[0] == "one_shot"} == set(range(len(pw.CACHE_SHAPES)))
    assert {op[1] for op in every if op[0] == "cache_configure"} == {0, pw.CACHE_LIMIT}
    # the model: least recently used out first
    m = pw.CacheModel(2)
    assert not m.take("a")
    m.put("a"), m.put("b")
    assert m.take("a")
    m.put("a"), m.put("c")
    assert m.keys == ["a", "c"] and not m.take("b")
    m.configure(0)
    m.put("d")
    assert m.keys == []
