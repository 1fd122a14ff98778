"""Random walks of one live plan on the GPU (tests/plan_walk.py): every kind x the committed seeds, and walks of the one-shot and
two-step entries over the plan cache.

Every walk is about 70 calls on ONE plan -- images, the four convolve entries, kernel preparation, every option that can be
changed on a live plan, rectangles, stream switches, spectrum hand-over, calls that must be refused -- with every map of its 17
convolves held against the float64 oracle (fp32: util.rel_err < 1e-5, a rectangle against the maximum of its window; 16-bit maps: the same plus half an ulp), device
destinations between poisoned guard bands, and an epilogue that must reproduce the bits of a fresh plan.  The cases run in the
module's child process (test_accuracy_gpu._Child), which exits with the module: a case that times out or takes the child down
ends it and nothing more starts.  A failing walk prints its ops as a literal; tools/plan_walk.py replays (--kind K --seed S
--upto I) and shrinks (--shrink) it, and the shrunk sequence of a defect goes into REGRESSIONS.

Proof that the walk has teeth (the convention of test_stream_order_host.py): one-line mutations of the library, each built in a
scratch copy, never committed, whose only effect is wrong values; this file run once against each on an MI355X.

  1. "flip_kernels" loses OPT_FORGETS in kLongOptions (no ColumnCache::forget: prepared column spectra survive a change of the
     flip): test_plan_walk[specialised-4], [exact-3], [bluestein-3] and [exact-sentinel0] fail, each at a convolve_packed of a
     prepared set, maps off by 1.3 - 1.5 of the window's maximum.
  2. ColumnCache::consume (csrc/column_cache.hpp) no longer clears the record it found -- `state_ = Empty;` dropped (consumed
     column spectra count again): test_plan_walk[generic-4], [save_blocks-1], [save_blocks-4] and [save_blocks-sentinel1] fail
     (a packed set convolved again after other kernels went through A; on the overlap-save plan two host sets of one size and
     count, told apart by nothing but their contents).
  3. evict_lru in plan_cache.cpp picks the MOST recently used plan (`<` turned into `>`): test_cache_walk[1], [2] and [3] fail, at
     calls 14, 5 and 11: last_call_timing's cache_hit disagrees with the model's view of which keys are resident.
  4. `c.hits++;` dropped in cache_take: test_cache_walk[1], [2] and [3] fail at the first call served from the cache (calls 1, 1
     and 5): hits + misses grew by 0 over a call with one look-up.
  5. "kernel_chunk_mb" loses OPT_FORGETS: the 32 random walks and the cache walks PASS -- the wrong map needs four calls in a row
     (a small "batch_maps", a prepare, a chunk budget that then holds more kernels, a packed convolve of the prepared set), which the
     generator did not deal.  sentinel2 below was written by hand for it and test_plan_walk[generic-sentinel2] alone fails under
     this mutation; the generator itself still lacks the transition.

(1, 2 and 5 were run again, with the failures named above, when the record of what A holds became one object, ColumnCache:
fftconv_plan::a_holds.  tests/test_column_cache_host.py holds that object alone to a model of A over every short call sequence.)

Four more invalidations were tried or read and CANNOT change what a caller sees; none of them counts above (the counts of passes
are those of the lines the calls below replaced; these four runs were not repeated).  All four are still
there, each as ONE call on the cache; what the cache has made impossible to write is half of one -- clearing the ready record
and leaving the request, or the reverse -- because the two are states of one record.
`a_holds.source_overwritten(dk)` behind the pin_k gather of fftconv_plan_convolve and `a_holds.forget()` before the one-shot
entry in plan_cache.cpp hands its plan back (35 passed under each): both guard a record that names the plan's own pinned
kernel buffer pin_k, and only the one-shot entry ever prepares from that buffer.  Inside that entry the request is taken by the
set_image that follows and the ready record by run_group_impl's consume (mutation 2 above) before the call returns; a call that
fails in between is an allocation or HIP failure whose plan is destroyed, not cached.  (The first was two lines, one per record,
the second a call beside two direct writes of the request's flag: that a line of either is missing can no longer be written.)
`a_holds.forget()` in prepare_kernels (37 passed): on the direct path ready() replaces the record three lines on, and
only a launch that fails in between sees the difference; on the deferred path request() replaces it -- a stale ready record beside
the new request, which the old pair of records could spell, is not a state of the cache.  The flush in fftconv_plan_set_stream,
`if (a_holds.pending()) flush_pending_prepare()` (37 passed): without it the request is launched later, still on the
stream it was asked for, and the header has the caller order the two streams around the switch, so the values cannot differ.
All four are second guards, dead while the calls behind them stand.
"""
import pytest

import plan_walk
from test_accuracy_gpu import _Child

pytestmark = pytest.mark.gpu

SEEDS = (1, 2, 3, 4)         # consecutive: together they deal every (entry, family) pair of a kind (plan_walk.combos)
CACHE_SEEDS = (1, 2, 3)
WALK_LENGTH = 70

# (kind, ops, what was wrong): shrunk sequences of defects the walk found, replayed with the committed seeds.  None so far: the
# committed seeds and a soak of 22 115 walks found the library clean.
REGRESSIONS = []
# (kind, ops, what it guards): the shortest sequences at which one invalidation is all that stands between the caller and a wrong
# map, replayed as cases sentinel0.. beside the random walks.  0 and 1: what `tools/plan_walk.py --shrink` made of exact-3 under
# mutation 1 and of save_blocks-1 under mutation 2 of the docstring.  2: written by hand for mutation 5 -- one kernel's column
# spectra are prepared (one map per launch, no chunk budget), then the budget holds all three kernels of the set.
SENTINELS = [
    ("exact", [("set_image", 2), ("prepare", 1), ("set_option", "flip_kernels", 1), ("convolve_packed", 1)],
     "prepared column spectra must not survive a change of flip_kernels"),
    ("save_blocks", [("set_image", 0), ("convolve_to_device", 2, 1), ("convolve_out", 1)],
     "column spectra consumed by one convolve must not count for the next set staged at the same address"),
    ("generic", [("set_image", 1), ("set_option", "batch_maps", 1), ("prepare", 2), ("set_option", "kernel_chunk_mb", 1), ("convolve_packed", 2)],
     "column spectra prepared for one chunk of kernels must not count for a larger chunk"),
]
REPLAYS = {"regression%d" % i: r for i, r in enumerate(REGRESSIONS)}
REPLAYS.update(("sentinel%d" % i, r) for i, r in enumerate(SENTINELS))


@pytest.fixture(scope="module")
def device():
    child = _Child(globals())
    yield child
    if child.gone:
        child.kill()
    else:
        child.ex.shutdown(wait=True)


# ---- the child's side

def _case_walk(kind, seed):
    ops = REPLAYS[seed][1] if isinstance(seed, str) else plan_walk.draw_walk(kind, seed, WALK_LENGTH)
    return plan_walk.run_walk(kind, ops, seed=seed)


def _case_cache_walk(seed):
    return plan_walk.run_cache_walk(plan_walk.draw_cache_walk(seed), seed=seed)


# ---- the tests

CASES = [(kind, seed) for kind in plan_walk.KIND_NAMES for seed in SEEDS] + [(r[0], name) for name, r in REPLAYS.items()]


@pytest.mark.parametrize("kind,seed", CASES, ids=["%s-%s" % c for c in CASES])
def test_plan_walk(device, kind, seed):
    stats = device("_case_walk", kind, seed)
    print("%s seed %s: %d ops, %d convolves, %d maps, %d refusals; worst fp32 error %.2e, worst 16-bit excess %.2e"
          % (kind, seed, stats["ops"], stats["convolves"], stats["maps"], stats["refusals"], stats["worst"], stats["worst16"]))
    assert stats["convolves"] >= 15 or isinstance(seed, str)


@pytest.mark.parametrize("seed", CACHE_SEEDS)
def test_cache_walk(device, seed):
    stats = device("_case_cache_walk", seed)
    print("cache walk seed %d: %d calls, %d convolves (%d from a cached plan), %d maps, %d refusals; worst fp32 error %.2e, worst 16-bit excess %.2e"
          % (seed, stats["ops"], stats["convolves"], stats["hits"], stats["maps"], stats["refusals"], stats["worst"], stats["worst16"]))
    assert stats["ops"] == 40 and stats["hits"] > 0
