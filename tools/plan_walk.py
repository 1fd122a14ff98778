#!/usr/bin/env python3
"""Soak, replay and shrink the random walks of one live plan (tests/plan_walk.py; GPU box, repository root).

tools/fuzz_gpu.py builds a fresh plan per case; this tool changes options, images, streams, regions and formats on a LIVE plan and
checks every map of every convolve against the float64 oracle (kind "cache": the one-shot and two-step entries over the plan
cache).  One line per walk; the exit status is 1 after a failing walk, 2 after a fault, abort or timeout.

    python tools/plan_walk.py --kind exact --seed 3               # the walk tests/test_plan_walk_gpu.py runs as exact-3
    python tools/plan_walk.py --kind exact --seed 3 --upto 17     # its first 18 ops
    python tools/plan_walk.py --seconds 600 --seed 1000           # fresh seeds from 1000 on, every kind in turn
    python tools/plan_walk.py --walks 50 --kind save_blocks
    python tools/plan_walk.py --kind exact --seed 3 --shrink      # a walk that failed NUMERICALLY, down to a minimal literal

The walks run in one child process under a time limit per walk, as in the test.  A child that dies or runs out of time is never
replaced: the tool stops there and says so -- a fault is a finding to be read out of the code, not to be run again.  --shrink
deletes one op at a time, greedily, running every candidate the model can follow on a fresh plan, until no single deletion keeps
the failure (wrong values, a wrong shape, an unexpected status), and prints the minimal sequence for REGRESSIONS.
"""
import argparse, concurrent.futures, multiprocessing, os, sys, time
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import plan_walk as pw

WALK_TIMEOUT_S = 120


def child_walk(kind, seed, ops, upto, epilogue):
    """(figures, None) or (None, the failure's report)"""
    try:
        if kind == "cache":
            return pw.run_cache_walk(ops if upto is None else ops[:upto + 1], seed=seed), None
        return pw.run_walk(kind, ops, seed=seed, upto=upto, epilogue=epilogue), None
    except pw.WalkFailure as e:
        return None, str(e)


class Stopped(Exception):
    pass


class Child:
    def __init__(self):
        self.ex = concurrent.futures.ProcessPoolExecutor(max_workers=1, mp_context=multiprocessing.get_context("spawn"))

    def __call__(self, *args):
        try:
            return self.ex.submit(child_walk, *args).result(timeout=WALK_TIMEOUT_S)
        except (concurrent.futures.TimeoutError, concurrent.futures.process.BrokenProcessPool) as e:
            procs = list((self.ex._processes or {}).values())
            self.ex.shutdown(wait=False, cancel_futures=True)
            for p in procs:
                p.kill()
            for p in procs:
                p.join(10)
            raise Stopped("%s in walk %s: nothing more is run" % (type(e).__name__, args[:2]))

    def close(self):
        self.ex.shutdown(wait=True)


def draw(kind, seed, length):
    return pw.draw_cache_walk(seed, length or 40) if kind == "cache" else pw.draw_walk(kind, seed, length or 70)


def shrink(child, kind, seed, ops):
    """greedy one-op deletions that keep a numerical failure"""
    valid = (lambda o: True) if kind == "cache" else (lambda o: pw.valid_walk(kind, o))
    stats, why = child(kind, seed, ops, None, False)
    if why is None:
        stats, why = child(kind, seed, ops, None, True)
        if why is None:
            print("the walk passes: nothing to shrink")
            return 0
        print("only the epilogue fails: the sequence is kept whole\n%s" % why)
        return 1
    first = why.splitlines()[0]
    index = int(first.split("op index ")[1].split(":")[0])
    ops = ops[:index + 1]
    runs, changed = 1, True
    while changed:
        changed = False
        for i in range(len(ops) - 2, -1, -1):          # (the failing op itself stays)
            cand = ops[:i] + ops[i + 1:]
            if not valid(cand):
                continue
            _, w = child(kind, seed, cand, None, False)
            runs += 1
            if w is not None and w.splitlines()[0].split("op index ")[1].split(":", 1)[0] == str(len(cand) - 1):
                ops, why, changed = cand, w, True
    print("shrunk to %d ops in %d runs:\n%s" % (len(ops), runs, why))
    print("REGRESSIONS entry:\n    (%r, %r, \"...\")," % (kind, ops))
    return 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kind", default="", help="one of %s, cache; default: every one in turn" % ", ".join(pw.KIND_NAMES))
    ap.add_argument("--seed", type=int, default=1, help="the seed of the (first) walk")
    ap.add_argument("--seconds", type=float, default=0.0)
    ap.add_argument("--walks", type=int, default=0)
    ap.add_argument("--length", type=int, default=0, help="ops per walk (default: the test's)")
    ap.add_argument("--upto", type=int, default=-1, help="replay ops 0..UPTO only")
    ap.add_argument("--shrink", action="store_true")
    ap.add_argument("--quiet", action="store_true")
    args = ap.parse_args()
    kinds = [args.kind] if args.kind else pw.KIND_NAMES + ["cache"]
    for k in kinds:
        if k != "cache" and k not in pw.KINDS:
            ap.error("unknown kind %r" % k)
    child = Child()
    t0 = time.time()
    total = dict(walks=0, ops=0, convolves=0, maps=0, refusals=0, worst=0.0, worst16=0.0)
    failures = []
    try:
        if args.shrink:
            return shrink(child, kinds[0], args.seed, draw(kinds[0], args.seed, args.length))
        n = 0
        while True:
            if args.walks and n >= args.walks:
                break
            if args.seconds and time.time() - t0 > args.seconds:
                break
            if not args.walks and not args.seconds and n >= len(kinds):
                break
            kind, seed = kinds[n % len(kinds)], args.seed + n // len(kinds)
            n += 1
            t1 = time.time()
            upto = args.upto if args.upto >= 0 else None
            stats, why = child(kind, seed, draw(kind, seed, args.length), upto, upto is None)
            total["walks"] += 1
            if why is not None:
                failures.append((kind, seed))
                print("FAIL %s seed %d (--kind %s --seed %d)\n%s" % (kind, seed, kind, seed, why), flush=True)
                continue
            for key in ("ops", "convolves", "maps", "refusals"):
                total[key] += stats[key]
            for key in ("worst", "worst16"):
                total[key] = max(total[key], stats[key])
            if not args.quiet:
                print("ok   %s seed %d: %d ops, %d convolves, %d maps, %d refusals, worst fp32 %.2e, worst 16-bit excess %.2e, %.1f s"
                      % (kind, seed, stats["ops"], stats["convolves"], stats["maps"], stats["refusals"], stats["worst"], stats["worst16"], time.time() - t1), flush=True)
    except Stopped as e:
        print("STOPPED: %s" % e, flush=True)
        return 2
    finally:
        if not args.shrink:
            print("# %d walks in %.0f s: %d ops, %d convolves, %d maps checked, %d refusals; %d failed %s; worst relative error of an fp32 map %.2e, "
                  "worst excess of a 16-bit map over half an ulp %.2e" % (total["walks"], time.time() - t0, total["ops"], total["convolves"], total["maps"],
                                                                           total["refusals"], len(failures), failures, total["worst"], total["worst16"]), flush=True)
    child.close()
    return 1 if failures else 0


if __name__ == "__main__":
    sys.exit(main())
