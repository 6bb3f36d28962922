#!/usr/bin/env python3
"""A resident run of an ensemble of small worlds against the calls it is another route for: the same worlds, the same GPU, the
same process.

    python tools/ensemble_resident_timing.py [--out FILE] [--trials 5]

Four shapes of worlds of at most 256 bodies — 4 096 worlds x 3 bodies, 4 096 x 64, 1 024 x 256 (nb.Ensemble / nb.Ensemble64) and a
ragged handle of 1 024 worlds of 3 .. 256 bodies (nb.RaggedEnsemble / nb.RaggedEnsemble64) — in float32 and float64, under
arith="exact" and arith="fast", for 1 000 steps and again for 1 024 steps, which is one full launch of a resident run.  Per shape:
  run                 one run(delta, n_steps): one launch per 1 024 steps, every world in LDS throughout;
  update              one update(delta, n_steps) of the same handle: one launch per step;
  sweep               one sweep(delta[k], n_steps=n_steps) with a delta of its own per world: one launch per step.
Before anything is timed the rows after run(delta, n_steps) and after update(delta, n_steps) on a twin handle are compared bit for
bit.  After one warm-up pass of everything, a TRIAL times each in turn with the host clock around the call (every call ends in a
synchronise of the handle's stream).  Reported: the median over the trials of the seconds per call, and the least and the largest
trial.  These are end-to-end times of host calls; they are no kernel times.  Every timed call steps the worlds on from where the
last one left them: the positions drift, the work per call does not.  Last, update() at 256 worlds x 1 024 bodies x 20 steps under
arith="exact": the shape the README quotes for the stepping kernels, which this tool does not change.  There is no threshold in
this file: it records.  This is a tool, not a test: it needs an MI355X and fails without one.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

H = 100_000
DELTA = 0.01
SHAPES = (("4096 x 3", 4096, 3), ("4096 x 64", 4096, 64), ("1024 x 256", 1024, 256), ("ragged 1024 x 3..256", 1024, None))


def stats(v):
    return sorted(v)[len(v) // 2], min(v), max(v)


def make(nb, np, dtype, worlds, n, arith):
    """-> a function that makes a fresh handle of the shape, and its ordered pairs per step."""
    rng = np.random.default_rng(0x5E51 + worlds + (n or 0) + np.dtype(dtype).itemsize)
    if n is None:
        sizes = 3 + (np.arange(worlds) * 253) // (worlds - 1)          # 3 .. 256, every size about four times
        rng.shuffle(sizes)
        ps = [rng.uniform(0.0, H, (k, 2)).astype(dtype) for k in sizes]
        vs = [rng.standard_normal((k, 2)).astype(dtype) for k in sizes]
        ws = [rng.integers(1, 13, k).astype(np.uint32) for k in sizes]
        cls = nb.RaggedEnsemble if dtype == np.float32 else nb.RaggedEnsemble64
        return (lambda: cls(ps, vs, ws, arith=arith)), int((sizes * (sizes - 1)).sum())
    pos = rng.uniform(0.0, H, (worlds, n, 2)).astype(dtype)
    vel = rng.standard_normal((worlds, n, 2)).astype(dtype)
    w = rng.integers(1, 13, (worlds, n)).astype(np.uint32)
    cls = nb.Ensemble if dtype == np.float32 else nb.Ensemble64
    return (lambda: cls(pos, vel, w, arith=arith)), worlds * n * (n - 1)


def rows(np, e):
    p, v, _ = e.particles()
    return [np.concatenate(x) if isinstance(x, list) else x for x in (p, v)]


def measure(nb, np, dtype, worlds, n, arith, steps, trials):
    new, pairs = make(nb, np, dtype, worlds, n, arith)
    own_delta = (DELTA * (0.5 + np.arange(worlds) / worlds)).astype(dtype)          # pairwise distinct
    # the bits, before anything is timed
    with new() as a, new() as b:
        a.run(DELTA, n_steps=steps)
        b.update(DELTA, None, n_steps=steps)
        same = all(x.tobytes() == y.tobytes() for x, y in zip(rows(np, a), rows(np, b)))
    ens = new()
    t = {name: [] for name in ("run", "update", "sweep")}

    def timed(name, fn, record):
        t0 = time.perf_counter()
        fn()
        if record:
            t[name].append(time.perf_counter() - t0)

    for trial in range(trials + 1):                 # the first pass is the warm-up
        timed("run", lambda: ens.run(DELTA, n_steps=steps), trial > 0)
        timed("update", lambda: ens.update(DELTA, None, n_steps=steps), trial > 0)
        timed("sweep", lambda: ens.sweep(own_delta, n_steps=steps), trial > 0)
    ens.close()
    return same, pairs, {k: stats(v) for k, v in t.items()}


def quoted_shape(nb, np, dtype, trials):
    """update() at 256 x 1 024 x 20 steps under EXACT, as tools/ensemble_wsweep_timing.py has the shape."""
    rng = np.random.default_rng(0x3A7C + 1024 + np.dtype(dtype).itemsize)
    pos = rng.uniform(0.0, H, (256, 1024, 2)).astype(dtype)
    vel = rng.standard_normal((256, 1024, 2)).astype(dtype)
    w = rng.integers(1, 13, (256, 1024)).astype(np.uint32)
    t = []
    with (nb.Ensemble if dtype == np.float32 else nb.Ensemble64)(pos, vel, w, arith="exact") as e:
        for trial in range(trials + 1):
            t0 = time.perf_counter()
            e.update(DELTA, None, n_steps=20)
            if trial:
                t.append(time.perf_counter() - t0)
    return stats(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--trials", type=int, default=5)
    a = ap.parse_args()
    if not os.path.exists("/dev/kfd"):
        print("ensemble_resident_timing: no GPU here; a measurement path does not fall back", file=sys.stderr)
        return 2
    import numpy as np
    import nbody_simulation_amd as nb
    lab = os.environ.get("NBODY_HIP_LIBRARY", "") == "lab"
    lines = []

    def say(line):
        lines.append(line)
        print(line, flush=True)
        if a.out:                                   # (kept up to date line by line: a run that is cut short leaves what it measured)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    say(f"# tools/ensemble_resident_timing.py ({'laboratory' if lab else 'product'} library): {a.trials} trials after one warm-up pass; a trial times one")
    say("# run(delta, n_steps), one update(delta, n_steps) and one sweep(n_steps) with a delta per world on the same handle, in that order;")
    say(f"# delta = {DELTA:g}; 1 024 steps are one full launch of a resident run, 1 000 steps one launch of 1 000")
    say("# milliseconds per call, host clock around calls that end in a stream synchronise: median (least .. largest trial)")
    for dtype in (np.float32, np.float64):
        for arith in ("exact", "fast"):
            for name, worlds, n in SHAPES:
                for steps in (1000, 1024):
                    same, pairs, t = measure(nb, np, dtype, worlds, n, arith, steps, a.trials)
                    say(f"{name} {np.dtype(dtype).name} {arith} {steps} steps: {pairs} ordered pairs per step; "
                        f"rows of run() against update(): {'equal' if same else 'DIFFER'}")
                    for call, (med, lo, hi) in t.items():
                        say(f"    {call:>8} {med * 1e3:10.3f} ms ({lo * 1e3:9.3f} .. {hi * 1e3:9.3f})   {med / steps * 1e6:9.3f} us per step"
                            f"   {t['update'][0] / med:7.2f} x update's rate")
    say("# update(delta, n_steps=20) of 256 worlds x 1 024 bodies under arith=\"exact\": the stepping kernels' quoted shape")
    for dtype in (np.float32, np.float64):
        med, lo, hi = quoted_shape(nb, np, dtype, a.trials)
        say(f"256 x 1024 {np.dtype(dtype).name} exact 20 steps: update {med * 1e3:10.3f} ms ({lo * 1e3:9.3f} .. {hi * 1e3:9.3f})")
    return 0


if __name__ == "__main__":
    sys.exit(main())
