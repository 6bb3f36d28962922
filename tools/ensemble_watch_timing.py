#!/usr/bin/env python3
"""A watched run of an ensemble against the run alone and against what a user did before it: the same worlds, the same GPU, the
same process.

    NBODY_HIP_LIBRARY=lab python tools/ensemble_watch_timing.py [--out FILE] [--trials 5] [--steps 20]

Three shapes: the bodies of 256 worlds x 1 024 bodies in float32 (nb.Ensemble) and in float64 (nb.Ensemble64), and the tracers of
64 worlds x 1 024 bodies x 16 384 tracers (nb.RestrictedEnsemble, float32).  Every handle runs under arith="exact".  Per shape, for
`steps` steps:
  update()            the run alone: one update(delta, n_steps=steps);
  watch()             one watch(delta, steps) with all six per-target arrays: steps + 1 samples, the reduce, the copies;
  records only        the same with rows=False;
  stride 4            the same with stride=4 and rows=False: a quarter of the samples;
  loop on the host    what a user did before: steps + 1 times encounters(rows=True) and particles() (or tracers()), with
                      update(delta, 1) in between, folded on the host in NumPy — its records and rows are compared bit for bit
                      with watch()'s before anything is timed.
With the laboratory library the watch() and records-only columns are measured twice, with one and with two targets per lane of
the sampling kernel (NBODY_WATCH_PER_LANE); the product library has the one ensemble_watch.h names.  After one warm-up pass of
everything, a TRIAL times each in turn with the host clock around the call (every call ends in a synchronise of the handle's
stream).  Reported: the median over the trials of the seconds per call, and the least and the largest trial.  These are end-to-end
times of host calls; they are no kernel times.  Every timed call steps the worlds on from where the last one left them: the
positions drift, the work per call does not.  There is no threshold in this file: it records.  This is a tool, not a test: it
needs an MI355X and fails without one.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

H = 100_000
LIMIT2 = 1.0e4      # squared world units: some pairs of every world are close, most are not
DELTA = 0.01
NEVER = 0xffffffff


def fold(np, seen, limit, dtype):
    """The contract's fold of one world's samples on the host: seen = [(s, nn_index, nn_d2, positions)]."""
    n = seen[0][1].shape[0]
    rows = dict(min_d2=np.full(n, np.inf, dtype), min_index=np.full(n, -1, np.int32), min_sample=np.full(n, NEVER, np.uint32),
                first_close=np.full(n, NEVER, np.uint32), close_samples=np.zeros(n, np.uint32), first_out=np.full(n, NEVER, np.uint32))
    for s, idx, d2, pos in seen:
        has = idx >= 0
        close = has & (d2 < dtype(limit))
        out = ~((pos[:, 1] < H) & (pos[:, 0] < H) & (pos[:, 1] >= 0) & (pos[:, 0] >= 0))
        take = has & ((rows["min_index"] < 0) | (d2 < rows["min_d2"]))
        rows["min_d2"] = np.where(take, d2, rows["min_d2"])
        rows["min_index"] = np.where(take, idx, rows["min_index"]).astype(np.int32)
        rows["min_sample"] = np.where(take, np.uint32(s), rows["min_sample"]).astype(np.uint32)
        rows["first_close"] = np.where(close & (rows["first_close"] == NEVER), np.uint32(s), rows["first_close"]).astype(np.uint32)
        rows["close_samples"] = (rows["close_samples"] + close).astype(np.uint32)
        rows["first_out"] = np.where(out & (rows["first_out"] == NEVER), np.uint32(s), rows["first_out"]).astype(np.uint32)
    return rows


def measure(dtype, worlds, n, m, trials, steps, lanes):
    import numpy as np
    import nbody_simulation_amd as nb
    rng = np.random.default_rng(0x3A7C + n + m + np.dtype(dtype).itemsize)
    pos = rng.uniform(0.0, H, (worlds, n, 2)).astype(dtype)
    vel = rng.standard_normal((worlds, n, 2)).astype(dtype)
    w = rng.integers(1, 13, (worlds, n)).astype(np.uint32)
    limit2 = np.full(worlds, LIMIT2, np.float32)
    tr = (rng.uniform(0.0, H, (worlds, m, 2)).astype(dtype), rng.standard_normal((worlds, m, 2)).astype(dtype)) if m else None

    def make():
        if m:
            return nb.RestrictedEnsemble(pos, vel, w, tr, arith="exact")
        return (nb.Ensemble if dtype == np.float32 else nb.Ensemble64)(pos, vel, w, arith="exact")

    def watch(ens, rows=True, stride=1):
        kw = dict(tracers=True) if m else {}
        return ens.watch(DELTA, n_steps=steps, limit2=limit2, height=H, stride=stride, rows=rows, **kw)

    def loop(ens):
        seen = [[] for _ in range(worlds)]
        for s in range(steps + 1):
            _, idx, d2, _ = ens.encounters(limit2, True, True) if m else ens.encounters(limit2, True)
            p = ens.tracers()[0] if m else ens.particles()[0]
            for k in range(worlds):
                seen[k].append((s, idx[k], d2[k], p[k]))
            if s < steps:
                ens.update(DELTA)
        return [fold(np, seen[k], LIMIT2, dtype) for k in range(worlds)]

    # the bits, on fresh handles, for every variant of the sampling kernel to be timed
    same = True
    with make() as a:
        want = loop(a)
    for lane in lanes:
        if lane:
            os.environ["NBODY_WATCH_PER_LANE"] = str(lane)
        with make() as b:
            rec, rows = watch(b)
            same = same and all(rows[name][k].tobytes() == want[k][name].tobytes() for k in range(worlds) for name in want[k])
            same = same and int(rec["samples"][0]) == steps + 1
    ens = make()
    names = ["update"] + [f"{what}{lane}" for lane in lanes for what in ("watch", "records")] + ["stride4", "loop"]
    t = {name: [] for name in names}

    def timed(name, fn):
        t0 = time.perf_counter()
        fn()
        t[name].append(time.perf_counter() - t0)

    def one_pass(record):
        keep = {k: list(v) for k, v in t.items()}
        timed("update", lambda: ens.update(DELTA, n_steps=steps))
        for lane in lanes:
            if lane:
                os.environ["NBODY_WATCH_PER_LANE"] = str(lane)
            timed(f"watch{lane}", lambda: watch(ens))
            timed(f"records{lane}", lambda: watch(ens, rows=False))
        timed("stride4", lambda: watch(ens, rows=False, stride=4))
        timed("loop", lambda: loop(ens))
        if not record:
            t.update(keep)

    one_pass(False)                 # warm-up
    for _ in range(trials):
        one_pass(True)
    ens.close()
    return same, {k: (sorted(v)[len(v) // 2], min(v), max(v)) for k, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    a = ap.parse_args()
    if not os.path.exists("/dev/kfd"):
        print("ensemble_watch_timing: no GPU here; a measurement path does not fall back", file=sys.stderr)
        return 2
    import numpy as np
    lab = os.environ.get("NBODY_HIP_LIBRARY", "") == "lab"
    lanes = (1, 2) if lab else (0,)     # 0: the library's own choice
    lines = [f"# tools/ensemble_watch_timing.py ({'laboratory' if lab else 'product'} library): {a.trials} trials after one warm-up pass; a trial times one",
             f"# update(delta, {a.steps}), one watch(delta, {a.steps}) with rows and one without per variant of the sampling kernel, one with stride 4",
             f"# without rows, and one loop of {a.steps + 1} x (encounters(rows=True) + download) with update(delta, 1) in between, folded in NumPy,",
             f"# in that order, under arith=\"exact\"; limit2 = {LIMIT2:g}, height = {H}; targets per lane: " +
             (", ".join(str(v) for v in lanes) if lab else "the product's (kWatchPerLane)"),
             "# milliseconds per call, host clock around calls that end in a stream synchronise: median (least .. largest trial)"]
    for dtype, worlds, n, m in ((np.float32, 256, 1024, 0), (np.float64, 256, 1024, 0), (np.float32, 64, 1024, 16384)):
        same, t = measure(dtype, worlds, n, m, a.trials, a.steps, lanes)
        pairs = worlds * (m * n if m else n * (n - 1))
        lines.append(f"{worlds} x {n} x {m} {np.dtype(dtype).name} {'tracers' if m else 'bodies'}: {pairs} ordered pairs per sample and per step; "
                     f"bits of watch() against the loop: {'equal' if same else 'DIFFER'}")
        for name, (med, lo, hi) in t.items():
            lines.append(f"    {name:>10} {med * 1e3:10.3f} ms ({lo * 1e3:9.3f} .. {hi * 1e3:9.3f})   {med / t['update'][0]:8.2f} x update")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
