#!/usr/bin/env python3
"""A watched sweep of an ensemble against the sweep alone and against what it replaces: the same worlds, the same GPU, the same
process.

    NBODY_HIP_LIBRARY=lab python tools/ensemble_wsweep_timing.py [--out FILE] [--trials 5] [--steps 20]

Three shapes, as tools/ensemble_watch_timing.py has them: the bodies of 256 worlds x 1 024 bodies in float32 (nb.Ensemble) and in
float64 (nb.Ensemble64), and the tracers of 64 worlds x 1 024 bodies x 16 384 tracers (nb.RestrictedEnsemble, float32).  Every
handle runs under arith="exact".  Per shape, for `steps` steps:
  uniform             one watch_sweep() in which every world has the same delta and stride 1, with all six per-target arrays:
                      steps + 1 samples of every world, the reduce, the copies — a watch() through the sweep's kernels;
  varied              one watch_sweep() with a delta of its own per world and strides 1, 2, 3, 4, 1, ... (world k: k % 4 + 1):
                      still steps + 1 sampling launches, in which world k's blocks work at every (k % 4 + 1)-th s alone — with 20
                      steps 21, 11, 7 and 6 samples, 45 of every 84 (world, sample) pairs;
  sweep               the run alone: one sweep(delta, n_steps=steps) with the varied deltas;
  handles             what watch_sweep() replaces: one single-world handle per value, made before anything is timed, each
                      calling watch(delta[k], steps, stride=stride[k]) in turn — its records and rows are compared bit for bit
                      with the varied watch_sweep()'s before anything is timed.
After one warm-up pass of everything, a TRIAL times each in turn with the host clock around the call (every call ends in a
synchronise of the handle's stream).  Reported: the median over the trials of the seconds per call, and the least and the largest
trial.  These are end-to-end times of host calls; they are no kernel times.  Every timed call steps the worlds on from where the
last one left them: the positions drift, the work per call does not.  There is no threshold in this file: it records.  This is a
tool, not a test: it needs an MI355X and fails without one.
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
ROWS = ("min_d2", "min_index", "min_sample", "first_close", "close_samples", "first_out")


def measure(dtype, worlds, n, m, trials, steps):
    import numpy as np
    import nbody_simulation_amd as nb
    rng = np.random.default_rng(0x3A7C + n + m + np.dtype(dtype).itemsize)
    pos = rng.uniform(0.0, H, (worlds, n, 2)).astype(dtype)
    vel = rng.standard_normal((worlds, n, 2)).astype(dtype)
    w = rng.integers(1, 13, (worlds, n)).astype(np.uint32)
    limit2 = np.full(worlds, LIMIT2, np.float32)
    tr = (rng.uniform(0.0, H, (worlds, m, 2)).astype(dtype), rng.standard_normal((worlds, m, 2)).astype(dtype)) if m else None
    same_delta = np.full(worlds, DELTA, dtype)
    own_delta = (DELTA * (0.5 + np.arange(worlds) / worlds)).astype(dtype)          # pairwise distinct
    stride = (np.arange(worlds) % 4 + 1).astype(np.int32)
    kw = dict(tracers=True) if m else {}

    def make(sel=slice(None)):
        if m:
            return nb.RestrictedEnsemble(pos[sel], vel[sel], w[sel], (tr[0][sel], tr[1][sel]), arith="exact")
        return (nb.Ensemble if dtype == np.float32 else nb.Ensemble64)(pos[sel], vel[sel], w[sel], arith="exact")

    def varied(ens):
        return ens.watch_sweep(own_delta, n_steps=steps, stride=stride, limit2=limit2, height=H, **kw)

    def handles(singles):
        return [e.watch(float(own_delta[k]), n_steps=steps, stride=int(stride[k]), limit2=limit2[k:k + 1], height=H, **kw)
                for k, e in enumerate(singles)]

    singles = [make(slice(k, k + 1)) for k in range(worlds)]
    # the bits, before anything is timed: every world of the varied call against its single-world handle
    with make() as a:
        rec, rows = varied(a)
    alone = handles(singles)
    same = all(rec[k].tobytes() == alone[k][0][0].tobytes() and
               all(rows[name][k].tobytes() == alone[k][1][name][0].tobytes() for name in ROWS) for k in range(worlds))
    ens = make()
    t = {name: [] for name in ("uniform", "varied", "sweep", "handles")}

    def timed(name, fn):
        t0 = time.perf_counter()
        fn()
        t[name].append(time.perf_counter() - t0)

    def one_pass(record):
        keep = {k: list(v) for k, v in t.items()}
        timed("uniform", lambda: ens.watch_sweep(same_delta, n_steps=steps, limit2=limit2, height=H, **kw))
        timed("varied", lambda: varied(ens))
        timed("sweep", lambda: ens.sweep(own_delta, n_steps=steps))
        timed("handles", lambda: handles(singles))
        if not record:
            t.update(keep)

    one_pass(False)                 # warm-up
    for _ in range(trials):
        one_pass(True)
    ens.close()
    for e in singles:
        e.close()
    return same, {k: (sorted(v)[len(v) // 2], min(v), max(v)) for k, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    a = ap.parse_args()
    if not os.path.exists("/dev/kfd"):
        print("ensemble_wsweep_timing: no GPU here; a measurement path does not fall back", file=sys.stderr)
        return 2
    import numpy as np
    lab = os.environ.get("NBODY_HIP_LIBRARY", "") == "lab"
    lines = [f"# tools/ensemble_wsweep_timing.py ({'laboratory' if lab else 'product'} library): {a.trials} trials after one warm-up pass; a trial times one",
             f"# watch_sweep(n_steps={a.steps}) with one delta and stride 1 in every world, one with a delta per world and strides k % 4 + 1, one",
             f"# sweep(n_steps={a.steps}) with those deltas, and one loop over a single-world handle per world calling watch(delta[k], {a.steps},",
             f"# stride[k]), in that order, all with rows, under arith=\"exact\"; limit2 = {LIMIT2:g}, height = {H}",
             "# milliseconds per call, host clock around calls that end in a stream synchronise: median (least .. largest trial)"]
    for dtype, worlds, n, m in ((np.float32, 256, 1024, 0), (np.float64, 256, 1024, 0), (np.float32, 64, 1024, 16384)):
        same, t = measure(dtype, worlds, n, m, a.trials, a.steps)
        pairs = worlds * (m * n if m else n * (n - 1))
        lines.append(f"{worlds} x {n} x {m} {np.dtype(dtype).name} {'tracers' if m else 'bodies'}: {pairs} ordered pairs per full sample and per step; "
                     f"bits of the varied watch_sweep() against the handles: {'equal' if same else 'DIFFER'}")
        for name, (med, lo, hi) in t.items():
            lines.append(f"    {name:>10} {med * 1e3:10.3f} ms ({lo * 1e3:9.3f} .. {hi * 1e3:9.3f})   {med / t['sweep'][0]:8.2f} x sweep")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
