#!/usr/bin/env python3
"""What a sweep (nbody_sweep_*: a time step, a clamp and a number of steps per world) costs and what it saves: the same worlds, the
same GPU, the same process.

    python tools/ensemble_sweep_timing.py [--out FILE] [--trials 5] [--worlds 256] [--bodies 1024] [--steps 20]

256 worlds x 1 024 bodies in float32 (nb.Ensemble), every world a Plummer sphere of its own seed, FAST and EXACT arithmetic.
Three questions, each answered with host-clock times around synchronous calls from Python, after one warm-up call of every way,
as the median over `trials` (and the least and the largest trial).  These are end-to-end times of calls that end in a stream
synchronise, the conversion and the copy of the per-world arrays included; they are no kernel times.
  1. per-world parameters   sweep(delta[256 distinct], clamp[256], n_steps=steps) against update(0.1, n_steps=steps) of the SAME
                            handle: the same launches and the same pairs, so the difference is what reading the parameters per
                            world costs (the table's upload, the scalar loads per block, the second instantiation).
  2. against the old way    the same sweep against what the library offered before: one single-world nb.Ensemble per distinct
                            parameter value, created and uploaded beforehand and set to its clamp, each stepped with
                            update(delta[k], n_steps=steps) in turn.
  3. standing still         a convergence ladder: four groups of worlds/4 worlds taking 4, 8, 16 and 32 steps of a call of 32
                            (delta = T / steps), against the same call with every world taking all 32 steps.  A finished world's
                            blocks only carry their positions over; the launches stay whole.
There is no threshold in this file: it records.  This is a tool, not a test: it needs an MI355X and fails without one.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LADDER = (4, 8, 16, 32)


def _timed(f):
    t = time.perf_counter()
    f()
    return time.perf_counter() - t


def measure(worlds, n, steps, arith, trials):
    import numpy as np
    import nbody_simulation_amd as nb
    scenes = [nb.scenes.plummer(n, seed=0x5EE90000 + k) for k in range(worlds)]
    pos, vel, w = (np.stack([s[i] for s in scenes]) for i in range(3))
    delta = (0.05 + 0.1 * np.arange(worlds) / worlds).astype(np.float32)       # pairwise distinct
    clamp = np.where(np.arange(worlds) % 2 == 0, 1e-3, 1e-2).astype(np.float32)
    ens = nb.Ensemble(pos, vel, w, arith=arith)
    singles = []
    for k in range(worlds):
        s = nb.Ensemble(pos[k], vel[k], w[k], arith=arith, clamp=float(clamp[k]))
        singles.append(s)
    ladder_steps = np.repeat(np.array(LADDER, np.int32), (worlds + 3) // 4)[:worlds]
    ladder_delta = (3.2 / ladder_steps).astype(np.float32)
    full_steps = np.full(worlds, LADDER[-1], np.int32)

    def loop():
        for k, s in enumerate(singles):
            s.update(float(delta[k]), None, n_steps=steps)

    ways = dict(
        update=lambda: ens.update(0.1, None, n_steps=steps),
        sweep=lambda: ens.sweep(delta, clamp, None, n_steps=steps),
        loop=loop,
        ladder=lambda: ens.sweep(ladder_delta, clamp, ladder_steps, n_steps=LADDER[-1]),
        ladder_full=lambda: ens.sweep(ladder_delta, clamp, full_steps, n_steps=LADDER[-1]),
    )
    for f in ways.values():     # warm-up: code objects, the sweep's table
        f()
    t = {k: [] for k in ways}
    for _ in range(trials):     # (the ways alternate inside a trial)
        for k, f in ways.items():
            t[k].append(_timed(f))
    for s in singles:
        s.close()
    ens.close()
    return {k: (sorted(v)[len(v) // 2], min(v), max(v)) for k, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--worlds", type=int, default=256)
    ap.add_argument("--bodies", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=20)
    a = ap.parse_args()
    if not os.path.exists("/dev/kfd"):
        print("ensemble_sweep_timing: no GPU here; a measurement path does not fall back", file=sys.stderr)
        return 2
    lines = [f"# tools/ensemble_sweep_timing.py: {a.worlds} worlds x {a.bodies} bodies, float32; {a.trials} trials after one warm-up call of every way,",
             "# the ways alternating inside a trial; seconds of one whole call from Python (it ends in a stream synchronise):",
             "# median (least .. largest trial)",
             f"#   update       update(0.1, n_steps={a.steps}) of the ensemble",
             f"#   sweep        sweep({a.worlds} distinct deltas, two clamps, n_steps={a.steps}) of the same ensemble",
             f"#   loop         one single-world Ensemble per world, update(delta[k], n_steps={a.steps}) of each in turn",
             f"#   ladder       sweep with n_steps = {LADDER[-1]}, four groups of worlds taking {', '.join(map(str, LADDER))} steps",
             f"#   ladder_full  the same call with every world taking all {LADDER[-1]} steps",
             f"{'arith':>6} {'way':>12} {'seconds per call':>40}   against"]
    for arith in ("fast", "exact"):
        t0 = time.perf_counter()
        t = measure(a.worlds, a.bodies, a.steps, arith, a.trials)
        print(f"ensemble_sweep_timing: {arith} took {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)

        def fmt(k):
            med, lo, hi = t[k]
            return f"{med * 1e3:10.3f} ms ({lo * 1e3:9.3f} .. {hi * 1e3:9.3f})"

        lines.append(f"{arith:>6} {'update':>12} {fmt('update'):>40}")
        lines.append(f"{arith:>6} {'sweep':>12} {fmt('sweep'):>40}   sweep / update = {t['sweep'][0] / t['update'][0]:.3f}")
        lines.append(f"{arith:>6} {'loop':>12} {fmt('loop'):>40}   loop / sweep = {t['loop'][0] / t['sweep'][0]:.1f}")
        lines.append(f"{arith:>6} {'ladder':>12} {fmt('ladder'):>40}   ladder / ladder_full = {t['ladder'][0] / t['ladder_full'][0]:.3f} "
                     f"(steps taken: {sum(LADDER) / (4 * LADDER[-1]):.3f} of the full call's)")
        lines.append(f"{arith:>6} {'ladder_full':>12} {fmt('ladder_full'):>40}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
