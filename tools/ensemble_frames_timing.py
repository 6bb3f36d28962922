#!/usr/bin/env python3
"""Frames of an ensemble against the ways a user had before them: the same worlds, the same bytes, the same GPU, the same process.

    python tools/ensemble_frames_timing.py [--out FILE] [--trials 7] [--calls 100]

Two shapes: 256 worlds x 1 024 bodies (nb.Ensemble), and 64 worlds x 1 024 bodies x 16 384 tracers (nb.RestrictedEnsemble, the
tracers painted).  Each at render_px = 100, the largest the LDS route takes, and at render_px = 125, the global route.  Three ways
to the same [worlds, render_px, render_px, 4] bytes, which are compared before anything is timed:
  frames          one call of frames(render_px=...) on the ensemble;
  download+host   what a user did before: particles() (and tracers()) and the oracle's draw() per world on the host;
  world loop      one nb.World per world, created and uploaded beforehand, frame() of each in turn.
After one warm-up pass of everything, a TRIAL times each way in turn (the ways alternate within a trial): the host clock around
`calls` calls of frames, and around one pass of each of the other two; every call ends in a synchronise of its stream.  Reported
per way: the median over the trials of the seconds per frame of all worlds, and the least and the largest trial.  These are
end-to-end times of host calls, device-to-host copy of the tiles included; they are no kernel times.  There is no threshold in
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


def scene(np, worlds, n, m, seed):
    rng = np.random.default_rng(seed)
    pos = rng.uniform(-0.02 * H, 1.02 * H, (worlds, n, 2)).astype(np.float32)
    vel = (rng.standard_normal((worlds, n, 2)) * 8.0).astype(np.float32)
    w = rng.integers(1, 13, (worlds, n)).astype(np.uint32)        # one in six heavy
    tpos = rng.uniform(-0.02 * H, 1.02 * H, (worlds, m, 2)).astype(np.float32)
    tvel = (rng.standard_normal((worlds, m, 2)) * 8.0).astype(np.float32)
    return pos, vel, w, tpos, tvel


def measure(worlds, n, m, render_px, trials, calls):
    import numpy as np
    import nbody_simulation_amd as nb
    from oracle import oracle as orc
    orc.lib()
    pos, vel, w, tpos, tvel = scene(np, worlds, n, m, 0xF7A3E5 + n + m)
    tr = m > 0
    ens = nb.RestrictedEnsemble(pos, vel, w, (tpos, tvel)) if tr else nb.Ensemble(pos, vel, w)
    singles = [nb.World(pos[k], vel[k], w[k], method="direct", tracers=(tpos[k], tvel[k]) if tr else None) for k in range(worlds)]

    def frames():
        return ens.frames(H, render_px, True) if tr else ens.frames(H, render_px)

    def host():
        p, v, ww = ens.particles()
        if tr:
            tp, tv = ens.tracers()
            one = np.ones(m, np.uint32)
            return np.stack([orc.draw(np.concatenate([p[k], tp[k]]), np.concatenate([v[k], tv[k]]), np.concatenate([ww[k], one]), H, render_px)
                             for k in range(worlds)])
        return np.stack([orc.draw(p[k], v[k], ww[k], H, render_px) for k in range(worlds)])

    def loop():
        return np.stack([s.frame(H, render_px, tracers=tr) for s in singles])

    a, b, c = frames(), host(), loop()     # warm-up of every way, and the bytes
    same = bool(np.array_equal(a, b) and np.array_equal(a, c))
    for _ in range(3):
        frames()
    t = dict(frames=[], host=[], loop=[])
    for _ in range(trials):
        t0 = time.perf_counter()
        for _ in range(calls):
            frames()
        t["frames"].append((time.perf_counter() - t0) / calls)
        t0 = time.perf_counter()
        host()
        t["host"].append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        loop()
        t["loop"].append(time.perf_counter() - t0)
    for s in singles:
        s.close()
    ens.close()
    return same, {k: (sorted(v)[len(v) // 2], min(v), max(v)) for k, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--trials", type=int, default=7)
    ap.add_argument("--calls", type=int, default=100)
    a = ap.parse_args()
    if not os.path.exists("/dev/kfd"):
        print("ensemble_frames_timing: no GPU here; a measurement path does not fall back", file=sys.stderr)
        return 2
    lines = [f"# tools/ensemble_frames_timing.py: {a.trials} trials after one warm-up pass; a trial times {a.calls} calls of frames(), one pass of",
             "# download + host draw() per world, and one pass of one nb.World per world calling frame(), in that order",
             "# seconds per frame of ALL worlds, host clock around calls that end in a stream synchronise: median (least .. largest trial)",
             "# route: render_px 100 = one block per world, pixels in LDS; render_px 125 = work buffer in device memory, two launches",
             f"{'worlds x bodies x tracers':>28} {'px':>4} {'route':>7} {'frames()':>34} {'download + host draw':>34} {'nb.World loop':>34} {'host/frames':>12} {'loop/frames':>12}  bytes"]
    for worlds, n, m in ((256, 1024, 0), (64, 1024, 16384)):
        for px in (100, 125):
            same, t = measure(worlds, n, m, px, a.trials, a.calls)

            def fmt(k):
                med, lo, hi = t[k]
                return f"{med * 1e3:9.3f} ms ({lo * 1e3:8.3f} .. {hi * 1e3:8.3f})"

            lines.append(f"{f'{worlds} x {n} x {m}':>28} {px:>4} {'LDS' if px * px * 8 <= 81920 else 'global':>7} {fmt('frames'):>34} {fmt('host'):>34} "
                         f"{fmt('loop'):>34} {t['host'][0] / t['frames'][0]:12.1f} {t['loop'][0] / t['frames'][0]:12.1f}  {'equal' if same else 'DIFFER'}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
